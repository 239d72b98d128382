"""Cost of the device-resident drifters (nxs_dyn_drifters_*) at 2 km, against the only route without them: nxs_dyn_get_state of M_UT, M_UM and M_conc, the host
interleave of Drifters::move, two point locators built from host coordinates (nxs_regrid_create + nxs_regrid_interp_nodes twice), a numpy mask, and
nxs_dyn_put_state of a zeroed M_UT -- which needs the whole prognostic state.

    python scripts/time_drifters.py [mesh] [--out DIR]     measure on the GPU, write DIR/drifters.json (default profiles/) and DESIGN.md's table
    python scripts/time_drifters.py --from-json FILE       no GPU: copy FILE to profiles/drifters.json and rewrite DESIGN.md's table from it

Workload: equally spaced drifters over the mesh's bounding box, about 1e5 and about 1.5e6 of them; M_UT and M_UM after three steps of the arctic case.
Reported per count: device time of `move` (its kernel; the undisplaced locator exists), of `conc` + `mask` with a current displaced locator, and of the
displaced locator's rebuild on its own (HIP events, option "drifters_timing"), warm, medians of 9; the wall time of the same calls; the host route's wall time
and the ratio of the two wall times.  No threshold: the numbers are the result."""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- drifters-measurement:begin (written by scripts/time_drifters.py) -->", "<!-- drifters-measurement:end -->"
CONC_LIM = 0.15
REPS = 9


def measure(kind, out_dir, counts=(100_000, 1_500_000)):
    import numpy as np
    from nextsim_amd import dynamics, forcing as F, interp, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Nn, Ne = lm.num_nodes, lm.num_elements
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    for _ in range(3):
        fe.step()
    fe.synchronize()
    state = fe.get_state()
    full = dict(f); full.update(state)                       # what put_state needs: every member
    import torch
    res = {"mesh": kind, "num_nodes": Nn, "num_elements": Ne, "conc_lim": CONC_LIM, "samples": REPS, "counts": [],
           "conditions": {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "unknown", "state": "arctic case after 3 steps (BBM, 120 sub-steps)",
                          "timing": "HIP events on the handle's stream (option drifters_timing) for *_us; time.perf_counter around synchronised calls for *_ms; 2 warm-up repetitions dropped"}}
    idx = np.ascontiguousarray(lm.indices)
    med = lambda v: float(np.median(np.asarray(v)))          # noqa: E731
    for want in counts:
        side = int(round(np.sqrt(want * np.ptp(lm.coord_y) / np.ptp(lm.coord_x))))
        nx = int(round(want / side))
        gx, gy = np.meshgrid(np.linspace(lm.coord_x.min(), lm.coord_x.max(), nx), np.linspace(lm.coord_y.min(), lm.coord_y.max(), side))
        px, py = np.ascontiguousarray(gx.ravel()), np.ascontiguousarray(gy.ravel())
        ids = np.arange(px.size, dtype=np.int32)
        r = {"num_drifters": int(px.size)}
        # ---- the device route
        fe.set_option("drifters_timing", 1)
        dev = {k: [] for k in ("move_us", "conc_us", "mask_us", "rebuild_us")}
        wall = {k: [] for k in ("move_ms", "conc_mask_ms", "conc_mask_rebuild_ms")}
        left = moved = None
        for rep in range(REPS + 2):
            fe.put_state(full)                               # M_UT back, the displaced locator stale
            fe.drifters_set(0, px, py, ids)
            fe.synchronize()
            t0 = time.perf_counter(); fe.drifters_move(); fe.synchronize(); t1 = time.perf_counter()
            fe.drifters_conc(0, want_host=False)             # rebuilds the displaced locator
            t_re = fe.debug_array("drifters_ms")
            fe.synchronize()
            t2 = time.perf_counter(); fe.drifters_conc(0, want_host=False); left = fe.drifters_mask(0, CONC_LIM); fe.synchronize(); t3 = time.perf_counter()
            t = fe.debug_array("drifters_ms")
            if rep < 2:
                continue
            dev["move_us"].append(t[1] * 1e3); dev["conc_us"].append(t[2] * 1e3); dev["mask_us"].append(t[3] * 1e3); dev["rebuild_us"].append(t_re[0] * 1e3)
            wall["move_ms"].append((t1 - t0) * 1e3); wall["conc_mask_ms"].append((t3 - t2) * 1e3)
        # (wall time of conc + mask when the locator has to be rebuilt first)
        for rep in range(REPS):
            fe.put_state(full); fe.drifters_set(0, px, py, ids); fe.drifters_move(); fe.synchronize()
            t0 = time.perf_counter(); fe.drifters_conc(0, want_host=False); fe.drifters_mask(0, CONC_LIM); fe.synchronize()
            wall["conc_mask_rebuild_ms"].append((time.perf_counter() - t0) * 1e3)
        moved = fe.drifters_get(0)
        fe.set_option("drifters_timing", 0)
        r["device"] = {k: med(v) for k, v in dev.items()}
        r["device"].update({k: med(v) for k, v in wall.items()})
        r["device"]["total_wall_ms"] = r["device"]["move_ms"] + r["device"]["conc_mask_rebuild_ms"]
        r["left_after_mask"] = int(left)
        # ---- the route available without them
        parts = {k: [] for k in ("get_state_ms", "move_interp_ms", "conc_interp_ms", "mask_ms", "put_state_ms", "total_ms")}
        host_left = None
        for rep in range(REPS + 2):
            fe.put_state(full); fe.synchronize()
            t0 = time.perf_counter()
            s = fe.get_state()
            t1 = time.perf_counter()
            inter = np.empty((Nn, 2)); inter[:, 0] = s["UT"][:Nn]; inter[:, 1] = s["UT"][Nn:]          # drifters.cpp:483-487
            rg = interp.Regrid(idx, lm.coord_x, lm.coord_y)
            d = rg.interp_nodes(inter, px, py, isdefault=True, defaultvalue=0.)
            rg.close()
            qx, qy = px + d[:, 0], py + d[:, 1]
            t2 = time.perf_counter()
            rg = interp.Regrid(idx, lm.coord_x + s["UM"][:Nn], lm.coord_y + s["UM"][Nn:])
            v = rg.interp_nodes(s["conc"][:, None], qx, qy, isdefault=True, defaultvalue=0.)[:, 0]
            rg.close()
            cd = np.maximum(0., np.minimum(1., v))
            t3 = time.perf_counter()
            keep = cd > CONC_LIM
            hx, hy, hi, hc = qx[keep], qy[keep], ids[keep], cd[keep]
            t4 = time.perf_counter()
            z = dict(full); z.update(s); z["UT"] = np.zeros(2 * Nn)
            fe.put_state(z)
            t5 = time.perf_counter()
            host_left = int(keep.sum())
            if rep < 2:
                continue
            for k, a, b in (("get_state_ms", t0, t1), ("move_interp_ms", t1, t2), ("conc_interp_ms", t2, t3), ("mask_ms", t3, t4), ("put_state_ms", t4, t5), ("total_ms", t0, t5)):
                parts[k].append((b - a) * 1e3)
        r["host_route"] = {k: med(v) for k, v in parts.items()}
        r["same_result"] = bool(host_left == left and np.array_equal(hx, moved["x"]) and np.array_equal(hy, moved["y"]) and np.array_equal(hi, moved["id"])
                                and np.array_equal(hc, moved["conc"]))
        r["host_over_device_ratio"] = r["host_route"]["total_ms"] / r["device"]["total_wall_ms"]
        print(json.dumps(r), flush=True)
        res["counts"].append(r)
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "drifters.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    return res


def design_table(r):
    rows = [f"Mesh {r['mesh']}: {r['num_elements']} triangles, {r['num_nodes']} nodes; equally spaced drifters over its bounding box; `conc_lim` {r['conc_lim']}; medians of "
            f"{r['samples']} warm repetitions on {r.get('conditions', {}).get('device', 'one GPU')}; device times from HIP events on the handle's stream, wall times around the calls with a synchronisation.", "",
            "| quantity | " + " | ".join(f"{c['num_drifters']} drifters" for c in r["counts"]) + " |", "|---|" + "---|" * len(r["counts"])]

    def line(name, fn):
        rows.append(f"| {name} | " + " | ".join(fn(c) for c in r["counts"]) + " |")
    line("`move`: kernel", lambda c: f"{c['device']['move_us']:.0f} µs")
    line("`conc`: kernel", lambda c: f"{c['device']['conc_us']:.0f} µs")
    line("`mask`: flags, scan, scatter, count read back", lambda c: f"{c['device']['mask_us']:.0f} µs")
    line("rebuild of the displaced locator (after a step or `put_state`)", lambda c: f"{c['device']['rebuild_us']:.0f} µs")
    line("wall: `move` + `M_UT = 0`", lambda c: f"{c['device']['move_ms']:.2f} ms")
    line("wall: `conc` + `mask`, locator current", lambda c: f"{c['device']['conc_mask_ms']:.2f} ms")
    line("wall: `conc` + `mask`, locator rebuilt first", lambda c: f"{c['device']['conc_mask_rebuild_ms']:.2f} ms")
    line("wall: the device route (`move`, rebuild, `conc`, `mask`)", lambda c: f"{c['device']['total_wall_ms']:.2f} ms")
    line("wall: the route without it", lambda c: f"{c['host_route']['total_ms']:.1f} ms = {c['host_route']['get_state_ms']:.1f} (`get_state`) + {c['host_route']['move_interp_ms']:.1f} "
         f"(interleave, locator, `interp_nodes`) + {c['host_route']['conc_interp_ms']:.1f} (displaced locator, `interp_nodes`) + {c['host_route']['mask_ms']:.1f} (numpy mask) + "
         f"{c['host_route']['put_state_ms']:.1f} (`put_state`, zeroed `UT`)")
    line("ratio of the two wall times", lambda c: f"{c['host_over_device_ratio']:.1f} x")
    line("both routes leave the same drifters, bit for bit", lambda c: "yes" if c["same_result"] else "NO")
    return "\n".join(rows)


def write_design(r):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no drifters-measurement markers")
    text = re.sub(re.escape(BEGIN) + r".*?" + re.escape(END), lambda _: BEGIN + "\n" + design_table(r) + "\n" + END, text, flags=re.S)
    open(path, "w").write(text)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--from-json":
        r = json.load(open(args[1]))
        with open(os.path.join(ROOT, "profiles", "drifters.json"), "w") as fh:
            json.dump(r, fh, indent=1)
        write_design(r)
    else:
        out = os.path.join(ROOT, "profiles")
        if "--out" in args:
            i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
        r = measure(args[0] if args else "2km", out)
        if os.path.abspath(out) == os.path.join(ROOT, "profiles"):
            write_design(r)
