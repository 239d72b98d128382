"""Cost of the device-resident Moorings means (nxs_dyn_means_update) at 2 km, against the only route without them: nxs_dyn_ice_diagnostics to the host,
nxs_dyn_get_state / nxs_dyn_get_diag of the members the variables need, numpy sums.

    python scripts/time_means.py [mesh] [--out DIR]      measure on the GPU, write DIR/means_accumulate.json (default profiles/) and DESIGN.md's table
    python scripts/time_means.py --from-json FILE        no GPU: copy FILE to profiles/means_accumulate.json and rewrite DESIGN.md's table from it
    python scripts/time_means.py --thermo [mesh] [--out DIR]   the thermodynamic variables: DIR/means_thermo.json (see measure_thermo); --old-only: its first part

Workload: ten elemental variables + VT_x, VT_y, taux, tauy.  Reported: device time of means_update from HIP events (option "means_timing"), warm, median
of 25, for both read-modify-write patterns (option "means_stage"); its share of the step; the bytes it has to move (every distinct source field once +
the rows read and written) and the GB/s that makes; the GB/s of a plain device-to-device copy of 1 GiB in the same run (bytes read + bytes written, the
same accounting); the host route's wall time.
"""
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ELEMENTAL = ("conc", "thick", "snow", "damage", "ridge_ratio", "conc_young", "sigma_n", "sigma_s", "divergence", "ice_mask")
NODAL = ("VT_x", "VT_y", "taux", "tauy")
BEGIN, END = "<!-- means-measurement:begin (written by scripts/time_means.py) -->", "<!-- means-measurement:end -->"


def model_bytes(Nn, Neo, Ne, W1):
    """what k_means_elements / k_means_nodes load and store for the lists above (nextsim_amd/csrc/nxs_dyn_kernels.inl), each array entry once"""
    # elements: conc, thick, snow, ridge, conc_young, h_young, hs_young (8 B each); sigma + damage: one 32-byte record (or 3 + 1 arrays: the same 32 B); divergence: three node ids
    # of the element + x0, y0, M_UM (2), M_VT (2) of every node
    el_src = Neo * (7 * 8 + 32 + 12) + Nn * 6 * 8
    el_rows = Neo * len(ELEMENTAL) * 16
    # nodes: M_VT, M_wind, D_tau_w (16 B each), the node's row of NodalElementConnectivity (4 W1), D_tau_ow, M_surface, M_conc of every element
    nod_src = Nn * (3 * 16 + 4 * W1) + Ne * 3 * 8
    nod_rows = Nn * len(NODAL) * 16
    return {"elemental_source_bytes": el_src, "elemental_row_bytes": el_rows, "nodal_source_bytes": nod_src, "nodal_row_bytes": nod_rows,
            "total_bytes": el_src + el_rows + nod_src + nod_rows}


def measure(kind, out_dir):
    import numpy as np
    import torch
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Nn, Ne = lm.num_nodes, lm.num_elements
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    tau_ow = np.full(Ne, 1.3e-3)
    fe.means_set_tau_ow(tau_ow)
    fe.means_configure(ELEMENTAL, NODAL)
    for _ in range(3):
        fe.step()
    fe.synchronize()
    fe.set_option("timing_reset", 1)
    for _ in range(10):
        fe.step()
    fe.synchronize()
    step = fe.timing()
    traffic = fe.traffic_model()
    fe.set_option("means_timing", 1)
    res = {"mesh": kind, "num_nodes": Nn, "num_elements": Ne, "elemental": ELEMENTAL, "nodal": NODAL, "step_total_ms": step["total_ms"],
           "step_update_ms": step["update_ms"], "k_update_model_bytes": traffic["update_bytes"], "substep_kernel": traffic["substep_kernel_name"]}
    if step["update_ms"] > 0:
        res["k_update_GBps"] = traffic["update_bytes"] / (step["update_ms"] * 1e-3) / 1e9
    nec, _ = dynamics.mesh_connectivity(lm.indices, Nn)
    mb = model_bytes(Nn, lm.local_nelements, Ne, nec.shape[1])
    res["model"] = mb
    for stage in (1, 0):
        fe.set_option("means_stage", stage)
        for _ in range(3):
            fe.means_update(0.01)
        t = []
        for _ in range(25):
            fe.means_update(0.01)
            t.append(fe.debug_array("means_update_ms"))
        t = np.array(t) * 1e3
        el, nod, tot = (float(np.median(v)) for v in (t[:, 0], t[:, 1], t.sum(1)))
        res["stage" if stage else "direct"] = {
            "elemental_us": el, "nodal_us": nod, "total_us": tot, "samples": len(t),
            "elemental_GBps": (mb["elemental_source_bytes"] + mb["elemental_row_bytes"]) / (el * 1e-6) / 1e9,
            "nodal_GBps": (mb["nodal_source_bytes"] + mb["nodal_row_bytes"]) / (nod * 1e-6) / 1e9,
            "total_GBps": mb["total_bytes"] / (tot * 1e-6) / 1e9, "share_of_step": tot * 1e-3 / step["total_ms"]}
        print(("LDS-staged" if stage else "direct"), res["stage" if stage else "direct"], flush=True)
    fe.set_option("means_stage", 1)
    fe.set_option("means_timing", 0)
    # a plain device-to-device copy of 1 GiB, bytes read + bytes written
    a = torch.empty(2 ** 27, dtype=torch.float64, device="cuda").fill_(1.0); b = torch.empty_like(a)
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    res["d2d_copy_bytes"] = int(a.numel() * 8)
    res["d2d_copy_GBps"] = 2 * a.numel() * 8 / (float(np.median(ts[2:])) * 1e-3) / 1e9
    del a, b
    # the route without the feature: diagnostics and state to the host, numpy sums (one array per variable, as the reference's data_mesh)
    acc_el = {k: np.zeros(Ne) for k in ELEMENTAL}; acc_nod = {k: np.zeros(Nn) for k in NODAL}
    host = {k: np.empty(Ne) for k in ("conc", "thick", "damage", "ridge_ratio", "conc_young", "h_young")}
    host["VT"] = np.empty(2 * Nn)
    s = _abi.State()
    for k, v in host.items():
        setattr(s, k, _abi.dptr(v))
    cols = []
    for j in range(nec.shape[1]):                 # the gather's index lists, built once (not timed)
        ok = ~np.isnan(nec[:, j]); e = np.where(ok, nec[:, j], 1.).astype(np.int64) - 1
        ok &= e >= 0
        cols.append((np.flatnonzero(ok), e[ok]))
    wind = f["wind"]; tf = 0.01
    walls = []
    for _ in range(7):
        fe.synchronize()
        t0 = time.perf_counter()
        ice, _ = fe.updateIceDiagnostics()
        assert fe.L.nxs_dyn_get_state(fe.h, C.byref(s)) == 0
        dg = fe.get_diag()
        t1 = time.perf_counter()
        for k, src in (("conc", ice["D_conc"]), ("thick", ice["D_thick"]), ("snow", ice["D_snow_thick"]), ("damage", host["damage"]), ("ridge_ratio", host["ridge_ratio"]),
                       ("conc_young", host["conc_young"]), ("sigma_n", ice["D_sigma0"]), ("sigma_s", ice["D_sigma1"]), ("divergence", ice["D_divergence"])):
            acc_el[k] += src * tf
        acc_el["ice_mask"] += np.where(host["thick"] + host["h_young"] > 0., 1., 0.)
        acc_nod["VT_x"] += host["VT"][:Nn] * tf; acc_nod["VT_y"] += host["VT"][Nn:] * tf
        ta = np.zeros(Nn); cc = np.zeros(Nn); ss = np.zeros(Nn)
        for idx, e in cols:
            a_ = dg["surface"][e]
            ta[idx] += tau_ow[e] * a_; cc[idx] += host["conc"][e] * a_; ss[idx] += a_
        ta /= ss; cc /= ss
        w2 = np.hypot(wind[:Nn], wind[Nn:])
        acc_nod["taux"] += (dg["D_tau_w"][:Nn] * cc + ta * (w2 * wind[:Nn]) * (1. - cc)) * tf
        acc_nod["tauy"] += (dg["D_tau_w"][Nn:] * cc + ta * (w2 * wind[Nn:]) * (1. - cc)) * tf
        t2 = time.perf_counter()
        walls.append((t1 - t0, t2 - t1))
    w = np.array(walls[2:]) * 1e3
    res["host_route"] = {"transfer_ms": float(np.median(w[:, 0])), "numpy_ms": float(np.median(w[:, 1])), "total_ms": float(np.median(w.sum(1))), "samples": len(w)}
    best = min(res["stage"]["total_us"], res["direct"]["total_us"])
    res["host_over_device_ratio"] = res["host_route"]["total_ms"] * 1e3 / res["stage"]["total_us"]
    res["fraction_of_copy_bandwidth"] = res["stage"]["total_GBps"] / res["d2d_copy_GBps"]
    res["faster_pattern"] = "stage" if best == res["stage"]["total_us"] else "direct"
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "means_accumulate.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res), flush=True)
    return res


# the 24-variable thermodynamic list: 19 rows of the slab (five of them negated), four of its state, tsurf -- what a time-mean Moorings file with the heat and
# fresh-water budget asks for
THERMO = ("Qa", "Qsw", "Qlw", "Qsh", "Qlh", "Qo", "delS", "evap", "rain", "sialb", "albedo", "vice_melt", "del_hi", "newice", "snow2ice", "mlt_top", "mlt_bot",
          "fwflux_ice", "fwflux", "QNoSw", "QSwOcean", "saltflux", "sst", "tsurf")
THERMO_SLAB_ROWS = ("Qa", "Qsw", "Qlw", "Qsh", "Qlh", "Qo", "delS", "evap", "rain", "sialb", "albedo", "vice_melt", "del_hi", "newice", "snow2ice", "mlt_top", "mlt_bot",
                    "fwflux_ice", "fwflux", "Qnosun", "Qsw_ocean", "brine")                    # the same rows under the names of nxs_dyn_slab_get
THERMO_FLUX_ROWS = ("sst", "tice0", "tsurf_young")                                              # ... and of nxs_dyn_flux_get (tsurf's sources beside conc, conc_young)


def _timed_updates(fe, np, n=25):
    """the elemental launch of n warm means_update calls [us]: median, smallest, largest -- the spread a comparison of two builds has to exceed"""
    for _ in range(3):
        fe.means_update(0.01)
    t = []
    for _ in range(n):
        fe.means_update(0.01)
        t.append(fe.debug_array("means_update_ms")[0])
    t = np.array(t) * 1e3
    return {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()), "samples": n}


def measure_thermo(kind, out_dir, old_only=False):
    """Two figures of the same run on the mesh `kind`, the designed thermodynamic inputs of tests/slab_ref.py, WINTON, the young-ice category:
    nxs_dyn_means_update with the 24-variable list THERMO (device time of the elemental launch, HIP events), and what a host pays for the same variables
    without it: nxs_dyn_slab_get / nxs_dyn_flux_get of those rows into host memory (wall time, the copies alone: the sums come on top).
    Before them the twenty ids the handle always had (_abi.MEANS_ELEMENTAL), a list that launches the kernel it always launched: with --old-only the script stops
    there, which is the part an earlier build of the library can run too -- the figure to hold against this one's, with the spread printed."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import column_ref as CR
    import fluxes_ref as FR
    import slab_ref as R
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Ne = lm.num_elements
    tri = lm.indices.reshape(-1, 3).astype(np.int64) - 1
    inp, _, _ = R.make_inputs(lm.coord_x, lm.coord_y, tri)
    inp = R.sane_inputs(inp, f)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    fe, f = R.gpu_handle(p, lm, f, inp, finp, CR.default_config(thermo_type="winton"), R.default_config(), put=R.SLAB_STATE)
    fe.fluxes(); fe.column(R.DT); fe.slab(R.DT, R.clock()); fe.step()
    fe.synchronize()
    fe.set_option("means_timing", 1)
    res = {"mesh": kind, "num_elements": int(Ne), "device": dynamics.device_name(0)}
    fe.means_configure(_abi.MEANS_ELEMENTAL)
    res["old_20_variables"] = _timed_updates(fe, np)
    print("old 20-variable list", res["old_20_variables"], flush=True)
    if not old_only:
        fe.means_configure(THERMO)
        res["thermo_24_variables"] = dict(_timed_updates(fe, np), variables=THERMO)
        # sources: 22 slab rows + sst, tice0, tsurf_young, conc, conc_young once each, 8 B; the rows read and written, 16 B per column
        nbytes = lm.local_nelements * ((len(THERMO_SLAB_ROWS) + 5) * 8 + len(THERMO) * 16)
        res["thermo_24_variables"]["model_bytes"] = int(nbytes)
        res["thermo_24_variables"]["GBps"] = nbytes / (res["thermo_24_variables"]["median_us"] * 1e-6) / 1e9
        print("thermo 24-variable list", res["thermo_24_variables"], flush=True)
        walls = []
        for _ in range(7):
            fe.synchronize()
            t0 = time.perf_counter()
            fe.slab_rows(THERMO_SLAB_ROWS); fe.flux_get(THERMO_FLUX_ROWS)
            walls.append((time.perf_counter() - t0) * 1e3)
        w = np.array(walls[2:])
        res["host_fetch"] = {"median_ms": float(np.median(w)), "min_ms": float(w.min()), "max_ms": float(w.max()), "samples": len(w),
                             "rows": len(THERMO_SLAB_ROWS) + len(THERMO_FLUX_ROWS), "bytes": int(Ne * 8 * (len(THERMO_SLAB_ROWS) + len(THERMO_FLUX_ROWS)))}
        res["host_fetch_over_means_update"] = res["host_fetch"]["median_ms"] * 1e3 / res["thermo_24_variables"]["median_us"]
        print("host fetch of the same rows", res["host_fetch"], flush=True)
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "means_thermo_old_only.json" if old_only else "means_thermo.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res), flush=True)
    return res


def design_table(r):
    s, d, h = r["stage"], r["direct"], r["host_route"]
    rows = [
        "| quantity | value |", "|---|---|",
        f"| mesh | {r['mesh']}: {r['num_elements']} triangles, {r['num_nodes']} nodes; {len(r['elemental'])} elemental + {len(r['nodal'])} nodal variables |",
        f"| `means_update`, rows staged through LDS (default) | {s['total_us']:.1f} µs = {s['elemental_us']:.1f} (elements) + {s['nodal_us']:.1f} (nodes); median of {s['samples']} |",
        f"| `means_update`, every thread walks its own row (`means_stage` 0) | {d['total_us']:.1f} µs = {d['elemental_us']:.1f} + {d['nodal_us']:.1f} |",
        f"| share of the step (`total_ms` {r['step_total_ms']:.3f}) | {100 * s['share_of_step']:.2f} % |",
        f"| bytes it must move | {r['model']['total_bytes'] / 1e6:.1f} MB (sources {(r['model']['elemental_source_bytes'] + r['model']['nodal_source_bytes']) / 1e6:.1f}, rows read + written {(r['model']['elemental_row_bytes'] + r['model']['nodal_row_bytes']) / 1e6:.1f}) |",
        f"| resulting rate | {s['total_GBps']:.0f} GB/s (elements {s['elemental_GBps']:.0f}, nodes {s['nodal_GBps']:.0f}); direct rows: {d['total_GBps']:.0f} GB/s |",
        f"| device-to-device copy of {r['d2d_copy_bytes'] / 2 ** 30:.0f} GiB, same run | {r['d2d_copy_GBps']:.0f} GB/s (read + written) -> `means_update` reaches {100 * r['fraction_of_copy_bandwidth']:.0f} % of it |",
    ]
    if "k_update_GBps" in r:
        rows.append(f"| `k_update` in the same run, for scale | {r['k_update_GBps']:.0f} GB/s of its model bytes |")
    rows += [
        f"| the route without the feature (diagnostics + state to the host, numpy sums) | {h['total_ms']:.1f} ms = {h['transfer_ms']:.1f} (copies) + {h['numpy_ms']:.1f} (sums) |",
        f"| ratio host route / `means_update` | {r['host_over_device_ratio']:.0f} x |",
    ]
    return "\n".join(rows)


def write_design(r):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    if BEGIN not in text or END not in text:
        raise SystemExit("DESIGN.md has no means-measurement markers")
    text = re.sub(re.escape(BEGIN) + r".*?" + re.escape(END), lambda _: BEGIN + "\n" + design_table(r) + "\n" + END, text, flags=re.S)
    open(path, "w").write(text)


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--from-json":
        r = json.load(open(args[1]))
        with open(os.path.join(ROOT, "profiles", "means_accumulate.json"), "w") as fh:
            json.dump(r, fh, indent=1)
        write_design(r)
    else:
        out = os.path.join(ROOT, "profiles")
        if "--out" in args:
            i = args.index("--out"); out = args[i + 1]; del args[i:i + 2]
        if "--thermo" in args:
            args.remove("--thermo")
            old_only = "--old-only" in args
            if old_only:
                args.remove("--old-only")
            measure_thermo(args[0] if args else "2km", out, old_only)
            sys.exit(0)
        r = measure(args[0] if args else "2km", out)
        if os.path.abspath(out) == os.path.join(ROOT, "profiles"):
            write_design(r)
