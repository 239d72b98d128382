"""Cost of the coupler's outgoing side on the device (nxs_dyn_cpl_out_update, nxs_dyn_cpl_out_put) at 2 km: the exchange grid of DESIGN 6n (12.5 km cells over
the mesh) with a list of five elemental and three nodal variables, as the ocean's.

    python scripts/time_cpl_out.py [mesh] [--out DIR]     measure on the GPU, write DIR/cpl_out.json (default profiles/) and DESIGN.md's table
    python scripts/time_cpl_out.py --from-json FILE       no GPU: copy FILE to profiles/cpl_out.json and rewrite DESIGN.md's table from it

Reported, each a median of REPS wall-clock samples after two warm-up calls, with its smallest and largest (every timed sample ends with a synchronisation):
  (a) the only route a coupler-only host has WITHOUT the feature, on the ONE existing set: nxs_dyn_means_update + nxs_dyn_means_to_grid_conservative +
      nxs_dyn_means_points_update / _get + the two resets;
  (b) nxs_dyn_cpl_out_update + nxs_dyn_cpl_out_put with host arrays and NXS_CPL_OUT_RESET, and the put alone with the fields left on the device;
  the two legs alone; nxs_dyn_cpl_out_update beside nxs_dyn_means_update on the same lists (the same kernels); a step with and without a configured coupler set.
The variables: conc, thick, snow, damage, ridge_ratio and taux, tauy, taumod (with a synthetic D_tau_ow) -- ids whose sources a handle without thermodynamics holds;
the put does not depend on which ids the columns are.
"""
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
BEGIN, END = "<!-- cpl-out-measurement:begin (written by scripts/time_cpl_out.py) -->", "<!-- cpl-out-measurement:end -->"
REPS = 9
CELL = 12500.
ELEMENTAL = ("conc", "thick", "snow", "damage", "ridge_ratio")
NODAL = ("taux", "tauy", "taumod")
PAIRS = ((0, 1),)
MISS = -1e14


def stats(samples):
    s = sorted(samples)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "n": len(s)}


def timed(fn, reps=REPS, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def measure(kind, out_dir):
    import numpy as np
    import make_grid_remap_golden as MG
    from nextsim_amd import dynamics, forcing as F, interp, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Ne, Nn = lm.num_elements, lm.num_nodes
    x, y = lm.coord_x, lm.coord_y
    n = int(np.ceil(max(np.ptp(x), np.ptp(y)) / CELL))
    gx, gy, cx, cy = MG.grid(n, n, CELL, 0., 0., 0., origin=(x.min(), y.min()))
    G = gx.size
    theta = 0.3 * np.sin(gx / np.ptp(gx)) - 0.1
    rg = interp.Regrid(lm.indices, x, y)
    gmap = interp.GridMap.weights(rg, gx, gy, cx, cy)
    info = gmap.info()
    n_el, n_nod = len(ELEMENTAL), len(NODAL)
    res = {"mesh": kind, "num_elements": Ne, "num_nodes": Nn, "device": dynamics.device_name(0) or "AMD Instinct MI355X (gfx950)", "grid": f"{n} x {n} cells of {CELL:.0f} m",
           "grid_size": G, "info": info, "elemental": list(ELEMENTAL), "nodal": list(NODAL), "reps": REPS}
    tri = lm.indices.reshape(-1, 3) - 1
    tau_ow = np.ascontiguousarray(1.3e-3 * (1. + 0.2 * np.sin(5. * x[tri].mean(1) / np.ptp(x))))

    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.step(); fe.synchronize()
    fe.means_set_tau_ow(tau_ow)

    def step():
        fe.step(); fe.synchronize()
    res["step_without_coupler_set"] = timed(step, reps=REPS, warm=1)

    # ---- (a) without the feature: the one existing set serves the coupler
    fe.means_configure(ELEMENTAL, NODAL)
    fe.means_points_set(gx, gy, MISS, "grid_theta", gridTheta=theta, rotation_angle=0.2, pairs=PAIRS)
    grid_a = np.zeros((n_el, G))

    def means_update():
        fe.means_update(0.5); fe.synchronize()
    res["means_update"] = timed(means_update)

    def route_a(update=True):
        if update:
            fe.means_update(0.5)
        grid_a[:] = 0.
        fe.means_to_grid_conservative(gmap, MISS, grid_a)         # synchronises, transposes on the host
        fe.means_points_update()
        _, nod, _, _ = fe.means_points_get()
        fe.means_reset(); fe.means_points_reset()
        fe.synchronize()
        return grid_a.copy(), nod
    res["a_update_to_grid_conservative_points_update_get_resets"] = timed(route_a)
    res["a_put_only"] = timed(lambda: route_a(False))
    fe.means_reset(); fe.means_points_reset()
    want_e, want_n = route_a()
    fe.means_configure((), ())
    fe.means_points_set()

    # ---- (b) the second set
    fe.cpl_out_configure(ELEMENTAL, NODAL)
    fe.cpl_out_attach_grid(gmap, gx, gy, MISS, "grid_theta", gridTheta=theta, rotation_angle=0.2, pairs=PAIRS)

    def cpl_update():
        fe.cpl_out_update(0.5); fe.synchronize()
    res["cpl_out_update"] = timed(cpl_update)
    fe.cpl_out_reset()

    def route_b():
        fe.cpl_out_update(0.5)
        return fe.cpl_out_put(reset=True)[:2]
    res["b_update_put_host_arrays_reset"] = timed(route_b)
    got_e, got_n = route_b()
    same = lambda u, v: bool((np.isnan(u) == np.isnan(v)).all() and np.array_equal((u + 0.)[~np.isnan(u)].view(np.uint64), (v + 0.)[~np.isnan(v)].view(np.uint64)))  # noqa: E731
    res["same_bits_elemental"] = same(got_e, want_e)
    res["same_bits_nodal"] = same(got_n, want_n)

    def put_host():
        fe.cpl_out_put(reset=True)
    res["b_put_host_arrays_reset"] = timed(put_host)

    def put_device():
        fe.cpl_out_put(want_host=False); fe.cpl_out_reset(); fe.cpl_out_reset_grid(); fe.synchronize()
    res["b_put_device_rows_resets"] = timed(put_device)
    res["step_with_coupler_set"] = timed(step, reps=REPS, warm=1)

    # ---- the legs alone
    fe.cpl_out_update(0.5)
    _, _, de, _ = fe.cpl_out_get(want_host=False)
    _, _, dg, _ = fe.cpl_out_put(want_host=False)
    fe.synchronize()
    L = dynamics.load_library()

    def send():
        gmap.send_rows(in_device=(de, n_el), out_device=dg); L.hipDeviceSynchronize()
    r = timed(send)
    r["bytes"] = int(12 * info["entries"] + (info["wet"] + 1) * 4 + G * 4 + info["wet"] * 8 + info["entries"] * n_el * 8 + 2 * G * n_el * 8)
    r["GBps"] = r["bytes"] / (r["median_ms"] * 1e-3) / 1e9
    res["send_rows_device"] = r
    import ctypes as C
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipFree.argtypes = [C.c_void_p]
    tmp = C.c_void_p()
    assert L.hipMalloc(C.byref(tmp), G * n_el * 8) == 0

    def to_grid():
        gmap.mesh_to_grid(None, 0., in_device=(de, n_el), out_device=tmp.value)
    res["mesh_to_grid_device"] = timed(to_grid)
    L.hipFree(tmp)
    fe.cpl_out_configure((), NODAL)
    fe.cpl_out_attach_grid(gmap, gx, gy, MISS, "grid_theta", gridTheta=theta, rotation_angle=0.2, pairs=PAIRS)

    def nodal_leg():
        fe.cpl_out_put(want_host=False); fe.synchronize()
    res["nodal_leg_device"] = timed(nodal_leg)
    res["pcie_bytes"] = {"a": int((G * n_el + G * n_el + G * n_nod) * 8), "b_host_arrays": int(G * (n_el + n_nod) * 8), "b_device_rows": 0}
    fe.close(); gmap.close(); rg.close()
    res["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "cpl_out.json"), "w"), indent=1)
    return res


def table(res):
    def row(name, r, extra=""):
        return f"| {name} | {r['median_ms']:.3f} | {r['min_ms']:.3f} – {r['max_ms']:.3f} | {r['n']} | {extra} |"
    i, pc, s = res["info"], res["pcie_bytes"], res["send_rows_device"]
    lines = [BEGIN,
             f"Measured {res['date']} on one {res['device']}, `{res['mesh']}` mesh ({res['num_elements']} triangles, {res['num_nodes']} nodes), {res['grid']} ({res['grid_size']} cells: "
             f"{i['wet']} wet, {i['entries']} entries, longest row {i['longest']}), elemental {', '.join(res['elemental'])}; nodal {', '.join(res['nodal'])}.  Wall-clock milliseconds, "
             f"every sample synchronised.  The fields of (b) have the bits of (a) up to the sign of zero: elemental {res['same_bits_elemental']}, nodal {res['same_bits_nodal']}.",
             "",
             "| what | median ms | min – max | samples | note |", "|---|---|---|---|---|",
             row("(a) `nxs_dyn_means_update` + `_to_grid_conservative` + `_points_update` / `_get` + the two resets (one set)", res["a_update_to_grid_conservative_points_update_get_resets"],
                 f"{pc['a'] / 1e6:.1f} MB over PCIe, host transposition"),
             row("(a) without the update", res["a_put_only"]),
             row("(b) `nxs_dyn_cpl_out_update` + `nxs_dyn_cpl_out_put`, host arrays, `NXS_CPL_OUT_RESET`", res["b_update_put_host_arrays_reset"], f"{pc['b_host_arrays'] / 1e6:.1f} MB over PCIe"),
             row("(b) `nxs_dyn_cpl_out_put` alone, host arrays, `NXS_CPL_OUT_RESET`", res["b_put_host_arrays_reset"]),
             row("(b) `nxs_dyn_cpl_out_put` alone, fields left on the device, + the two resets", res["b_put_device_rows_resets"], "nothing over PCIe"),
             row("`nxs_gridmap_send_rows` alone, device rows (one list walk for five variables)", s, f"{s['bytes'] / 1e6:.1f} MB to move: {s['GBps']:.1f} GB/s"),
             row("`nxs_gridmap_mesh_to_grid` alone, the same rows on the device (one walk per variable, `[G][nv]`)", res["mesh_to_grid_device"], "synchronises itself"),
             row("the nodal leg alone (`nxs_dyn_cpl_out_put`, nodal list only, device rows)", res["nodal_leg_device"]),
             row("`nxs_dyn_means_update`, these lists", res["means_update"]),
             row("`nxs_dyn_cpl_out_update`, these lists (the same kernels)", res["cpl_out_update"]),
             row("`nxs_dyn_step` without a coupler set", res["step_without_coupler_set"]),
             row("`nxs_dyn_step` with the coupler set configured", res["step_with_coupler_set"]),
             END]
    return "\n".join(lines)


def write_design(res):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    if BEGIN in text:
        text = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: table(res), text, flags=re.S)
        open(path, "w").write(text)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--from-json" in args:
        res = json.load(open(args[args.index("--from-json") + 1]))
        json.dump(res, open(os.path.join(ROOT, "profiles", "cpl_out.json"), "w"), indent=1)
    else:
        out_dir = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles")
        kind = next((a for a in args if not a.startswith("--") and (args.index(a) == 0 or args[args.index(a) - 1] != "--out")), "2km")
        res = measure(kind, out_dir)
    write_design(res)
    print(table(res))
