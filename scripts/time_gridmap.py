"""Cost of the conservative remapping between the mesh and a coupling grid on the device (nxs_gridmap_*, nxs_dyn_means_to_grid_conservative) at 2 km:
a polar-stereographic grid of 12.5 km cells over the mesh.

    python scripts/time_gridmap.py [mesh] [--out DIR]     measure on the GPU, write DIR/gridmap.json (default profiles/) and DESIGN.md's table
    python scripts/time_gridmap.py --from-json FILE       no GPU: copy FILE to profiles/gridmap.json and rewrite DESIGN.md's table from it

Reported, each a median of REPS >= 5 wall-clock samples with its smallest and largest: the weights build on the device (context given); the same core
compiled for the host on one core (tests/native/gridmap_host.cpp: a RESTATEMENT -- the real routine has no door on the GPU machine -- fed with the
seeds the device found, its time includes reading its input file and both applications); mesh_to_grid and grid_to_mesh of 10 variables from device rows
to device rows, with the bytes they must move (12 B per entry plus rows and grid) and the rate that makes beside a device-to-device copy of the same run;
nxs_dyn_means_to_grid_conservative; and the route it replaces: nxs_dyn_means_get of [Ne][10] to the host plus a vectorised numpy application.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
ELEMENTAL = ("conc", "thick", "snow", "damage", "ridge_ratio", "conc_young", "sigma_n", "sigma_s", "divergence", "ice_mask")
BEGIN, END = "<!-- gridmap-measurement:begin (written by scripts/time_gridmap.py) -->", "<!-- gridmap-measurement:end -->"
REPS = 9
CELL = 12500.


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
    import grid_remap_ref as R
    import make_grid_remap_golden as MG
    from nextsim_amd import dynamics, forcing as F, interp, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Ne = lm.num_elements
    x, y = lm.coord_x, lm.coord_y
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3) - 1, np.int32)
    n = int(np.ceil(max(np.ptp(x), np.ptp(y)) / CELL))
    gx, gy, cx, cy = MG.grid(n, n, CELL, 0., 0., 0., origin=(x.min(), y.min()))
    G = gx.size
    L = dynamics.load_library()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipFree.argtypes = [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    rg = interp.Regrid(lm.indices, x, y)
    maps = []

    def build():
        while maps:
            maps.pop().close()
        maps.append(interp.GridMap.weights(rg, gx, gy, cx, cy))
    res = {"mesh": kind, "num_elements": Ne, "grid": f"{n} x {n} cells of {CELL:.0f} m", "grid_size": G, "reps": REPS}
    res["weights_device"] = timed(build, reps=5, warm=1)
    gmap = maps[0]
    info = gmap.info()
    res["info"] = info
    res["chunks"] = interp.gridmap_debug_chunk(0)
    e = gmap.export()

    # ---- the same core on one host core (a restatement), seeds from the device's rows: the seed is the first entry of a row
    seed = np.full(G, -1, np.int32); seed[e["gridP"]] = e["tris"][e["off"][:-1]]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gridmap_host")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                               os.path.join(ROOT, "tests", "native", "gridmap_host.cpp"), "-o", exe])
        host = R.run_host(exe, tmp, x, y, tri, gx, gy, cx.ravel(), cy.ravel(), np.ones((Ne, 1)), np.ones((G, 1)), seed=seed)
    res["weights_host_one_core_restatement"] = {"ms": host["program_ms"], "n": 1, "same_lists_as_device": bool(
        np.array_equal(host["gridP"], e["gridP"]) and np.array_equal(host["tris"], e["tris"]) and np.array_equal(host["w"].view(np.uint64), e["w"].view(np.uint64)))}

    # ---- the two applications, 10 variables, device rows to device rows
    nv = len(ELEMENTAL)
    rng = np.random.default_rng(0)
    rows, cells = rng.random((Ne, nv)), rng.random((G, nv))
    d = [C.c_void_p() for _ in range(4)]
    for ptr, nbytes in zip(d, (rows.nbytes, G * nv * 8, cells.nbytes, rows.nbytes)):
        assert L.hipMalloc(C.byref(ptr), nbytes) == 0
    assert L.hipMemcpy(d[0], rows.ctypes.data, rows.nbytes, 1) == 0 and L.hipMemcpy(d[2], cells.ctypes.data, cells.nbytes, 1) == 0
    m2g = timed(lambda: gmap.mesh_to_grid(None, 0., in_device=(d[0].value, nv), out_device=d[1].value))
    g2m = timed(lambda: gmap.grid_to_mesh(None, in_device=(d[2].value, nv), out_device=d[3].value))
    touched = int(np.unique(e["tris"]).size)
    m2g["bytes"] = 12 * info["entries"] + touched * nv * 8 + G * nv * 8 + info["wet"] * 20
    g2m["bytes"] = 16 * info["entries"] + info["wet"] * nv * 8 + Ne * nv * 8 + Ne * 4
    for r in (m2g, g2m):
        r["GBps"] = r["bytes"] / (r["median_ms"] * 1e-3) / 1e9
    res["mesh_to_grid_10_vars_device_rows"], res["grid_to_mesh_10_vars_device_rows"] = m2g, g2m
    copy = timed(lambda: (L.hipMemcpy(d[3], d[0], rows.nbytes, 3), L.hipDeviceSynchronize()))
    copy["bytes"] = 2 * rows.nbytes
    copy["GBps"] = copy["bytes"] / (copy["median_ms"] * 1e-3) / 1e9
    res["device_copy_same_run"] = copy
    for ptr in d:
        L.hipFree(ptr)

    # ---- the handle's call and the route it replaces
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.means_configure(ELEMENTAL, ())
    fe.step(); fe.means_update(1.); fe.synchronize()
    grid = np.zeros((nv, G))
    res["means_to_grid_conservative"] = timed(lambda: fe.means_to_grid_conservative(gmap, -1e14, grid))
    tr, w, off, gp = e["tris"], e["w"], e["off"], e["gridP"]
    r_area = 1. / np.abs(0.5 * ((cx[gp] * np.roll(cy[gp], -1, 1)).sum(1) - (cy[gp] * np.roll(cx[gp], -1, 1)).sum(1)))

    def host_route():
        el = fe.means_get()[0]
        out = np.zeros((G, nv))
        out[gp] = np.add.reduceat(el[tr] * w[:, None], off[:-1], axis=0) * r_area[:, None]
        grid2 = out.T.copy()
        return grid2
    res["replaced_route_means_get_plus_numpy_application"] = timed(host_route, reps=5, warm=1)
    fe.close(); gmap.close(); rg.close()
    res["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "gridmap.json"), "w"), indent=1)
    return res


def table(res):
    def row(name, r, extra=""):
        return f"| {name} | {r['median_ms']:.3f} | {r['min_ms']:.3f} – {r['max_ms']:.3f} | {r['n']} | {extra} |"
    i = res["info"]
    m, gq, cp = res["mesh_to_grid_10_vars_device_rows"], res["grid_to_mesh_10_vars_device_rows"], res["device_copy_same_run"]
    h = res["weights_host_one_core_restatement"]
    lines = [BEGIN,
             f"Measured {res['date']} on one MI355X, `{res['mesh']}` mesh ({res['num_elements']} triangles), {res['grid']} ({res['grid_size']} cells: {i['wet']} wet, "
             f"{i['entries']} entries, longest row {i['longest']}, {i['failed']} failed, {res['chunks']} chunks).  Wall-clock milliseconds around the synchronous calls.",
             "",
             "| what | median ms | min – max | samples | note |", "|---|---|---|---|---|",
             row("`nxs_gridmap_create` (context given)", res["weights_device"]),
             f"| the same core on one host core (a restatement, input file and both applications included) | {h['ms']:.0f} | | 1 | same lists as the device: {h['same_lists_as_device']} |",
             row("`nxs_gridmap_mesh_to_grid`, 10 variables, device rows", m, f"{m['bytes'] / 1e6:.1f} MB to move: {m['GBps']:.1f} GB/s"),
             row("`nxs_gridmap_grid_to_mesh`, 10 variables, device rows", gq, f"{gq['bytes'] / 1e6:.1f} MB to move: {gq['GBps']:.1f} GB/s"),
             row("device-to-device copy of the rows, same run", cp, f"{cp['bytes'] / 1e6:.1f} MB: {cp['GBps']:.1f} GB/s"),
             row("`nxs_dyn_means_to_grid_conservative` (grids on the host)", res["means_to_grid_conservative"]),
             row("replaced route: `nxs_dyn_means_get` of [Ne][10] + numpy application", res["replaced_route_means_get_plus_numpy_application"]),
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
        json.dump(res, open(os.path.join(ROOT, "profiles", "gridmap.json"), "w"), indent=1)
    else:
        out_dir = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles")
        kind = next((a for a in args if not a.startswith("--") and (args.index(a) == 0 or args[args.index(a) - 1] != "--out")), "2km")
        res = measure(kind, out_dir)
    write_design(res)
    print(table(res))
