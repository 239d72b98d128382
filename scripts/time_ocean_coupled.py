"""Cost of a coupled ocean's receive on the device (nxs_dyn_ocean_coupled_receive, nxs_gridmap_receive_rows) at 2 km: a NEMO-like exchange grid of 12.5 km
cells over the mesh, the three fields of the reference's default receive (I_SST, I_SSS, I_FrcQsr).

    python scripts/time_ocean_coupled.py [mesh] [--out DIR]     measure on the GPU, write DIR/ocean_coupled.json (default profiles/) and DESIGN.md's table
    python scripts/time_ocean_coupled.py --from-json FILE       no GPU: copy FILE to profiles/ocean_coupled.json and rewrite DESIGN.md's table from it

Reported, each a median of REPS wall-clock samples after two warm-up calls, with its smallest and largest (every timed call ends with a synchronisation):
  (a) the route a host has WITHOUT the feature: transform and interleave in numpy, nxs_gridmap_grid_to_mesh with host arrays, de-interleave,
      nxs_dyn_column_set_forcing (two of the three rows have a row there; qsrml had none);
  (b) nxs_dyn_ocean_coupled_receive from host fields and from device fields;
  the kernel alone (nxs_gridmap_receive_rows, device fields to device rows) reading the lists through the index list and through copies in transposed order,
  with the bytes each must move and the rate that makes, beside a device-to-device copy of the same run.
"""
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
BEGIN, END = "<!-- ocean-coupled-measurement:begin (written by scripts/time_ocean_coupled.py) -->", "<!-- ocean-coupled-measurement:end -->"
REPS = 9
CELL = 12500.
ROWS = ("ocean_temp", "ocean_salt", "qsrml")


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
    Ne = lm.num_elements
    x, y = lm.coord_x, lm.coord_y
    n = int(np.ceil(max(np.ptp(x), np.ptp(y)) / CELL))
    gx, gy, cx, cy = MG.grid(n, n, CELL, 0., 0., 0., origin=(x.min(), y.min()))
    G = gx.size
    L = dynamics.load_library()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipFree.argtypes = [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    rg = interp.Regrid(lm.indices, x, y)
    gmap = interp.GridMap.weights(rg, gx, gy, cx, cy)
    info = gmap.info()
    nv = len(ROWS)
    res = {"mesh": kind, "num_elements": Ne, "device": dynamics.device_name(0) or "AMD Instinct MI355X (gfx950)", "grid": f"{n} x {n} cells of {CELL:.0f} m", "grid_size": G, "info": info,
           "fields": list(ROWS), "reps": REPS}
    rng = np.random.default_rng(0)
    fields = [np.ascontiguousarray(rng.random(G)) for _ in ROWS]
    a, b = np.ones(nv), np.zeros(nv)

    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)

    # ---- (a) without the feature: numpy transform + interleave, grid_to_mesh from host arrays, de-interleave, column_set_forcing
    def route_a():
        data = np.empty((G, nv))
        for v in range(nv):
            data[:, v] = fields[v] * a[v] + b[v]
        out = gmap.grid_to_mesh(data)
        rows = [np.ascontiguousarray(1. * out[:, v] + 0.) for v in range(nv)]
        fe.column_set_forcing(ocean_temp=rows[0], ocean_salt=rows[1])
        fe.synchronize()
        return rows
    res["a_numpy_grid_to_mesh_host_set_forcing"] = timed(route_a, reps=5, warm=1)
    rows_a = route_a()

    # ---- (b) the receive on the handle
    fe.ocean_coupled_attach(gmap, rows=ROWS)

    def host_fields():
        fe.ocean_coupled_receive(fields)
        fe.synchronize()
    res["b_receive_host_fields"] = timed(host_fields)
    d_in = [C.c_void_p() for _ in ROWS]
    for ptr, fld in zip(d_in, fields):
        assert L.hipMalloc(C.byref(ptr), fld.nbytes) == 0 and L.hipMemcpy(ptr, fld.ctypes.data, fld.nbytes, 1) == 0
    dev_ptrs = [ptr.value for ptr in d_in]

    def device_fields():
        fe.ocean_coupled_receive(dev_ptrs, device=True)
        fe.synchronize()
    res["b_receive_device_fields"] = timed(device_fields)
    got = fe.ocean_coupled_get(ROWS)
    same = lambda u, v: bool((np.isnan(u) == np.isnan(v)).all() and np.array_equal(u[~np.isnan(u)].view(np.uint64), v[~np.isnan(v)].view(np.uint64)))  # noqa: E731
    res["same_bits_as_route_a"] = all(same(got[k], rows_a[i]) for i, k in enumerate(ROWS))
    res["nan_elements"] = int(np.isnan(got["qsrml"]).sum())
    res["pcie_bytes"] = {"a_host_rows_up_and_down": int(G * nv * 8 + Ne * nv * 8 + 2 * Ne * 8), "b_host_fields": int(G * nv * 8), "b_device_fields": 0}

    # ---- the kernel alone, device fields to device rows, both ways of reading the lists
    d_out = [C.c_void_p() for _ in ROWS]
    for ptr in d_out:
        assert L.hipMalloc(C.byref(ptr), Ne * 8) == 0
    out_ptrs = [ptr.value for ptr in d_out]
    touched_cells = info["wet"]
    for mode, name, per_entry in ((0, "kernel_through_index_list", 16), (1, "kernel_through_transposed_copies", 12)):
        interp.gridmap_debug_receive_lists(mode)
        r = timed(lambda: gmap.receive_rows(dev_ptrs, in_device=True, out_device=out_ptrs))
        r["bytes"] = int(per_entry * info["entries"] + (Ne + 1) * 4 + touched_cells * nv * 8 + Ne * nv * 8)
        r["GBps"] = r["bytes"] / (r["median_ms"] * 1e-3) / 1e9
        res[name] = r
    interp.gridmap_debug_receive_lists(1)   # (the default)
    res["transposed_copies_extra_bytes"] = int(12 * info["entries"])
    g2m_in = C.c_void_p(); g2m_out = C.c_void_p()
    assert L.hipMalloc(C.byref(g2m_in), G * nv * 8) == 0 and L.hipMalloc(C.byref(g2m_out), Ne * nv * 8) == 0
    assert L.hipMemcpy(g2m_in, np.ascontiguousarray(np.stack(fields, axis=1)).ctypes.data, G * nv * 8, 1) == 0
    r = timed(lambda: gmap.grid_to_mesh(None, in_device=(g2m_in.value, nv), out_device=g2m_out.value))
    res["grid_to_mesh_same_variables_device_rows"] = r
    big = C.c_void_p()
    assert L.hipMalloc(C.byref(big), Ne * nv * 8) == 0
    copy = timed(lambda: (L.hipMemcpy(big, g2m_out, Ne * nv * 8, 3), L.hipDeviceSynchronize()))
    copy["bytes"] = 2 * Ne * nv * 8
    copy["GBps"] = copy["bytes"] / (copy["median_ms"] * 1e-3) / 1e9
    res["device_copy_same_run"] = copy
    for ptr in d_in + d_out + [g2m_in, g2m_out, big]:
        L.hipFree(ptr)
    fe.ocean_coupled_detach()
    fe.close(); gmap.close(); rg.close()
    res["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "ocean_coupled.json"), "w"), indent=1)
    return res


def table(res):
    def row(name, r, extra=""):
        return f"| {name} | {r['median_ms']:.3f} | {r['min_ms']:.3f} – {r['max_ms']:.3f} | {r['n']} | {extra} |"
    i, pc = res["info"], res["pcie_bytes"]
    k0, k1, cp = res["kernel_through_index_list"], res["kernel_through_transposed_copies"], res["device_copy_same_run"]
    lines = [BEGIN,
             f"Measured {res['date']} on one {res['device']}, `{res['mesh']}` mesh ({res['num_elements']} triangles), {res['grid']} ({res['grid_size']} cells: {i['wet']} wet, "
             f"{i['entries']} entries, longest row {i['longest']}), fields {', '.join(res['fields'])}; {res['nan_elements']} triangles no wet cell touches.  Wall-clock "
             f"milliseconds, every call synchronised.  Rows of (b) have the bits of (a): {res['same_bits_as_route_a']}.",
             "",
             "| what | median ms | min – max | samples | note |", "|---|---|---|---|---|",
             row("(a) numpy transform + interleave, `nxs_gridmap_grid_to_mesh` host arrays, de-interleave, `nxs_dyn_column_set_forcing`",
                 res["a_numpy_grid_to_mesh_host_set_forcing"], f"{pc['a_host_rows_up_and_down'] / 1e6:.1f} MB over PCIe"),
             row("(b) `nxs_dyn_ocean_coupled_receive`, host fields", res["b_receive_host_fields"], f"{pc['b_host_fields'] / 1e6:.1f} MB over PCIe"),
             row("(b) `nxs_dyn_ocean_coupled_receive`, device fields", res["b_receive_device_fields"], "nothing over PCIe"),
             row("`nxs_gridmap_receive_rows` alone, lists through the index list", k0, f"{k0['bytes'] / 1e6:.1f} MB to move: {k0['GBps']:.1f} GB/s"),
             row("`nxs_gridmap_receive_rows` alone, lists through transposed copies", k1,
                 f"{k1['bytes'] / 1e6:.1f} MB to move: {k1['GBps']:.1f} GB/s; {res['transposed_copies_extra_bytes'] / 1e6:.1f} MB more resident"),
             row("`nxs_gridmap_grid_to_mesh`, the same variables interleaved, device rows", res["grid_to_mesh_same_variables_device_rows"], "one list walk per variable"),
             row("device-to-device copy of the rows, same run", cp, f"{cp['bytes'] / 1e6:.1f} MB: {cp['GBps']:.1f} GB/s"),
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
        json.dump(res, open(os.path.join(ROOT, "profiles", "ocean_coupled.json"), "w"), indent=1)
    else:
        out_dir = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles")
        kind = next((a for a in args if not a.startswith("--") and (args.index(a) == 0 or args[args.index(a) - 1] != "--out")), "2km")
        res = measure(kind, out_dir)
    write_design(res)
    print(table(res))
