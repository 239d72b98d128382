"""Cost of the nodal half of a coupled run's receive on the device (nxs_nodemap_*, nxs_dyn_nodes_coupled_receive) at 2 km: a NEMO-like exchange grid of 12.5 km
points over the mesh, triangulated, the three fields of ocean_cpl_nodes (I_Uocn, I_Vocn, I_SSH) with the gridTheta rotation of the pair.

    python scripts/time_nodal_receive.py [mesh] [--out DIR]     measure on the GPU, write DIR/nodal_receive.json (default profiles/) and DESIGN.md's table
    python scripts/time_nodal_receive.py --from-json FILE       no GPU: copy FILE to profiles/nodal_receive.json and rewrite DESIGN.md's table from it
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_nodal_receive.py [mesh] --trace-loop 200
                                                                 nothing timed here: 200 receives (device fields to device rows) and 200 device-to-device copies of
                                                                 the three output rows, for the profiler's kernel statistics (the kernels' own times: DESIGN.md 6p)

Reported, each a median of REPS wall-clock samples after two warm-up calls, with its smallest and largest (every timed call ends with a synchronisation):
  (a) the route a host has WITHOUT the feature: a, b and the rotation in numpy, nxs_regrid_interp_nodes on a kept context (which locates every node again), then
      nxs_dyn_set_forcing_pair with the three half-rows in it;
  (b) nxs_dyn_nodes_coupled_receive from host fields and from device fields;
  nxs_nodemap_receive_rows alone, device fields to device rows (both kernels), the same with a one-target map on the same source (the source kernel and the launch
  overheads) -- wall clock, which a call of tens of microseconds does not resolve: the kernels' own times are the trace's --, a device-to-device copy of the output rows in the same run, nxs_nodemap_create once, and nxs_dyn_step with and without
  an attachment.
"""
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BEGIN, END = "<!-- nodal-receive-measurement:begin (written by scripts/time_nodal_receive.py) -->", "<!-- nodal-receive-measurement:end -->"
REPS = 9
CELL = 12500.
PI = 3.141592653589793


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


def exchange_grid(x, y, n):
    """n x n points over the box of the mesh, the four sides bulging outwards (a strictly convex boundary: no node of the mesh is beyond the hull), and its triangles"""
    import numpy as np
    U, V = np.meshgrid(np.linspace(-1., 1., n), np.linspace(-1., 1., n), indexing="ij")
    cx, cy = 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max())
    gx = (cx + 0.505 * np.ptp(x) * U * (1. + 0.02 * (1. - V * V))).ravel()
    gy = (cy + 0.505 * np.ptp(y) * V * (1. + 0.02 * (1. - U * U))).ravel()
    theta = (0.3 * np.sin(2. * U) + 0.2 * V - 0.1).ravel()
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    c0, c1, c2, c3 = (i * n + j).ravel(), ((i + 1) * n + j).ravel(), ((i + 1) * n + j + 1).ravel(), (i * n + j + 1).ravel()
    tri = np.concatenate([np.stack([c0, c1, c2], 1), np.stack([c0, c2, c3], 1)]).astype(np.int32)
    return np.ascontiguousarray(gx), np.ascontiguousarray(gy), np.ascontiguousarray(theta), np.ascontiguousarray(tri)


def measure(kind, out_dir):
    import numpy as np
    from nextsim_amd import dynamics, forcing as F, interp, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Nn = lm.num_nodes
    x, y = np.asarray(lm.coord_x, np.float64), np.asarray(lm.coord_y, np.float64)
    n = int(np.ceil(max(np.ptp(x), np.ptp(y)) / CELL))
    gx, gy, theta, tri = exchange_grid(x, y, n)
    G = gx.size
    L = dynamics.load_library()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipFree.argtypes = [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    nv = 3
    res = {"mesh": kind, "num_nodes": Nn, "device": dynamics.device_name(0) or "AMD Instinct MI355X (gfx950)", "grid": f"{n} x {n} points {CELL:.0f} m apart", "grid_size": G,
           "source_triangles": int(tri.shape[0]), "reps": REPS}

    rg = interp.Regrid(tri + 1, gx, gy)
    t0 = time.perf_counter()
    nm = interp.NodeMap.weights(rg, x, y)
    res["create_ms"] = (time.perf_counter() - t0) * 1e3      # (with the context's tables and completion, made by this first use)
    t0 = time.perf_counter()
    interp.NodeMap.weights(rg, x, y).close()
    res["create_again_ms"] = (time.perf_counter() - t0) * 1e3
    res["info"] = nm.info()
    rotation = -45. * PI / 180.
    nm.set_source(G, None, rotation="grid_theta", map_rotation=rotation, theta=theta)
    rng = np.random.default_rng(0)
    fields = [np.ascontiguousarray(0.2 * rng.standard_normal(G)) for _ in range(nv)]
    a, b = np.array([1., 1., 0.5]), np.array([0., 0., 0.01])
    cs, sn = np.cos(rotation - theta), np.sin(rotation - theta)

    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)

    def step():
        fe.step(); fe.synchronize()
    res["step_without_attachment"] = timed(step, reps=5, warm=1)

    # ---- (a) without the feature
    def route_a():
        t = [fields[v] * a[v] + b[v] for v in range(nv)]
        data = np.stack([cs * t[0] + sn * t[1], -sn * t[0] + cs * t[1], t[2]], axis=1)
        out = rg.interp_nodes(data, x, y, isdefault=False)
        f0 = dict(wind=f["wind"], ocean=np.concatenate([out[:, 0], out[:, 1]]), ssh=np.ascontiguousarray(out[:, 2]), element_depth=f["element_depth"])
        fe.set_forcing_pair(f0, f0)
        fe.synchronize()
        return out
    res["a_numpy_interp_nodes_set_forcing_pair"] = timed(route_a, reps=5, warm=1)
    rows_a = route_a()

    # ---- (b) the receive on the handle
    fe.nodes_coupled_attach("ocean", nm, a=a, b=b)

    def host_fields():
        fe.nodes_coupled_receive("ocean", fields)
        fe.synchronize()
    res["b_receive_host_fields"] = timed(host_fields)
    d_in = [C.c_void_p() for _ in range(nv)]
    for ptr, fld in zip(d_in, fields):
        assert L.hipMalloc(C.byref(ptr), fld.nbytes) == 0 and L.hipMemcpy(ptr, fld.ctypes.data, fld.nbytes, 1) == 0
    dev_ptrs = [ptr.value for ptr in d_in]

    def device_fields():
        fe.nodes_coupled_receive("ocean", dev_ptrs, device=True)
        fe.synchronize()
    res["b_receive_device_fields"] = timed(device_fields)
    got = fe.nodes_coupled_get("ocean")
    # (numpy's cos / sin are the C library's here; where they are not, the rotated pair may differ in the last bit and this says so)
    res["same_bits_as_route_a"] = bool(all(np.array_equal(got[v].view(np.uint64), np.ascontiguousarray(rows_a[:, v]).view(np.uint64)) for v in range(nv)))
    res["pcie_bytes"] = {"a": int(G * nv * 8 + 2 * Nn * 8 + Nn * nv * 8 + 2 * 5 * Nn * 8), "b_host_fields": int(G * nv * 8), "b_device_fields": 0}
    res["step_with_attachment"] = timed(step, reps=5, warm=1)

    # ---- the kernels alone
    d_out = [C.c_void_p() for _ in range(nv)]
    for ptr in d_out:
        assert L.hipMalloc(C.byref(ptr), Nn * 8) == 0
    out_ptrs = [ptr.value for ptr in d_out]
    kw = dict(a=a, b=b, pairs=[(0, 1)], in_device=True)
    both = timed(lambda: nm.receive_rows(dev_ptrs, out_device=out_ptrs, **kw))
    e1 = nm.export()
    one = interp.NodeMap.import_(dict(v=e1["v"][:1], a=e1["a"][:1], nods_src=G))
    one.set_source(G, None, rotation="grid_theta", map_rotation=rotation, theta=theta)
    src_only = timed(lambda: one.receive_rows(dev_ptrs, out_device=out_ptrs[:], **kw))
    both["bytes"] = int(G * nv * 8 * 2 + 2 * G * 8 + Nn * 36 + G * nv * 8 + Nn * nv * 8)
    res["kernels_both"] = both
    res["kernels_source_and_one_target"] = src_only
    gather_ms = both["median_ms"] - src_only["median_ms"]
    res["gather"] = {"median_ms": gather_ms, "bytes": int(Nn * 36 + G * nv * 8 + Nn * nv * 8)}
    res["gather"]["GBps"] = res["gather"]["bytes"] / max(gather_ms, 1e-6) / 1e6
    big = C.c_void_p()
    assert L.hipMalloc(C.byref(big), Nn * nv * 8) == 0
    big2 = C.c_void_p()
    assert L.hipMalloc(C.byref(big2), Nn * nv * 8) == 0
    copy = timed(lambda: (L.hipMemcpy(big, big2, Nn * nv * 8, 3), L.hipDeviceSynchronize()))
    copy["bytes"] = 2 * Nn * nv * 8
    copy["GBps"] = copy["bytes"] / (copy["median_ms"] * 1e-3) / 1e9
    res["device_copy_same_run"] = copy
    for ptr in d_in + d_out + [big, big2]:
        L.hipFree(ptr)
    fe.nodes_coupled_detach("ocean")
    fe.close(); one.close(); nm.close(); rg.close()
    res["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "nodal_receive.json"), "w"), indent=1)
    return res


def trace_loop(kind, loops):
    import numpy as np
    from nextsim_amd import dynamics, interp, mesh as M
    lm = M.localize(M.make_mesh(kind), 1)[0]
    x, y = np.asarray(lm.coord_x, np.float64), np.asarray(lm.coord_y, np.float64)
    Nn = x.size
    gx, gy, theta, tri = exchange_grid(x, y, int(np.ceil(max(np.ptp(x), np.ptp(y)) / CELL)))
    G = gx.size
    rg = interp.Regrid(tri + 1, gx, gy)
    nm = interp.NodeMap.weights(rg, x, y)
    nm.set_source(G, None, rotation="grid_theta", map_rotation=-45. * PI / 180., theta=theta)
    L = dynamics.load_library()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def dev(nbytes, src=None):
        ptr = C.c_void_p()
        assert L.hipMalloc(C.byref(ptr), nbytes) == 0 and (src is None or L.hipMemcpy(ptr, src.ctypes.data, nbytes, 1) == 0)
        return ptr
    rng = np.random.default_rng(0)
    fin = [dev(G * 8, np.ascontiguousarray(rng.standard_normal(G))) for _ in range(3)]
    out = [dev(Nn * 8) for _ in range(3)]
    big, big2 = dev(3 * Nn * 8), dev(3 * Nn * 8)
    for _ in range(loops):
        nm.receive_rows([q.value for q in fin], a=[1., 1., .5], b=[0., 0., .01], pairs=[(0, 1)], in_device=True, out_device=[q.value for q in out])
        L.hipMemcpy(big, big2, 3 * Nn * 8, 3)
    L.hipDeviceSynchronize()
    print(f"{loops} receives and copies: {Nn} nodes, {G} source nodes")


def table(res):
    def row(name, r, extra=""):
        return f"| {name} | {r['median_ms']:.3f} | {r['min_ms']:.3f} – {r['max_ms']:.3f} | {r['n']} | {extra} |"
    i, pc, cp = res["info"], res["pcie_bytes"], res["device_copy_same_run"]
    lines = [BEGIN,
             f"Measured {res['date']} on one {res['device']}, `{res['mesh']}` mesh ({res['num_nodes']} nodes), {res['grid']} ({res['grid_size']} source nodes, "
             f"{res['source_triangles']} triangles; {i['beyond_hull']} nodes beyond the hull), fields I_Uocn, I_Vocn, I_SSH with the gridTheta rotation.  Wall-clock milliseconds, "
             f"every call synchronised.  Rows of (b) have the bits of (a): {res['same_bits_as_route_a']}.  `nxs_nodemap_create`: {res['create_ms']:.1f} ms the first time on a "
             f"context (its tables and completion included), {res['create_again_ms']:.1f} ms again.",
             "",
             "| what | median ms | min – max | samples | note |", "|---|---|---|---|---|",
             row("(a) numpy a, b, rotation; `nxs_regrid_interp_nodes` on a kept context; `nxs_dyn_set_forcing_pair`", res["a_numpy_interp_nodes_set_forcing_pair"],
                 f"{pc['a'] / 1e6:.1f} MB over PCIe; locates every node again"),
             row("(b) `nxs_dyn_nodes_coupled_receive`, host fields", res["b_receive_host_fields"], f"{pc['b_host_fields'] / 1e6:.1f} MB over PCIe"),
             row("(b) `nxs_dyn_nodes_coupled_receive`, device fields", res["b_receive_device_fields"], "nothing over PCIe"),
             row("`nxs_nodemap_receive_rows` alone, device to device: both kernels and the call (wall clock)", res["kernels_both"], "launch and synchronisation dominate"),
             row("... with a one-target map on the same source: `k_nodemap_source` and the call (wall clock)", res["kernels_source_and_one_target"],
                 "the kernels' own times: the trace below the table"),
             row("device-to-device copy of the three output rows, same run (wall clock)", cp, "the call included"),
             row("`nxs_dyn_step` without an attachment", res["step_without_attachment"], ""),
             row("`nxs_dyn_step` with `ocean_cpl_nodes` attached and received", res["step_with_attachment"], "the receive is not part of the step"),
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
    if "--trace-loop" in args:
        trace_loop(args[0] if not args[0].startswith("--") else "2km", int(args[args.index("--trace-loop") + 1]))
        sys.exit(0)
    if "--from-json" in args:
        res = json.load(open(args[args.index("--from-json") + 1]))
        json.dump(res, open(os.path.join(ROOT, "profiles", "nodal_receive.json"), "w"), indent=1)
    else:
        out_dir = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles")
        kind = next((a for a in args if not a.startswith("--") and (args.index(a) == 0 or args[args.index(a) - 1] != "--out")), "2km")
        res = measure(kind, out_dir)
    write_design(res)
    print(table(res))
