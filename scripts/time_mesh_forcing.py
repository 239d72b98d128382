"""Cost of ingesting forcing given on a triangulated source on the device (nxs_nodemap_load_rows, nxs_dyn_forcing_ingest_mesh, nxs_dyn_thermo_forcing_ingest_mesh)
at 2 km: a TOPAZ-like source of 12.5 km points over the mesh, triangulated; u, v, ssh with the uniform rotation at the nodes (topaz4r_nodes) and three scalars at
the element barycentres (topaz4r_elements), two forcing steps each.

    python scripts/time_mesh_forcing.py [mesh] [--out DIR]     measure on the GPU, write DIR/mesh_forcing.json (default profiles/) and DESIGN.md's table
    python scripts/time_mesh_forcing.py --from-json FILE       no GPU: copy FILE to profiles/mesh_forcing.json and rewrite DESIGN.md's table from it
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_mesh_forcing.py [mesh] --trace-loop 200
                                                                nothing timed here: 200 loads (device fields to device rows, six columns at the nodes) and 200
                                                                device-to-device copies of the six output rows, for the profiler's kernel statistics

Reported, each a median of REPS wall-clock samples after warm-up calls, with its smallest and largest (every timed call ends with a synchronisation):
  (a) the route a host has WITHOUT the feature: the load tail and the rotation in numpy, nxs_regrid_interp_nodes on a kept context with six columns (which locates
      every node and every barycentre again), then nxs_dyn_set_forcing_pair / nxs_dyn_thermo_forcing_pair;
  (b) the two ingests from host fields and from device fields;
  nxs_nodemap_load_rows alone, device fields to device rows, a device-to-device copy of the six output rows in the same run, nxs_nodemap_create once per target
  set, and nxs_dyn_step with and without an attachment.
"""
import ctypes as C
import json
import math
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from time_nodal_receive import CELL, exchange_grid, timed  # noqa: E402

BEGIN, END = "<!-- mesh-forcing-measurement:begin (written by scripts/time_mesh_forcing.py) -->", "<!-- mesh-forcing-measurement:end -->"
REPS = 9
ANGLE = 0.4
NODE_ROWS, ELEM_ROWS = ["ocean_u", "ocean_v", "ssh"], ["ocean_temp", "ocean_salt", "mld"]
COEF = dict(scale_factor=[1., 1., 0.01, 1., 1., 0.02], add_offset=[0., 0., 1.5, 0., 0., 1.25], a=[1., -0.5, 1., 1., -0.5, 1.5], b=[0., 0.25, 0., 0., 0.25, -0.125])


def setup(kind):
    import numpy as np
    from nextsim_amd import interp, mesh as M
    gm = M.make_mesh(kind)
    lm = M.localize(gm, 1)[0]
    x, y = np.asarray(lm.coord_x, np.float64), np.asarray(lm.coord_y, np.float64)
    t = np.asarray(lm.indices, np.int64).reshape(-1, 3) - 1
    bx, by = np.ascontiguousarray((x[t[:, 0]] + x[t[:, 1]] + x[t[:, 2]]) / 3.), np.ascontiguousarray((y[t[:, 0]] + y[t[:, 1]] + y[t[:, 2]]) / 3.)
    n = int(np.ceil(max(np.ptp(x), np.ptp(y)) / CELL))
    gx, gy, _, tri = exchange_grid(x, y, n)
    rg = interp.Regrid(tri + 1, gx, gy)
    return gm, lm, (x, y), (bx, by), n, gx.size, tri, rg


def numpy_load(fields, co, pair, c, s):
    """the tail of loadDataset and the uniform rotation on the host: [G, 6] in loadDataset's order"""
    import numpy as np
    cols = []
    for k, d in enumerate(fields):
        t = (d * co["scale_factor"][k] + co["add_offset"][k]) * co["a"][k] + co["b"][k]
        cols.append(np.where(np.isnan(t), 0., t))
    if pair:
        for s0 in (0, 3):
            t0, t1 = cols[s0], cols[s0 + 1]
            cols[s0], cols[s0 + 1] = c * t0 + s * t1, -s * t0 + c * t1
    return np.stack(cols, axis=1)


def measure(kind, out_dir):
    import numpy as np
    from nextsim_amd import dynamics, forcing as F, interp

    gm, lm, (x, y), (bx, by), n, G, tri, rg = setup(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    f = F.localize_fields(F.global_fields(gm, p, "arctic", C_fix, C_alea), lm, gm.num_nodes)
    Nn, Ne = lm.num_nodes, lm.num_elements
    L = dynamics.load_library()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipFree.argtypes = [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    res = {"mesh": kind, "num_nodes": Nn, "num_elements": Ne, "device": dynamics.device_name(0) or "AMD Instinct MI355X (gfx950)", "grid": f"{n} x {n} points {CELL:.0f} m apart",
           "grid_size": G, "source_triangles": int(tri.shape[0]), "reps": REPS}

    t0 = time.perf_counter()
    nm = interp.NodeMap.weights(rg, x, y)
    res["create_nodes_ms"] = (time.perf_counter() - t0) * 1e3      # (with the context's tables and completion, made by this first use)
    t0 = time.perf_counter()
    nme = interp.NodeMap.weights(rg, bx, by)
    res["create_elements_ms"] = (time.perf_counter() - t0) * 1e3
    res["info_nodes"], res["info_elements"] = nm.info(), nme.info()
    c, s = math.cos(-ANGLE), math.sin(-ANGLE)
    nm.set_source(G, None, rotation="uniform", cos_m_diff_angle=c, sin_m_diff_angle=s)
    nme.set_source(G, None)
    rng = np.random.default_rng(0)
    nodal = [np.ascontiguousarray(0.2 * rng.standard_normal(G)) for _ in range(6)]
    elem = [np.ascontiguousarray(rng.standard_normal(G)) for _ in range(6)]
    for fl in nodal + elem:
        fl[rng.integers(0, G, 50)] = np.nan      # missing values at wet points
    co = {k: np.array(v) for k, v in COEF.items()}

    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)

    def step():
        fe.step(); fe.synchronize()
    res["step_without_attachment"] = timed(step, reps=5, warm=1)

    # ---- (a) without the feature
    def route_a():
        dn, de = numpy_load(nodal, co, True, c, s), numpy_load(elem, co, False, c, s)
        on = rg.interp_nodes(dn, x, y, isdefault=False)
        oe = rg.interp_nodes(de, bx, by, isdefault=False)
        snap = [dict(wind=f["wind"], ocean=np.concatenate([on[:, 3 * k], on[:, 3 * k + 1]]), ssh=np.ascontiguousarray(on[:, 3 * k + 2]), element_depth=f["element_depth"]) for k in range(2)]
        fe.set_forcing_pair(snap[0], snap[1])
        fe.thermo_forcing_pair({r: np.ascontiguousarray(oe[:, j]) for j, r in enumerate(ELEM_ROWS)}, {r: np.ascontiguousarray(oe[:, 3 + j]) for j, r in enumerate(ELEM_ROWS)})
        fe.synchronize()
        return on, oe
    res["a_numpy_interp_nodes_pairs"] = timed(route_a, reps=5, warm=1)
    on, oe = route_a()

    # ---- (b) the ingests on the handle
    fe.forcing_attach_mesh(1, nm); fe.thermo_forcing_attach_mesh(1, nme)

    def host_fields():
        fe.forcing_ingest_mesh(1, nodal, NODE_ROWS, pairs=[(0, 1)], **co)
        fe.thermo_forcing_ingest_mesh(1, elem, ELEM_ROWS, **co)
        fe.synchronize()
    res["b_ingest_host_fields"] = timed(host_fields)
    d_in = [C.c_void_p() for _ in range(12)]
    for ptr, fld in zip(d_in, nodal + elem):
        assert L.hipMalloc(C.byref(ptr), fld.nbytes) == 0 and L.hipMemcpy(ptr, fld.ctypes.data, fld.nbytes, 1) == 0
    dn_ptrs, de_ptrs = [q.value for q in d_in[:6]], [q.value for q in d_in[6:]]

    def device_fields():
        fe.forcing_ingest_mesh(1, dn_ptrs, NODE_ROWS, pairs=[(0, 1)], device=True, **co)
        fe.thermo_forcing_ingest_mesh(1, de_ptrs, ELEM_ROWS, device=True, **co)
        fe.synchronize()
    res["b_ingest_device_fields"] = timed(device_fields)
    same = True
    for k in range(2):
        gn, ge = fe.forcing_get(k, NODE_ROWS), fe.thermo_forcing_get(k, ELEM_ROWS)
        for j in range(3):
            same = same and np.array_equal(gn[NODE_ROWS[j]].view(np.uint64), np.ascontiguousarray(on[:, 3 * k + j]).view(np.uint64))
            same = same and np.array_equal(ge[ELEM_ROWS[j]].view(np.uint64), np.ascontiguousarray(oe[:, 3 * k + j]).view(np.uint64))
    res["same_bits_as_route_a"] = bool(same)
    res["pcie_bytes"] = {"a": int(2 * 6 * G * 8 + 2 * (Nn + Ne) * 8 + 6 * (Nn + Ne) * 8 + 10 * Nn * 8 + 6 * Ne * 8), "b_host_fields": int(12 * G * 8), "b_device_fields": 0}
    fe.set_forcing_time_rows({g: dict(mode="linear", fcoeff0=0.5, fcoeff1=0.5) for g in ("ocean", "ssh")})
    res["step_with_attachment"] = timed(step, reps=5, warm=1)

    # ---- the load alone, and a copy of its output rows
    d_out = [C.c_void_p() for _ in range(6)]
    for ptr in d_out:
        assert L.hipMalloc(C.byref(ptr), Nn * 8) == 0
    out_ptrs = [q.value for q in d_out]
    load = timed(lambda: nm.load_rows(dn_ptrs, n_step=2, pairs=[(0, 1)], in_device=True, out_device=out_ptrs, **co))
    load["gather_bytes"] = int(Nn * 36 + 6 * G * 8 + 6 * Nn * 8)
    res["load_rows_device_to_device"] = load
    big, big2 = C.c_void_p(), C.c_void_p()
    assert L.hipMalloc(C.byref(big), Nn * 6 * 8) == 0 and L.hipMalloc(C.byref(big2), Nn * 6 * 8) == 0
    copy = timed(lambda: (L.hipMemcpy(big, big2, Nn * 6 * 8, 3), L.hipDeviceSynchronize()))
    copy["bytes"] = 2 * Nn * 6 * 8
    res["device_copy_same_run"] = copy
    for ptr in d_in + d_out + [big, big2]:
        L.hipFree(ptr)
    fe.close(); nm.close(); nme.close(); rg.close()
    res["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "mesh_forcing.json"), "w"), indent=1)
    return res


def trace_loop(kind, loops):
    import numpy as np
    from nextsim_amd import dynamics, interp
    _, lm, (x, y), _, n, G, tri, rg = setup(kind)
    Nn = x.size
    nm = interp.NodeMap.weights(rg, x, y)
    nm.set_source(G, None, rotation="uniform", cos_m_diff_angle=math.cos(-ANGLE), sin_m_diff_angle=math.sin(-ANGLE))
    L = dynamics.load_library()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def dev(nbytes, src=None):
        ptr = C.c_void_p()
        assert L.hipMalloc(C.byref(ptr), nbytes) == 0 and (src is None or L.hipMemcpy(ptr, src.ctypes.data, nbytes, 1) == 0)
        return ptr
    rng = np.random.default_rng(0)
    fin = [dev(G * 8, np.ascontiguousarray(rng.standard_normal(G))) for _ in range(6)]
    out = [dev(Nn * 8) for _ in range(6)]
    big, big2 = dev(6 * Nn * 8), dev(6 * Nn * 8)
    co = {k: np.array(v) for k, v in COEF.items()}
    for _ in range(loops):
        nm.load_rows([q.value for q in fin], n_step=2, pairs=[(0, 1)], in_device=True, out_device=[q.value for q in out], **co)
        L.hipMemcpy(big, big2, 6 * Nn * 8, 3)
    L.hipDeviceSynchronize()
    print(f"{loops} loads and copies: {Nn} nodes, {G} source nodes")


def table(res):
    def row(name, r, extra=""):
        return f"| {name} | {r['median_ms']:.3f} | {r['min_ms']:.3f} – {r['max_ms']:.3f} | {r['n']} | {extra} |"
    pc, cp = res["pcie_bytes"], res["device_copy_same_run"]
    lines = [BEGIN,
             f"Measured {res['date']} on one {res['device']}, `{res['mesh']}` mesh ({res['num_nodes']} nodes, {res['num_elements']} elements), {res['grid']} "
             f"({res['grid_size']} source nodes, {res['source_triangles']} triangles; {res['info_nodes']['beyond_hull']} nodes and {res['info_elements']['beyond_hull']} "
             f"barycentres beyond the hull); u, v, ssh with the uniform rotation at the nodes, three scalars at the barycentres, two forcing steps each (twelve columns).  "
             f"Wall-clock milliseconds, every call synchronised.  Rows of (b) have the bits of (a): {res['same_bits_as_route_a']}.  `nxs_nodemap_create`: "
             f"{res['create_nodes_ms']:.1f} ms for the nodes (the context's tables and completion included), {res['create_elements_ms']:.1f} ms for the barycentres, once per mesh.",
             "",
             "| what | median ms | min – max | samples | note |", "|---|---|---|---|---|",
             row("(a) numpy load tail and rotation; `nxs_regrid_interp_nodes` on a kept context, six columns, twice; `nxs_dyn_set_forcing_pair`, `nxs_dyn_thermo_forcing_pair`",
                 res["a_numpy_interp_nodes_pairs"], f"{pc['a'] / 1e6:.1f} MB over PCIe; locates every node and barycentre again"),
             row("(b) `nxs_dyn_forcing_ingest_mesh` + `nxs_dyn_thermo_forcing_ingest_mesh`, host fields", res["b_ingest_host_fields"], f"{pc['b_host_fields'] / 1e6:.1f} MB over PCIe"),
             row("(b) the same, device fields", res["b_ingest_device_fields"], "nothing over PCIe"),
             row("`nxs_nodemap_load_rows` alone, six columns at the nodes, device to device: both kernels and the call (wall clock)", res["load_rows_device_to_device"],
                 "launch and synchronisation dominate"),
             row("device-to-device copy of the six output rows, same run (wall clock)", cp, "the call included"),
             row("`nxs_dyn_step` without an attachment", res["step_without_attachment"], ""),
             row("`nxs_dyn_step` with both datasets attached and ingested", res["step_with_attachment"], "the ingest is not part of the step"),
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
        json.dump(res, open(os.path.join(ROOT, "profiles", "mesh_forcing.json"), "w"), indent=1)
    else:
        out_dir = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles")
        kind = next((a for a in args if not a.startswith("--") and (args.index(a) == 0 or args[args.index(a) - 1] != "--out")), "2km")
        res = measure(kind, out_dir)
    write_design(res)
    print(table(res))
