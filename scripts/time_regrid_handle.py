"""Cost of a regrid's state side at 2 km: nxs_dyn_regrid (the state stays on the device) against the host route of tests/test_regrid_cycle.py -- get_state,
numpy packing, the two nxs_regrid_* interpolations on host arrays, numpy clipping, set_mesh + put_state -- on the same mesh pair (bench.py's aux_regrid pair:
3 % of the triangles split) in the same process.

    python scripts/time_regrid_handle.py [mesh] [--out DIR]      measure on the GPU, print one JSON line, write DIR/regrid_handle.json (default profiles/)

Two handles are stepped identically; one takes each route.  Both routes build the old mesh's regrid context themselves and both end with the handle on the
new mesh, state in place (forcing not included: it is the same set_forcing after either).  Two rounds; the second (warm allocator) is the one to quote."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ELT = ("conc", "thick", "snow_thick", "damage", "ridge_ratio", "sigma0", "sigma1", "sigma2", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi")


def measure(kind):
    import numpy as np
    import bench
    from nextsim_amd import dynamics, forcing as F, mesh as M
    from nextsim_amd.interp import Regrid
    gm = M.make_mesh(kind)
    xn, yn, trin, prev = bench.split_adapted_mesh(gm, 0.03, 9)
    old_of = prev.astype(np.int64) - 1
    inherit = lambda a: np.where(old_of >= 0, a[np.maximum(old_of, 0)], False)   # noqa: E731  (the remesher's new vertices are interior)
    gm2 = M.GlobalMesh(x=xn, y=yn, tri=np.ascontiguousarray(trin, np.int32), dirichlet=inherit(gm.dirichlet), neumann=inherit(gm.neumann),
                       lat=M.polar_stereographic_lat(xn, yn), name=kind + "-adapted")
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    lm, lm2 = M.localize(gm, 1)[0], M.localize(gm2, 1)[0]
    f = F.localize_fields(F.global_fields(gm, p, "arctic", C_fix, C_alea), lm, gm.num_nodes)
    f2 = F.localize_fields(F.global_fields(gm2, p, "arctic", C_fix, C_alea), lm2, gm2.num_nodes)
    inputs = {k: f2[k] for k in dynamics.REGRID_INPUTS}
    idx_old = (gm.tri + 1).astype(np.int32).ravel(); idx_new = np.ascontiguousarray(trin + 1, np.int32).ravel()
    Nn, n2 = lm.num_nodes, lm2.num_nodes
    rounds = []
    for _ in range(2):
        fes = []
        for _k in range(2):
            fe = dynamics.FiniteElementDynamics(p)
            fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
            fe.step(); fe.step(); fe.synchronize()
            fes.append(fe)
        host, dev = fes
        um = host.get_state()["UM"]
        xm, ym = lm.coord_x + um[:Nn], lm.coord_y + um[Nn:]          # M_mesh_root.move(um_root, 1.): the host has them, it ran the remesher on them
        # ---- the host route
        t0 = time.perf_counter()
        st = host.get_state()
        t1 = time.perf_counter()
        elt_in = np.column_stack([st[k] for k in ELT])
        nod_in = np.column_stack([st["VT"][:Nn], st["VT"][Nn:], st["UM"][:Nn], st["UM"][Nn:], st["UT"][:Nn], st["UT"][Nn:]])
        t2 = time.perf_counter()
        rg = Regrid(idx_old, xm, ym)
        elt_out, ri = rg.remap_elements(elt_in, idx_new, xn, yn, prev, 0, return_info=True)
        nod_out = rg.interp_nodes(nod_in, xn, yn, False, 0.0)
        rg.close()
        t3 = time.perf_counter()
        s2 = {k: np.ascontiguousarray(elt_out[:, i]) for i, k in enumerate(ELT)}
        s2["conc"] = np.clip(s2["conc"], 0., 1.); s2["damage"] = np.clip(s2["damage"], 0., 1.)
        s2["VT"] = np.concatenate([nod_out[:, 0], nod_out[:, 1]]); s2["UM"] = np.zeros(2 * n2); s2["UT"] = np.zeros(2 * n2)
        s2.update(inputs)
        t4 = time.perf_counter()
        host.set_mesh(lm2)
        t5 = time.perf_counter()
        host.put_state(s2)
        t6 = time.perf_counter()
        # ---- nxs_dyn_regrid
        t7 = time.perf_counter()
        info = dev.regrid(lm2, prev, 0, inputs, moved=(xm, ym))
        t8 = time.perf_counter()
        a, b = host.get_state(), dev.get_state()
        same = {k: bool(np.array_equal(a[k], b[k])) for k in ("VT", "UM", "UT", "sigma0", "sigma1", "sigma2", "thick", "snow_thick")}
        rounds.append({"host_route_ms": (t6 - t0) * 1e3,
                       "host_route_breakdown_ms": {"get_state": (t1 - t0) * 1e3, "numpy_pack": (t2 - t1) * 1e3, "context_and_two_interpolations": (t3 - t2) * 1e3,
                                                   "numpy_unpack_and_clip": (t4 - t3) * 1e3, "set_mesh": (t5 - t4) * 1e3, "put_state": (t6 - t5) * 1e3},
                       "regrid_call_ms": (t8 - t7) * 1e3, "regrid_info": info, "remap_failed_host_route": int(ri["num_failed"]),
                       "same_bits_where_the_routes_apply_the_same_rule": same})
        host.close(); dev.close()
    return {"workload": f"regrid of the {kind} mesh: {gm.num_elements} triangles / {gm.num_nodes} nodes -> {trin.shape[0]} / {xn.size}; 13 element variables, 6 nodal columns",
            "first_round": rounds[0], "second_round": rounds[1],
            "note": "host_route_ms = get_state + numpy + nxs_regrid_create / remap_elements / interp_nodes on host arrays + numpy + set_mesh + put_state (tests/test_regrid_cycle.py); "
                    "regrid_call_ms = FiniteElementDynamics.regrid, wall clock around the call, context built inside; regrid_info = nxs_dyn_regrid_info (set_mesh_ms holds the "
                    "same nxs_dyn_set_mesh work -- the patch cutter -- as the host route's set_mesh)"}


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles")
    if "--out" in args:
        i = args.index("--out"); out_dir = args[i + 1]; del args[i:i + 2]
    res = measure(args[0] if args else "2km")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "regrid_handle.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
