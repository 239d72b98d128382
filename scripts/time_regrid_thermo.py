"""Cost of carrying the thermodynamic state across a regrid at 2 km (nxs_dyn_regrid_carry_thermo), on bench.py's aux_regrid pair (3 % of the triangles split)
with everything a wave-coupled WINTON run with young ice carries: 13 state columns, 12 FSD bins, 12 mechanical bins, cum_damage and the 17 carried rows of
nxs_dyn_flux_state / _column_state / _slab_state -- 55 columns, two LDS tiles.

    python scripts/time_regrid_thermo.py [mesh] [--out DIR]      measure on the GPU, print one JSON line, write DIR/regrid_thermo.json (default profiles/)

Two comparisons, one handle, one process; before every regrid the handle is put back on the old mesh with the same state (set_mesh, put_state, the coupled
columns, the 20 thermodynamic rows):
  1. option "regrid_tile" 1 (rows wider than 31 columns through LDS in column tiles) against 0 (every thread walks its own row in global memory): median of
     REPEATS regrids each, interleaved, behind one untimed regrid per setting; the figure is collect_ms + redistribute_ms of nxs_dyn_regrid_info.
  2. the carry against the route it replaces -- flux_get + column_get + slab_get, nxs_dyn_regrid with those rows as host extras, flux_put + column_put +
     slab_put --, two rounds; the state side of each is its wall clock without set_mesh_ms.  The script fails if the carry's is the larger in either round."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEATS = 5
NBINS = 12
MU = 0.055
DRAG_ICE_T = 1.3e-3


def measure(kind):
    import numpy as np
    import bench
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M
    gm = M.make_mesh(kind)
    xn, yn, trin, prev = bench.split_adapted_mesh(gm, 0.03, 9)
    old_of = prev.astype(np.int64) - 1
    inherit = lambda a: np.where(old_of >= 0, a[np.maximum(old_of, 0)], False)   # noqa: E731  (the remesher's new vertices are interior)
    gm2 = M.GlobalMesh(x=xn, y=yn, tri=np.ascontiguousarray(trin, np.int32), dirichlet=inherit(gm.dirichlet), neumann=inherit(gm.neumann),
                       lat=M.polar_stereographic_lat(xn, yn), name=kind + "-adapted")
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE), gm, alea_factor=0.33)
    lm, lm2 = M.localize(gm, 1)[0], M.localize(gm2, 1)[0]
    f = F.localize_fields(F.global_fields(gm, p, "arctic", C_fix, C_alea), lm, gm.num_nodes)
    f2 = F.localize_fields(F.global_fields(gm2, p, "arctic", C_fix, C_alea), lm2, gm2.num_nodes)
    inputs = {k: f2[k] for k in dynamics.REGRID_INPUTS}
    Ne, Ne2 = lm.num_elements, lm2.num_elements
    rng = np.random.default_rng(3)
    tice = lambda: np.where(f["thick"] > 0, rng.uniform(-30., -0.5, Ne), -MU * 5.)   # noqa: E731
    rows = dict(tice0=rng.uniform(-30., -0.5, Ne), tsurf_young=rng.uniform(-20., 0., Ne), sst=rng.uniform(-1.8, 5., Ne), sss=rng.uniform(28., 35., Ne),
                drag_ti=rng.uniform(1e-3, 2e-3, Ne), drag_ti_young=rng.uniform(1e-3, 2e-3, Ne), pond_fraction=rng.uniform(0., 0.3, Ne),
                lid_volume=rng.uniform(0., 0.01, Ne), tice1=tice(), tice2=tice(), conc_upd=rng.uniform(-1.2, 1.2, Ne), pond_volume=rng.uniform(0., 0.05, Ne),
                del_vi_tend=rng.normal(0., 0.01, Ne), freeze_days=rng.uniform(-5., 200., Ne), freeze_onset=rng.uniform(0., 1., Ne),
                conc_summer=rng.uniform(0., 1., Ne), thick_summer=rng.uniform(0., 3., Ne), fyi_fraction=rng.uniform(0., 1.1, Ne), age_det=rng.uniform(0., 3e7, Ne),
                age=rng.uniform(0., 3e7, Ne))
    cum = rng.uniform(0., 0.2, Ne)
    bins = np.ascontiguousarray(rng.dirichlet(np.ones(NBINS), Ne).T * f["conc"])
    mech = np.ascontiguousarray(rng.dirichlet(np.ones(NBINS), Ne).T * f["conc"])
    groups = (("flux", _abi.FLUX_STATE), ("column", _abi.COL_STATE), ("slab", _abi.SLAB_STATE))
    moved = (lm.coord_x, lm.coord_y)                       # (no step has run: M_UM = 0)

    fe = dynamics.FiniteElementDynamics(p)
    fe.column_configure(thermo_type="winton", freezingpoint_mu=MU)

    def put_rows(r):
        fe.flux_put(**{k: r[k] for k in _abi.FLUX_STATE}); fe.column_put(**{k: r[k] for k in _abi.COL_STATE}); fe.slab_put(**{k: r[k] for k in _abi.SLAB_STATE})

    def get_rows():
        return dict(fe.flux_get(), **fe.column_get(), **fe.slab_get(_abi.SLAB_STATE))

    def old_mesh(carry, tile=1):
        fe.set_option("regrid_tile", tile)
        fe.regrid_carry_thermo(carry=carry, drag_ice_t=DRAG_ICE_T)
        fe.set_mesh(lm); fe.put_state(f)
        fe.put_coupled(cum_damage=cum, conc_fsd=bins); fe.fsd_put(conc_mech_fsd=mech)
        put_rows(rows)
        fe.synchronize()

    # ---- 1. the two instances for wide rows
    two = {0: [], 1: []}
    seen = {}
    for rep in range(REPEATS + 1):
        for tile in (0, 1):
            old_mesh(True, tile)
            info = fe.regrid(lm2, prev, 0, inputs, moved=moved, freezingpoint_mu=MU)
            t = fe.regrid_thermo_info()
            assert t["tiled"] == tile and t["nb_var_element"] == 13 + 2 * NBINS + 1 + 17 and info["num_failed"] == 0, (t, info)
            if rep == 0:                                   # untimed; the two instances leave the same bits
                seen[tile] = get_rows()
            else:
                two[tile].append({k: info[k] for k in ("collect_ms", "redistribute_ms")})
    same_tiles = all(np.array_equal(seen[0][k].view(np.uint64), seen[1][k].view(np.uint64)) for k in seen[0])
    med = {tile: float(np.median([x["collect_ms"] + x["redistribute_ms"] for x in two[tile]])) for tile in (0, 1)}

    # ---- 2. the carry against fetch, host extras, put back
    rounds = []
    for _ in range(2):
        old_mesh(True)
        t0 = time.perf_counter()
        info_c = fe.regrid(lm2, prev, 0, inputs, moved=moved, freezingpoint_mu=MU)
        t1 = time.perf_counter()
        carried = get_rows()
        old_mesh(False)
        t2 = time.perf_counter()
        got = get_rows()
        extras, names = [], []
        for name, k, lo, hi, is_tice in dynamics.REGRID_THERMO_COLUMNS:
            x = dict(old=got[name], transformation=k, is_tice=is_tice)
            if lo is not None:
                x["min"] = lo
            if hi is not None:
                x["max"] = hi
            extras.append(x); names.append(name)
        info_h = fe.regrid(lm2, prev, 0, inputs, extras, moved=moved, freezingpoint_mu=MU)
        back = {k: x["new"] for k, x in zip(names, extras)}
        back.update(drag_ti=np.full(Ne2, DRAG_ICE_T), drag_ti_young=np.full(Ne2, DRAG_ICE_T), pond_fraction=np.zeros(Ne2))
        put_rows(back)
        fe.synchronize()
        t3 = time.perf_counter()
        hosted = get_rows()
        same = all(np.array_equal(carried[k].view(np.uint64), hosted[k].view(np.uint64)) for k in carried)
        rounds.append({"carry_call_ms": (t1 - t0) * 1e3, "carry_state_side_ms": (t1 - t0) * 1e3 - info_c["set_mesh_ms"], "carry_info": info_c,
                       "host_extras_route_ms": (t3 - t2) * 1e3, "host_extras_state_side_ms": (t3 - t2) * 1e3 - info_h["set_mesh_ms"], "host_extras_info": info_h,
                       "same_bits_in_all_20_rows": bool(same)})
    fe.close()
    ok = all(r["carry_state_side_ms"] <= r["host_extras_state_side_ms"] for r in rounds)
    n = 13 + 2 * NBINS + 1 + 17
    return {"workload": f"regrid of the {kind} mesh: {Ne} -> {Ne2} triangles; {n} element columns (13 state, {NBINS} + {NBINS} FSD bins, cum_damage, 17 carried "
                        f"thermodynamic rows), WINTON, young ice",
            "wide_rows": {"regrid_tile_0_global_walk_median_ms": med[0], "regrid_tile_1_column_tiles_median_ms": med[1], "repeats": REPEATS,
                          "what": "collect_ms + redistribute_ms of nxs_dyn_regrid_info", "samples": two, "same_bits": bool(same_tiles),
                          "tiled_not_slower": bool(med[1] <= med[0])},
            "carry_against_host_extras": {"first_round": rounds[0], "second_round": rounds[1], "carry_state_side_not_slower_in_both_rounds": bool(ok)},
            "note": "state side = wall clock of the route without set_mesh_ms (the patch cutter, the same work on either route).  host_extras route = flux_get + "
                    "column_get + slab_get, nxs_dyn_regrid with the 17 rows as host extras, flux_put + column_put + slab_put with the three re-made rows."}


if __name__ == "__main__":
    args = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles")
    if "--out" in args:
        i = args.index("--out"); out_dir = args[i + 1]; del args[i:i + 2]
    res = measure(args[0] if args else "2km")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "regrid_thermo.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    if not res["carry_against_host_extras"]["carry_state_side_not_slower_in_both_rounds"]:
        sys.exit("the carry's state side was slower than the route it replaces")
