"""Cost of thermo()'s ice columns on the device (nxs_dyn_column) at 2 km.

    python scripts/time_column.py [mesh] [--out DIR]     measure on the GPU, print the figures, write DIR/column.json (default profiles/)

Workload: the arctic mesh with the designed inputs of tests/column_ref.py (every branch of both column models taken somewhere), WINTON, the young-ice category, the
default configuration otherwise (BASIC, constant ocean, precip * snowfr, constant mixed layer depth).  Wall time per call of REPS calls enqueued back to back and
synchronised once (the calls are asynchronous), median of 7 such batches after a warm-up batch; the temperatures of one call feed the next, as in a run.  Bytes
moved: what the launch must read and write once per element -- 22 rows read (precip, snowfr, sst, sss, conc, thick, snow_thick, conc_young, h_young, hs_young,
tice0/1/2, tsurf_young and the eight flux rows) and 28 written (the 22 rows and the six rows updated in place).  No threshold: the numbers are the result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS, BATCHES = 20, 7


def measure(kind, out_dir):
    import numpy as np
    import column_ref as R
    import fluxes_ref as FR
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Ne = lm.num_elements
    tri = lm.indices.reshape(-1, 3).astype(np.int64) - 1
    inp, _, _ = R.make_inputs(lm.coord_x, lm.coord_y, tri)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    f = dict(f, **{k: inp[k] for k in ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young")})
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.flux_configure()
    fe.flux_set_atmosphere(tair=inp["tair"], mslp=finp["mslp"], Qsw_in=finp["Qsw_in"], humidity=finp["dair"], longwave=finp["Qlw_in"])
    fe.flux_put(**dict({k: finp[k] for k in _abi.FLUX_STATE}, tice0=inp["tice0"], tsurf_young=inp["tsurf_young"], sst=inp["sst"], sss=inp["sss"]))
    fe.column_configure(thermo_type="winton")
    fe.column_set_forcing(precip=inp["precip"], snow=inp["snowfr"])
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    fe.fluxes()
    t = []
    for b in range(BATCHES + 1):
        fe.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fe.column(R.DT)
        fe.synchronize()
        if b:
            t.append((time.perf_counter() - t0) / REPS * 1e6)
    us = float(np.median(np.asarray(t)))
    nbytes = Ne * (22 + 28) * 8
    res = {"mesh": kind, "num_elements": int(Ne), "device": dynamics.device_name(0), "calls_per_batch": REPS, "batches": BATCHES, "column_us": us,
           "bytes_per_call": int(nbytes), "GB_per_s": nbytes / us * 1e-3}
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "column.json"), "w"), indent=1)
    print(f"{kind}: {Ne} triangles, {res['device']}")
    print(f"  nxs_dyn_column {us / 1e3:9.4f} ms per call, {nbytes / 1e6:.0f} MB moved, {res['GB_per_s']:.0f} GB/s")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    measure(a.mesh, a.out)
