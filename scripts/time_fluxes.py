"""Cost of thermo()'s atmospheric bulk fluxes on the device (nxs_dyn_fluxes) at 2 km.

    python scripts/time_fluxes.py [mesh] [--out DIR]     measure on the GPU, print the figures, write DIR/fluxes.json (default profiles/)

Workload: the arctic case with the inputs of tests/fluxes_ref.py (every branch taken somewhere), the young-ice category, the default configuration.  Wall time per
call of REPS calls enqueued back to back and synchronised once (the calls are asynchronous), median of 7 such batches after a warm-up batch.  Bytes moved: what
the launch must read and write once -- 3 indices and 6 gathered wind values, 18 rows read, 4 drags and 25 rows written per element.  No threshold: the numbers are
the result."""
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
    import fluxes_ref as R
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Ne = lm.num_elements
    tri = lm.indices.reshape(-1, 3).astype(np.int64) - 1
    inp, _ = R.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    f = dict(f, wind=inp["wind"], drag_ui=inp["drag_ui"], drag_ui_young=inp["drag_ui_young"])
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.flux_configure()
    fe.flux_set_atmosphere(tair=inp["tair"], mslp=inp["mslp"], Qsw_in=inp["Qsw_in"], humidity=inp["dair"], longwave=inp["Qlw_in"])
    fe.flux_put(**{k: inp[k] for k in _abi.FLUX_STATE})
    t = []
    for b in range(BATCHES + 1):
        fe.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fe.fluxes()
        fe.synchronize()
        if b:
            t.append((time.perf_counter() - t0) / REPS * 1e6)
    us = float(np.median(np.asarray(t)))
    nbytes = Ne * (3 * 4 + (6 + 18 + 4 + 25) * 8)
    res = {"mesh": kind, "num_elements": int(Ne), "device": dynamics.device_name(0), "calls_per_batch": REPS, "batches": BATCHES, "fluxes_us": us,
           "bytes_per_call": int(nbytes), "GB_per_s": nbytes / us * 1e-3}
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "fluxes.json"), "w"), indent=1)
    print(f"{kind}: {Ne} triangles, {res['device']}")
    print(f"  nxs_dyn_fluxes {us / 1e3:9.4f} ms per call, {nbytes / 1e6:.0f} MB moved, {res['GB_per_s']:.0f} GB/s")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    measure(a.mesh, a.out)
