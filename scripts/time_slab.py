"""Cost of thermo()'s slab loop from new ice to tracers on the device (nxs_dyn_slab) at 2 km.

    python scripts/time_slab.py [mesh] [--out DIR]     measure on the GPU, print the figures, write DIR/slab.json (default profiles/)

Workload: the arctic mesh with the designed inputs of tests/slab_ref.py (every decision of the loop taken somewhere), WINTON, the young-ice category, the default
configuration (newice_type 4, melt_type 2, no assimilation flux, no ponds, no temperature-dependent healing).  A slab() needs the column() before it, so the PAIR
column(dt); slab(dt, clock) is timed -- wall time per pair of REPS pairs enqueued back to back and synchronised once (the calls are asynchronous), median of 7
such batches after a warm-up batch -- and the column's own figure, measured the same way in the same process, is subtracted; the state of one pair feeds the
next, as in a run.  Bytes moved: what the launch must read and write once per element in that configuration -- 59 rows read (18 flux rows, 19 column rows,
precip, conc, thick, ridge_ratio, the young ice's three, conc_myi, thick_myi, sst, sss, tice0/1/2 and eight rows of the slab state) and 51 written (the 29 rows,
conc, thick, snow_thick, ridge_ratio, the young ice's three, conc_myi, thick_myi, sst, sss, tice0/1/2, the eight rows of the slab state) plus the 4-byte branch
word.  No threshold: the numbers are the result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS, BATCHES = 20, 7
ROWS_READ, ROWS_WRITTEN = 59, 51


def measure(kind, out_dir):
    import numpy as np
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
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    fe, f = R.gpu_handle(p, lm, f, inp, finp, CR.default_config(thermo_type="winton"), R.default_config(), put=R.SLAB_STATE)
    clock = R.clock()
    fe.fluxes()

    def batches(pair):
        t = []
        for b in range(BATCHES + 1):
            fe.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fe.column(R.DT)
                if pair:
                    fe.slab(R.DT, clock)
            fe.synchronize()
            if b:
                t.append((time.perf_counter() - t0) / REPS * 1e6)
        return float(np.median(np.asarray(t)))

    column_us = batches(False)
    pair_us = batches(True)
    us = pair_us - column_us
    nbytes = Ne * ((ROWS_READ + ROWS_WRITTEN) * 8 + 4)
    res = {"mesh": kind, "num_elements": int(Ne), "device": dynamics.device_name(0), "calls_per_batch": REPS, "batches": BATCHES, "pair_us": pair_us,
           "column_us": column_us, "slab_us": us, "rows_read": ROWS_READ, "rows_written": ROWS_WRITTEN, "bytes_per_element": (ROWS_READ + ROWS_WRITTEN) * 8 + 4,
           "bytes_per_call": int(nbytes), "GB_per_s": nbytes / us * 1e-3}
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "slab.json"), "w"), indent=1)
    print(f"{kind}: {Ne} triangles, {res['device']}")
    print(f"  column + slab {pair_us / 1e3:9.4f} ms per pair, column alone {column_us / 1e3:9.4f} ms")
    print(f"  nxs_dyn_slab  {us / 1e3:9.4f} ms per call, {nbytes / 1e6:.0f} MB moved, {res['GB_per_s']:.0f} GB/s")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    measure(a.mesh, a.out)
