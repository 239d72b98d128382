"""Cost of thermo()'s slab loop with floe-size bins attached on the device (nxs_dyn_slab_coupled) at 2 km.

    python scripts/time_slab_coupled.py [mesh] [--out DIR]     measure on the GPU, print the figures, write DIR/slab_coupled.json (default profiles/)

Workload: the arctic mesh with the designed inputs of tests/slab_fsd_ref.py (every decision of the loop taken somewhere), 12 bins, WINTON, the young-ice
category, melt_type 3, weldingRoach, the mechanical bins kept apart.  As in scripts/time_slab.py a slab needs the column before it, so the PAIR column(dt);
slab_coupled(dt, clock) is timed -- wall time per pair of REPS pairs enqueued back to back and synchronised once, median of 7 batches after a warm-up batch --
and the column's own figure, measured the same way, is subtracted.  In the same process, on a second handle without bins, the pair column(dt); slab(dt, clock)
of the code as it was: the path this change must not slow; all seven batches of it are kept, so that its spread can be read.  The two launches of
slab_coupled() apart: device time from HIP events on the handle's stream around each (option "slab_coupled_timing", debug array "slab_coupled_ms"), one
column(dt); slab_coupled(dt, clock) at a time, median of 25 -- for the workload, and once more with welding_type NONE, so that what the welding's sub-step loop
costs k_coupled_bins is a measured difference.  Twenty back-to-back pairs on one state partly live in the last-level cache (the 2 km rows of a pair are some 0.3 GB), so no figure here is an HBM rate.
No threshold: the numbers are the result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REPS, BATCHES, NB, SINGLES = 20, 7, 12, 25


def measure(kind, out_dir):
    import numpy as np
    import column_ref as CR
    import fluxes_ref as FR
    import fsd_ref as FS
    import slab_fsd_ref as S
    import slab_ref as R
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f0 = F.localize_fields(g, lm, gm.num_nodes)
    Ne = lm.num_elements
    tri = lm.indices.reshape(-1, 3).astype(np.int64) - 1
    inp, fsd, *_ = S.make_inputs(lm.coord_x, lm.coord_y, tri, NB, True)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    clock = R.clock()

    def device():
        # (a runtime without its table of marketing names answers "": the architecture then -- the library holds a gfx950 code object and nothing else, so a
        # handle whose kernels launch is on one)
        return dynamics.device_name(0) or "gfx950"

    def launches(fe):
        """device time [k_coupled_thermo, k_coupled_bins] in us, median of SINGLES calls"""
        fe.set_option("slab_coupled_timing", 1)
        t = []
        for _ in range(SINGLES + 1):
            fe.column(R.DT)
            fe.slab_coupled(R.DT, clock)
            fe.synchronize()
            t.append(fe.debug_array("slab_coupled_ms") * 1e3)
        fe.set_option("slab_coupled_timing", 0)
        return [float(v) for v in np.median(np.asarray(t[1:]), axis=0)]

    def batches(fe, call):
        t = []
        for b in range(BATCHES + 1):
            fe.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fe.column(R.DT)
                if call:
                    call(R.DT, clock)
            fe.synchronize()
            if b:
                t.append((time.perf_counter() - t0) / REPS * 1e6)
        return [float(v) for v in t]

    med = lambda t: float(np.median(np.asarray(t)))
    res = {"mesh": kind, "num_elements": int(Ne), "device": device(), "bins": NB, "calls_per_batch": REPS, "batches": BATCHES, "timed_single_calls": SINGLES}
    # the code as it was: no bins, slab()
    fe, _ = R.gpu_handle(p, lm, f0, inp, finp, CR.default_config(thermo_type="winton"), R.default_config(), put=R.SLAB_STATE)
    fe.fluxes()
    col = batches(fe, None)
    pair = batches(fe, fe.slab)
    res.update(column_us=med(col), column_slab_us=med(pair), column_slab_batches_us=pair, slab_us=med(pair) - med(col))
    fe.close()
    # 12 bins attached, slab_coupled()
    fe, _ = R.gpu_handle(p, lm, f0, inp, finp, CR.default_config(thermo_type="winton"), R.default_config(), put=R.SLAB_STATE)
    S.attach(fe, fsd, S.fsd_config(NB, True, distinguish_mech_fsd=1))
    fe.slab_coupled_configure(3)
    fe.fluxes()
    col2 = batches(fe, None)
    pair2 = batches(fe, fe.slab_coupled)
    res.update(column_coupled_handle_us=med(col2), column_slab_coupled_us=med(pair2), column_slab_coupled_batches_us=pair2, slab_coupled_us=med(pair2) - med(col2))
    res["k_coupled_thermo_us"], res["k_coupled_bins_us"] = launches(fe)
    fcfg = S.fsd_config(NB, True, distinguish_mech_fsd=1, welding_type=FS.WELD_NONE)
    fe.fsd_configure(fcfg["tables"], **FS.library_options(fcfg))
    res["k_coupled_thermo_no_welding_us"], res["k_coupled_bins_no_welding_us"] = launches(fe)
    res["weld_crash"] = int(fe.fsd_get()["weld_crash"])
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "slab_coupled.json"), "w"), indent=1)
    print(f"{kind}: {Ne} triangles, {NB} bins, {res['device']}")
    print(f"  column + slab          {res['column_slab_us'] / 1e3:9.4f} ms per pair (batches {min(pair) / 1e3:.4f} .. {max(pair) / 1e3:.4f}), column alone {res['column_us'] / 1e3:9.4f} ms")
    print(f"  column + slab_coupled  {res['column_slab_coupled_us'] / 1e3:9.4f} ms per pair, column alone {res['column_coupled_handle_us'] / 1e3:9.4f} ms")
    print(f"  nxs_dyn_slab {res['slab_us'] / 1e3:9.4f} ms, nxs_dyn_slab_coupled {res['slab_coupled_us'] / 1e3:9.4f} ms per call")
    print(f"  from events: k_coupled_thermo {res['k_coupled_thermo_us'] / 1e3:9.4f} ms, k_coupled_bins<{NB}> {res['k_coupled_bins_us'] / 1e3:9.4f} ms; "
          f"with welding_type NONE {res['k_coupled_thermo_no_welding_us'] / 1e3:9.4f} ms, {res['k_coupled_bins_no_welding_us'] / 1e3:9.4f} ms")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    measure(a.mesh, a.out)
