"""Cost of thermo()'s ten element forcing rows per model step and per forcing interval, uploaded by the host or kept on the device (nxs_dyn_thermo_forcing_*), at 2 km.

    python scripts/time_thermo_forcing.py [mesh] [--out DIR]     measure on the GPU, print the figures, write DIR/thermo_forcing.json (default profiles/)

Per model step:
  1. today's route: nxs_dyn_flux_set_atmosphere + nxs_dyn_column_set_forcing with ten [Ne] host rows (what a host must do when its datasets are interpolated
     linearly in time: the bits change every step) -- with pageable host rows and with page-locked ones (option pin_host, the rate scripts/time_copies.py reports)
  2. nxs_dyn_thermo_forcing_time: eight LINEAR and two STEP rows (snowfr and mld: datasets with one snapshot), one launch
Per forcing interval (a 0.25-degree-like 1440 x 361 grid, seven columns: two snapshots of three variables and one skipped, as one loadDataset call carries them):
  3. nxs_interp_grid_to_mesh (InterpFromGridToMeshx to host arrays) + the de-interleaving of its [Ne][N_data] result + nxs_dyn_thermo_forcing_pair
  4. nxs_dyn_thermo_forcing_ingest
(1) and (3) run on the same build in the same process and are the baseline of (2) and (4).  Wall time per call, a batch of calls enqueued back to back and
synchronised once (each batch about 0.2 s of work: 100 uploads, 4000 blends, 8 host routes, 300 ingests), median of BATCHES batches after a warm-up batch.  Back
to back the blend's 326 MB partly live in the 256 MiB last-level cache: its rate is not an HBM rate.  Bytes of the blend: per LINEAR row two rows read and one
written, per STEP row one and one (30 rows x 8 B x Ne when all ten are LINEAR).  No threshold: the numbers are the result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = 5
REPS = {"upload": 100, "blend": 4000, "host_route": 8, "ingest": 300}


def measure(kind, out_dir):
    import numpy as np
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M
    from nextsim_amd.interp import InterpFromGridToMeshx

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE), gm, alea_factor=0.33)
    lm = M.localize(gm, 1)[0]
    Ne = lm.num_elements
    rng = np.random.default_rng(0)
    s0 = {k: rng.normal(size=Ne) for k in _abi.TF_ROWS}
    s1 = {k: rng.normal(size=Ne) for k in _abi.TF_ROWS if k not in ("snow", "mld")}
    host = {k: rng.normal(size=Ne) for k in _abi.TF_ROWS}
    tab = {k: dict(mode="linear" if k in s1 else "step", fcoeff0=0.3, fcoeff1=0.7, factor=0.9, bias=0.1) for k in _abi.TF_ROWS}
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)

    def batches(call, reps):
        t = []
        for b in range(BATCHES + 1):
            fe.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            fe.synchronize()
            if b:
                t.append((time.perf_counter() - t0) / reps * 1e6)
        return float(np.median(np.asarray(t)))

    def upload():
        fe.flux_set_atmosphere(**{k: host[k] for k in _abi.FLUX_ATMOSPHERE})
        fe.column_set_forcing(**{k: host[k] for k in _abi.COL_FORCING})

    upload_us = batches(upload, REPS["upload"])
    fe.set_option("pin_host", 1)
    upload_pinned_us = batches(upload, REPS["upload"])
    fe.set_option("pin_host", 0)
    fe.thermo_forcing_pair(s0, s1)
    blend_us = batches(lambda: fe.thermo_forcing_time(tab), REPS["blend"])
    lin = len(s1)
    blend_bytes = Ne * 8 * (3 * lin + 2 * (len(s0) - lin))

    # the forcing interval: one dataset's grid onto the element barycentres
    tri = lm.indices.reshape(-1, 3).astype(np.int64) - 1
    bx, by = np.ascontiguousarray(lm.coord_x[tri].mean(1)), np.ascontiguousarray(lm.coord_y[tri].mean(1))
    N, M_, N_data = 1440, 361, 7
    xs = np.linspace(bx.min() - 1e4, bx.max() + 1e4, N); ys = np.linspace(by.max() + 1e4, by.min() - 1e4, M_)
    data = rng.normal(size=(M_, N, N_data))
    row = ["tair", "mslp", "Qsw_in", None, "tair", "mslp", "Qsw_in"]
    snap = [0, 0, 0, 0, 1, 1, 1]

    def host_route():
        out = InterpFromGridToMeshx(xs, ys, data, bx, by, 1e8, 1)
        cols = [np.ascontiguousarray(out[:, j]) for j in range(N_data)]
        fe.thermo_forcing_pair({row[j]: cols[j] for j in range(N_data) if row[j] and snap[j] == 0}, {row[j]: cols[j] for j in range(N_data) if row[j] and snap[j] == 1})

    fe.thermo_forcing_targets(0, bx, by)
    host_route_us = batches(host_route, REPS["host_route"])
    ingest_us = batches(lambda: fe.thermo_forcing_ingest(0, xs, ys, data, row, snap, 1e8, 1), REPS["ingest"])
    res = {"mesh": kind, "num_elements": int(Ne), "device": dynamics.device_name(0), "batches": BATCHES, "calls_per_batch": REPS,
           "step_upload_ten_rows_us": upload_us, "step_upload_ten_rows_pinned_us": upload_pinned_us, "step_upload_bytes": int(Ne * 8 * 10),
           "step_upload_GB_per_s": Ne * 80 / upload_us * 1e-3, "step_upload_pinned_GB_per_s": Ne * 80 / upload_pinned_us * 1e-3,
           "step_thermo_forcing_time_us": blend_us, "blend_linear_rows": lin, "blend_step_rows": len(s0) - lin, "blend_bytes": int(blend_bytes),
           "blend_GB_per_s": blend_bytes / blend_us * 1e-3,
           "interval_grid": [M_, N, N_data], "interval_grid_to_mesh_plus_pair_us": host_route_us, "interval_thermo_forcing_ingest_us": ingest_us}
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "thermo_forcing.json"), "w"), indent=1)
    print(f"{kind}: {Ne} triangles, {res['device']}")
    print(f"  per step     1. ten host rows through the old calls  {upload_us / 1e3:9.4f} ms pageable ({res['step_upload_GB_per_s']:.1f} GB/s), "
          f"{upload_pinned_us / 1e3:9.4f} ms page-locked ({res['step_upload_pinned_GB_per_s']:.1f} GB/s: the copy rate)")
    print(f"               2. nxs_dyn_thermo_forcing_time           {blend_us / 1e3:9.4f} ms, {blend_bytes / 1e6:.0f} MB moved, {res['blend_GB_per_s']:.0f} GB/s")
    print(f"  per interval 3. nxs_interp_grid_to_mesh + pair        {host_route_us / 1e3:9.3f} ms ({M_} x {N} x {N_data})")
    print(f"               4. nxs_dyn_thermo_forcing_ingest         {ingest_us / 1e3:9.3f} ms")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    measure(a.mesh, a.out)
