"""Cost of one reload of the dynamics' wind dataset and of the per-step time blend, on the host route and on the device (nxs_dyn_forcing_*), at 2 km.

    python scripts/time_nodal_forcing.py [mesh] [--out DIR]     measure on the GPU, print the figures (the block of DESIGN section 6l), write DIR/nodal_forcing.json

Per reload (an ERA5-like 281 x 1440 lat-lon grid, 0.25 degrees, 90 N .. 20 N, cyclic in longitude; two snapshots of the wind as east/north pairs: four columns):
  1. the route it replaces, timed in the same run: transformData on the host (the library's host body of forward_mapx over whole arrays, the rest in numpy:
     NOT the reference's scalar loop, which is slower), the wrap column in numpy, nxs_interp_grid_to_mesh to host arrays at the nodes, the de-interleaving, and
     nxs_dyn_set_forcing_pair (six nodal vectors and the depth up) -- with its parts timed separately
  2. nxs_dyn_forcing_ingest with the same grid, pair descriptor and targets
Per step:
  3. nxs_dyn_set_forcing_time (one pair of coefficients)        4. nxs_dyn_set_forcing_time_rows (all three groups LINEAR)
  5. a device-to-device copy that moves the same bytes as (4): 10 Nn doubles read, 5 Nn written
The targets are synthetic (lon, lat) of the nodes (the mesh's own polar coordinates); convertTargetXY stays the host's and is not timed.  Wall time per call, a
batch of calls enqueued back to back and synchronised once (about 0.15 s of work), median of BATCHES batches after a warm-up batch; (3) and (4) alternate twice.
Back to back the blend's 88 MB live in the 256 MiB last-level cache: its rate is not an HBM rate.  No threshold: the numbers are the result."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = 5
REPS = {"host_route": 2, "ingest": 300, "blend": 10000, "copy": 10000}      # about 0.15 s of work per batch


def host_transform(dynamics, m, data, lat, lon, pairs):
    """transformData's east/north branch and pole row over whole arrays (externaldata.cpp:1155-1243); the projection is the library's host body"""
    import numpy as np
    out = data.copy()
    M_, N = data.shape[:2]
    LAT, LON = np.repeat(lat, N), np.tile(lon, M_)
    R, PI = 6371.228 * 1000., 3.141592653589793
    x, y = dynamics.mapx_forward(m, LAT, LON)
    for j0, j1 in pairs:
        t0, t1 = out[:, :, j0].ravel(), out[:, :, j1].ravel()
        below = LAT < 90.
        with np.errstate(divide="ignore", invalid="ignore"):
            d0 = np.where(below, t0 / (R * np.cos(LAT * PI / 180.)) * 180. / PI, 0.)
        d1 = np.where(below, t1 / R * 180. / PI, 0.)
        lat_b, lon_b = LAT + d1, LON + d0
        lon_b = lon_b - 360. * np.floor(lon_b / 360.)
        xb, yb = dynamics.mapx_forward(m, lat_b, lon_b)
        n0, n1 = xb - x, yb - y
        speed, new = np.hypot(t0, t1), np.hypot(n0, n1)
        with np.errstate(divide="ignore", invalid="ignore"):
            n0 = np.where(new > 0., n0 / new * speed, n0)
            n1 = np.where(new > 0., n1 / new * speed, n1)
        n0, n1 = n0.reshape(M_, N), n1.reshape(M_, N)
        for row, nxt in ((0, 1), (M_ - 1, M_ - 2)):
            if lat[row] == 90.:
                n0[row], n1[row] = n0[nxt].sum() / N, n1[nxt].sum() / N
        out[:, :, j0], out[:, :, j1] = n0, n1
    return out


def measure(kind, out_dir):
    import numpy as np
    from nextsim_amd import dynamics, forcing as F, mesh as M
    from nextsim_amd.interp import InterpFromGridToMeshx

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    lm = M.localize(gm, 1)[0]
    Nn, Ne = lm.num_nodes, lm.num_elements
    rng = np.random.default_rng(0)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    L = dynamics.load_library()

    def batch_list(call, reps, after_warm_up=None):
        t = []
        for b in range(BATCHES + 1):
            fe.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            fe.synchronize()
            if b:
                t.append((time.perf_counter() - t0) / reps * 1e3)
            elif after_warm_up:
                after_warm_up()
        return t

    def batches(call, reps, after_warm_up=None):
        return float(np.median(np.asarray(batch_list(call, reps, after_warm_up))))

    # the dataset: ERA5-like, latitudes descending from the pole, cyclic in longitude
    M_, N, N_data = 281, 1440, 4
    lat, lon = 90. - 0.25 * np.arange(M_), 0.25 * np.arange(N)
    data = rng.uniform(-25., 25., (M_, N, N_data))
    pairs = [(0, 1, True), (2, 3, True)]
    m = dynamics.mapx_polar_north()
    rx = np.degrees(np.arctan2(lm.coord_x, -lm.coord_y)) % 360.                        # synthetic node longitudes ...
    r = np.hypot(lm.coord_x, lm.coord_y)
    ry = 90. - 65. * r / r.max()                                                        # ... and latitudes, 25 N .. 90 N
    depth = np.full(Ne, 1000.)
    ocean, ssh = np.zeros(2 * Nn), np.zeros(Nn)
    parts = {}

    def timed(name, f):
        t0 = time.perf_counter()
        out = f()
        parts.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return out

    def host_route():
        g = timed("transform", lambda: host_transform(dynamics, m, data, lat, lon, [(0, 1), (2, 3)]))
        g = timed("wrap", lambda: np.concatenate([g, g[:, :1]], axis=1))
        out = timed("grid_to_mesh", lambda: InterpFromGridToMeshx(np.append(lon, lon[-1] + (lon[-1] - lon[-2])), lat, g, rx, ry, 1e8, 1))
        w0, w1 = timed("deinterleave", lambda: (np.concatenate([out[:, 0], out[:, 1]]), np.concatenate([out[:, 2], out[:, 3]])))
        timed("set_forcing_pair", lambda: (fe.set_forcing_pair(dict(wind=w0, ocean=ocean, ssh=ssh, element_depth=depth), dict(wind=w1, ocean=ocean, ssh=ssh, element_depth=depth)),
                                          fe.synchronize()))

    host_ms = batches(host_route, REPS["host_route"], parts.clear)      # (the parts are medians over the calls of the timed batches)
    part_ms = {k: float(np.median(np.asarray(v))) for k, v in parts.items()}
    fe.forcing_targets(0, rx, ry)
    vec = dict(pairs=pairs, lat=lat, lon=lon, map=m)
    ingest = lambda: fe.forcing_ingest(0, lon, lat, data, ["wind_u", "wind_v", "wind_u", "wind_v"], [0, 0, 1, 1], 1e8, 1, False, True, False, vec)  # noqa: E731
    ingest_ms = batches(ingest, REPS["ingest"])
    fe.set_option("pin_host", 1)
    ingest_pinned_ms = batches(ingest, REPS["ingest"])
    fe.set_option("pin_host", 0)
    # the two routes agree: the host route's snapshots against the ingest's (numpy's transform is not the device's bits)
    host_route()
    h0 = fe.forcing_get(0, ["wind_u", "wind_v"])
    ingest()
    d0 = fe.forcing_get(0, ["wind_u", "wind_v"])
    agree = max(float(np.abs(h0[k] - d0[k]).max()) for k in h0)

    rows = {g: dict(mode="linear", fcoeff0=0.3, fcoeff1=0.7) for g in ("wind", "ocean", "ssh")}
    t_time, t_rows = [], []
    for _ in range(2):      # the two blends alternate: the median over both rounds
        t_time += batch_list(lambda: fe.set_forcing_time(0.3, 0.7), REPS["blend"])
        t_rows += batch_list(lambda: fe.set_forcing_time_rows(rows), REPS["blend"])
    time_ms, rows_ms = float(np.median(np.asarray(t_time))), float(np.median(np.asarray(t_rows)))
    n_copy = (15 * Nn) // 2
    src, dst = C.c_void_p(), C.c_void_p()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.hipFree.argtypes = [C.c_void_p]
    assert L.hipMalloc(C.byref(src), n_copy * 8) == 0 and L.hipMalloc(C.byref(dst), n_copy * 8) == 0
    L.hipDeviceSynchronize.argtypes = []

    def copy_batches():
        t = []
        for b in range(BATCHES + 1):
            L.hipDeviceSynchronize()
            t0 = time.perf_counter()
            for _ in range(REPS["copy"]):
                L.hipMemcpyAsync(dst, src, n_copy * 8, 3, None)      # hipMemcpyDeviceToDevice
            L.hipDeviceSynchronize()
            if b:
                t.append((time.perf_counter() - t0) / REPS["copy"] * 1e3)
        return float(np.median(np.asarray(t)))
    copy_ms = copy_batches()
    L.hipFree(src); L.hipFree(dst)
    blend_bytes = 15 * Nn * 8
    res = {"mesh": kind, "num_nodes": int(Nn), "num_elements": int(Ne), "device": dynamics.device_name(0), "batches": BATCHES, "calls_per_batch": REPS,
           "grid": [M_, N, N_data], "forward_mapx_calls_per_reload": 2 * M_ * N * 2, "upload_bytes_device_route": int(data.nbytes), "upload_bytes_host_route": int(10 * Nn * 8 + Ne * 8),
           "reload_host_route_ms": host_ms, "reload_host_route_parts_ms": part_ms, "reload_forcing_ingest_ms": ingest_ms, "reload_forcing_ingest_pinned_ms": ingest_pinned_ms,
           "reload_ratio_host_over_device": host_ms / ingest_ms, "routes_largest_difference_m_per_s": agree,
           "step_set_forcing_time_ms": time_ms, "step_set_forcing_time_rows_ms": rows_ms, "step_copy_same_bytes_ms": copy_ms, "blend_bytes": int(blend_bytes),
           "blend_rows_GB_per_s": blend_bytes / rows_ms * 1e-6, "blend_time_GB_per_s": blend_bytes / time_ms * 1e-6, "copy_GB_per_s": blend_bytes / copy_ms * 1e-6,
           "ratio_time_over_rows": time_ms / rows_ms, "ratio_rows_over_copy": rows_ms / copy_ms}
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "nodal_forcing.json"), "w"), indent=1)
    print(f"{kind}: {Nn} nodes, {Ne} triangles, {res['device']}; grid {M_} x {N}, {N_data} columns (two snapshots of one east/north pair), cyclic longitude")
    print(f"  per reload  1. host route                          {host_ms:9.2f} ms  (" + ", ".join(f"{k} {v:.2f}" for k, v in part_ms.items()) + ")")
    print(f"              2. nxs_dyn_forcing_ingest               {ingest_ms:9.2f} ms pageable, {ingest_pinned_ms:.2f} ms page-locked; host / device = {host_ms / ingest_ms:.1f}")
    print(f"                 the two routes' snapshots differ by at most {agree:.2e} m/s")
    print(f"  per step    3. nxs_dyn_set_forcing_time             {time_ms:9.4f} ms ({res['blend_time_GB_per_s']:.0f} GB/s)")
    print(f"              4. nxs_dyn_set_forcing_time_rows        {rows_ms:9.4f} ms ({res['blend_rows_GB_per_s']:.0f} GB/s); (3) / (4) = {time_ms / rows_ms:.2f}")
    print(f"              5. device-to-device copy, same bytes    {copy_ms:9.4f} ms ({res['copy_GB_per_s']:.0f} GB/s); (4) / (5) = {rows_ms / copy_ms:.2f}")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    measure(a.mesh, a.out)
