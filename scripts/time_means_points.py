"""Cost of one updateGridMean() on a LOADED Moorings grid plus the fetch of the gridded means: the device route (nxs_dyn_means_points_update + _get) against the
host route it replaces, at 2 km, on a TOPAZ-sized curvilinear grid of 800 x 760 points with 8 elemental and 6 nodal variables (three vector pairs).

    python scripts/time_means_points.py [mesh] [--out DIR]     measure on the GPU, print the figures (the block of DESIGN section 6m), write DIR/means_points.json

Both routes run in the same process on the same handle and must give EQUAL BITS (asserted):
  1. the route it replaces: nxs_dyn_means_get of both accumulator sets and the fetch of M_UM (nxs_dyn_get_state with only UM asked for), the displaced
     coordinates, three nxs_interp_mesh_to_mesh_2d calls with host arrays (proc mask, elemental rows, nodal rows; isdefault = true, 0.), then rotateVectors, the
     product with the proc mask, the accumulation and the ice-mask rule in numpy over whole arrays -- with its parts timed separately
  2. nxs_dyn_means_points_update + nxs_dyn_means_points_get (synchronised), with the displaced locator STALE before every call (what happens after a step) ...
  3. ... and with the locator current (a second Moorings object, or the drifters, built it already)
  4. the split of (2) by option "drifters_timing": locator build, kernel [device ms]
  5. a device-to-device copy that moves the bytes the kernel must move at least (its operands counted once; the locator's own traffic is not counted)
Wall time per call, median of BATCHES batches after a warm-up batch.  No threshold: the numbers are the result."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = 5
REPS = {"host_route": 1, "device_stale": 5, "device_current": 20, "copy": 200}
NU, NV = 800, 760
ELEMENTAL = ("conc", ("thick", True), "snow", "damage", "ridge_ratio", "conc_cons", "sigma_11", "ice_mask")
NODAL = ("VT_x", ("VT_y", True), "VT_x", "VT_y", "VT_x", "VT_y")
EL_MASK, NOD_MASK, ICE_COL = (0, 1, 0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), 7
PAIRS = ((0, 1), (2, 3), (4, 5))
MISS, ROTATION_ANGLE = -1e14, -45. * 3.141592653589793 / 180.


def grid(np, x, y):
    """a rotated, stretched NU x NV grid reaching 10 % beyond the mesh's box; gridLON in degrees"""
    U, V = np.meshgrid(np.linspace(-1., 1., NU), np.linspace(-1., 1., NV), indexing="ij")
    t = np.deg2rad(20.)
    X = np.cos(t) * U * (1. + 0.10 * V) - np.sin(t) * V * (1. + 0.15 * U * U)
    Y = np.sin(t) * U * (1. - 0.20 * V * V) + np.cos(t) * V * (1. + 0.05 * U)
    X, Y = X / np.abs(X).max(), Y / np.abs(Y).max()
    gx = (0.5 * (x.min() + x.max()) + 0.55 * np.ptp(x) * X).ravel()
    gy = (0.5 * (y.min() + y.max()) + 0.55 * np.ptp(y) * Y).ravel()
    return np.ascontiguousarray(gx), np.ascontiguousarray(gy), np.ascontiguousarray(np.degrees(np.arctan2(gx, -gy)) + 45.)


def measure(kind, out_dir):
    import numpy as np
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M
    from nextsim_amd.interp import InterpFromMeshToMesh2dx

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    lm = M.localize(gm, 1)[0]
    Nn, Ne = lm.num_nodes, lm.num_elements
    rng = np.random.default_rng(0)
    state = {k: rng.standard_normal(2 * Nn) for k in _abi.STATE_NODAL}
    state.update({k: rng.random(Ne) for k in _abi.STATE_ELEMENT + _abi.STATE_INPUT})
    tri = lm.indices.reshape(-1, 3) - 1
    xs, ys = lm.coord_x[tri], lm.coord_y[tri]
    h = float(np.sqrt(2. * (0.5 * np.abs((xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (xs[:, 2] - xs[:, 0]) * (ys[:, 1] - ys[:, 0]))).min()))
    Lx = max(np.ptp(lm.coord_x), np.ptp(lm.coord_y))
    state["UM"] = np.concatenate([0.04 * h * np.sin(3. * lm.coord_x / Lx), 0.04 * h * np.cos(2. * lm.coord_y / Lx)])
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    fe.means_configure(ELEMENTAL, NODAL)
    fe.put_state(state)
    fe.means_update(1.0)
    fe.means_update(0.5)
    gx, gy, lon = grid(np, lm.coord_x, lm.coord_y)
    G = gx.size
    n_el, n_nod = len(ELEMENTAL), len(NODAL)
    fe.means_points_set(gx, gy, MISS, "north_east", gridLON=lon, rotation_angle=ROTATION_ANGLE, pairs=PAIRS)
    cs = np.array([math.cos(ROTATION_ANGLE - float(v) * 3.141592653589793 / 180) for v in lon])
    sn = np.array([math.sin(ROTATION_ANGLE - float(v) * 3.141592653589793 / 180) for v in lon])
    L = dynamics.load_library()
    parts = {}

    def timed(name, f):
        t0 = time.perf_counter()
        out = f()
        parts.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
        return out

    def fetch_um():
        um = np.empty(2 * Nn)
        s = _abi.State()
        s.UM = _abi.dptr(um)
        assert L.nxs_dyn_get_state(fe.h, C.byref(s)) == 0
        return um

    def restale():
        """M_UM given again (a partial nxs_dyn_put_state): the displaced locator is stale, as after a step"""
        s = _abi.State()
        s.UM = _abi.dptr(state["UM"])
        assert L.nxs_dyn_put_state(fe.h, C.byref(s)) == 0

    ge_h, gn_h = np.zeros((n_el, G)), np.zeros((n_nod, G))
    ones = np.ones(Ne)      # (one rank: every element is owned)

    def host_route():
        el, nod, _, _ = timed("means_get", fe.means_get)
        um = timed("fetch_UM", fetch_um)
        x, y = timed("displace", lambda: (lm.coord_x + um[:Nn], lm.coord_y + um[Nn:]))
        pm = timed("interp_proc_mask", lambda: InterpFromMeshToMesh2dx(lm.indices, x, y, ones[:, None], gx, gy, True, 0.))[:, 0]
        oe = timed("interp_elemental", lambda: InterpFromMeshToMesh2dx(lm.indices, x, y, el, gx, gy, True, 0.))
        on = timed("interp_nodal", lambda: InterpFromMeshToMesh2dx(lm.indices, x, y, nod, gx, gy, True, 0.))

        def arithmetic():
            proc_mask = np.zeros(G) + pm
            for nv in range(n_el):
                ge_h[nv] += oe[:, nv]
            for first, second in PAIRS:
                sel = on[:, first] != MISS
                u = cs * on[:, first] - sn * on[:, second]
                v = sn * on[:, first] + cs * on[:, second]
                on[sel, first] = u[sel]
                on[sel, second] = v[sel]
            for nv in range(n_nod):
                gn_h[nv] += on[:, nv] * proc_mask
            for g, masks in ((gn_h, NOD_MASK), (ge_h, EL_MASK)):
                for nv, m in enumerate(masks):
                    if m:
                        g[nv][(ge_h[ICE_COL] <= 0.) & (g[nv] != MISS)] = 0.
        timed("numpy_arithmetic", arithmetic)

    def batch_list(call, reps, before_each=None):
        t = []
        for b in range(BATCHES + 1):
            tb = 0.
            for _ in range(reps):
                if before_each:
                    before_each()
                fe.synchronize()
                t0 = time.perf_counter()
                call()
                tb += time.perf_counter() - t0
            if b:
                t.append(tb / reps * 1e3)
            else:
                parts.clear()
        return float(np.median(np.asarray(t)))

    def device_route():
        fe.means_points_update()
        return fe.means_points_get()

    # equal bits first: one call of each route from zeroed accumulators
    host_route()
    ge_d, gn_d, _, _ = device_route()
    same = bool(np.array_equal(ge_d.view(np.uint64), ge_h.view(np.uint64)) and np.array_equal(gn_d.view(np.uint64), gn_h.view(np.uint64)))
    found = int((InterpFromMeshToMesh2dx(lm.indices, lm.coord_x, lm.coord_y, ones[:, None], gx, gy, True, 0.)[:, 0] > 0).sum())
    assert same, "the two routes differ"

    host_ms = batch_list(host_route, REPS["host_route"])
    part_ms = {k: float(np.median(np.asarray(v))) for k, v in parts.items()}
    stale_ms = batch_list(device_route, REPS["device_stale"], restale)
    current_ms = batch_list(device_route, REPS["device_current"])
    get_ms = batch_list(fe.means_points_get, REPS["device_current"])
    fe.set_option("drifters_timing", 1)
    split = []
    for _ in range(BATCHES):
        restale()
        fe.means_points_update()
        split.append(fe.debug_array("means_points_ms"))
    build_ms, kernel_stale_ms = (float(v) for v in np.median(np.asarray(split), axis=0))
    kern = []
    for _ in range(BATCHES):
        fe.means_points_update()
        kern.append(fe.debug_array("means_points_ms")[1])
    kernel_ms = float(np.median(np.asarray(kern)))
    fe.set_option("drifters_timing", 0)
    # the bytes the kernel must move at least: coordinates, cos, sin, one elemental row and three nodal rows per point, the grid rows read and written
    kernel_bytes = G * 8 * (4 + n_el + 3 * n_nod + 2 * (n_el + n_nod))
    n_copy = kernel_bytes // 2
    src, dst = C.c_void_p(), C.c_void_p()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.hipFree.argtypes = [C.c_void_p]
    L.hipDeviceSynchronize.argtypes = []
    assert L.hipMalloc(C.byref(src), n_copy) == 0 and L.hipMalloc(C.byref(dst), n_copy) == 0
    t = []
    for b in range(BATCHES + 1):
        L.hipDeviceSynchronize()
        t0 = time.perf_counter()
        for _ in range(REPS["copy"]):
            L.hipMemcpyAsync(dst, src, n_copy, 3, None)      # hipMemcpyDeviceToDevice
        L.hipDeviceSynchronize()
        if b:
            t.append((time.perf_counter() - t0) / REPS["copy"] * 1e3)
    copy_ms = float(np.median(np.asarray(t)))
    L.hipFree(src); L.hipFree(dst)
    res = {"mesh": kind, "num_nodes": int(Nn), "num_elements": int(Ne), "device": dynamics.device_name(0), "batches": BATCHES, "calls_per_batch": REPS,
           "grid": [NU, NV], "grid_points": int(G), "grid_points_in_the_mesh": found, "num_elemental": n_el, "num_nodal": n_nod, "pairs": len(PAIRS),
           "equal_bits": same, "host_route_ms": host_ms, "host_route_parts_ms": part_ms,
           "device_route_stale_locator_ms": stale_ms, "device_route_current_locator_ms": current_ms, "points_get_ms": get_ms,
           "ratio_host_over_device_stale": host_ms / stale_ms, "ratio_host_over_device_current": host_ms / current_ms,
           "locator_build_device_ms": build_ms, "kernel_device_ms": kernel_ms, "kernel_after_a_build_device_ms": kernel_stale_ms,
           "kernel_min_bytes": int(kernel_bytes), "kernel_GB_per_s": kernel_bytes / kernel_ms * 1e-6, "copy_same_bytes_ms": copy_ms, "copy_GB_per_s": kernel_bytes / copy_ms * 1e-6,
           "download_bytes_device_route": int((n_el + n_nod) * G * 8), "download_bytes_host_route": int((n_el * Ne + n_nod * Nn + 2 * Nn) * 8)}
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "means_points.json"), "w"), indent=1)
    print(f"{kind}: {Nn} nodes, {Ne} triangles, {res['device']}; grid {NU} x {NV} = {G} points ({found} in the mesh), {n_el} elemental + {n_nod} nodal variables, {len(PAIRS)} pairs")
    print(f"  1. host route                                   {host_ms:9.2f} ms  (" + ", ".join(f"{k} {v:.2f}" for k, v in part_ms.items()) + ")")
    print(f"  2. points_update + points_get, locator stale    {stale_ms:9.2f} ms  host / device = {host_ms / stale_ms:.1f}")
    print(f"  3. points_update + points_get, locator current  {current_ms:9.2f} ms  host / device = {host_ms / current_ms:.1f}   (points_get alone {get_ms:.2f} ms)")
    print(f"  4. device time: locator build {build_ms:.3f} ms, kernel {kernel_ms:.3f} ms ({res['kernel_GB_per_s']:.0f} GB/s of {kernel_bytes / 1e6:.1f} MB)")
    print(f"  5. device-to-device copy of the same bytes      {copy_ms:9.4f} ms ({res['copy_GB_per_s']:.0f} GB/s)")
    print(f"  equal bits: {same}")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    measure(a.mesh, a.out)
