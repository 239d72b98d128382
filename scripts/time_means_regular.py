"""Cost of one updateGridMean() on the REGULAR Moorings grid plus the fetch of the gridded means: the device route (nxs_dyn_means_regular_update + _get) against
the route through the host it stands beside (nxs_dyn_means_to_grid), at 2 km with the reference's default spacing of 10 km (model/options.cpp:144) over the mesh's
box and its default variable list (options.cpp:150: conc, thick, snow, conc_young, h_young, hs_young, velocity -- the velocity is masked, so ice_mask joins).

    python scripts/time_means_regular.py [mesh] [--out DIR]     measure on the GPU, print the figures (the block of DESIGN section 6r), write DIR/means_regular.json

Both routes run in the same process on the same handle and must give EQUAL BITS from zeroed accumulators (asserted; rotation NONE, the host route has no other):
  1. nxs_dyn_means_to_grid into zeroed host arrays: the fetch of M_UM, the host loops over nodes and elements, three uploads, three launches, three copies back
  2. nxs_dyn_means_regular_update + nxs_dyn_means_regular_get (synchronised)
  3. nxs_dyn_means_regular_update alone, synchronised, and nxs_dyn_means_regular_get alone
  4. the split of the update by option "means_timing": the search (memset + k_means_regular_hits), the gather (k_means_regular_gather) [device ms]
  5. the same with rotation NORTH_EAST (cos / sin read, one pair rotated)
Wall time per call, median of BATCHES batches after a warm-up batch.  No threshold: the numbers are the result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = 5
REPS = {"host_route": 2, "device_route": 400}
SPACING = 10e3
ELEMENTAL = ("conc", "thick", "snow", "conc_young", "h_young", "hs_young", "ice_mask")
NODAL = (("VT_x", True), ("VT_y", True))
PAIRS = ((0, 1),)
MISS, ROTATION_ANGLE = -1e14, -45. * 3.141592653589793 / 180.


def measure(kind, out_dir, spacing):
    import numpy as np
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

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
    # the grid of initRegularGrid: the mesh's box at the spacing asked for
    xmin, ymax = float(lm.coord_x.min()), float(lm.coord_y.max())
    ncols, nrows = int(np.ceil(np.ptp(lm.coord_x) / spacing)), int(np.ceil(np.ptp(lm.coord_y) / spacing))
    G = ncols * nrows
    n_el, n_nod = len(ELEMENTAL), len(NODAL)
    gx = np.tile(xmin + spacing * np.arange(ncols), nrows)
    gy = np.repeat((ymax - spacing * np.arange(nrows))[::-1], ncols)
    lon = np.degrees(np.arctan2(gx, -gy)) + 45.

    def batch_list(call, reps):
        t = []
        for b in range(BATCHES + 1):
            tb = 0.
            for _ in range(reps):
                fe.synchronize()
                t0 = time.perf_counter()
                call()
                tb += time.perf_counter() - t0
            if b:
                t.append(tb / reps * 1e3)
        return float(np.median(np.asarray(t)))

    def host_route():
        return fe.means_to_grid(xmin, ymax, spacing, ncols, nrows, MISS)

    def device_route():
        fe.means_regular_update()
        return fe.means_regular_get()

    def update_sync():
        fe.means_regular_update()
        fe.synchronize()

    def split():
        fe.set_option("means_timing", 1)
        rows = []
        for _ in range(BATCHES * 4):
            fe.means_regular_update()
            rows.append(fe.debug_array("means_regular_ms"))
        fe.set_option("means_timing", 0)
        return [float(v) for v in np.median(np.asarray(rows), axis=0)]

    fe.means_regular_set(xmin, ymax, spacing, ncols, nrows, MISS)
    lsm = fe.means_regular_lsm()
    # equal bits first: one call of each route from zeroed accumulators
    ge_h, gn_h = host_route()
    ge_d, gn_d, _, _ = device_route()
    same = bool(np.array_equal(ge_d.view(np.uint64), ge_h.view(np.uint64)) and np.array_equal(gn_d.view(np.uint64), gn_h.view(np.uint64)))
    assert same, "the two routes differ"
    host_ms = batch_list(host_route, REPS["host_route"])
    device_ms = batch_list(device_route, REPS["device_route"])
    update_ms = batch_list(update_sync, REPS["device_route"])
    get_ms = batch_list(fe.means_regular_get, REPS["device_route"])
    hits_ms, gather_ms = split()
    fe.means_regular_set(xmin, ymax, spacing, ncols, nrows, MISS, "north_east", gridLON=lon, rotation_angle=ROTATION_ANGLE, pairs=PAIRS)
    device_ne_ms = batch_list(device_route, REPS["device_route"])
    hits_ne_ms, gather_ne_ms = split()
    res = {"mesh": kind, "num_nodes": int(Nn), "num_elements": int(Ne), "device": dynamics.device_name(0), "batches": BATCHES, "calls_per_batch": REPS,
           "mooring_spacing_m": spacing, "grid": [ncols, nrows], "grid_points": int(G), "grid_points_in_the_mesh": int(lsm.sum()), "num_elemental": n_el, "num_nodal": n_nod,
           "equal_bits": same, "means_to_grid_ms": host_ms, "regular_update_plus_get_ms": device_ms, "ratio_host_over_device": host_ms / device_ms,
           "regular_update_synchronised_ms": update_ms, "regular_get_ms": get_ms, "search_device_ms": hits_ms, "gather_device_ms": gather_ms,
           "north_east": {"regular_update_plus_get_ms": device_ne_ms, "search_device_ms": hits_ne_ms, "gather_device_ms": gather_ne_ms},
           "download_bytes_device_route": int((n_el + n_nod) * G * 8), "download_bytes_host_route": int((3 * (n_el + n_nod) + 1) * G * 8 + 2 * Nn * 8),
           "upload_bytes_host_route_per_call": int(3 * (3 * Ne * 4 + 2 * Nn * 8))}
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "means_regular.json"), "w"), indent=1)
    print(f"{kind}: {Nn} nodes, {Ne} triangles, {res['device']}; grid {ncols} x {nrows} = {G} points at {spacing / 1e3:g} km ({int(lsm.sum())} in the mesh), {n_el} elemental + {n_nod} nodal variables")
    print(f"  1. means_to_grid (through the host)          {host_ms:9.2f} ms")
    print(f"  2. regular_update + regular_get              {device_ms:9.3f} ms  host / device = {host_ms / device_ms:.1f}")
    print(f"  3. regular_update, synchronised              {update_ms:9.3f} ms; regular_get alone {get_ms:.3f} ms")
    print(f"  4. device time: search {hits_ms:.4f} ms, gather {gather_ms:.4f} ms")
    print(f"  5. NORTH_EAST: update + get {device_ne_ms:.3f} ms; search {hits_ne_ms:.4f} ms, gather {gather_ne_ms:.4f} ms")
    print(f"  equal bits: {same}")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--spacing", type=float, default=SPACING)
    a = ap.parse_args()
    measure(a.mesh, a.out, a.spacing)
