"""Cost of the device-resident floe-size distribution (nxs_dyn_fsd_*) at 2 km, against the round trip it replaces: a wave-coupled host without these kernels
pulls the bins (nxs_dyn_get_coupled) and conc, conc_young, thick, h_young, damage (nxs_dyn_get_state of the five members), runs updateFSD / redistributeFSD
on the CPU and pushes bins and cum_damage back (nxs_dyn_put_coupled) -- every step.

    python scripts/time_fsd.py [mesh] [--bins N] [--out DIR]     measure on the GPU, print the table, write DIR/fsd.json (default profiles/)

Workload: the arctic case after one step, N bins (default 12) with a random distribution, waves (M_wlbk < 499) on half of the elements, freezing on half.
Per kernel: wall time per call of REPS calls enqueued back to back and synchronised once (the calls are asynchronous; M_wlbk is passed as a device pointer;
fsd_weld's figure includes its upload of the [Ne] freezing mask, which the call waits for), median of 7 such batches after a warm-up batch.  The round trip:
wall time of get_coupled + get_state + put_coupled, synchronised, median of 7 -- WITHOUT the host's own loops, so it is the floor of what the kernels replace.
No threshold: the numbers are the result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, BATCHES = 10, 7


def measure(kind, n, out_dir):
    import ctypes as C

    import numpy as np
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(g, lm, gm.num_nodes)
    Ne = lm.num_elements
    rng = np.random.default_rng(1)
    ctot = f["conc"] + f["conc_young"]
    bins = np.ascontiguousarray(rng.dirichlet([1.] * n, Ne).T * ctot)
    wlbk = np.where(rng.random(Ne) < 0.5, rng.uniform(20., 300., Ne), 1000.)
    freezing = (rng.random(Ne) < 0.5).astype(np.uint8)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.put_coupled(cum_damage=np.zeros(Ne), conc_fsd=bins)
    fe.fsd_put(conc_mech_fsd=bins, cum_wave_damage=np.zeros(Ne))
    tables = dynamics.fsd_bins("constant_size", n, 10., 10., True)
    ddt = 900.
    fe.fsd_configure(tables, breakup_type="uniform_size", welding_type="roach", fsd_damage_type=2, distinguish_mech_fsd=1, breakup_coef1=0.5, breakup_coef2=0.05,
                     breakup_coef3=0.1, breakup_prob_cutoff=0.0015, breakup_timescale_tuning=1800., cpl_time_step=2400., floes_flex_young=4e9, breakup_thick_min=0.1,
                     fsd_damage_max=0.99, welding_kappa=2. / (ddt * tables["area_scaled_up"][n - 1]))
    fe.step(); fe.synchronize()
    d_wlbk = dynamics.device_put(wlbk)                       # M_wlbk in a plain device buffer: fsd_breakup then returns without waiting
    calls = {"fsd_init": fe.fsd_init, "fsd_update": fe.fsd_update, "fsd_breakup": lambda: fe.fsd_breakup(d_wlbk, want_flags=False),
             "fsd_weld": lambda: fe.fsd_weld(ddt, freezing)}
    med = lambda v: float(np.median(np.asarray(v)))          # noqa: E731
    res = {"mesh": kind, "num_elements": Ne, "num_bins": n, "device": dynamics.device_name(0), "calls_per_batch": REPS, "batches": BATCHES, "kernels_us": {}}
    for name in ("fsd_update", "fsd_breakup", "fsd_weld", "fsd_init"):
        t = []
        for b in range(BATCHES + 1):
            fe.put_coupled(cum_damage=np.zeros(Ne), conc_fsd=bins); fe.fsd_put(conc_mech_fsd=bins, cum_wave_damage=np.zeros(Ne)); fe.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                calls[name]()
            fe.synchronize()
            if b:
                t.append((time.perf_counter() - t0) / REPS * 1e6)
        res["kernels_us"][name] = med(t)
    # the round trip the kernels replace
    st = _abi.State()
    five = {k: np.empty(Ne) for k in ("conc", "conc_young", "thick", "h_young", "damage")}
    for k, v in five.items():
        setattr(st, k, _abi.dptr(v))
    t = []
    for b in range(BATCHES + 1):
        fe.synchronize()
        t0 = time.perf_counter()
        c = fe.get_coupled(True, n)
        fe._chk(fe.L.nxs_dyn_get_state(fe.h, C.byref(st)))
        fe.put_coupled(cum_damage=c["cum_damage"], conc_fsd=c["conc_fsd"])
        fe.synchronize()
        if b:
            t.append((time.perf_counter() - t0) * 1e3)
    res["round_trip_ms"] = med(t)
    res["round_trip_bytes"] = int((2 * n + 2 + 5) * Ne * 8)
    dynamics.device_free(d_wlbk)
    fe.close()
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "fsd.json"), "w"), indent=1)
    print(f"{kind}: {Ne} triangles, {n} bins, {res['device']}")
    for k, v in res["kernels_us"].items():
        print(f"  {k:12s} {v:9.1f} us per call")
    print(f"  round trip   {res['round_trip_ms'] * 1e3:9.1f} us  (get_coupled + get_state of five members + put_coupled, {res['round_trip_bytes'] / 1e6:.0f} MB over PCIe, no host loop)")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mesh", nargs="?", default="2km")
    ap.add_argument("--bins", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    measure(a.mesh, a.bins, a.out)
