"""Cost per model step of nesting and of the slab ocean's diffusion on the device (nxs_dyn_nesting_ice, nxs_dyn_nesting_dynamics, nxs_dyn_diffuse), at 2 km, beside the
route they replace and a device-to-device copy of the same run.

    python scripts/time_nesting.py [mesh] [--out DIR]     measure on the GPU, print the table, write DIR/nesting.json (default profiles/) and DESIGN.md's table
    python scripts/time_nesting.py --from-json FILE       write DESIGN.md's table (between its markers) and profiles/nesting.json from an earlier measurement

  1. the three calls, each a batch enqueued back to back and synchronised once, median of BATCHES batches after a warm-up batch; the young-ice category, every
     dataset LINEAR (both snapshots read), M_sigma / M_damage in the records a step left behind.  Bytes each must move: nesting_ice 26 rows of Ne doubles (the
     distance's two snapshots, per field two snapshots and the row read and written); nesting_dynamics 22 rows of Ne (12 snapshot rows, the 32-byte record and
     M_ridge_ratio read and written) and 10 of Nn; diffuse 76 B per element (pack: 16 in, 16 out; then 12 of indices, the element's own pair, 16 B of gathers per
     element on average -- every pair is gathered three times but has to arrive once --, 16 out).
  2. the route they replace, per step: get_state + flux_get, the three loops in numpy, put_state + flux_put (wall time, the whole state over PCIe twice).
  3. a device-to-device copy of 26 rows of Ne doubles (bytes read + bytes written).
Repeated back to back the calls work on 100 .. 300 MB, which partly live in the 256 MiB last-level cache: their rates are not HBM rates, and neither is the
copy's.  No threshold: the numbers are the result."""
import ctypes as C
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BATCHES = 5
REPS = {"kernel": 200, "host_route": 3, "copy": 200}
BEGIN = "<!-- nesting-measurement:begin (written by scripts/time_nesting.py) -->"
END = "<!-- nesting-measurement:end -->"
CFG = dict(nudge_function="linear", nudge_timescale=86400., nudge_scale=50e3, nest_dynamic_vars=True, time_step=200, dtime_step=200.)
DIFF = dict(diffusivity_sst=100., diffusivity_sss=100., dx=2000., dtime_step=200.)


def measure(kind, out_dir):
    import numpy as np
    from nextsim_amd import _abi, dynamics, forcing as F, mesh as M

    gm = M.make_mesh(kind)
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE), gm, alea_factor=0.33)
    lm = M.localize(gm, 1)[0]
    f = F.localize_fields(F.global_fields(gm, p, "arctic", C_fix, C_alea), lm, gm.num_nodes)
    Ne, Nn = lm.num_elements, lm.num_nodes
    rng = np.random.default_rng(0)
    src = dict(thick="thick", conc="conc", snow_thick="snow_thick", h_young="h_young", conc_young="conc_young", hs_young="hs_young", sigma1="sigma0", sigma2="sigma1",
               sigma3="sigma2", damage="damage", ridge_ratio="ridge_ratio")
    s0 = {k: f[v] * 0.9 for k, v in src.items()}
    s1 = {k: f[v] * 1.1 for k, v in src.items()}
    for s in (s0, s1):
        s["dist"], s["dist_nodes"] = rng.uniform(0., 2. * CFG["nudge_scale"], Ne), rng.uniform(0., 2. * CFG["nudge_scale"], Nn)
        s["VT1"], s["VT2"] = f["VT"][:Nn] * 0.9, f["VT"][Nn:] * 0.9
    times = {k: dict(mode="linear", fcoeff0=0.25, fcoeff1=0.75) for k in _abi.NEST_DATASETS}
    sst, sss = rng.normal(size=Ne), 33. + rng.normal(size=Ne)
    ec = dynamics.mesh_element_connectivity(lm.indices, Nn)
    nb = np.where(np.isnan(ec), 0, ec).astype(np.int64) - 1

    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    fe.flux_put(sst=sst, sss=sss)
    fe.nesting_configure(**CFG); fe.nesting_time(times); fe.nesting_pair(s0, s1); fe.diffusion_configure(**DIFF)
    fe.step(); fe.synchronize()                                              # the records are home
    records_home = int(fe.debug_array("update_launch")[0])

    def batches(call, reps):
        t = []
        for b in range(BATCHES + 1):
            fe.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            fe.synchronize()
            if b:
                t.append((time.perf_counter() - t0) / reps * 1e3)
        return {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "n": len(t), "calls_per_batch": reps}

    def with_bytes(r, nbytes):
        r["bytes"] = int(nbytes)
        r["GBps"] = nbytes / (r["median_ms"] * 1e-3) / 1e9
        return r

    res = {"mesh": kind, "num_elements": int(Ne), "num_nodes": int(Nn), "device": dynamics.device_name(0), "records_home": records_home}
    res["diffuse"] = with_bytes(batches(fe.diffuse, REPS["kernel"]), 76 * Ne)      # (first: the state is still a model state)
    res["nesting_ice"] = with_bytes(batches(fe.nesting_ice, REPS["kernel"]), 26 * 8 * Ne)
    res["nesting_dynamics"] = with_bytes(batches(fe.nesting_dynamics, REPS["kernel"]), 22 * 8 * Ne + 10 * 8 * Nn)
    res["three_calls_ms"] = sum(res[k]["median_ms"] for k in ("diffuse", "nesting_ice", "nesting_dynamics"))

    # the device-to-device copy of nesting_ice's bytes
    L = dynamics.load_library()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipFree.argtypes = [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    half = 13 * 8 * Ne
    d = [C.c_void_p(), C.c_void_p()]
    for ptr in d:
        assert L.hipMalloc(C.byref(ptr), half) == 0

    def copy_batch():
        assert L.hipMemcpy(d[1], d[0], half, 3) == 0
    res["device_copy_same_run"] = with_bytes(batches(lambda: (copy_batch(), L.hipDeviceSynchronize()), REPS["copy"]), 2 * half)
    for ptr in d:
        L.hipFree(ptr)

    # the replaced route: the whole state to the host, the three loops in numpy (tests/nesting_ref.py says them line by line), and back
    q, qd, scale = CFG["time_step"] / CFG["nudge_timescale"], CFG["dtime_step"] / CFG["nudge_timescale"], CFG["nudge_scale"]
    fac = [DIFF[k] * DIFF["dtime_step"] / DIFF["dx"] ** 2 for k in ("diffusivity_sst", "diffusivity_sss")]

    def target(k):
        return 1. * (0.25 * s0[k] + 0.75 * s1[k]) + 0.

    def host_route():
        st = fe.get_state()
        oc = fe.flux_get(("sst", "sss"))
        w = (1. - np.minimum(1., target("dist") / scale)) * q
        for k, v in src.items():
            st[v] += w * (target(k) - st[v])
        wn = (1. - np.minimum(1., target("dist_nodes") / scale)) * qd
        st["VT"][:Nn] += wn * (target("VT1") - st["VT"][:Nn])
        st["VT"][Nn:] += wn * (target("VT2") - st["VT"][Nn:])
        for k, fk in zip(("sst", "sss"), fac):
            old = oc[k]
            flux = [np.where(nb[:, j] >= 0, fk * (old[np.maximum(nb[:, j], 0)] - old), 0.) for j in range(3)]
            oc[k] = old + (flux[0] + flux[1] + flux[2])
        fe.put_state(dict(f, **st))
        fe.flux_put(**oc)
    res["replaced_host_route"] = batches(host_route, REPS["host_route"])
    fe.close()
    res["date"] = time.strftime("%Y-%m-%d")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(res, open(os.path.join(out_dir, "nesting.json"), "w"), indent=1)
    return res


def table(res):
    def row(name, r, extra=""):
        return f"| {name} | {r['median_ms']:.4f} | {r['min_ms']:.4f} – {r['max_ms']:.4f} | {r['n']} x {r['calls_per_batch']} | {extra} |"

    def rate(r):
        return f"{r['bytes'] / 1e6:.0f} MB to move: {r['GBps']:.0f} GB/s, {100 * r['GBps'] / res['device_copy_same_run']['GBps']:.0f} % of the copy's rate"
    cp, host = res["device_copy_same_run"], res["replaced_host_route"]
    lines = [BEGIN,
             f"Measured {res['date']} on one {res['device'] or 'MI355X'}, `{res['mesh']}` mesh ({res['num_elements']} triangles, {res['num_nodes']} nodes), the young-ice category, every "
             f"dataset LINEAR, records home: {bool(res['records_home'])}.  Wall-clock milliseconds per call; the device calls in batches enqueued back to back and synchronised "
             "once, so their working sets are partly warm in the 256 MiB last-level cache -- as the copy's is.",
             "",
             "| what | median ms | min – max | batches x calls | note |", "|---|---|---|---|---|",
             row("`nxs_dyn_nesting_ice`", res["nesting_ice"], rate(res["nesting_ice"])),
             row("`nxs_dyn_nesting_dynamics`", res["nesting_dynamics"], rate(res["nesting_dynamics"])),
             row("`nxs_dyn_diffuse` (two launches)", res["diffuse"], rate(res["diffuse"])),
             f"| the three calls together | {res['three_calls_ms']:.4f} | | | {host['median_ms'] / res['three_calls_ms']:.0f} times less than the route below |",
             row("device-to-device copy, same run", cp, f"{cp['bytes'] / 1e6:.0f} MB read + written: {cp['GBps']:.0f} GB/s"),
             row("replaced route: `get_state` + `flux_get`, the loops in numpy, `put_state` + `flux_put`", host),
             END]
    return "\n".join(lines)


def write_design(res):
    path = os.path.join(ROOT, "DESIGN.md")
    text = open(path).read()
    if BEGIN in text:
        text = re.sub(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: table(res), text, flags=re.S)
        open(path, "w").write(text)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--from-json" in args:
        res = json.load(open(args[args.index("--from-json") + 1]))
        json.dump(res, open(os.path.join(ROOT, "profiles", "nesting.json"), "w"), indent=1)
    else:
        out_dir = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles")
        kind = next((a for a in args if not a.startswith("--") and (args.index(a) == 0 or args[args.index(a) - 1] != "--out")), "2km")
        res = measure(kind, out_dir)
    write_design(res)
    print(table(res))
