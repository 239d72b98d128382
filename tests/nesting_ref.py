"""nestingIce(), nestingDynamics() and diffuse() of model/finiteelement.cpp (FE.cpp) and ExternalData::get of model/externaldata.cpp restated in numpy, statement by
statement with the reference's line beside each -- what tests/test_nesting_host_kernel.py and tests/test_gpu_nesting.py compare with.  numpy rounds every product and
sum on its own (no contraction), like the library's build; the state is a dict of arrays named like the reference's members without "M_", updated in place."""
import math

import numpy as np

from nextsim_amd import _abi

OFF, LINEAR, STEP = _abi.NXS_TF_OFF, _abi.NXS_TF_LINEAR, _abi.NXS_TF_STEP
f64 = np.float64


def get(time, d0, d1):
    """ExternalData::get for every index of one variable; time = (mode, fcoeff0, fcoeff1, factor, bias) of its dataset"""
    mode, c0, c1, factor, bias = time
    with np.errstate(all="ignore"):
        if mode == LINEAR:                                                   # externaldata.cpp:366
            value = f64(factor) * (f64(c0) * d0 + f64(c1) * d1)              # externaldata.cpp:401-403
        else:
            value = f64(factor) * d0                                         # externaldata.cpp:434 (interpolated_data[1] is not read)
        return value + f64(bias)                                             # externaldata.cpp:438


def f_nudge(function, dist, nudge_scale):
    with np.errstate(all="ignore"):
        if function == "linear":
            r = dist / f64(nudge_scale)
            return 1. - np.where(r < 1., r, 1.)                              # FE.cpp:4893  1. - std::min(1., r); std::min(a, b) is (b < a) ? b : a
        if function == "exponential":
            # FE.cpp:4895  std::exp is the C library's: math.exp calls it (numpy's vectorised exp is another implementation, a last bit away here and there)
            return np.array([math.exp(v) for v in (-dist / f64(nudge_scale)).tolist()], f64).reshape(np.shape(dist))
    raise ValueError("M_nudge_function not known: use exponential or linear")   # FE.cpp:4888


def _target(nest, times, name):
    ds = dataset_of(name)
    d0, d1 = nest[0][name], (nest[1] or {}).get(name)
    return get(times[ds], d0, d1)


def dataset_of(name):
    """the dataset each variable of forcingNesting() is read from (FE.cpp:11062-11121)"""
    if name == "dist":
        return "distance_elements"
    if name == "dist_nodes":
        return "distance_nodes"
    if name in ("VT1", "VT2"):
        return "nodes"
    return "dynamics_elements" if name in ("sigma1", "sigma2", "sigma3", "damage", "ridge_ratio") else "ice_elements"


def nesting_ice(st, nest, times, cfg, young):
    """FE.cpp:4878-4908.  st: the state (updated in place); nest: (snapshot 0, snapshot 1) dicts; times: {dataset: (mode, c0, c1, factor, bias)};
    cfg: dict(nudge_function, nudge_timescale, nudge_scale, time_step, dtime_step)"""
    nudge_time = f64(cfg["nudge_timescale"])                                 # FE.cpp:4880
    nudge_scale = f64(cfg["nudge_scale"])                                    # FE.cpp:4881
    time_step = int(cfg["time_step"])
    with np.errstate(all="ignore"):
        fNudge = f_nudge(cfg["nudge_function"], _target(nest, times, "dist"), nudge_scale)                                  # FE.cpp:4892-4895
        q = f64(time_step) / nudge_time                                      # (time_step/nudge_time): int / double
        st["conc"] += (fNudge * q * (_target(nest, times, "conc") - st["conc"]))                                            # FE.cpp:4897
        st["thick"] += (fNudge * q * (_target(nest, times, "thick") - st["thick"]))                                         # FE.cpp:4898
        st["snow_thick"] += (fNudge * q * (_target(nest, times, "snow_thick") - st["snow_thick"]))                          # FE.cpp:4899
        if young:                                                            # FE.cpp:4900
            st["conc_young"] += (fNudge * q * (_target(nest, times, "conc_young") - st["conc_young"]))                      # FE.cpp:4902
            st["h_young"] += (fNudge * q * (_target(nest, times, "h_young") - st["h_young"]))                               # FE.cpp:4903
            st["hs_young"] += (fNudge * q * (_target(nest, times, "hs_young") - st["hs_young"]))                            # FE.cpp:4904
    return st


def nesting_dynamics(st, nest, times, cfg):
    """FE.cpp:4915-4958.  st holds sigma0, sigma1, sigma2, damage, ridge_ratio [Ne] and VT [2 Nn] (u then v)."""
    nudge_time = f64(cfg["nudge_timescale"])                                 # FE.cpp:4917
    nudge_scale = f64(cfg["nudge_scale"])                                    # FE.cpp:4918
    time_step, dtime_step = int(cfg["time_step"]), f64(cfg["dtime_step"])
    with np.errstate(all="ignore"):
        fNudge = f_nudge(cfg["nudge_function"], _target(nest, times, "dist"), nudge_scale)                                  # FE.cpp:4929-4932
        q = f64(time_step) / nudge_time
        st["sigma0"] += (fNudge * q * (_target(nest, times, "sigma1") - st["sigma0"]))                                      # FE.cpp:4933
        st["sigma1"] += (fNudge * q * (_target(nest, times, "sigma2") - st["sigma1"]))                                      # FE.cpp:4934
        st["sigma2"] += (fNudge * q * (_target(nest, times, "sigma3") - st["sigma2"]))                                      # FE.cpp:4935
        st["damage"] += (fNudge * q * (_target(nest, times, "damage") - st["damage"]))                                      # FE.cpp:4936
        st["ridge_ratio"] += (fNudge * q * (_target(nest, times, "ridge_ratio") - st["ridge_ratio"]))                       # FE.cpp:4937
        Nn = st["VT"].size // 2
        fNudge = f_nudge(cfg["nudge_function"], _target(nest, times, "dist_nodes"), nudge_scale)                            # FE.cpp:4950-4953
        qd = dtime_step / nudge_time                                         # (dtime_step/nudge_time)
        st["VT"][:Nn] += (fNudge * qd * (_target(nest, times, "VT1") - st["VT"][:Nn]))                                      # FE.cpp:4954
        st["VT"][Nn:] += (fNudge * qd * (_target(nest, times, "VT2") - st["VT"][Nn:]))                                      # FE.cpp:4955
    return st


def diffuse(variable_elt, diffusivity_parameters, dx, dtime_step, element_connectivity):
    """FE.cpp:2760-2815 on one rank.  element_connectivity: bamgmesh->ElementConnectivity, [3 Ne] doubles, 1-based, NaN on the boundary.  Returns the new field."""
    if diffusivity_parameters <= 0.:                                         # FE.cpp:2762
        return variable_elt
    factor = f64(diffusivity_parameters) * f64(dtime_step) / f64(np.power(f64(dx), 2.))                                     # FE.cpp:2775
    old_variable_elt = variable_elt.copy()                                   # FE.cpp:2776
    num_elements = variable_elt.size
    ec = np.asarray(element_connectivity, f64).reshape(num_elements, 3)
    fluxes_source = np.zeros((3, num_elements))
    with np.errstate(all="ignore"):
        for i in range(3):                                                   # FE.cpp:2790
            neighbour_double = ec[:, i]                                      # FE.cpp:2792
            neighbour_int = np.where(np.isnan(neighbour_double), 0, neighbour_double).astype(np.int64)                      # FE.cpp:2793
            has = ~np.isnan(neighbour_double) & (neighbour_int > 0)          # FE.cpp:2798
            fluxes_source_id = np.where(has, neighbour_int - 1, 0)           # FE.cpp:2800
            flux = factor * (old_variable_elt[fluxes_source_id] - old_variable_elt)                                         # FE.cpp:2801
            fluxes_source[i] = np.where(has, flux, 0.)                       # FE.cpp:2805
        out = variable_elt.copy()
        out += fluxes_source[0] + fluxes_source[1] + fluxes_source[2]        # FE.cpp:2809
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


# ---- inputs the two test files share --------------------------------------------------------------------------------------------------------
ICE_ROWS = ("thick", "conc", "snow_thick", "h_young", "conc_young", "hs_young")
DYN_ROWS = ("sigma1", "sigma2", "sigma3", "damage", "ridge_ratio")
# LINEAR and STEP mixed, factor / bias not 1 / 0
TIMES = {"distance_elements": (STEP, 0., 0., 1., 0.), "ice_elements": (LINEAR, 0.3125, 0.6875, 1.25, -0.125), "dynamics_elements": (STEP, 0., 0., 0.75, 0.5),
         "distance_nodes": (LINEAR, 0.5, 0.5, 1., 0.), "nodes": (LINEAR, 0.8125, 0.1875, 0.5, 0.015625)}
TIMES_B = {"distance_elements": (LINEAR, 0.25, 0.75, 1., 0.), "ice_elements": (STEP, 0., 0., 0.875, 0.25), "dynamics_elements": (LINEAR, 1., 0., 1., -0.),
           "distance_nodes": (STEP, 0., 0., 1., 0.), "nodes": (STEP, 0., 0., 2., -0.5)}
CFG = dict(nudge_function="linear", nudge_timescale=86400. / 7., nudge_scale=30000., time_step=900, dtime_step=900.5, nest_dynamic_vars=True)


def time_arg(times):
    """the argument of FiniteElementDynamics.nesting_time for a table of TIMES' form"""
    return {k: dict(mode=m, fcoeff0=c0, fcoeff1=c1, factor=f, bias=b) for k, (m, c0, c1, f, b) in times.items()}


def _dist(n, rng, times, ds, scale, zero):
    """distances whose TARGET (what the kernels divide by nudge_scale) lies below, exactly at and beyond nudge_scale: fNudge = 1, in between, exactly 0"""
    d = rng.uniform(0., 1.6 * scale, n)
    if zero:
        d[:] = 0.
    else:
        d[0 % n] = 0.
        d[(n // 2) % n] = scale
        d[n - 1] = 2.5 * scale
    mode = times[ds][0]
    if mode == LINEAR:                                                       # both snapshots the same and fcoeff0 + fcoeff1 = 1 exactly (dyadic): the blend is d
        return d, d.copy()
    d1 = np.full(n, np.nan)
    return d, d1


def snapshots(Ne, Nn, times, scale, seed=0, zero_dist=False):
    """(snapshot 0, snapshot 1) with every row of forcingNesting(): ordinary values, signed zeros, and under STEP NaN / +-Inf in snapshot 1 (never read)"""
    rng = np.random.default_rng(1000 * seed + 7 * Ne + Nn)
    s0, s1 = {}, {}
    s0["dist"], s1["dist"] = _dist(Ne, rng, times, "distance_elements", scale, zero_dist)
    s0["dist_nodes"], s1["dist_nodes"] = _dist(Nn, rng, times, "distance_nodes", scale, zero_dist)
    for k in ICE_ROWS + DYN_ROWS + ("VT1", "VT2"):
        n = Nn if k.startswith("VT") else Ne
        s0[k] = rng.normal(size=n) * (1e4 if k.startswith("sigma") else 1.)
        s1[k] = rng.normal(size=n) * (1e4 if k.startswith("sigma") else 1.)
        s0[k][n // 3] = -0.
        s1[k][n // 3] = 0.
        if times[dataset_of(k)][0] == STEP:
            s1[k][::3] = np.nan
            s1[k][1 % n] = np.inf
            s1[k][n - 1] = -np.inf
    return s0, s1


def state(Ne, Nn, seed=0):
    """the rows the two loops update, with -0.0 and +0.0 where fNudge is exactly 0 (the last entry) and where it is 1 (the first)"""
    rng = np.random.default_rng(77 + seed + Ne)
    st = {k: rng.normal(size=Ne) for k in ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young", "sigma0", "sigma1", "sigma2", "damage", "ridge_ratio")}
    st["VT"] = rng.normal(size=2 * Nn) * 0.1
    for j, k in enumerate(st):
        if k == "VT":
            continue
        st[k][Ne - 1] = -0. if j % 2 else 0.
        st[k][0] = 0. if j % 2 else -0.
    st["VT"][Nn - 1] = -0.
    st["VT"][2 * Nn - 1] = 0.
    return st
