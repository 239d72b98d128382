"""A line-faithful restatement of the floe-size-distribution code of the wave-coupled build (#ifdef OASIS) in model/finiteelement.cpp ("FE.cpp"): the tables
of initFsd() (FE.cpp:7408-7533), its first distribution (7562-7576), updateFSD() (4674-4732), redistributeFSD() (4268-4483), weldingRoach() (4737-4870) and the
mechanical healing of thermo() (5888-5896).  Scalar loops per element in the reference's statement and operand order, on Python floats (IEEE doubles, one
rounding per operation, no contraction); the libm calls are Python's math module, i.e. the host's libm.  model/ cannot be compiled here, so this is what the
library (nxs_fsd_bins, nxs_dyn_fsd_*) is compared with.  Shared by tests/test_fsd_ref.py and tests/test_gpu_fsd.py.

State: a dict of arrays -- conc, conc_young, thick, h_young, damage, time_relaxation_damage [Ne]; conc_fsd, conc_mech_fsd [n, Ne]; cum_damage, cum_wave_damage
[Ne] -- changed in place.  cfg: a dict named after nxs_dyn_fsd_config, with the tables of fsd_tables() under "tables" and "young" for M_ice_cat_type ==
YOUNG_ICE.  Every function also returns the branch each element took, so that a test can show that its inputs reach every branch."""
from __future__ import annotations

import math

import numpy as np

FLOE_SHAPE = 0.66          # M_floe_shape, FE.cpp:7414
PI = 3.141592653589793238462643383279502884197169399375105820974944592308   # contrib/bamg/include/OppositeAngle.h:4
RHOW = 1025.               # physical::rhow, model/constants.hpp:62
G = 9.8                    # physical::g, model/constants.hpp:35
NONE, UNIFORM_SIZE, ZHANG, DUMONT = range(4)    # setup::BreakupType, model/enums.hpp:110-116
WELD_NONE, WELD_ROACH = 0, 1                    # setup::WeldingType, model/enums.hpp:99-103
CONSTANT_SIZE, CONSTANT_AREA = 0, 1             # setup::FSDType, model/enums.hpp:105-109


def _div(a, b):
    """a / b as the hardware divides (a zero divisor gives inf or NaN: FE.cpp:4694 divides by a zero ctot2)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def fsd_tables(fsd_type, n, min_floe_size, bin_cst_width, use_scaled_area, pow2=lambda x: x * x):
    """FE.cpp:7408-7533.  pow2: std::pow(x, 2) -- x * x (what a compiler makes of the literal exponent) or math.pow(x, 2.) (the libm's)."""
    widths, low, up, centres = [0.] * n, [0.] * n, [0.] * n, [0.] * n
    area_up, area_low, area_centered, area_binwidth = [0.] * n, [0.] * n, [0.] * n, [0.] * n
    lims, lims_scaled = [0.] * (n + 1), [0.] * (n + 1)
    if fsd_type == CONSTANT_SIZE:
        low[0] = min_floe_size
        widths[0] = bin_cst_width
        up[0] = min_floe_size + bin_cst_width
        centres[0] = (up[0] + low[0]) / 2
        for m in range(1, n):
            widths[m] = bin_cst_width
            low[m] = low[m - 1] + bin_cst_width
            up[m] = up[m - 1] + bin_cst_width
            centres[m] = (up[m] + low[m]) / 2
        for m in range(n):
            area_up[m] = FLOE_SHAPE * pow2(up[m])
            area_low[m] = FLOE_SHAPE * pow2(low[m])
            area_centered[m] = FLOE_SHAPE * pow2(centres[m])
            lims[m] = area_low[m]
            area_binwidth[m] = area_up[m] - area_low[m]
        lims[n] = area_up[n - 1]
    elif fsd_type == CONSTANT_AREA:
        low[0] = min_floe_size
        area_binwidth[0] = FLOE_SHAPE * (pow2(bin_cst_width) + 2 * min_floe_size * bin_cst_width)
        area_low[0] = FLOE_SHAPE * pow2(low[0])
        area_up[0] = area_low[0] + area_binwidth[0]
        for m in range(1, n):
            area_binwidth[m] = area_binwidth[0]
            area_low[m] = area_up[m - 1]
            area_up[m] = area_up[m - 1] + area_binwidth[m]
        for m in range(n):
            lims[m] = area_low[m]
            low[m] = math.sqrt(area_low[m] / FLOE_SHAPE)
            up[m] = math.sqrt(area_up[m] / FLOE_SHAPE)
            widths[m] = up[m] - low[m]
            centres[m] = (up[m] + low[m]) / 2
            area_centered[m] = FLOE_SHAPE * pow2(centres[m])
        lims[n] = area_up[n - 1]
    else:
        raise ValueError("Wrong fsd_type")
    if use_scaled_area:
        widest = max(area_binwidth)
        for m in range(n + 1):
            lims_scaled[m] = (lims[m] - lims[0]) / widest
    else:
        for m in range(n + 1):
            lims_scaled[m] = (lims[m] - lims[0])
    s_up, s_low, s_centered, s_binwidth = [0.] * n, [0.] * n, [0.] * n, [0.] * n
    for m in range(n):
        s_up[m] = lims_scaled[m + 1]
        s_low[m] = lims_scaled[m]
        s_centered[m] = (s_up[m] + s_low[m]) / 2.
        s_binwidth[m] = s_up[m] - s_low[m]
    alpha = np.full((n, n), -999, np.int32)
    for m in range(n):
        for k in range(n):
            test = s_up[m] - s_centered[k]
            for p in range(n):
                if (test >= s_low[p]) and (test < s_up[p]):
                    alpha[m, k] = p + 1
    f = lambda v: np.array(v, np.float64)
    return {"bin_widths": f(widths), "bin_low_limits": f(low), "bin_up_limits": f(up), "bin_centres": f(centres), "area_scaled_up": f(s_up),
            "area_scaled_low": f(s_low), "area_scaled_centered": f(s_centered), "area_scaled_binwidth": f(s_binwidth), "alpha_merge": alpha}


def _ctot(st, cfg, i):
    ctot = float(st["conc"][i])
    if cfg["young"]:
        ctot += float(st["conc_young"][i])
    return ctot


def init_fsd(st, cfg):
    """FE.cpp:7562-7576"""
    n = cfg["num_bins"]
    for i in range(st["conc"].size):
        st["conc_fsd"][n - 1][i] = st["conc"][i]
        if cfg["young"]:
            st["conc_fsd"][n - 1][i] += st["conc_young"][i]
        for k in range(n - 1):
            st["conc_fsd"][k][i] = 0.
        if cfg["distinguish_mech_fsd"]:
            for k in range(n):
                st["conc_mech_fsd"][k][i] = st["conc_fsd"][k][i]


UPDATE_BRANCHES = ("ctot_ge_1", "ctot2_zero", "within_1e-11", "rescaled", "no_ice")


def _update_bins(rows, n, cpt, ctot):
    """FE.cpp:4687-4706 (and 4710-4728 for the mechanical bins); returns the branch"""
    ctot2 = float(rows[0][cpt])
    for j in range(1, n):
        ctot2 += float(rows[j][cpt])
    if ctot >= 1.:
        for k in range(n):
            rows[k][cpt] *= _div(ctot, ctot2)
        return "ctot_ge_1"
    elif abs(ctot - ctot2) > 1e-11:
        if (ctot2 == 0.) and (ctot > 0.):
            rows[n - 1][cpt] = ctot
            return "ctot2_zero"
        else:
            for k in range(n):
                rows[k][cpt] *= _div(ctot, ctot2)
            return "rescaled"
    return "no_ice" if ctot == 0. else "within_1e-11"


def update_fsd(st, cfg):
    """updateFSD(), FE.cpp:4674-4732.  Returns the branch of the real bins per element."""
    n = cfg["num_bins"]
    branch = []
    with np.errstate(all="ignore"):     # (a bin times the inf or NaN of a division by a zero ctot2)
        for cpt in range(st["conc"].size):
            ctot = _ctot(st, cfg, cpt)
            branch.append(_update_bins(st["conc_fsd"], n, cpt, ctot))
            if cfg["distinguish_mech_fsd"]:
                _update_bins(st["conc_mech_fsd"], n, cpt, ctot)
    return np.array(branch)


def breakup_constants(cfg):
    """What does not depend on the element in redistributeFSD (the library computes the same on the host): P for P_inf = 0 and 1, the redistributors."""
    t = cfg["tables"]
    n = cfg["num_bins"]
    tau_w = cfg["breakup_timescale_tuning"]
    pfac = [P * (1. - math.exp(-P * cfg["cpl_time_step"] / tau_w)) for P in (0., 1.)]
    beta = np.zeros((n, n))
    for j in range(n):
        for k in range(j + 1):
            if cfg["breakup_type"] == ZHANG:
                beta[j, k] = t["bin_widths"][k] / (t["bin_up_limits"][j] - t["bin_low_limits"][0])
            elif cfg["breakup_type"] == UNIFORM_SIZE:
                beta[j, k] = (math.pow(t["bin_up_limits"][k], 3) - math.pow(t["bin_low_limits"][k], 3)) / (math.pow(t["bin_up_limits"][j], 3) - math.pow(t["bin_low_limits"][0], 3))
    return pfac, beta


def redistribute_fsd(st, cfg, wlbk):
    """redistributeFSD(), FE.cpp:4268-4483.  Returns (M_breakup_in_dt, crash, per element: 0 = no ice (bins cleared), 1 = ice, not broken, 2 = broken)."""
    n = cfg["num_bins"]
    t = cfg["tables"]
    centres, low, up, widths = (t[k].tolist() for k in ("bin_centres", "bin_low_limits", "bin_up_limits", "bin_widths"))
    fsd, mech = st["conc_fsd"], st.get("conc_mech_fsd")
    P = [0.] * n
    poisson = 0.3
    coef1, coef2, coef3 = cfg["breakup_coef1"], cfg["breakup_coef2"], cfg["breakup_coef3"]
    prob_cutoff = cfg["breakup_prob_cutoff"]
    crash = False
    breakup_in_dt = False
    what = np.zeros(st["conc"].size, np.int8)
    for i in range(st["conc"].size):
        ctot = _ctot(st, cfg, i)
        if ctot > 0:
            what[i] = 1
            P_inf = 0.
            if wlbk[i] < 500. - 1.:
                P_inf = 1.
            if P_inf <= prob_cutoff:
                continue
            what[i] = 2
            breakup_in_dt = True
            if cfg["distinguish_mech_fsd"]:
                for j in range(n):
                    fsd[j][i] = mech[j][i]
            sea_ice_thickness = 0
            if cfg["breakup_cell_average_thickness"]:
                sea_ice_thickness = float(st["thick"][i])
            elif cfg["young"]:
                sea_ice_thickness = (float(st["thick"][i]) + float(st["h_young"][i])) / ctot
            sea_ice_thickness = max(cfg["breakup_thick_min"], sea_ice_thickness)
            d_flex = 0.5 * math.pow(math.pow(PI, 4) * cfg["floes_flex_young"] * math.pow(sea_ice_thickness, 3) /
                                    (48 * RHOW * G * (1 - math.pow(poisson, 2))), 0.25)
            lam = float(wlbk[i])
            tau_w = 0.
            for j in range(n):
                P[j] = P_inf
                broken_area = 0.
                if cfg["breakup_prob_type"] == 0:
                    tau_w = cfg["breakup_timescale_tuning"]
                    P[j] = P[j] * (1. - math.exp(-P[j] * cfg["cpl_time_step"] / tau_w))
                else:
                    raise ValueError("Wrong breakup_prob_type")
                lim_lambda = max(0., math.tanh((centres[j] - coef1 * lam) / (coef2 * lam)))
                lim_dflex = max(0., math.tanh((centres[j] - d_flex) / (coef3 * d_flex)))
                bt = cfg["breakup_type"]
                if bt == ZHANG:
                    P[j] = P[j] * lim_dflex * lim_lambda
                    if P[j] > 0.:
                        broken_area = float(fsd[j][i]) * P[j]
                        fsd[j][i] -= broken_area
                        for k in range(j + 1):
                            beta = widths[k] / (up[j] - low[0])
                            fsd[k][i] += broken_area * beta
                elif bt == UNIFORM_SIZE:
                    P[j] = P[j] * lim_dflex * lim_lambda
                    if P[j] > 0.:
                        broken_area = float(fsd[j][i]) * P[j]
                        fsd[j][i] -= broken_area
                        for k in range(j + 1):
                            beta = (math.pow(up[k], 3) - math.pow(low[k], 3)) / (math.pow(up[j], 3) - math.pow(low[0], 3))
                            fsd[k][i] += broken_area * beta
                elif bt == DUMONT:
                    fragility = lim_dflex * lim_lambda
                    if fragility > 0:
                        broken_area = float(fsd[j][i]) * P[j] * fragility
                        fsd[j][i] -= broken_area
                        ksi = 2
                        exponent = max(2. - (2. + math.log(fragility) / math.log(ksi)), 1e-6)
                        for k in range(j + 1):
                            beta = (math.pow(up[k], exponent) - math.pow(low[k], exponent)) / (math.pow(up[j], exponent) - math.pow(low[0], exponent))
                            fsd[k][i] += broken_area * beta
                elif bt == NONE:
                    pass
                else:
                    raise ValueError("Wrong breakup_type")
            if cfg["distinguish_mech_fsd"]:
                for j in range(n):
                    mech[j][i] = fsd[j][i]
            ctot2 = float(fsd[0][i])
            for j in range(1, n):
                ctot2 += float(fsd[j][i])
            if (abs(ctot - ctot2) > 2e-7) and cfg["debug_fsd"]:
                crash = True
            if st["thick"][i] > 0.:
                damage_max = cfg["fsd_damage_max"]
                dmg = float(st["damage"][i])
                tmp = dmg
                dt = cfg["fsd_damage_type"]
                if dt == 0:
                    pass
                elif dt in (1, 2):
                    if dt == 1:   # no break at FE.cpp:4454: falls through into case 2
                        tmp = max(dmg, 1. - float(mech[n - 1][i]) / ctot)
                    tot_broken_area = float(mech[0][i]) * P[0]
                    for j in range(1, n):
                        tot_broken_area += float(mech[j][i]) * P[j]
                    tmp = dmg * (1. - tot_broken_area / ctot) + tot_broken_area / ctot * damage_max
                else:
                    raise ValueError("Wrong M_fsd_damage_type")
                if st.get("cum_wave_damage") is not None:
                    st["cum_wave_damage"][i] += max(tmp - dmg, 0.)
                if st.get("cum_damage") is not None:
                    st["cum_damage"][i] += max(tmp - dmg, 0.)
                st["damage"][i] = max(dmg, min(tmp, damage_max))
        else:
            for j in range(n):
                fsd[j][i] = 0.
                if mech is not None:
                    mech[j][i] = 0.
    return breakup_in_dt, crash, what


def welding_roach(st, cfg, cpt, ddt):
    """weldingRoach(cpt, ddt), FE.cpp:4737-4870.  Returns (ndt_mrg or 0 below the gate, crash, a bin in (-1e-12, 0) was zeroed)."""
    n = cfg["num_bins"]
    t = cfg["tables"]
    asu, asc, asb = (t[k].tolist() for k in ("area_scaled_up", "area_scaled_centered", "area_scaled_binwidth"))
    alpha = t["alpha_merge"].tolist()
    kappa = cfg["welding_kappa"]
    fsd = st["conc_fsd"]
    c_fsd_broken = float(fsd[0][cpt])
    crash = False
    zeroed = False
    old_conc_fsd = [float(fsd[j][cpt]) for j in range(n)]
    old_conc_tot = 0.
    for v in old_conc_fsd:
        old_conc_tot = old_conc_tot + v
    for j in range(1, n - 1):
        c_fsd_broken += float(fsd[j][cpt])
    if not ((c_fsd_broken > 0.01) and (old_conc_tot > 0.1)):
        return 0, crash, zeroed
    unbroken_area_loss = 0.
    stability = ddt * kappa * old_conc_tot * asu[n - 1]
    ndt_mrg = int(math.floor(abs(stability + 0.5) + 0.5) * (1 if stability + 0.5 >= 0 else -1))   # std::round: half away from zero
    subdt = _div(ddt, float(np.float32(ndt_mrg)))
    tmp = list(old_conc_fsd)
    coag_pos = [0.] * n
    coag_neg = [0.] * n
    for _ in range(ndt_mrg):
        for kx in range(n):
            coag_pos[kx] = 0.
            for ky in range(kx + 1):
                a = alpha[kx][ky]
                sum_mergers = 0.
                if a < n:
                    for p in range(a, n):
                        sum_mergers += tmp[p]
                coag_pos[kx] = coag_pos[kx] + asc[ky] * tmp[ky] * old_conc_tot * (
                    sum_mergers + (tmp[a - 1] / asb[a - 1]) * (asu[a - 1] - asu[kx] + asc[ky]))
        coag_neg[0] = 0.
        tmp[0] = tmp[0] - subdt * kappa * (coag_pos[0] - coag_neg[0])
        for m in range(1, n):
            coag_neg[m] = coag_pos[m - 1]
            tmp[m] = tmp[m] - subdt * kappa * (coag_pos[m] - coag_neg[m])
        unbroken_area_loss = unbroken_area_loss + subdt * kappa * coag_pos[n - 1]
        if cfg["debug_fsd"]:
            for m in range(n):
                if tmp[m] < -1e-11 or tmp[m] > 1. or subdt * kappa * coag_pos[m] < -1e-11:
                    crash = True
    tmp[n - 1] = tmp[n - 1] + unbroken_area_loss
    new_tot = 0.
    for v in tmp:
        new_tot = new_tot + v
    conc_loss = new_tot - old_conc_tot
    if abs(conc_loss) > 1.e-6:
        crash = True
    for m in range(n):
        v = _div(tmp[m] * old_conc_tot, new_tot)
        if v < 0.:
            if v < -1e-12:
                crash = True
            else:
                v = 0.
                zeroed = True
        fsd[m][cpt] = v
    return ndt_mrg, crash, zeroed


def weld(st, cfg, ddt, freezing):
    """What nxs_dyn_fsd_weld does: per element with freezing set (thermo's del_hi > 0) weldingRoach (FE.cpp:5783-5796) and then the mechanical healing
    (FE.cpp:5888-5896).  Returns (ndt_mrg per element: -1 = not freezing, 0 = below the gate; crash; number of zeroed bins' elements)."""
    n = cfg["num_bins"]
    ndt = np.full(st["conc"].size, -1, np.int64)
    crash = False
    zeroed = 0
    for i in range(st["conc"].size):
        if not freezing[i]:
            continue
        ndt[i] = 0
        if cfg["welding_type"] == WELD_ROACH:
            ndt[i], c, z = welding_roach(st, cfg, i, ddt)
            crash |= c
            zeroed += z
        if cfg["distinguish_mech_fsd"]:
            w = min(1., _div(ddt, float(st["time_relaxation_damage"][i])))
            for m in range(n):
                st["conc_mech_fsd"][m][i] = float(st["conc_mech_fsd"][m][i]) * (1. - w) + w * float(st["conc_fsd"][m][i])
    return ndt, crash, zeroed


def default_config(n, tables, young, **over):
    """The options of model/options.cpp for wave_coupling.* where they matter to the loops, as a cfg dict."""
    cfg = dict(num_bins=n, tables=tables, young=bool(young), breakup_type=UNIFORM_SIZE, breakup_prob_type=0, fsd_damage_type=0, welding_type=WELD_ROACH,
               distinguish_mech_fsd=0, debug_fsd=0, breakup_cell_average_thickness=0, breakup_coef1=0.5, breakup_coef2=0.05, breakup_coef3=0.1,
               breakup_prob_cutoff=0.0015, breakup_timescale_tuning=1800., cpl_time_step=2400., floes_flex_young=4.e9, breakup_thick_min=0.1, fsd_damage_max=0.99,
               welding_kappa=0.01)
    cfg.update(over)
    return cfg


def library_options(cfg):
    """The keyword options of FiniteElementDynamics.fsd_configure for a cfg dict."""
    return {k: v for k, v in cfg.items() if k not in ("tables", "young", "num_bins")}


# ---- inputs that reach every branch (shared by the CPU invariants and the GPU comparisons) ------------------------------------------------------------------

def standard_tables(n):
    """CONSTANT_SIZE bins of 10 m from 10 m, scaled areas: what the tests configure the library with."""
    return fsd_tables(CONSTANT_SIZE, n, 10., 10., True)


def _groups(rng, Ne, fractions):
    """A random group number per element with (at least) the given fractions."""
    g = np.repeat(np.arange(len(fractions)), np.ceil(np.asarray(fractions) * Ne).astype(int) + 1)[:Ne]
    g = np.concatenate([g, np.full(Ne - g.size, len(fractions) - 1, g.dtype)])
    return rng.permutation(g)


def _weights(rng, n, Ne, top=1.):
    """[n, Ne] positive weights that sum to one per element (more of it in the highest bin with top > 1)."""
    w = rng.dirichlet([1.] * (n - 1) + [top], Ne).T if n > 1 else np.ones((1, Ne))
    return np.ascontiguousarray(w)


def _split_young(rng, ctot, young):
    """conc and conc_young whose sum is ctot bit for bit (the young share is zero without the category)."""
    cy = np.where(ctot > 0., rng.uniform(0.05, 0.3, ctot.size) * ctot, 0.) if young else np.zeros_like(ctot)
    conc = ctot - cy
    fix = (conc + cy) != ctot
    cy[fix] = 0.; conc[fix] = ctot[fix]
    return conc, cy


def update_inputs(n, Ne, young, seed=1):
    """A state for updateFSD with every branch of UPDATE_BRANCHES on at least 5 % of the elements (a few of the ctot >= 1 elements with ctot2 == 0)."""
    rng = np.random.default_rng(seed)
    g = _groups(rng, Ne, [0.15, 0.15, 0.15, 0.2, 0.35])
    ctot = rng.uniform(0.2, 0.95, Ne)
    ctot[g == 0] = 0.
    ctot[g == 1] = 1.
    w, wm = _weights(rng, n, Ne, 3.), _weights(rng, n, Ne, 2.)
    scale = np.where(g == 4, rng.uniform(0.8, 1.2, Ne), 1.)            # g == 3: the sum of the bins is ctot up to the rounding of n additions
    scale[g == 1] = rng.uniform(0.9, 1.3, (g == 1).sum())
    fsd, mech = w * ctot * scale, wm * ctot * scale
    fsd[:, (g == 0) | (g == 2)] = 0.; mech[:, (g == 0) | (g == 2)] = 0.
    zero_at_one = np.flatnonzero(g == 1)[:3]
    fsd[:, zero_at_one] = 0.
    conc, cy = _split_young(rng, ctot, young)
    return dict(conc=conc, conc_young=cy, conc_fsd=np.ascontiguousarray(fsd), conc_mech_fsd=np.ascontiguousarray(mech))


WELD_K = 6.   # ddt * welding_kappa * area_scaled_up[n - 1]: stability = WELD_K * old_conc_tot


def weld_inputs(n, Ne, seed=2):
    """Bins for weldingRoach: by total concentration below the gate (< 0.1), ndt_mrg = 1 (0.12 .. 0.16), 2 (0.2 .. 0.3) and >= 5 (0.7 .. 0.95) with
    welding_kappa = WELD_K / (ddt * area_scaled_up[n - 1]); a fifth of the elements not freezing; mechanical bins of their own and healing times on both sides
    of ddt."""
    rng = np.random.default_rng(seed)
    g = _groups(rng, Ne, [0.2, 0.2, 0.2, 0.2, 0.2])
    lo = np.array([0.02, 0.12, 0.2, 0.7, 0.3])[g]; hi = np.array([0.09, 0.16, 0.3, 0.95, 0.9])[g]
    tot = rng.uniform(lo, hi)
    fsd = _weights(rng, n, Ne, 2.) * tot
    mech = _weights(rng, n, Ne, 2.) * tot
    freezing = (g != 4).astype(np.uint8)
    theal = np.where(rng.random(Ne) < 0.5, rng.uniform(100., 800., Ne), rng.uniform(1e3, 1e6, Ne))
    return dict(conc_fsd=np.ascontiguousarray(fsd), conc_mech_fsd=np.ascontiguousarray(mech), time_relaxation_damage=theal, conc=tot.copy(),
                conc_young=np.zeros(Ne)), freezing, g


def breakup_inputs(n, Ne, young, tables, seed=3):
    """A state and M_wlbk for redistributeFSD: 15 % without ice, 25 % with wlbk >= 499 (untouched), 15 % of the rest with M_thick exactly 0; wavelengths between
    a fifth of the smallest and five times the largest bin centre (both sides of the zero of tanh((D - coef1 lambda) / (coef2 lambda)), far into its
    saturation), thicknesses 0.05 .. 3 m (d_flex on both sides of the lowest centres)."""
    rng = np.random.default_rng(seed)
    g = _groups(rng, Ne, [0.15, 0.25, 0.15, 0.45])
    ctot = rng.uniform(0.15, 0.98, Ne)
    ctot[g == 0] = 0.
    c = tables["bin_centres"]
    wlbk = np.exp(rng.uniform(np.log(c[0] / 5.), np.log(min(5. * c[-1], 498.)), Ne))
    wlbk[g == 1] = rng.choice([499., 500., 1000.], (g == 1).sum())
    wlbk[np.flatnonzero(g == 3)[:2]] = [498.999, 5.]
    thick = rng.uniform(0.05, 3., Ne) * ctot
    thick[(g == 2) | (g == 0)] = 0.
    fsd = _weights(rng, n, Ne, 4.) * ctot
    mech = _weights(rng, n, Ne, 4.) * ctot
    conc, cy = _split_young(rng, ctot, young)
    hy = np.where(cy > 0., rng.uniform(0.01, 0.1, Ne), 0.)
    st = dict(conc=conc, conc_young=cy, thick=thick, h_young=hy, damage=rng.uniform(0., 0.9, Ne), conc_fsd=np.ascontiguousarray(fsd),
              conc_mech_fsd=np.ascontiguousarray(mech), cum_damage=rng.uniform(0., 0.3, Ne), cum_wave_damage=rng.uniform(0., 0.1, Ne))
    return st, wlbk, g


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
