"""A line-faithful restatement of thermo()'s slab loop in model/finiteelement.cpp ("FE.cpp") as an OASIS (wave-coupled) build compiles it, FE.cpp:5413-6133,
without the OceanType::COUPLED guards (5826-5841: M_sst and M_sss are updated as by a slab ocean): everything tests/slab_ref.py restates, line by line again, plus
melt_type 3 (5592-5640), the FSD branches of the limit block (5729-5764, the else of 5754 where the reference has it), redistributeThermoFSD (5768-5776,
4487-4670), the in-loop weldingRoach (5779-5797: fsd_ref.welding_roach) and the mechanical healing of 9.b (5883-5898).  Scalar per element in the manner of
slab_ref (numpy float64 scalars, the reference's operand order, std::max / std::min argument order, no contraction); pow is the C library's through ctypes.
abs(lat_melt_rate) of FE.cpp:4519 is unqualified in the reference: the floating-point absolute value is taken (an integer abs would make every melt rate 0).
Beside slab_ref's word, slab_coupled() returns a second word per element with a bit per FSD decision, in the order of nextsim_amd._abi.SLAB_FSD_BRANCHES
(NXS_SLAB_FSD_BR_* of include/nxs_dyn.h).

PARITY WITH THE REFERENCE IS NOT PINNED, as for slab_ref: model/ cannot be compiled here, so no binary of the reference produced these numbers.
tests/test_slab_fsd_ref.py pins this restatement against slab_ref.slab (melt_type 1, 2: the same bits on every row) and against hand-computed elements.
Shared by tests/test_slab_fsd_ref.py, test_slab_fsd_abi.py, test_gpu_slab_fsd.py and scripts/time_slab_coupled.py."""
from __future__ import annotations

import numpy as np

import column_ref as CR
import fluxes_ref as FR
import fsd_ref as FS
import slab_ref as R
from column_ref import F, _max, _min, rhow, cpw, rhoi, rhos, Lf, C, ki, si, hmin
from slab_ref import BIT, ROWS, FLUX, COL, IN_PLACE, cmin, days_in_sec, melt_ponds, _pow, _round, _shift
from nextsim_amd import _abi

BRANCHES2 = _abi.SLAB_FSD_BRANCHES
BIT2 = {k: 1 << i for i, k in enumerate(BRANCHES2)}
# the planted mistakes of tests/test_slab_fsd_ref.py: slab_coupled(drop=...) makes one of them
MISTAKES = ("no_factor_2", "unbroken_le", "else_outer", "ctot_init_4565", "m_lt_nb_4545", "heal_old_theal")


def took2(words2, name):
    return (words2 & np.uint32(BIT2[name])) != 0


def redistribute_thermo_fsd(M_conc_fsd, M_conc_mech_fsd, M_fsd_bin_widths, M_fsd_bin_centres, M_num_fsd_bins, M_distinguish_mech_fsd, M_debug_fsd, i, ddt, lat_melt_rate,
                            young_ice_growth, old_conc, old_conc_young, M_conc, M_conc_young, young, drop=()):
    """redistributeThermoFSD(i, ddt, lat_melt_rate, young_ice_growth, old_conc, old_conc_young), FE.cpp:4487-4670.  Returns (the branch bits, crash: what the
    reference throws on under M_debug_fsd).  The mechanical bins' sum of 4631-4646 is checked where they are kept apart (elsewhere the reference has no M_conc_mech_fsd to read)."""
    z = F(0.)
    br2 = 0
    crash = False
    del_c_young = z
    del_c_fsd = M_conc - old_conc
    cat0_del_c = z
    ctot_init = z
    for m in range(M_num_fsd_bins):
        ctot_init = ctot_init + M_conc_fsd[m][i]
    fsd_init = [F(M_conc_fsd[m][i]) for m in range(M_num_fsd_bins)]
    if young:
        del_c_young = M_conc_young - old_conc_young
    del_c_fsd = del_c_fsd + del_c_young
    if (np.abs(lat_melt_rate) > 0.) and (ctot_init > 1e-12):
        br2 |= BIT2["lateral"]
        fsd_dr = [z] * (M_num_fsd_bins + 1)
        dfsd_dr = [z] * M_num_fsd_bins
        for m in range(1, M_num_fsd_bins - 1):
            fsd_dr[m] = M_conc_fsd[m][i] / M_fsd_bin_widths[m]
        for m in range(M_num_fsd_bins):
            dfsd_dr[m] = fsd_dr[m + 1] - fsd_dr[m]
        acc = z
        for v in dfsd_dr:
            acc = acc + v
        if (np.abs(acc) > 1e-11) and M_debug_fsd:
            crash = True
        for m in range(M_num_fsd_bins if "m_lt_nb_4545" in drop else M_num_fsd_bins - 1):
            del_c_bin_melt = ddt * lat_melt_rate * (-dfsd_dr[m] + fsd_init[m] * 2. / M_fsd_bin_centres[m])
            M_conc_fsd[m][i] = M_conc_fsd[m][i] + del_c_bin_melt
        if lat_melt_rate < 0.:
            br2 |= BIT2["lat_melting"]
            cat0_del_c = lat_melt_rate * fsd_init[0] / M_fsd_bin_widths[0] * ddt
            M_conc_fsd[0][i] = M_conc_fsd[0][i] + cat0_del_c
        else:
            M_conc_fsd[M_num_fsd_bins - 1][i] = M_conc_fsd[M_num_fsd_bins - 1][i] + fsd_init[M_num_fsd_bins - 1] / M_fsd_bin_widths[M_num_fsd_bins - 1] * ddt * lat_melt_rate
        ctot = z
        for m in range(M_num_fsd_bins):
            ctot = ctot + M_conc_fsd[m][i]
        if young_ice_growth < 0:
            br2 |= BIT2["young_shrinks"]
            for m in range(M_num_fsd_bins):
                M_conc_fsd[m][i] = M_conc_fsd[m][i] + (young_ice_growth) * M_conc_fsd[m][i] / (ctot_init if "ctot_init_4565" in drop else ctot)
        if (M_conc_fsd[M_num_fsd_bins - 1][i] < -1e-11) and M_debug_fsd:
            crash = True
    else:
        if young:
            if M_conc + M_conc_young == 1.:
                br2 |= BIT2["fills_lead"]
                M_conc_fsd[M_num_fsd_bins - 1][i] = 1.
                for m in range(M_num_fsd_bins - 1):
                    M_conc_fsd[m][i] = 0.
            elif del_c_fsd >= 0:
                br2 |= BIT2["del_c_fsd_ge0"]
                M_conc_fsd[M_num_fsd_bins - 1][i] = M_conc_fsd[M_num_fsd_bins - 1][i] + del_c_fsd
            else:
                for m in range(M_num_fsd_bins):
                    M_conc_fsd[m][i] = M_conc_fsd[m][i] + del_c_fsd * M_conc_fsd[m][i] / ctot_init
        else:
            M_conc_fsd[M_num_fsd_bins - 1][i] = M_conc_fsd[M_num_fsd_bins - 1][i] + del_c_fsd
    if M_distinguish_mech_fsd:
        ctot_mech = F(M_conc_mech_fsd[0][i])
        for j in range(1, M_num_fsd_bins):
            ctot_mech = ctot_mech + M_conc_mech_fsd[j][i]
        if del_c_fsd >= 0:
            M_conc_mech_fsd[M_num_fsd_bins - 1][i] = M_conc_mech_fsd[M_num_fsd_bins - 1][i] + del_c_fsd
        else:
            for m in range(M_num_fsd_bins):
                M_conc_mech_fsd[m][i] = M_conc_mech_fsd[m][i] + del_c_fsd * M_conc_mech_fsd[m][i] / ctot_mech
    if M_debug_fsd:
        if M_conc_fsd[M_num_fsd_bins - 1][i] < -1e-11:
            crash = True
        ctot = M_conc
        if young:
            ctot = ctot + M_conc_young
        ctot2 = F(M_conc_fsd[0][i])
        for j in range(1, M_num_fsd_bins):
            ctot2 = ctot2 + M_conc_fsd[j][i]
        if np.abs(ctot - ctot2) > 1e-7:
            crash = True
        if M_distinguish_mech_fsd:
            ctot3 = F(M_conc_mech_fsd[0][i])
            for j in range(1, M_num_fsd_bins):
                ctot3 = ctot3 + M_conc_mech_fsd[j][i]
            if np.abs(ctot - ctot3) > 1e-7:
                crash = True
    return br2, crash


def slab_coupled(inp, fsd, cfg, ccfg, fcfg, ocean_albedo, tri, young, dt, clock, melt_type=None, drop=(), qassm_shift=0, wspeed_shift=0, dtw_shift=0):
    """thermo(), FE.cpp:5413-6133 as an OASIS build compiles it.  inp, cfg, ccfg, ocean_albedo, tri, young, dt, clock: as slab_ref.slab.  fsd: {"conc_fsd":
    [nb, Ne], "conc_mech_fsd": [nb, Ne] or None}, updated in place like the IN_PLACE rows of inp.  fcfg: a cfg of fsd_ref.default_config (num_bins, tables,
    welding_type, welding_kappa, distinguish_mech_fsd, debug_fsd).  melt_type: what nxs_dyn_slab_coupled_configure overrides (None: cfg's).  Returns (the 29
    rows, the NXS_SLAB_BR_* words, the NXS_SLAB_FSD_BR_* words, info): info has thermo_fsd_crash, weld_crash and ndt_mrg [Ne] (-1: no welding asked, 0: below the
    gate).  drop: one of slab_ref.MISTAKES or of MISTAKES.  dtw_shift moves tw_new - tfrw, the argument of melt_type 3's pow, by that many units in the last
    place; qassm_shift / wspeed_shift as in slab_ref.slab."""
    Ne = tri.shape[0]
    ddt = F(dt)
    dtime_step = F(dt)
    qi = Lf * rhoi
    qs = Lf * rhos
    winton = ccfg["thermo_type"] == "winton"
    mu, M_ks = F(ccfg["freezingpoint_mu"]), F(ccfg["snow_cond"])
    newice_type, melt_type = int(cfg["newice_type"]), int(cfg["melt_type"] if melt_type is None else melt_type)
    assert 1 <= newice_type <= 4 and 1 <= melt_type <= 3
    nb = int(fcfg["num_bins"])
    M_conc_fsd, M_conc_mech_fsd = fsd["conc_fsd"], fsd.get("conc_mech_fsd")
    assert M_conc_fsd.shape == (nb, Ne) and nb >= 1                                  # the throw of FE.cpp:5595
    M_distinguish_mech_fsd, M_debug_fsd = bool(fcfg["distinguish_mech_fsd"]), bool(fcfg["debug_fsd"])
    assert not M_distinguish_mech_fsd or M_conc_mech_fsd is not None
    M_fsd_bin_widths, M_fsd_bin_centres = (np.asarray(fcfg["tables"][k], np.float64) for k in ("bin_widths", "bin_centres"))
    info = {"thermo_fsd_crash": False, "weld_crash": False, "ndt_mrg": np.full(Ne, -1, np.int64)}
    rh0 = F(1.) / F(cfg["hnull"])
    rPhiF = F(1.) / F(cfg["PhiF"])
    PhiF, PhiM = F(cfg["PhiF"]), F(cfg["PhiM"])
    h_young_min = F(cfg["h_young_min"])
    h_young_max_sharp = F(.5) * (h_young_min + F(cfg["h_young_max"]))          # FE.cpp:1198
    reset_by_date = bool(cfg["reset_by_date"])
    use_young_ice_in_myi_reset = bool(cfg["include_young_ice"]) and reset_by_date   # FE.cpp:5649-5650
    if "c_myi_max_no_young" in drop:
        use_young_myi_max = False
    else:
        use_young_myi_max = use_young_ice_in_myi_reset
    freeze_days_threshold = F(cfg["reset_freeze_days"])
    time_relaxation_damage, deltaT_relaxation_damage = F(cfg["time_relaxation_damage"]), F(cfg["deltaT_relaxation_damage"])
    M_ocean_albedo = F(ocean_albedo)
    out = {k: np.zeros(Ne) for k in ROWS}
    words = np.zeros(Ne, np.uint32)
    words2 = np.zeros(Ne, np.uint32)
    wspeed_row = None
    if newice_type == 3:
        wspeed_row = FR.wind_speed_element(inp["wind"], tri)
    fl = {k[2:]: inp[k] for k in FLUX}
    co = {k[2:]: inp[k] for k in COL}
    z = F(0.)
    with np.errstate(all="ignore"):
        for i in range(Ne):
            br = 0
            br2 = 0
            lat_melt_rate = z                                                # FE.cpp:5471
            young_ice_growth = z                                             # FE.cpp:5473
            Qow = F(fl["Qow"][i])
            Qlw_ow, Qsw_ow, Qlh_ow, Qsh_ow, evap = fl["Qlw_ow"][i], fl["Qsw_ow"][i], fl["Qlh_ow"][i], fl["Qsh_ow"][i], fl["evap"][i]
            Qia, Qlwi, Qswi, Qlhi, Qshi, albedo = fl["Qia"][i], fl["Qlwi"][i], fl["Qswi"][i], fl["Qlhi"][i], fl["Qshi"][i], fl["albedo"][i]
            if young:
                Qia_young, Qlw_young, Qsw_young, Qlh_young, Qsh_young, albedo_young = (fl[k + "_young"][i] for k in ("Qia", "Qlw", "Qsw", "Qlh", "Qsh", "albedo"))
            else:
                Qia_young = Qlw_young = Qsw_young = Qlh_young = Qsh_young = albedo_young = z                   # FE.cpp:5265-5273
            tmp_snowfall, Qdw, Fdw, tfrw = co["snowfall"][i], co["Qdw"][i], co["Fdw"][i], co["tfrw"][i]
            Qio, hi, hs, hi_old, del_hi, del_hs_mlt, mlt_hi_top, mlt_hi_bot, del_hi_s2i = (F(co[k][i]) for k in CR.ICE_ROWS)
            Qio_young, _, _, _, del_hi_young, del_hs_young_mlt, mlt_hi_top_young, mlt_hi_bot_young, del_hi_s2i_young = (F(co[k][i]) for k in CR.YOUNG_ROWS)
            M_precip = inp["precip"][i]
            mld = F(inp["mld"][i]) if ccfg["mld_source"] == "row" else F(ccfg["constant_mld"])
            M_conc, M_thick, M_ridge_ratio = F(inp["conc"][i]), F(inp["thick"][i]), F(inp["ridge_ratio"][i])
            M_conc_myi, M_thick_myi = F(inp["conc_myi"][i]), F(inp["thick_myi"][i])
            M_conc_young = M_h_young = M_hs_young = z
            if young:
                M_conc_young, M_h_young, M_hs_young = F(inp["conc_young"][i]), F(inp["h_young"][i]), F(inp["hs_young"][i])
            M_sst, M_sss = F(inp["sst"][i]), F(inp["sss"][i])
            tice0 = F(inp["tice0"][i])
            tice1, tice2 = (F(inp["tice1"][i]), F(inp["tice2"][i])) if winton else (z, z)
            M_del_vi_tend, M_freeze_days, M_freeze_onset = F(inp["del_vi_tend"][i]), F(inp["freeze_days"][i]), F(inp["freeze_onset"][i])
            M_conc_summer, M_thick_summer = F(inp["conc_summer"][i]), F(inp["thick_summer"][i])
            M_fyi_fraction, M_age_det, M_age = F(inp["fyi_fraction"][i]), F(inp["age_det"][i]), F(inp["age"][i])
            old_vol = M_thick
            old_conc = M_conc
            old_conc_young = M_conc_young
            old_conc_tot = old_conc + old_conc_young
            old_ow_fraction = 1. - old_conc_tot

            # FE.cpp:5413-5425
            Qassm = z
            if cfg["use_assim_flux"]:
                M_conc_upd = F(inp["conc_upd"][i])
                conc_pre_assim = old_conc + old_conc_young - M_conc_upd
                if conc_pre_assim > 0 and M_conc_upd < 0:
                    br |= BIT["assim"]
                    Qassm = (Qow * old_ow_fraction + Qio * old_conc + Qio_young * old_conc_young) * (
                        F(_pow(float(M_conc_upd / conc_pre_assim + 1), float(cfg["assim_flux_exponent"]))) - 1)
                    Qassm = _shift(Qassm, qassm_shift)

            # 6) FE.cpp:5434-5646
            tw_new = M_sst - ddt * (Qow + Qassm) / (mld * rhow * cpw)
            newice = z
            if (tw_new <= tfrw) if "tw_le" in drop else (tw_new < tfrw):
                br |= BIT["supercooled"]
                newice = old_ow_fraction * (tfrw - tw_new) * mld * rhow * cpw / qi
                Qow = -(tfrw - M_sst) * mld * rhow * cpw / ddt
            newice_stored = newice
            del_vi = newice + del_hi * old_conc
            mlt_vi_top = mlt_hi_top * old_conc
            mlt_vi_bot = mlt_hi_bot * old_conc
            del_vs_mlt = del_hs_mlt * old_conc
            snow2ice = del_hi_s2i * old_conc
            del_vi_young = z
            if young:
                del_vi_young = del_vi_young + del_hi_young * old_conc_young
                if "del_vi_no_young" not in drop:
                    del_vi = del_vi + del_hi_young * old_conc_young
                mlt_vi_top = mlt_vi_top + mlt_hi_top_young * old_conc_young
                mlt_vi_bot = mlt_vi_bot + mlt_hi_bot_young * old_conc_young
                snow2ice = snow2ice + del_hi_s2i_young * old_conc_young
                del_vs_mlt = del_vs_mlt + del_hs_young_mlt * old_conc_young
            del_c = z
            newsnow = z
            if newice_type == 1:
                del_c = newice * rh0
            elif newice_type == 2:
                if hi_old > 0.:
                    br |= BIT["n2_hi_old"]
                    del_c = newice * PhiF / hi_old
                elif newice > 0.:
                    br |= BIT["n2_newice"]
                    del_c = F(1.)
                else:
                    del_c = z
            elif newice_type == 3:
                wspeed = _shift(F(wspeed_row[i]), wspeed_shift)
                h0 = (1. + 0.1 * wspeed) / 15.
                if rPhiF * hi_old < h0:
                    br |= BIT["n3_h0"]
                del_c = newice / _max(rPhiF * hi_old, h0)
            else:
                M_h_young = M_h_young + newice
                M_conc_young = _min(1. - M_conc, M_conc_young + newice / h_young_min)
                newice = z
                newsnow = z
                if M_conc_young > 0.:
                    br |= BIT["n4_young"]
                    if M_h_young < h_young_min * M_conc_young:
                        br |= BIT["n4_not_filled"]
                        M_conc_young = M_h_young / h_young_min
                        young_ice_growth = M_conc_young - old_conc_young         # FE.cpp:5518
                    else:
                        hiy = M_h_young / M_conc_young
                        if hiy > h_young_max_sharp:
                            br |= BIT["n4_sharp"]
                            hsy = _max(0., M_hs_young / M_conc_young)
                            tmp = M_conc_young * (h_young_max_sharp - h_young_min) / (hiy - h_young_min)
                            del_c = _max(0., M_conc_young - tmp)
                            M_conc_young = tmp
                            tmp = M_conc_young * h_young_max_sharp
                            newice = _max(0., M_h_young - tmp)
                            M_h_young = tmp
                            tmp = M_conc_young * hsy
                            newsnow = _max(0., M_hs_young - tmp)
                            M_hs_young = tmp
                else:
                    br |= BIT["n4_no_room"]
                    if "no_room_no_thick" not in drop:
                        M_thick = M_thick + M_h_young
                    newice = M_h_young
                    newsnow = M_hs_young
                    M_h_young = z
                    M_hs_young = z
            if "no_del_c_bound" not in drop:
                del_c = _min(1. - M_conc, del_c)
            if del_hi < 0.:
                br |= BIT["melt"]
                if melt_type == 1:
                    if M_conc < 1.:
                        br |= BIT["melt_side"]
                        del_c = del_c + del_hi * M_conc * PhiM / hi_old
                    else:
                        del_c = del_c + 0.
                elif melt_type == 2:
                    if hi > 0.:
                        br |= BIT["melt_side"]
                        del_c = del_c + PhiM * (1. - M_conc) * _min(0., Qow) * ddt / (hi * qi + hs * qs)
                        if "qow_not_scaled" not in drop:
                            Qow = Qow * (1. - PhiM)
                    else:
                        del_c = -M_conc
                elif tw_new > tfrw:                                          # 3: FE.cpp:5592-5640
                    br2 |= BIT2["melt3"]
                    m1 = F(3.e-6)
                    m2 = F(1.36)
                    del_c_melt = z
                    cat0_del_c = z
                    if hi > 0:
                        ctot = M_conc + M_conc_young
                        if ctot < 1e-11:
                            br2 |= BIT2["ctot_break"]                          # the break of FE.cpp:5611
                        else:
                            h0 = z
                            if M_conc_young > 0.:
                                h0 = h_young_min + 2. * (M_h_young - h_young_min * M_conc_young) / (M_conc_young)
                            dist = np.abs(M_conc_fsd[nb - 1][i] - ctot)
                            if (dist <= 1e-7) if "unbroken_le" in drop else (dist < 1e-7):
                                br2 |= BIT2["unbroken"]
                                del_c_melt = del_c_melt + PhiM * (1. - ctot) * _min(0., Qow) * ddt / (hi * qi + hs * qs)
                                del_c_melt = _max(del_c_melt, -ctot)
                                Qow = Qow * (1. - PhiM)
                            else:
                                lat_melt_rate = -m1 * F(_pow(float(_shift(tw_new - tfrw, dtw_shift)), float(m2)))
                                if "no_factor_2" not in drop:
                                    lat_melt_rate = lat_melt_rate * 2.
                                cat0_del_c = lat_melt_rate * M_conc_fsd[0][i] / M_fsd_bin_widths[0] * ddt
                                del_c_melt = del_c_melt + cat0_del_c
                                for j in range(nb - 1):
                                    del_c_melt = del_c_melt + lat_melt_rate * (M_conc_fsd[j][i] * 2. / M_fsd_bin_centres[j]) * ddt
                                Qow = Qow - del_c_melt * (hi * qi * M_conc + h0 * qi * M_conc_young) / (ddt * ctot)
                            del_c = del_c + (M_conc / ctot) * del_c_melt
                            M_conc_young = M_conc_young + del_c_melt * (M_conc_young / ctot)

            def freeze_days_block(M_conc, M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br):   # FE.cpp:5649-5682
                if clock["first_step_of_day"]:
                    M_del_vi_tend = z
                M_del_vi_tend = M_del_vi_tend + del_vi * ddt
                if clock["last_step_of_day"]:
                    if M_del_vi_tend > 0.:
                        br |= BIT["day_freeze"]
                        M_freeze_days = M_freeze_days + 1.
                    elif M_del_vi_tend < 0.:
                        br |= BIT["day_melt"]
                        M_freeze_days = z
                        conc_summer = M_conc + _min(0., del_c)
                        thick_summer = M_thick + _min(0., del_vi)
                        if young and use_young_ice_in_myi_reset:
                            conc_summer = conc_summer + M_conc_young
                            thick_summer = thick_summer + M_h_young
                        M_conc_summer = _max(0., _min(1., conc_summer))
                        M_thick_summer = _max(0., thick_summer)
                return M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br

            if "freeze_days_after_conc" not in drop:
                M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br = freeze_days_block(M_conc, M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br)
            # FE.cpp:5685-5711
            M_conc = M_conc + del_c
            if "freeze_days_after_conc" in drop:
                M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br = freeze_days_block(M_conc, M_del_vi_tend, M_freeze_days, M_conc_summer, M_thick_summer, br)
            if M_conc >= cmin:
                br |= BIT["conc_ge_cmin"]
                hi = (hi * old_conc + newice) / M_conc
                if del_c < 0.:
                    br |= BIT["del_c_neg"]
                if (del_c >= 0.) if "hs_wrong_side" in drop else (del_c < 0.):
                    Qow = Qow - del_c * hs * qs / ddt
                else:
                    hs = (hs * old_conc + newsnow) / M_conc
                if winton:
                    f1 = M_thick / (M_thick + newice)
                    Tbar = f1 * (tice1 - Lf * mu * si / (C * tice1)) + (1 - f1) * tfrw
                    tice1 = (Tbar - np.sqrt(Tbar * Tbar + 4 * mu * si * Lf / C)) / 2.
                    tice2 = f1 * tice2 + (1 - f1) * tfrw
            # FE.cpp:5714-5728
            if M_conc < cmin or hi < hmin:
                br |= BIT["limit"]
                Qow = Qow + (M_conc * hi * qi / ddt + M_conc * hs * qs / ddt)
                M_conc = z
                tice0 = -mu * si
                if winton:
                    tice1 = tice2 = -mu * si
                hi = z
                hs = z
                M_ridge_ratio = z
                # FE.cpp:5729-5764: the else of 5754 belongs to if (M_distinguish_mech_fsd)
                ctot = z
                ctot_mech = z
                for m in range(nb):
                    ctot = ctot + M_conc_fsd[m][i]
                rescale = (ctot > old_conc) and young and (M_conc_young > 0.)
                if rescale:
                    br2 |= BIT2["limit_rescaled"]
                    for m in range(nb):
                        M_conc_fsd[m][i] = M_conc_fsd[m][i] + (-old_conc) * M_conc_fsd[m][i] / ctot
                if M_distinguish_mech_fsd:
                    for m in range(nb):
                        ctot_mech = ctot_mech + M_conc_mech_fsd[m][i]
                    if (ctot_mech > old_conc) and young and (M_conc_young > 0.):
                        br2 |= BIT2["limit_mech_rescaled"]
                        for m in range(nb):
                            M_conc_mech_fsd[m][i] = M_conc_mech_fsd[m][i] + (-old_conc) * M_conc_mech_fsd[m][i] / ctot_mech
                if (not rescale) if "else_outer" in drop else (not M_distinguish_mech_fsd):
                    br2 |= BIT2["limit_zeroed"]
                    for k in range(nb):
                        M_conc_fsd[k][i] = z
                        if M_distinguish_mech_fsd:
                            M_conc_mech_fsd[k][i] = z
            elif melt_type == 3:                                             # FE.cpp:5768-5776
                b, crash = redistribute_thermo_fsd(M_conc_fsd, M_conc_mech_fsd, M_fsd_bin_widths, M_fsd_bin_centres, nb, M_distinguish_mech_fsd, M_debug_fsd, i, ddt,
                                                   lat_melt_rate, young_ice_growth, old_conc, old_conc_young, M_conc, M_conc_young, young, drop)
                br2 |= b
                info["thermo_fsd_crash"] |= crash
            # 6.b) FE.cpp:5783-5796
            if del_hi > 0.:
                info["ndt_mrg"][i] = 0
                if fcfg["welding_type"] == FS.WELD_ROACH:
                    ndt, crash, _ = FS.welding_roach(fsd, fcfg, i, float(ddt))
                    info["ndt_mrg"][i] = ndt
                    info["weld_crash"] |= crash
                    if ndt > 0:
                        br2 |= BIT2["welded"]
            # 7)
            M_thick = hi * M_conc
            M_snow_thick = hs * M_conc
            # 8) FE.cpp:5812-5846
            rain_on_ice = _max(0., M_precip - tmp_snowfall)
            rain = (1. - old_conc - old_conc_young) * M_precip + (old_conc + old_conc_young) * rain_on_ice
            emp = evap * (1. - old_conc - old_conc_young) - rain
            if cfg["use_meltponds"]:
                pv, lv, pf, br = melt_ponds(cfg, mu, br, ddt, hi, hs, mlt_hi_top, del_hs_mlt, Qia, rain_on_ice, M_conc, M_thick, tice0, F(inp["pond_volume"][i]),
                                            F(inp["lid_volume"][i]), F(inp["pond_fraction"][i]))
                inp["pond_volume"][i], inp["lid_volume"][i], inp["pond_fraction"][i] = pv, lv, pf
            if "qio_mean_no_young" in drop:
                Qio_mean = Qio * old_conc
            else:
                Qio_mean = Qio * old_conc + Qio_young * old_conc_young
            Qow_mean = Qow * old_ow_fraction
            M_sst = M_sst - ddt * (Qio_mean + Qow_mean - Qdw + Qassm) / (rhow * cpw * mld)
            denominator = (mld * rhow - del_vi * rhoi - (del_vs_mlt * rhos + (emp - Fdw) * ddt))
            if not (denominator > 1. * rhow):
                br |= BIT["denom_clamp"]
                denominator = 1. * rhow
            si_eff = si if "si_not_eff" in drop else _min(M_sss, si)
            if M_sss < si:
                br |= BIT["sss_below_si"]
            delsss = ((M_sss - si_eff) * rhoi * del_vi + M_sss * (del_vs_mlt * rhos + (emp - Fdw) * ddt)) / denominator
            M_sss = M_sss + delsss
            if M_thick > old_vol:
                br |= BIT["ridge"]
            if (M_thick > old_vol) or ("ridge_on_melt" in drop and M_thick > 0.):
                M_ridge_ratio = M_ridge_ratio * (old_vol / M_thick)
            old_time_relaxation_damage = F(inp["time_relaxation_damage"][i])
            # 9) FE.cpp:5854-5881
            if cfg["temp_dep_healing"]:
                if M_thick > 0.:
                    br |= BIT["heal_ice"]
                    Tbot = F(CR.freezing_point(ccfg, M_sss))
                    if not winton:
                        Cc = ki * M_snow_thick / (M_ks * M_thick)
                        deltaT = _max(1e-36, Tbot - tice0) / (1. + Cc)
                    else:
                        Cc = ki * M_snow_thick / (M_ks * M_thick / 4.)
                        deltaT = _max(1e-36, Tbot + Cc * (Tbot - tice1) - tice0) / (1. + Cc)
                    inp["time_relaxation_damage"][i] = _max(time_relaxation_damage * deltaT_relaxation_damage / deltaT, ddt)
                else:
                    inp["time_relaxation_damage"][i] = 1e36
            # 9.b) FE.cpp:5883-5898
            if M_distinguish_mech_fsd and del_hi > 0.:
                br2 |= BIT2["healed"]
                theal = old_time_relaxation_damage if "heal_old_theal" in drop else F(inp["time_relaxation_damage"][i])
                fsd_mech_healing_weight = _min(1., ddt / theal)
                for m in range(nb):
                    M_conc_mech_fsd[m][i] = M_conc_mech_fsd[m][i] * (1. - fsd_mech_healing_weight) + fsd_mech_healing_weight * M_conc_fsd[m][i]
            # 10) FE.cpp:5903-5976
            o = {}
            o["Qa"] = Qia * old_conc + Qia_young * old_conc_young + Qow * old_ow_fraction
            o["Qsw"] = Qswi * old_conc + Qsw_young * old_conc_young + Qsw_ow * old_ow_fraction
            o["Qlw"] = Qlwi * old_conc + Qlw_young * old_conc_young + Qlw_ow * old_ow_fraction
            o["Qsh"] = Qshi * old_conc + Qsh_young * old_conc_young + Qsh_ow * old_ow_fraction
            o["Qlh"] = Qlhi * old_conc + Qlh_young * old_conc_young + Qlh_ow * old_ow_fraction
            o["Qo"] = Qio_mean + Qow_mean
            o["Qnosun"] = Qio_mean + old_ow_fraction * (Qlw_ow + Qlh_ow + Qsh_ow)
            o["Qsw_ocean"] = old_ow_fraction * Qsw_ow
            o["Qassim"] = Qassm
            o["delS"] = delsss * rhow * mld * days_in_sec / dtime_step
            o["fwflux_ice"] = -1. / ddt * ((1. - 1e-3 * si_eff) * rhoi * del_vi + rhos * del_vs_mlt)
            o["fwflux"] = o["fwflux_ice"] - emp
            o["brine"] = -1e-3 * si_eff * rhoi * del_vi / ddt
            o["evap"] = evap * (1. - old_conc - old_conc_young)
            o["rain"] = rain
            o["vice_melt"] = del_vi * days_in_sec / ddt
            o["del_vi_young"] = del_vi_young * days_in_sec / ddt
            o["del_hi"] = del_hi * days_in_sec / ddt
            o["del_hi_young"] = del_hi_young * days_in_sec / ddt
            o["newice"] = newice_stored * days_in_sec / ddt
            o["mlt_top"] = mlt_vi_top * days_in_sec / ddt
            o["mlt_bot"] = mlt_vi_bot * days_in_sec / ddt
            o["snow2ice"] = snow2ice * days_in_sec / ddt
            sialb = old_conc * albedo
            if young:
                sialb = sialb + old_conc_young * albedo_young
            o["albedo"] = sialb + _max(0., old_ow_fraction) * M_ocean_albedo
            o["sialb"] = (sialb / old_conc_tot) if old_conc_tot > 0. else z
            # 10) FE.cpp:5980-6132
            del_vi_rplnt_myi = del_ci_rplnt_myi = del_vi_mlt_myi = del_ci_mlt_myi = z
            if M_conc < cmin or M_thick < M_conc * hmin:
                br |= BIT["no_ice_tracers"]
                M_fyi_fraction = M_age_det = M_age = M_thick_myi = M_conc_myi = M_freeze_days = z
                M_freeze_onset = F(1.)
            else:
                if clock["fyi_reset_now"]:
                    M_fyi_fraction = z
                else:
                    conc_fyi = M_fyi_fraction + del_c
                    M_fyi_fraction = _max(0., _min(1., conc_fyi))
                if "w_age_new_conc" in drop:
                    w_age = z if M_conc <= 0 else _min(M_conc / M_conc, 1.)
                else:
                    w_age = z if old_conc <= 0 else _min(old_conc / M_conc, 1.)
                M_age_det = w_age * (M_age_det + ddt) + _max((1 - w_age) * ddt, 0.)
                w_age = z if old_vol <= 0 else _min(old_vol / M_thick, 1.)
                M_age = w_age * (M_age + ddt) + _max((1 - w_age) * ddt, 0.)
                reset_myi = False
                if reset_by_date:
                    if clock["myi_reset_now"]:
                        reset_myi = True
                elif M_freeze_days >= freeze_days_threshold:
                    br |= BIT["freeze_days_ge"]
                    if M_freeze_onset <= 0.5:
                        reset_myi = True
                        M_freeze_onset = F(1.)
                if clock["onset_reset_now"]:
                    M_freeze_onset = z
                    ctot = M_conc
                    if young:
                        ctot = ctot + M_conc_young
                    if ctot == 0.:
                        M_freeze_onset = F(1.)
                    conc_summer = M_conc
                    thick_summer = M_thick
                    if young and use_young_ice_in_myi_reset:
                        conc_summer = conc_summer + M_conc_young
                        thick_summer = thick_summer + M_h_young
                    M_conc_summer = _max(0., _min(1., conc_summer))
                    M_thick_summer = _max(0., thick_summer)
                M_freeze_onset = F(_round(M_freeze_onset))
                old_conc_myi = M_conc_myi
                old_thick_myi = M_thick_myi
                c_myi_max = M_conc
                v_myi_max = M_thick
                if young and use_young_myi_max:
                    c_myi_max = c_myi_max + M_conc_young
                    v_myi_max = v_myi_max + M_h_young
                if reset_myi:
                    br |= BIT["reset"]
                    if not reset_by_date:
                        c_myi_reset = _max(M_conc_summer, M_conc_myi)
                        v_myi_reset = _max(M_thick_summer, M_thick_myi)
                        M_conc_myi = _min(c_myi_max, c_myi_reset)
                        M_thick_myi = _min(v_myi_max, v_myi_reset)
                    else:
                        M_conc_myi = c_myi_max
                        M_thick_myi = v_myi_max
                    M_conc_myi = _max(0., _min(1., M_conc_myi))
                    M_thick_myi = _max(0., M_thick_myi)
                    del_ci_rplnt_myi = M_conc_myi - old_conc_myi
                    del_vi_rplnt_myi = M_thick_myi - old_thick_myi
                elif M_thick < old_vol and old_conc > 0 and old_vol > 0:
                    br |= BIT["old_melt"]
                    if cfg["equal_melting"]:
                        del_c_ratio = _min(M_conc / old_conc, 1.)
                        del_v_ratio = _min(M_thick / old_vol, 1.)
                        del_ci_mlt_myi = _min(0., M_conc_myi * (del_c_ratio - 1.))
                        del_vi_mlt_myi = _min(0., M_thick_myi * (del_v_ratio - 1.))
                    M_conc_myi = _max(0., _min(c_myi_max, M_conc_myi + del_ci_mlt_myi))
                    M_thick_myi = _max(0., _min(v_myi_max, M_thick_myi + del_vi_mlt_myi))
                    del_ci_mlt_myi = M_conc_myi - old_conc_myi
                    del_vi_mlt_myi = M_thick_myi - old_thick_myi
            o["del_ci_mlt_myi"] = del_ci_mlt_myi * days_in_sec / ddt
            o["del_vi_mlt_myi"] = del_vi_mlt_myi * days_in_sec / ddt
            o["del_ci_rplnt_myi"] = del_ci_rplnt_myi * days_in_sec / ddt
            o["del_vi_rplnt_myi"] = del_vi_rplnt_myi * days_in_sec / ddt
            for k in ROWS:
                out[k][i] = o[k]
            inp["conc"][i], inp["thick"][i], inp["snow_thick"][i], inp["ridge_ratio"][i] = M_conc, M_thick, M_snow_thick, M_ridge_ratio
            inp["conc_myi"][i], inp["thick_myi"][i] = M_conc_myi, M_thick_myi
            if young:
                inp["conc_young"][i], inp["h_young"][i], inp["hs_young"][i] = M_conc_young, M_h_young, M_hs_young
            inp["sst"][i], inp["sss"][i], inp["tice0"][i] = M_sst, M_sss, tice0
            if winton:
                inp["tice1"][i], inp["tice2"][i] = tice1, tice2
            inp["del_vi_tend"][i], inp["freeze_days"][i], inp["freeze_onset"][i] = M_del_vi_tend, M_freeze_days, M_freeze_onset
            inp["conc_summer"][i], inp["thick_summer"][i] = M_conc_summer, M_thick_summer
            inp["fyi_fraction"][i], inp["age_det"][i], inp["age"][i] = M_fyi_fraction, M_age_det, M_age
            words[i] = br
            words2[i] = br2
    return {k: np.ascontiguousarray(out[k], np.float64) for k in ROWS}, words, words2, info




# ---- designed inputs: slab_ref.make_inputs' strata, two of them split for the decisions only the bins bring, and bins that are unbroken on half of the ice
FSD_STRATA = ("ctot_break", "young_shrinks", "fills_lead")
WELD_K = FS.WELD_K   # ddt * welding_kappa * area_scaled_up[n - 1]: weldingRoach's stability = WELD_K * old_conc_tot, so ndt_mrg <= round(WELD_K + 0.5) = 7 below a full cell


def make_inputs(x, y, tri, nb, young, seed=5):
    """slab_ref.make_inputs bent for the coupled loop.  Half of "melt_nomyi" loses its ice but keeps a column that melts (ctot < 1e-11 with hi > 0: the break of
    FE.cpp:5611); half of "melt_myi" gets young ice thinner than h_young_min (young_ice_growth < 0 while it melts laterally); "sc_fills" gets conc in [0.5, 0.7],
    where 1. - conc is exact and conc + (1. - conc) == 1. whatever the last place of conc, and a heat loss that freezes more than the lead can hold (the young ice that
    fills the lead, FE.cpp:4579).  The bins [nb, Ne] sum
    to conc (+ conc_young in the young-ice category): on half of the elements everything is in the last bin, bit for bit (unbroken), on the other half every bin
    holds at least 2 % of it (broken; with one bin there is no such thing); the mechanical bins are spread likewise, on their own.  Returns (inp, fsd, strata,
    groups: per element 0 = unbroken, 1 = broken, and a dict of the element sets of FSD_STRATA)."""
    inp, s, calm = R.make_inputs(x, y, tri, seed)
    rng = np.random.default_rng(seed + 100)
    Ne = tri.shape[0]
    S = {k: i for i, k in enumerate(R.STRATA)}
    half = np.zeros(Ne, bool)
    for k in ("melt_nomyi", "melt_myi"):
        half[np.flatnonzero(s == S[k])[::2]] = True           # every other element of the stratum: 2.4 % of the mesh each
    sets = {"ctot_break": (s == S["melt_nomyi"]) & half, "young_shrinks": (s == S["melt_myi"]) & half, "fills_lead": s == S["sc_fills"]}
    m = sets["ctot_break"]
    for k in ("conc", "thick", "snow_thick", "ridge_ratio", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi", "fyi_fraction"):
        inp[k][m] = 0.
    m = sets["young_shrinks"]
    inp["h_young"][m] = (inp["conc_young"] * rng.uniform(0.015, 0.03, Ne))[m]
    m = sets["fills_lead"]
    scale = rng.uniform(0.5, 0.7, Ne) / np.where(inp["conc"] > 0, inp["conc"], 1.)
    for k in ("conc", "thick", "snow_thick", "conc_myi", "thick_myi", "fyi_fraction"):
        inp[k][m] = (inp[k] * scale)[m]
    inp["F:Qow"][m] = rng.uniform(4e4, 6e4, Ne)[m]   # newice / h_young_min = ddt * Qow / (qi * h_young_min) = 2.3 .. 3.5 times the open water: no milder loss fills a lead in one step
    tot = inp["conc"] + (inp["conc_young"] if young else 0.)
    broken = (rng.random(Ne) < 0.5) & (nb > 1)
    w = 0.02 + (1. - 0.02 * nb) * rng.dirichlet([1.] * nb, Ne).T
    wm = 0.02 + (1. - 0.02 * nb) * rng.dirichlet([1.] * nb, Ne).T
    conc_fsd = np.where(broken, w * tot, 0.)
    conc_fsd[nb - 1] = np.where(broken, conc_fsd[nb - 1], tot)
    mech = wm * tot
    fsd = {"conc_fsd": np.ascontiguousarray(conc_fsd), "conc_mech_fsd": np.ascontiguousarray(mech)}
    return {k: np.ascontiguousarray(v, np.float64) for k, v in inp.items()}, fsd, s, broken.astype(np.int64), sets


def fsd_config(nb, young, **over):
    """fsd_ref.default_config on the standard tables with welding_kappa = WELD_K / (DT * area_scaled_up[nb - 1])"""
    t = FS.standard_tables(nb)
    return FS.default_config(nb, t, young, **dict({"welding_kappa": WELD_K / (R.DT * float(t["area_scaled_up"][nb - 1]))}, **over))


def copy_fsd(fsd, mech=True):
    return {"conc_fsd": fsd["conc_fsd"].copy(), "conc_mech_fsd": fsd["conc_mech_fsd"].copy() if mech and fsd.get("conc_mech_fsd") is not None else None}


# ---- what tests/test_gpu_slab_fsd.py and scripts/time_slab_coupled.py share
def attach(fe, fsd, fcfg, mech=True):
    """the bins (and the mechanical bins) to the device, the FSD configured on them"""
    fe.put_coupled(conc_fsd=fsd["conc_fsd"])
    fe.fsd_put(conc_mech_fsd=fsd["conc_mech_fsd"] if mech else None)
    fe.fsd_configure(fcfg["tables"], **FS.library_options(fcfg))


def pow_taken(ref, words2):
    """the elements whose melt rate is a pow (FE.cpp:5627): melt_type 3 taken, the column still has ice, neither the break nor the unbroken rule"""
    return took2(words2, "melt3") & ~took2(words2, "unbroken") & ~took2(words2, "ctot_break") & (ref["K:hi"] > 0)


def gpu_round(fe, f, ref, bins, dt, clock, mech=True):
    """slab_ref.gpu_round with slab_coupled(dt, clock) for slab(dt, clock) and fsd_update() behind it: the designed flux and column rows of `ref` go through the two
    device_rows doors, the state and the bins are put, so the call runs on ref's and bins' bits.  Returns (the 29 rows, the rows written in place, both branch
    words, the bins and mechanical bins after slab_coupled and after fsd_update, the flux and column rows before and after)."""
    lib = R.hip()
    assert lib is not None, "the HIP runtime of the library was not found: no way through the device_rows doors"
    nb = bins["conc_fsd"].shape[0]
    fe.fluxes()
    _, fdev = fe.fluxes_get((), want_device=True)
    fe.synchronize()
    R._write_rows(fe, lib, fdev, {k[2:]: ref[k] for k in FLUX if k != "F:tau_ow"})
    fe.column(dt)
    _, kdev = fe.column_rows((), want_device=True)
    fe.synchronize()
    R._write_rows(fe, lib, kdev, {k[2:]: ref[k] for k in COL})
    fe.put_state(dict(f, **{k: ref[k] for k in R.STATE}))
    fe.flux_put(tice0=ref["tice0"])
    fe.column_put(tice1=ref["tice1"], tice2=ref["tice2"])
    fe.put_coupled(conc_fsd=bins["conc_fsd"])
    if mech:
        fe.fsd_put(conc_mech_fsd=bins["conc_mech_fsd"])
    before = dict(fe.fluxes_get(), **{"K:" + k: v for k, v in fe.column_rows().items()})
    fe.slab_coupled(dt, clock)
    rows = fe.slab_rows()
    words = fe.debug_array("slab_branches").astype(np.uint32)
    words2 = fe.debug_array("slab_fsd_branches").astype(np.uint32)
    after = dict(fe.fluxes_get(), **{"K:" + k: v for k, v in fe.column_rows().items()})
    st = R.device_state(fe)
    get = lambda: {"conc_fsd": fe.get_coupled(cum_damage=False, num_fsd_bins=nb)["conc_fsd"], "conc_mech_fsd": fe.fsd_get(nb)["conc_mech_fsd"] if mech else None}
    got = get()
    fe.fsd_update()
    return rows, st, words, words2, got, get(), before, after


def update_fsd(ref, bins, fcfg, young):
    """fsd_ref.update_fsd (updateFSD(), FE.cpp:4674-4732) on the restated state and bins"""
    st = {"conc": ref["conc"], "conc_young": ref["conc_young"], "conc_fsd": bins["conc_fsd"],
          "conc_mech_fsd": bins["conc_mech_fsd"] if bins["conc_mech_fsd"] is not None else np.zeros_like(bins["conc_fsd"])}
    FS.update_fsd(st, dict(fcfg, young=bool(young)))
