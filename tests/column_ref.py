"""A line-faithful restatement of sections 3.2 to 5 of thermo()'s slab loop in model/finiteelement.cpp ("FE.cpp"), FE.cpp:5306-5411: the snowfall rule
(5321-5332), the nudging flux (5343-5366), iceOceanHeatflux (6396-6428), freezingPoint (6432-6448), thermoWinton (6633-6853), thermoIce0 (6860-6962) and the
young-ice stores of FE.cpp:5409-5410.  The element-independent parts are whole rows in numpy; the two column models are scalar per element (numpy float64
scalars: one rounding per operation, 0 / 0 is NaN as in C), every statement in the reference's operand order, no contraction.  The library calls are the
host's: numpy's hypot, which calls the C library's (EXCHANGE; math.hypot is an implementation of Python's own and differs from it in the last
place on a few elements), and numpy's sqrt (correctly rounded).  std::max / std::min keep the reference's argument order.  Not restated: Winton's
LOG(WARNING) and assert(Msurf >= 0), the OceanType::COUPLED branch (#ifdef OASIS), thermo() from FE.cpp:5413 on.

PARITY WITH THE REFERENCE IS NOT PINNED: model/ cannot be compiled here (boost, MPI, netCDF), so no binary of the reference produced these numbers; the
restatement is what the library (nxs_dyn_column) and the kernel's source compiled for the host are compared with, and tests/test_column_ref.py checks it
against hand-computed answers.  Shared by tests/test_column_ref.py, test_column_host_kernel.py and test_gpu_column.py.

Inputs: a dict of rows -- VT, ocean [2 Nn]; tair, precip, snowfr, snowfall, ocean_temp, ocean_salt, mld, sst, sss [Ne]; the flux rows Qia, dQiadT, I, subl and
their _young twins [Ne]; conc, thick, snow_thick, conc_young [Ne]; and tice0, tice1, tice2, tsurf_young, h_young, hs_young [Ne], which column() updates IN
PLACE like the reference.  cfg: a dict named after nxs_dyn_column_config (enums by the names of nextsim_amd._abi.COL_ENUMS).  column() returns the 22 rows
and, per element, the branches it took (-1: that statement was not reached)."""
from __future__ import annotations

import json
import os

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_FIX = json.load(open(os.path.join(_GOLDEN, "reference_constants.json")))
_PHYS = _FIX["physical"]
CONSTANTS = ("rhow", "cpw", "rhoi", "rhos", "Lf", "C", "ki", "si", "hmin")
F = np.float64
rhow, cpw, rhoi, rhos, Lf, C, ki, si, hmin = (F(float.fromhex(_PHYS[k]["hex"])) for k in CONSTANTS)   # physical::
days_in_sec = float.fromhex(_FIX["members"]["days_in_sec"]["hex"]) if "hex" in _FIX["members"]["days_in_sec"] else float(_FIX["members"]["days_in_sec"]["value"])

ICE_ROWS = ("Qio", "hi", "hs", "hi_old", "del_hi", "del_hs_mlt", "mlt_hi_top", "mlt_hi_bot", "del_hi_s2i")
YOUNG_ROWS = ("Qio_young", "hi_young", "hs_young", "hi_young_old", "del_hi_young", "del_hs_young_mlt", "mlt_hi_top_young", "mlt_hi_bot_young", "del_hi_s2i_young")
HEAD_ROWS = ("snowfall", "Qdw", "Fdw", "tfrw")
ROWS = HEAD_ROWS + ICE_ROWS + YOUNG_ROWS
IN_PLACE = ("tice0", "tice1", "tice2", "tsurf_young", "h_young", "hs_young")
FLUX_IN = ("Qia", "dQiadT", "I", "subl")
DT = 900                      # thermo()'s integer argument the inputs of make_inputs are designed for
# the smallest terms: each is removed in turn by column(drop=...) to show that the comparison would see it missing
TERMS = ("gamma", "one_minus_beta_I", "B1_I", "E1_qi_Tfr_T1")
ICE0_REC = ("noice", "hs_pos", "clamped", "snow_exhausted", "flood", "hmin", "del_hi_neg")
WINTON_REC = ("noice", "surf_melt", "subl_branch", "Mbot_pos", "all_melts_bot", "all_melts_surf", "flood", "h2_gt_h1", "T2_warm", "hmin", "del_hi_neg")


def default_config(**over):
    """the defaults of model/options.cpp:112, 291-293, 383-420 (tests/golden/reference_constants.json), named after nxs_dyn_column_config"""
    opt, sopt = _FIX["options"], _FIX["string_options"]
    c = {"thermo_type": sopt.get("setup.thermo-type", "winton"), "qio_type": sopt.get("thermo.Qio-type", "basic"),
         "freezingpoint_type": sopt.get("thermo.freezingpoint-type", "linear"), "ocean_type": sopt.get("setup.ocean-type", "constant"),
         "snowfall_source": "precip_snowfr", "mld_source": "constant", "flooding": int(opt["thermo.flooding"]["value"]),
         "freezingpoint_mu": opt["thermo.freezingpoint_mu"]["value"], "snow_cond": opt["thermo.snow_cond"]["value"], "Csens_io": opt["thermo.Csens_io"]["value"],
         "constant_mld": opt["ideal_simul.constant_mld"]["value"], "nudge_timeT": days_in_sec * opt["thermo.ocean_nudge_timeT_days"]["value"],
         "nudge_timeS": days_in_sec * opt["thermo.ocean_nudge_timeS_days"]["value"],
         "Qdw_const": opt.get("ideal_simul.constant_Qdw", {"value": 0.})["value"], "Fdw_const": opt.get("ideal_simul.constant_Fdw", {"value": 0.})["value"]}
    for k, v in over.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


def _max(a, b):
    """std::max(a, b): (a < b) ? b : a"""
    return F(b) if a < b else F(a)


def _min(a, b):
    """std::min(a, b): (b < a) ? b : a"""
    return F(b) if b < a else F(a)


def freezing_point(cfg, sss):
    """freezingPoint, FE.cpp:6432-6448 (rows)"""
    if cfg["freezingpoint_type"] == "linear":
        return -cfg["freezingpoint_mu"] * sss
    return (-0.0575 + 1.710523e-3 * np.sqrt(sss) - 2.154996e-4 * sss) * sss


def thermo_ice0(cfg, dt, conc, voli, vols, snowfall, Qia, dQiadT, I, subl, Tbot, Qio, mlt_hi_bot, del_hi_s2i, Tsurf, drop=()):
    """thermoIce0, FE.cpp:6860-6962.  Returns (Qio, hi, hs, hi_old, del_hi, del_hs_mlt, mlt_hi_top, mlt_hi_bot, del_hi_s2i, Tsurf) and the branch record"""
    M_ks, mu = F(cfg["snow_cond"]), F(cfg["freezingpoint_mu"])
    qi = Lf * rhoi
    qs = Lf * rhos
    Tfr_ice = -mu * si
    beta = F(0.4)
    gamma = F(1.) if "gamma" in drop else F(1.065)
    del_hs_mlt = mlt_hi_top = F(0.)
    rec = dict.fromkeys(ICE0_REC, -1)
    if conc <= 0. or voli <= 0.:
        rec["noice"] = 1 if conc <= 0. else 2
        hi = hi_old = hs = del_hi = F(0.)
        Tsurf = Tfr_ice
    else:
        rec["noice"] = 0
        hi = voli / conc
        hi_old = hi
        hs = vols / conc
        Qia_mod = Qia if "one_minus_beta_I" in drop else Qia + (1. - beta) * I
        Qic = M_ks * (Tbot - Tsurf) / (hs + M_ks * hi / ki) * gamma
        Tsurf = Tsurf + (Qic - Qia_mod) / (M_ks / (hs + M_ks * hi / ki) + dQiadT)
        rec["hs_pos"] = int(hs > 0.)
        bound = F(0.) if hs > 0. else -mu * si
        rec["clamped"] = int(not (Tsurf < bound))
        Tsurf = _min(bound, Tsurf)
        del_hs_mlt = _min(Qia_mod - Qic, 0.) * dt / qs
        hs = hs + (del_hs_mlt - subl * dt / rhos)
        rec["snow_exhausted"] = int(hs < 0.)
        del_ht = _min(hs, 0.) * qs / qi
        hs = _max(0., hs)
        hs = hs + snowfall / rhos * dt
        del_hb = (Qic - Qio) * dt / qi
        del_hi = del_ht + del_hb
        hi = hi + del_hi
        mlt_hi_top = _min(del_ht, 0.)
        mlt_hi_bot = _min(del_hb, 0.)
        draft = (hi * rhoi + hs * rhos) / rhow
        rec["flood"] = int(bool(cfg["flooding"]) and draft > hi)
        if cfg["flooding"] and draft > hi:
            del_hi_s2i = del_hi_s2i + (draft - hi)
            hs = hs - (draft - hi) * rhoi / rhos
            hi = draft
        rec["hmin"] = int(hi < hmin)
        if hi < hmin:
            rec["del_hi_neg"] = int(del_hi < 0.)
            if del_hi < 0.:
                mlt_hi_top = mlt_hi_top * (-hi_old / del_hi)
                mlt_hi_bot = mlt_hi_bot * (-hi_old / del_hi)
            del_hi_s2i = F(0.)
            del_hi = -hi_old
            Qio = Qio + hi * qi / dt + hs * qs / dt
            hi = F(0.)
            hs = F(0.)
            Tsurf = Tfr_ice
    return (Qio, hi, hs, hi_old, del_hi, del_hs_mlt, mlt_hi_top, mlt_hi_bot, del_hi_s2i, Tsurf), rec


def thermo_winton(cfg, dt, conc, voli, vols, snowfall, Qia, dQiadT, I, subl, Tbot, Qio, mlt_hi_bot, del_hi_s2i, Tsurf, T1, T2, drop=()):
    """thermoWinton, FE.cpp:6633-6853.  Returns (Qio, hi, hs, hi_old, del_hi, del_hs_mlt, mlt_hi_top, mlt_hi_bot, del_hi_s2i, Tsurf, T1, T2) and the record"""
    M_ks, mu = F(cfg["snow_cond"]), F(cfg["freezingpoint_mu"])
    qi = Lf * rhoi
    qs = Lf * rhos
    Crho = C * rhoi
    Tfr_ice = -mu * si
    sqrt = np.sqrt
    del_hs_mlt = mlt_hi_top = F(0.)
    rec = dict.fromkeys(WINTON_REC, -1)
    if conc <= 0. or voli <= 0.:
        rec["noice"] = 1 if conc <= 0. else 2
        hi = hs = hi_old = del_hi = F(0.)
        Tsurf = T1 = T2 = Tfr_ice
    else:
        rec["noice"] = 0
        hi = voli / conc
        hi_old = hi
        hs = vols / conc
        Tfr_surf = F(0.) if hs > 0 else Tfr_ice
        K12 = 4 * ki * M_ks / (M_ks * hi + 4 * ki * hs)
        A = Qia - Tsurf * dQiadT
        B = dQiadT
        K32 = 2 * ki / hi
        A1 = hi * Crho / (2 * dt) + K32 * (4 * dt * K32 + hi * Crho) / (6 * dt * K32 + hi * Crho) + K12 * B / (K12 + B)
        if "B1_I" in drop:
            B1 = -hi / (2 * dt) * (Crho * T1 + qi * Tfr_ice / T1) - K32 * (4 * dt * K32 * Tbot + hi * Crho * T2) / (6 * dt * K32 + hi * Crho) + A * K12 / (K12 + B)
        else:
            B1 = -hi / (2 * dt) * (Crho * T1 + qi * Tfr_ice / T1) - I - K32 * (4 * dt * K32 * Tbot + hi * Crho * T2) / (6 * dt * K32 + hi * Crho) + A * K12 / (K12 + B)
        C1 = hi * qi * Tfr_ice / (2 * dt)
        T1 = -(B1 + sqrt(B1 * B1 - 4 * A1 * C1)) / (2 * A1)
        Tsurf = (K12 * T1 - A) / (K12 + B)
        Msurf = F(0.)
        rec["surf_melt"] = int(Tsurf > Tfr_surf)
        if Tsurf > Tfr_surf:
            Tsurf = Tfr_surf
            A1 = A1 + (K12 - K12 * B / (K12 + B))
            B1 = B1 - (K12 * Tsurf + A * K12 / (K12 + B))
            T1 = -(B1 + sqrt(B1 * B1 - 4 * A1 * C1)) / (2 * A1)
            Msurf = K12 * (T1 - Tsurf) - (A + B * Tsurf)
        T2 = (2 * dt * K32 * (T1 + 2 * Tbot) + hi * Crho * T2) / (6 * dt * K32 + hi * Crho)
        h1 = hi / 2.
        h2 = hi / 2.
        if "E1_qi_Tfr_T1" in drop:
            E1 = Crho * (T1 - Tfr_ice) - qi * F(1.)
        else:
            E1 = Crho * (T1 - Tfr_ice) - qi * (1 - Tfr_ice / T1)
        E2 = Crho * (T2 - Tfr_ice) - qi
        hs = hs + snowfall / rhos * dt
        if subl * dt <= hs * rhos:
            rec["subl_branch"] = 0
            hs = hs - subl * dt / rhos
        elif subl * dt - hs * rhos <= h1 * rhoi:
            rec["subl_branch"] = 1
            h1 = h1 - (subl * dt - hs * rhos) / rhoi
            hs = F(0.)
        elif subl * dt - h1 * rhoi - hs * rhos <= h2 * rhoi:
            rec["subl_branch"] = 2
            h2 = h2 - (subl * dt - h1 * rhoi - hs * rhos) / rhoi
            h1 = F(0.)
            hs = F(0.)
        else:
            rec["subl_branch"] = 3
            h2 = h1 = hs = F(0.)
        mlt_hi_top = _max(0., h1 + h2 - hi_old)
        Mbot = Qio - 4 * ki * (Tbot - T2) / hi
        del_hs_mlt = F(0.)
        rec["Mbot_pos"] = int(not (Mbot <= 0.))
        if Mbot <= 0.:
            Ebot = Crho * (Tbot - Tfr_ice) - qi
            delh2 = Mbot * dt / Ebot
            T2 = (delh2 * Tbot + h2 * T2) / (delh2 + h2)
            h2 = h2 + delh2
        else:
            delh2 = -_min(-Mbot * dt / E2, h2)
            delh1 = -_min(_max(-(Mbot * dt + E2 * h2) / E1, 0.), h1)
            del_hs_mlt = -_min(_max((Mbot * dt + E2 * h2 + E1 * h1) / qs, 0.), hs)
            rec["all_melts_bot"] = int(h2 + h1 + hs - delh2 - delh1 - del_hs_mlt <= 0.)
            if h2 + h1 + hs - delh2 - delh1 - del_hs_mlt <= 0.:
                Qio = Qio - _max(Mbot * dt - qs * hs + E1 * h1 + E2 * h2, 0.) / dt
            hs = hs + del_hs_mlt
            h1 = h1 + delh1
            h2 = h2 + delh2
            mlt_hi_bot = mlt_hi_bot + (delh1 + delh2)
        del_hs_mlt = del_hs_mlt - _min(Msurf * dt / qs, hs)
        delh1 = -_min(_max(-(Msurf * dt - qs * hs) / E1, 0.), h1)
        delh2 = -_min(_max(-(Msurf * dt - qs * hs + E1 * h1) / E2, 0.), h2)
        rec["all_melts_surf"] = int(h2 + h1 + hs - delh2 - delh1 - del_hs_mlt <= 0.)
        if h2 + h1 + hs - delh2 - delh1 - del_hs_mlt <= 0.:
            Qio = Qio - _max(Msurf * dt - qs * hs + E1 * h1 + E2 * h2, 0.) / dt
        hs = hs + del_hs_mlt
        h1 = h1 + delh1
        h2 = h2 + delh2
        mlt_hi_top = mlt_hi_top + (delh1 + delh2)
        freeboard = (hi * (rhow - rhoi) - hs * rhos) / rhow
        rec["flood"] = int(bool(cfg["flooding"]) and freeboard < 0)
        if cfg["flooding"] and freeboard < 0:
            hs = hs + _min(freeboard * rhoi / rhos, 0.)
            delh1 = _max(-freeboard, 0.)
            f1 = 1 - delh1 / (delh1 + h1)
            Tbar = f1 * (T1 + qi * Tfr_ice / (Crho * T1)) + (1 - f1) * Tfr_ice
            T1 = (Tbar - sqrt(Tbar * Tbar - 4 * Tfr_ice * qi / Crho)) / 2.
            h1 = h1 + delh1
            del_hi_s2i = del_hi_s2i + delh1
        hi = h1 + h2
        rec["h2_gt_h1"] = int(h2 > h1)
        if h2 > h1:
            f1 = h1 / hi * 2.
            Tbar = f1 * (T1 + qi * Tfr_ice / (Crho * T1)) + (1 - f1) * T2
            T1 = (Tbar - sqrt(Tbar * Tbar - 4 * Tfr_ice * qi / Crho)) / 2.
        elif hi > 0.:
            f1 = (2. * h1 - hi) / hi
            T2 = f1 * (T1 + qi * Tfr_ice / (Crho * T1)) + (1 - f1) * T2
            rec["T2_warm"] = int(T2 > Tfr_ice)
            if T2 > Tfr_ice:
                mlt_hi_top = mlt_hi_top - hi / 4 * Crho * (T2 - Tfr_ice) * T1 / (qi * T1 + (Crho * T1 - qi) * (Tfr_ice - T1))
                mlt_hi_bot = mlt_hi_bot - hi / 4 * Crho * (T2 - Tfr_ice) * T1 / (qi * T1 + (Crho * T1 - qi) * (Tfr_ice - T1))
                hi = hi - hi / 2 * Crho * (T2 - Tfr_ice) * T1 / (qi * T1 + (Crho * T1 - qi) * (Tfr_ice - T1))
                T2 = Tfr_ice
        del_hi = hi - hi_old
        rec["hmin"] = int(hi < hmin)
        if hi < hmin:
            Qio = Qio - (-qs * hs + (E1 + E2) * hi / 2.) / dt
            rec["del_hi_neg"] = int(del_hi < 0.)
            if del_hi < 0.:
                mlt_hi_top = mlt_hi_top * (-hi_old / del_hi)
                mlt_hi_bot = mlt_hi_bot * (-hi_old / del_hi)
            del_hi_s2i = F(0.)
            del_hi = -hi_old
            hi = F(0.)
            hs = F(0.)
            Tsurf = T1 = T2 = Tfr_ice
    return (Qio, hi, hs, hi_old, del_hi, del_hs_mlt, mlt_hi_top, mlt_hi_bot, del_hi_s2i, Tsurf, T1, T2), rec


def ice_ocean_heatflux(inp, cfg, tri, mld, dt, qio_shift=0):
    """iceOceanHeatflux, FE.cpp:6396-6428 (rows); qio_shift moves the result by that many units in the last place (tests/test_column_ref.py)"""
    sst = inp["sst"]
    Tbot = freezing_point(cfg, inp["sss"])
    if cfg["qio_type"] == "basic":
        q = (sst - Tbot) * rhow * cpw * mld / F(dt)
    else:
        VT, oc = inp["VT"], inp["ocean"]
        Nn = VT.size // 2
        welt = np.zeros(tri.shape[0])
        for i in range(3):
            nind = tri[:, i]
            du, dv = VT[nind] - oc[nind], VT[nind + Nn] - oc[nind + Nn]
            welt = welt + np.hypot(du, dv)
        norm = welt / 3.
        q = (sst - Tbot) * norm * cfg["Csens_io"] * rhow * cpw
    for _ in range(abs(qio_shift)):
        q = np.nextafter(q, np.inf if qio_shift > 0 else -np.inf)
    return q


def column(inp, cfg, tri, young, dt, drop=(), qio_shift=0):
    """thermo(), FE.cpp:5306-5411.  Returns (the 22 rows, the branch record); the six IN_PLACE rows of inp are updated."""
    Ne = tri.shape[0]
    ddt = F(dt)
    with np.errstate(all="ignore"):
        src = cfg["snowfall_source"]
        if src == "precip_snowfr":
            snowfall = inp["precip"] * inp["snowfr"]
        elif src == "snowfall":
            snowfall = inp["snowfall"].copy()
        else:
            snowfall = np.where(inp["tair"] < 0, inp["precip"], 0.)
        snowfall = np.where(np.less(0., snowfall), snowfall, 0.)      # std::max(0., tmp_snowfall)
        mld = inp["mld"] if cfg["mld_source"] == "row" else np.full(Ne, F(cfg["constant_mld"]))
        sst, sss = inp["sst"], inp["sss"]
        if cfg["ocean_type"] == "constant":
            Qdw, Fdw = np.full(Ne, F(cfg["Qdw_const"])), np.full(Ne, F(cfg["Fdw_const"]))
        else:
            Qdw = -(sst - inp["ocean_temp"]) * mld * rhow * cpw / F(cfg["nudge_timeT"])
            delS = sss - inp["ocean_salt"]
            Fdw = delS * mld * rhow / (F(cfg["nudge_timeS"]) * sss - ddt * delS)
        Qio0 = ice_ocean_heatflux(inp, cfg, tri, mld, dt, qio_shift)
        tfrw = freezing_point(cfg, sss)
        out = {k: np.zeros(Ne) for k in ROWS}
        out.update(snowfall=snowfall, Qdw=Qdw, Fdw=Fdw, tfrw=tfrw)
        winton = cfg["thermo_type"] == "winton"
        names = WINTON_REC if winton else ICE0_REC
        rec = {k: np.full(Ne, -1) for k in names}
        rec.update({k + "_young": np.full(Ne, -1) for k in (ICE0_REC if young else ())})
        rec["snow_tair_neg"] = (inp["tair"] < 0).astype(int) if src == "precip_tair" else np.full(Ne, -1)
        z = F(0.)
        for e in range(Ne):
            a = (cfg, ddt, inp["conc"][e], inp["thick"][e], inp["snow_thick"][e], snowfall[e], inp["Qia"][e], inp["dQiadT"][e], inp["I"][e], inp["subl"][e], tfrw[e], Qio0[e], z, z)
            if winton:
                r, b = thermo_winton(*a, inp["tice0"][e], inp["tice1"][e], inp["tice2"][e], drop=drop)
                inp["tice1"][e], inp["tice2"][e] = r[10], r[11]
            else:
                r, b = thermo_ice0(*a, inp["tice0"][e], drop=drop)
            inp["tice0"][e] = r[9]
            for k, v in zip(ICE_ROWS, r):
                out[k][e] = v
            for k, v in b.items():
                rec[k][e] = v
            if young:
                cy = inp["conc_young"][e]
                r, b = thermo_ice0(cfg, ddt, cy, inp["h_young"][e], inp["hs_young"][e], snowfall[e], inp["Qia_young"][e], inp["dQiadT_young"][e], inp["I_young"][e],
                                   inp["subl_young"][e], tfrw[e], Qio0[e], z, z, inp["tsurf_young"][e], drop=drop)
                inp["tsurf_young"][e] = r[9]
                inp["h_young"][e] = r[1] * cy
                inp["hs_young"][e] = r[2] * cy
                for k, v in zip(YOUNG_ROWS, r):
                    out[k][e] = v
                for k, v in b.items():
                    rec[k + "_young"][e] = v
    return {k: np.ascontiguousarray(out[k], np.float64) for k in ROWS}, rec


def same_record(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


# ---- designed inputs: every element belongs to one stratum, and a stratum is built to take one branch (tests/test_column_ref.py counts them)
STRATA = ("noice_conc", "noice_vol", "cold_snow", "cold_bare", "warm_snow", "warm_bare", "snow_exhaust", "flood", "melt_all_bottom", "thin_grow", "subl_h1", "subl_h2",
          "subl_all_cold", "subl_all_warm", "bottom_melt", "surf_melt_all", "warm_T2")


def _stratum_rows(rng, s, conc_lo, conc_hi):
    """the column inputs of one ice category for the stratum numbers s [Ne]: conc, hi, hs, Tsurf, T1, T2, Qia, dQiadT, I, subl, and what the stratum asks of the
    ocean (dsst = sst - the linear freezing point; NaN: no wish)"""
    Ne = s.size
    r = lambda a, b: a + (b - a) * rng.random(Ne)
    S = {k: i for i, k in enumerate(STRATA)}
    is_ = lambda *names: np.isin(s, [S[k] for k in names])
    conc = r(conc_lo, conc_hi)
    hi, hs = r(1., 3.), r(0.1, 0.3)
    Ts, T1, T2 = r(-20., -5.), r(-10., -3.), r(-5., -2.5)
    Qia, dQ, I, subl = r(20., 80.), r(10., 20.), r(0., 5.), r(0., 1e-6)
    dsst = r(-0.002, -0.0002)
    hs[is_("cold_bare", "warm_bare", "melt_all_bottom", "thin_grow", "subl_h2", "subl_all_cold", "subl_all_warm", "surf_melt_all", "warm_T2")] = 0.
    m = is_("warm_snow", "warm_bare", "snow_exhaust")
    Ts[m], T1[m], T2[m], Qia[m] = r(-1., -0.3)[m], r(-2., -1.)[m], r(-2., -1.8)[m], r(-150., -60.)[m]
    m = is_("snow_exhaust")
    hs[m], Qia[m] = r(0.0003, 0.0008)[m], r(-300., -200.)[m]
    m = is_("flood")
    hi[m], hs[m] = r(0.2, 0.4)[m], r(0.4, 0.6)[m]
    m = is_("melt_all_bottom")
    hi[m], dsst[m], subl[m], Ts[m], T1[m], T2[m] = r(0.011, 0.014)[m], r(0.2, 0.3)[m], 0., r(-3.2, -2.8)[m], r(-2.7, -2.4)[m], r(-2.2, -2.)[m]
    m = is_("thin_grow")
    hi[m], dsst[m], subl[m], Ts[m], T1[m], T2[m], Qia[m] = r(0.003, 0.005)[m], 0., 0., r(-2.6, -2.4)[m], r(-2.3, -2.2)[m], r(-2.1, -2.)[m], r(500., 600.)[m]
    m = is_("subl_h1")
    hs[m], subl[m] = r(0.0009, 0.0011)[m], r(1e-3, 1.2e-3)[m]
    m = is_("subl_h2", "subl_all_cold", "subl_all_warm")
    hi[m] = r(0.019, 0.021)[m]
    m = is_("subl_h2")
    subl[m] = (r(0.62, 0.88) * hi * float(rhoi) / DT)[m]
    m = is_("subl_all_cold", "subl_all_warm")
    subl[m] = (r(1.2, 1.5) * hi * float(rhoi) / DT)[m]
    m = is_("subl_all_warm")
    dsst[m] = r(0.05, 0.1)[m]
    m = is_("bottom_melt", "warm_T2")
    dsst[m] = r(0.005, 0.02)[m]
    m = is_("surf_melt_all")
    hi[m], Qia[m], dsst[m] = r(0.014, 0.016)[m], r(-9000., -8000.)[m], 0.
    m = is_("warm_T2")
    hi[m], Ts[m], T1[m], T2[m] = r(1., 2.)[m], r(-0.6, -0.5)[m], r(-0.32, -0.3)[m], r(-0.285, -0.28)[m]
    vol, svol = conc * hi, conc * hs
    m = is_("noice_conc")
    conc[m], vol[m], svol[m] = 0., 0., 0.
    m = is_("noice_vol")
    vol[m], svol[m] = 0., 0.
    dry = is_("subl_h1", "thin_grow")                  # no snowfall there: the snow must stay thinner than the sublimation / off the thin ice
    return dict(conc=conc, vol=vol, svol=svol, Ts=Ts, T1=T1, T2=T2, Qia=Qia, dQiadT=dQ, I=I, subl=subl, dsst=dsst, dry=dry)


def make_inputs(x, y, tri, seed=3):
    """Inputs on a mesh (node coordinates, [Ne, 3] 0-based triangles): DESIGNED STRATA, not noise.  Every element's old ice belongs to one of STRATA and its
    young ice to another (the old ice's stratum number plus 6); the ocean follows the old ice's stratum.  Returns (inp, strata [Ne], calm: the elements whose
    three nodes have M_VT == M_ocean exactly)."""
    rng = np.random.default_rng(seed)
    Nn, Ne = x.size, tri.shape[0]
    NS = len(STRATA)
    s = rng.permutation(Ne) % NS
    r = lambda a, b: a + (b - a) * rng.random(Ne)
    old = _stratum_rows(rng, s, 0.3, 0.7)
    yng = _stratum_rows(rng, (s + 6) % NS, 0.05, 0.25)
    inp = {}
    inp["VT"] = 0.3 * (rng.random(2 * Nn) - 0.5)
    inp["ocean"] = 0.2 * (rng.random(2 * Nn) - 0.5)
    calm = np.sort(rng.choice(Ne, 12, replace=False))
    for n in np.unique(tri[calm]):
        inp["ocean"][n], inp["ocean"][n + Nn] = inp["VT"][n], inp["VT"][n + Nn]
    inp["sss"] = r(28., 35.)
    inp["sst"] = -default_config()["freezingpoint_mu"] * inp["sss"] + old["dsst"]
    inp["tair"] = r(-30., 6.)
    precip = r(-2e-6, 3e-5)                            # (a few below zero: std::max(0., tmp_snowfall))
    precip[old["dry"] | yng["dry"]] = 0.
    inp["precip"] = precip
    inp["snowfr"] = np.where(rng.random(Ne) < 0.2, 0., r(0.2, 1.))
    inp["snowfall"] = precip * r(0.2, 1.)
    inp["ocean_temp"] = inp["sst"] + r(-0.5, 0.5)
    inp["ocean_salt"] = inp["sss"] + r(-0.5, 0.5)
    inp["mld"] = r(5., 40.)
    inp.update(conc=old["conc"], thick=old["vol"], snow_thick=old["svol"], tice0=old["Ts"], tice1=old["T1"], tice2=old["T2"])
    inp.update(conc_young=yng["conc"], h_young=yng["vol"], hs_young=yng["svol"], tsurf_young=yng["Ts"])
    for k in FLUX_IN:
        inp[k], inp[k + "_young"] = old[k], yng[k]
    return {k: np.ascontiguousarray(v, np.float64) for k, v in inp.items()}, s, calm


def moved_one_ulp(inp, direction):
    """every non-zero input moved to the neighbouring double away from (+1) or towards (-1) zero; a zero stays a zero (it is a value of its own: no ice, no
    snow, no sublimation); the calm elements stay calm (M_ocean is moved with M_VT)"""
    out = {}
    for k, v in inp.items():
        target = np.where(v > 0, np.inf, -np.inf) if direction > 0 else np.zeros(v.shape)
        out[k] = np.where(v == 0., v, np.nextafter(v, target))
    same = inp["VT"] == inp["ocean"]
    out["ocean"][same] = out["VT"][same]
    return out


def copy(inp):
    return {k: v.copy() for k, v in inp.items()}
