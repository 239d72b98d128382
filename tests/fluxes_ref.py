"""A line-faithful restatement of the atmospheric bulk fluxes of thermo() in model/finiteelement.cpp ("FE.cpp"): the call sequence of its "fluxes" timer
(FE.cpp:5222-5273), OWBulkFluxes (the non-AEROBULK loop FE.cpp:5096-5132 and the radiative loop 5138-5158), IABulkFluxes (6148-6353), specificHumidity
(4966-5019), albedo (6454-6535), windSpeedElement (6359-6370) and incomingLongwave (6376-6389).  Whole rows at a time in numpy, every statement in the
reference's operand order, one rounding per operation, no contraction; the libm calls (exp, pow, log, atan) are Python's math module element by element, i.e.
the host's libm; cbrt is that library's through ctypes (numpy's cbrt and math.hypot are implementations of their own); hypot is numpy's, which calls it.  std::max / std::min keep the reference's argument order (_max, _min below), so a NaN
behaves as there.  Not restated: the #ifdef AEROBULK branch, the OceanType::COUPLED term M_qsrml (FE.cpp:5153-5154), thermo() from FE.cpp:5279 on.

PARITY WITH THE REFERENCE IS NOT PINNED: model/ cannot be compiled here (it needs boost, MPI, netCDF and the rest of the model's build), so no
binary of the reference produced these numbers; the restatement is what the library (nxs_dyn_fluxes) is compared with, and tests/test_fluxes_ref.py checks it
against hand-computable answers.  Shared by tests/test_fluxes_ref.py and tests/test_gpu_fluxes.py.

Inputs: a dict of rows -- wind [2 Nn]; tair, mslp, Qsw_in, dair, sphuma, mixrat, Qlw_in, tcc [Ne]; conc, snow_thick, conc_young, hs_young [Ne]; tice0,
tsurf_young, sst, sss, pond_fraction, lid_volume [Ne]; drag_ui, drag_ti, drag_ui_young, drag_ti_young [Ne], which fluxes() updates IN PLACE like the reference.
cfg: a dict named after nxs_dyn_flux_config.  fluxes() returns the 25 rows and, per element, the branch it took."""
from __future__ import annotations

import ctypes
import ctypes.util
import json
import math
import os

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_PHYS = json.load(open(os.path.join(_GOLDEN, "reference_constants.json")))["physical"]
CONSTANTS = ("tfrwK", "Ra_dry", "Ra_vap", "cpa", "cpv", "Lv0", "eps", "sigma_sb", "vonKarman", "Gamma_d", "rhoa", "Lf", "g")
tfrwK, Ra_dry, Ra_vap, cpa, cpv, Lv0, eps, sigma_sb, vonKarman, Gamma_d, rhoa, Lf, g = (float.fromhex(_PHYS[k]["hex"]) for k in CONSTANTS)   # physical::

HUM = {"dewpoint": 0, "sphuma": 1, "mixrat": 2}
LW = {"Qlw_in": 0, "tcc": 1}
ICE_ROWS = ("Qia", "Qlw", "Qsw", "Qlh", "Qsh", "I", "subl", "dQiadT", "albedo")
ROWS = (("Qow", "Qlw_ow", "Qsw_ow", "Qlh_ow", "Qsh_ow", "evap", "tau_ow", "Qia", "Qlwi", "Qswi", "Qlhi", "Qshi", "I", "subl", "dQiadT", "albedo")
        + tuple(k + "_young" for k in ICE_ROWS))
DRAGS = ("drag_ui", "drag_ti", "drag_ui_young", "drag_ti_young")
# rows no libm call reaches (FE.cpp:5141, 6342-6346 with albedo()'s arithmetic): compared bit for bit
NO_LIBM = ("Qsw_ow", "albedo", "Qswi", "I", "albedo_young", "Qsw_young", "I_young")
# rows of a calm element (wspeed == 0) that are a product with that zero: +-0 whatever the libm says
CALM_ZERO = ("Qsh_ow", "Qlh_ow", "evap", "Qshi", "Qlhi", "subl", "Qsh_young", "Qlh_young", "subl_young")
# the smallest terms: each is removed in turn by fluxes(drop=...) to show that the comparison would see it missing
TERMS = ("Lv_cubic", "f_C_temp2", "retv_Tpot_wr", "zetah_zref_temp", "Bm2", "ice_constants")


def default_config(**over):
    """the thermo.* defaults of model/options.cpp:388-438 (tests/golden/thermo_flux_options.json), named after nxs_dyn_flux_config"""
    opt = json.load(open(os.path.join(_GOLDEN, "thermo_flux_options.json")))["options"]
    c = {"alb_scheme": opt["thermo.alb_scheme"]["value"], "humidity_source": "dewpoint",
         "longwave_source": "tcc" if opt["thermo.use_parameterised_long_wave_radiation"]["value"] else "Qlw_in",
         "force_neutral_atmosphere": int(opt["thermo.force_neutral_atmosphere"]["value"]), "ocean_albedo": opt["thermo.albedoW"]["value"]}
    for k in ("alb_ice", "alb_sn", "alb_ponds", "I_0", "drag_ocean_t", "drag_ocean_q", "zref_wind", "zref_temp", "limiting_lengthscale"):
        c[k] = opt["thermo." + k]["value"]
    for k, v in over.items():
        if k not in c:
            raise KeyError(k)
        c[k] = v
    return c


def _libm(fn):
    def f(a, *args):
        a = np.asarray(a, np.float64)
        out = np.empty(a.shape)
        o = out.reshape(-1)
        for i, v in enumerate(a.reshape(-1).tolist()):
            try:
                o[i] = fn(v, *args)
            except (ValueError, OverflowError):      # (a branch computed for an element that takes the other one)
                o[i] = math.nan
        return out
    return f


_LIBM = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_LIBM.cbrt.restype, _LIBM.cbrt.argtypes = ctypes.c_double, [ctypes.c_double]
_exp, _log, _atan, _pow, _cbrt = _libm(math.exp), _libm(math.log), _libm(math.atan), _libm(math.pow), _libm(_LIBM.cbrt)


def _max(a, b):
    """std::max(a, b): (a < b) ? b : a"""
    return np.where(np.less(a, b), b, a)


def _min(a, b):
    """std::min(a, b): (b < a) ? b : a"""
    return np.where(np.less(b, a), b, a)


def wind_speed_element(wind, tri):
    """windSpeedElement, FE.cpp:6359-6370.  tri: [Ne, 3] 0-based"""
    Nn = wind.size // 2
    wspd = np.zeros(tri.shape[0])
    for j in range(3):
        wspd = wspd + np.hypot(wind[tri[:, j]], wind[tri[:, j] + Nn])
    return wspd / 3.


def incoming_longwave(inp, cfg):
    """incomingLongwave, FE.cpp:6376-6389"""
    if LW[cfg["longwave_source"]] == 0:
        return inp["Qlw_in"]
    taa = inp["tair"] + tfrwK
    return sigma_sb * _pow(taa, 4.) * (1. - 0.261 * _exp(-7.77e-4 * _pow(taa - tfrwK, 2.))) * (1. + 0.275 * inp["tcc"])


def specific_humidity(scheme, inp, cfg, temp=None, drop=()):
    """specificHumidity, FE.cpp:4966-5019: (sphum, dsphumdT)"""
    A, B, C = 7.2e-4, 3.20e-6, 5.9e-10
    a, b, c, d = 6.1121e2, 18.729, 257.87, 227.3
    alpha, beta = 0.62197, 0.37803
    mslp = inp["mslp"]
    if scheme == "ATMOSPHERE":
        src = HUM[cfg["humidity_source"]]
        if src == 1:
            return _max(0., inp["sphuma"]), 0.
        if src == 2:
            return inp["mixrat"] / (1. + inp["mixrat"]), 0.
        temp = inp["dair"]
        salinity = 0
    elif scheme == "WATER":
        temp = inp["sst"]
        return 640380. / rhoa * _exp(-5107.4 / (temp + tfrwK)), 0.
    else:
        if "ice_constants" not in drop:
            A, B, C = 2.2e-4, 3.83e-6, 6.4e-10
            a, b, c, d = 6.1115e2, 23.036, 279.82, 333.7
        salinity = 0
    if "f_C_temp2" in drop:
        f = 1. + A + mslp * 1e-2 * (B + 0. * temp)
    else:
        f = 1. + A + mslp * 1e-2 * (B + C * temp * temp)
    est = a * _exp((b - temp / d) * temp / (temp + c)) * (1 - 5.37e-4 * salinity)
    sphum = alpha * f * est / (mslp - beta * f * est)
    if scheme == "ICE":
        dfdT = 2. * C * B * temp
        destdT = (b * c * d - temp * (2. * c + temp)) / (d * _pow(c + temp, 2.)) * est
        dsphumdT = alpha * mslp * (f * destdT + est * dfdT) / _pow(mslp - beta * est * f, 2.)
        return sphum, dsphumdT
    return sphum, 0.


def albedo(Tsurf, hs, frac_pnd, alb_scheme, alb_ice, alb_sn, alb_pnd, I_0):
    """albedo, FE.cpp:6454-6535: (albedo, pen_sw), and the two branches it records"""
    hs_pos, warm = hs > 0., Tsurf > -1.
    if alb_scheme in (1, 2):
        if alb_scheme == 2:
            snow = _min(alb_sn, alb_ice + (alb_sn - alb_ice) * hs / 0.2)
        else:
            snow = np.full(hs.shape, alb_sn)
        alb = np.where(hs_pos, snow, alb_ice)
        pen_sw = np.where(hs_pos, 0., I_0)
    elif alb_scheme == 3:
        albi = np.where(warm, alb_ice - 0.075 * (Tsurf + 1.), alb_ice)
        albs = np.where(warm, alb_sn - 0.124 * (Tsurf + 1.), alb_sn)
        frac_sn = hs / (hs + 0.02)
        alb = frac_sn * albs + frac_pnd * alb_pnd + (1. - frac_sn - frac_pnd) * albi
        pen_sw = (1. - frac_sn - frac_pnd) * I_0
    elif alb_scheme == 4:
        frac_sn = hs / (hs + 0.02)
        albs = np.where(warm, alb_sn - 0.124 * (Tsurf + 1.), alb_sn)
        alb = frac_sn * albs + frac_pnd * alb_pnd + (1. - frac_sn - frac_pnd) * alb_ice
        pen_sw = (1. - frac_sn - frac_pnd) * I_0
    else:
        raise ValueError("Wrong albedo_scheme")
    return alb, pen_sw, hs_pos, warm


def ow_bulk_fluxes(inp, cfg, tri, drop=()):
    """OWBulkFluxes, FE.cpp:5096-5132 and 5138-5158"""
    sphuma, _ = specific_humidity("ATMOSPHERE", inp, cfg, drop=drop)
    sphumw, _ = specific_humidity("WATER", inp, cfg)
    tair, mslp, sst = inp["tair"], inp["mslp"], inp["sst"]
    rhoair = mslp / (Ra_dry * (tair + tfrwK)) * (1. - sphuma * (1. - Ra_vap / Ra_dry))
    wspeed = wind_speed_element(inp["wind"], tri)
    Qsh = cfg["drag_ocean_t"] * rhoair * (cpa + sphuma * cpv) * wspeed * (sst - tair)
    Lv = Lv0 - 2.36418e3 * sst + 1.58927 * sst * sst
    if "Lv_cubic" not in drop:
        Lv = Lv - 6.14342e-2 * _pow(sst, 3.)
    raw = cfg["drag_ocean_q"] * rhoa * Lv * wspeed * (sphumw - sphuma)
    Qlh = _max(raw, 0.)
    evap = Qlh / Lv
    lin = 0.61 + 0.063 * wspeed
    drag_ocean_m = 1e-3 * _max(1., _min(2., lin))
    tau = rhoair * drag_ocean_m
    Qsw = -inp["Qsw_in"] * (1. - cfg["ocean_albedo"])
    Qlw_out = eps * sigma_sb * _pow(sst + tfrwK, 4.)
    Qlw = Qlw_out - incoming_longwave(inp, cfg)
    Qow = Qlw + Qsh + Qlh
    Qow = Qow + Qsw
    rec = {"Qlh_ow_clamped": np.less(raw, 0.), "drag_ocean_m": np.where(np.less(1., _min(2., lin)), np.where(np.less(lin, 2.), 1, 2), 0)}
    return {"Qow": Qow, "Qlw_ow": Qlw, "Qsw_ow": Qsw, "Qlh_ow": Qlh, "Qsh_ow": Qsh, "evap": evap, "tau_ow": tau}, rec


def stability_constants(cfg, quad_drag_coef_air):
    """the constants block of IABulkFluxes, FE.cpp:6168-6202"""
    k = {}
    zref_wind = cfg["zref_wind"]
    z0 = zref_wind * math.exp(-vonKarman / math.sqrt(quad_drag_coef_air))
    k["Linvrange"] = 1. / cfg["limiting_lengthscale"]
    am = 5.
    bm = am / 6.5
    Bm = _LIBM.cbrt((1 - bm) / bm)
    ah, bh, ch = 5., 5., 3.
    Bh = math.sqrt(5)
    k["Bm"], k["ch"] = Bm, ch
    k["C1"] = -3. * am / bm
    k["C2"] = 0.5 * am * Bm / bm
    k["C3"] = 1. / (1. + Bm)
    k["Bm2"] = Bm * Bm
    k["C4"] = 1. / (1. - Bm + k["Bm2"])
    sqrt3 = math.sqrt(3.)
    k["C5"] = 2. * sqrt3
    k["C6"] = 1. / (sqrt3 * Bm)
    k["C7"] = math.atan((2. - Bm) * k["C6"])
    k["D1"] = -0.5 * bh
    k["D2"] = -ah / Bh + 0.5 * bh * ch / Bh
    k["D3"] = ch - Bh
    k["D4"] = ch + Bh
    k["D5"] = math.log(k["D3"] / k["D4"])
    k["lambda_u"] = math.log(zref_wind / z0)
    k["lambda_h"] = math.log(zref_wind / z0)
    return k


def ia_bulk_fluxes(inp, cfg, tri, quad_drag_coef_air, Tsurf, snow_thick, conc, drag_ui, drag_ti, bulk_for_young, drop=()):
    """IABulkFluxes, FE.cpp:6148-6353; drag_ui and drag_ti are updated in place"""
    K = stability_constants(cfg, quad_drag_coef_air)
    retv = 0.6078
    zref_wind, zref_temp = cfg["zref_wind"], cfg["zref_temp"]
    mslp = inp["mslp"]
    with np.errstate(all="ignore"):
        Qlw_out = eps * sigma_sb * _pow(Tsurf + tfrwK, 4.)
        dQlwdT = 4. * eps * sigma_sb * _pow(Tsurf + tfrwK, 3.)
        sphumi, dsphumidT = specific_humidity("ICE", inp, cfg, Tsurf, drop=drop)
        sphuma, _ = specific_humidity("ATMOSPHERE", inp, cfg, drop=drop)
        tairK = inp["tair"] + tfrwK
        tsurfK = Tsurf + tfrwK
        rhoair = mslp / (Ra_dry * tairK) * (1. - sphuma * (1. - Ra_vap / Ra_dry))
        wspeed = wind_speed_element(inp["wind"], tri)
        Tpot = tairK + Gamma_d * zref_temp
        rec = {}
        if not cfg["force_neutral_atmosphere"]:
            ustar = np.sqrt(drag_ui) * wspeed
            Tvirt = Tpot * (1. + retv * sphuma)
            mixrat = sphuma / (1. - sphuma)
            wTpot = drag_ti * wspeed * (tsurfK - Tpot)
            wr = drag_ti * wspeed * (sphumi - sphuma) / ((1. - sphumi) * (1. - sphuma))
            wTvirt = wTpot * (1. + retv * mixrat)
            if "retv_Tpot_wr" not in drop:
                wTvirt = wTvirt + retv * Tpot * wr
            Linvrange = K["Linvrange"]
            Linv = _max(-Linvrange, _min(Linvrange, -vonKarman * g * wTvirt / (ustar * ustar * ustar * Tvirt)))
            zetam = zref_wind * Linv
            zetah = (zref_wind if "zetah_zref_temp" in drop else zref_temp) * Linv
            stable = Linv >= 0
            Bm, Bm2, ch = K["Bm"], (0. if "Bm2" in drop else K["Bm2"]), K["ch"]
            # the stable case
            x = _cbrt(1. + zetam)
            psim_s = K["C1"] * (x - 1.) + K["C2"] * (2. * _log((x + Bm) * K["C3"]) - _log((x * x - x * Bm + Bm2) * K["C4"]) + K["C5"] * (_atan((2. * x - Bm) * K["C6"]) - K["C7"]))
            psih_s = K["D1"] * _log(1. + ch * zetah + zetah * zetah) + K["D2"] * (_log((2. * zetah + K["D3"]) / (2. * zetah + K["D4"])) - K["D5"])
            # the unstable case
            x = np.sqrt(np.sqrt(1. - 16. * zetam))
            psim_u = 2. * _log(0.5 * (1. + x)) + _log(0.5 * (1. + x * x)) - 2. * _atan(x) + 0.5 * math.pi
            x = np.sqrt(np.sqrt(1. - 16. * zetah))
            psih_u = 2. * _log(0.5 * (1. + x * x))
            psim, psih = np.where(stable, psim_s, psim_u), np.where(stable, psih_s, psih_u)
            du = vonKarman / (K["lambda_u"] - psim)
            drag_ui[:] = du * du
            dt = vonKarman / (K["lambda_h"] - psih)
            drag_ti[:] = dt * dt
            rec.update(stable=stable, Linv_high=Linv == Linvrange, Linv_low=Linv == -Linvrange)
        Qsh = drag_ti * rhoair * cpa * wspeed * (tsurfK - Tpot)
        dQshdT = drag_ti * rhoair * cpa * wspeed
        Lsub = Lf + Lv0 - 240. - 290. * Tsurf - 4. * Tsurf * Tsurf
        Qlh = drag_ti * rhoair * Lsub * wspeed * (sphumi - sphuma)
        dQlhdT = drag_ti * Lsub * rhoair * wspeed * dsphumidT
        dQiadT = dQlwdT + dQshdT + dQlhdT
        ql = Qlh / Lsub
        subl = _max(0., ql)
        hs = np.where(conc > 0, snow_thick / conc, 0.)
        pf, lid = inp["pond_fraction"], inp["lid_volume"]
        pond_active = (pf > 0.) & (lid / pf <= 0.05)
        pond_fraction = np.where(pond_active, pf, 0.)
        if bulk_for_young:
            pond_fraction = np.zeros(pf.shape)
        alb_tot, pen_sw, hs_pos, warm = albedo(Tsurf, hs, pond_fraction, cfg["alb_scheme"], cfg["alb_ice"], cfg["alb_sn"], cfg["alb_ponds"], cfg["I_0"])
        Qsw = -inp["Qsw_in"] * (1. - alb_tot) * (1. - pen_sw)
        I = inp["Qsw_in"] * (1. - alb_tot) * pen_sw
        Qlw = Qlw_out - incoming_longwave(inp, cfg)
        Qia = Qsw + Qlw + Qsh + Qlh
    rec.update(Tsurf_warm=warm, hs_positive=hs_pos, pond_active=pond_active, subl_clamped=~np.less(0., ql))
    return dict(zip(ICE_ROWS, (Qia, Qlw, Qsw, Qlh, Qsh, I, subl, dQiadT, alb_tot))), rec


def fluxes(inp, cfg, tri, young, quad_drag_coef_air, drop=()):
    """thermo(), FE.cpp:5222-5273.  Returns (the 25 rows, the branch record); the four drags of inp are updated in place."""
    with np.errstate(all="ignore"):
        out, rec = ow_bulk_fluxes(inp, cfg, tri, drop)
    ice, r = ia_bulk_fluxes(inp, cfg, tri, quad_drag_coef_air, inp["tice0"], inp["snow_thick"], inp["conc"], inp["drag_ui"], inp["drag_ti"], False, drop)
    for k, name in zip(ICE_ROWS, ROWS[7:16]):
        out[name] = ice[k]
    rec.update(r)
    if young:
        ice, r = ia_bulk_fluxes(inp, cfg, tri, quad_drag_coef_air, inp["tsurf_young"], inp["hs_young"], inp["conc_young"], inp["drag_ui_young"], inp["drag_ti_young"], True, drop)
        for k in ICE_ROWS:
            out[k + "_young"] = ice[k]
        rec.update({k + "_young": v for k, v in r.items()})
    else:
        for k in ICE_ROWS:          # (albedo_young and I_young are value-initialised vectors nobody writes: zeros too)
            out[k + "_young"] = np.zeros(tri.shape[0])
    return {k: np.ascontiguousarray(out[k], np.float64) for k in ROWS}, rec


def same_record(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def make_inputs(x, y, tri, seed=1, drag_ui0=0.0049, drag_ti0=1.3e-3):
    """Inputs on a mesh (node coordinates, [Ne, 3] 0-based triangles) that put every recorded branch on both sides: four bands of wind speed across the mesh
    (below 1 m/s where the Obukhov length hits its limit, 2-6, 8-20 and 23-32 m/s for the three ranges of drag_ocean_m), a dozen calm elements, air on both
    sides of the surface temperatures, warm moist air over cold water (condensation: Qlh_ow clamped), bare and snow-covered ice, open and lidded ponds."""
    rng = np.random.default_rng(seed)
    Nn, Ne = x.size, tri.shape[0]
    u = (x - x.min()) / np.ptp(x)
    band = np.digitize(u, (0.2, 0.5, 0.7))
    lo = np.array([0.05, 2., 8., 23.])[band]
    hi = np.array([1.0, 6., 20., 32.])[band]
    speed = lo + (hi - lo) * rng.random(Nn)
    ang = 2. * np.pi * rng.random(Nn)
    wind = np.concatenate([speed * np.cos(ang), speed * np.sin(ang)])
    calm = rng.choice(Ne, 12, replace=False)
    for n in np.unique(tri[calm]):
        wind[n] = wind[n + Nn] = 0.
    r = lambda a, b: a + (b - a) * rng.random(Ne)
    inp = {"wind": wind}
    tair = r(-30., 4.)
    moist = rng.random(Ne) < 0.12
    tair[moist] = r(2., 6.)[moist]
    inp["tair"] = tair
    inp["dair"] = np.where(moist, tair - 0.3, tair - r(0.5, 8.))
    inp["mslp"] = r(96000., 104000.)
    inp["Qsw_in"] = r(0., 300.)
    inp["Qlw_in"] = r(150., 330.)
    inp["tcc"] = r(0., 1.)
    inp["sphuma"] = r(-2e-4, 4e-3)            # (a few below zero: std::max(0., M_sphuma[i]))
    inp["mixrat"] = r(2e-4, 4e-3)
    inp["sst"] = np.where(moist, r(-1.7, -1.2), r(-1.8, 8.))
    inp["sss"] = r(28., 35.)
    for name in ("tice0", "tsurf_young"):
        t = np.minimum(tair + 6. * rng.standard_normal(Ne), -1.2)
        warm = rng.random(Ne) < 0.15
        t[warm] = r(-0.95, 0.)[warm]
        inp[name] = t
    conc = np.where(rng.random(Ne) < 0.1, 0., r(0.05, 1.))
    inp["conc"] = conc
    inp["snow_thick"] = np.where(rng.random(Ne) < 0.2, 0., conc * r(0.01, 0.4))
    cy = np.where(rng.random(Ne) < 0.1, 0., r(0.01, 0.3))
    inp["conc_young"] = cy
    inp["hs_young"] = np.where(rng.random(Ne) < 0.3, 0., cy * r(0.005, 0.1))
    pf = np.where(rng.random(Ne) < 0.4, 0., r(0.01, 0.4))
    inp["pond_fraction"] = pf
    inp["lid_volume"] = pf * r(0., 0.1)
    inp["drag_ui"] = drag_ui0 * r(0.8, 1.2)
    inp["drag_ui_young"] = drag_ui0 * r(0.8, 1.2)
    inp["drag_ti"] = drag_ti0 * r(0.8, 1.2)
    inp["drag_ti_young"] = drag_ti0 * r(0.8, 1.2)
    return {k: np.ascontiguousarray(v, np.float64) for k, v in inp.items()}, np.sort(calm)


def moved_one_ulp(inp, direction):
    """every non-zero input moved to the neighbouring double away from (+1) or towards (-1) zero; a zero stays a zero (it is a value of its own: no ice, no
    snow, no wind)"""
    out = {}
    for k, v in inp.items():
        target = np.where(v > 0, np.inf, -np.inf) if direction > 0 else np.zeros(v.shape)
        out[k] = np.where(v == 0., v, np.nextafter(v, target))
    return out


def copy(inp):
    return {k: v.copy() for k, v in inp.items()}
