"""numpy restatement of FiniteElement::updateMeans (model/finiteelement.cpp:8518-8924, "FE.cpp" below) for the thermodynamic variables of nxs_dyn_means_*
(NXS_MEANS_THERMO_BEGIN ..): the cases tests/means_ref.py does not cover.

Every statement is `data_mesh[i] += field[i] * time_factor` (a rounded product and a rounded sum in fp64, what numpy does element by element), with three
exceptions: the five variables of the reversed sign convention are `-=` (FE.cpp:8829-8832, 8894-8909), the two ages are `field * time_factor / years_in_sec`
(a rounded product, then a rounded quotient: FE.cpp:8606-8614), and wspeed goes through hypot (windSpeedElement, FE.cpp:6359-6370).  tsurf is D_tsurf of
updateIceDiagnostics (FE.cpp:7875-7883), each product and sum rounded on its own.

Inputs are the host copies of the very rows the device holds, as one dict `src`:
  the rows of nxs_dyn_flux_state (tice0, tsurf_young, sst, sss, drag_ti, drag_ti_young, pond_fraction, lid_volume), of nxs_dyn_column_state (tice1, tice2), of
  nxs_dyn_slab_state (conc_upd ... age) and of nxs_dyn_slab_get (Qa ... del_vi_rplnt_myi) under the names of nextsim_amd._abi; the atmosphere (tair, mslp, Qsw_in,
  humidity, longwave) and the column's forcing (precip, snow, ocean_temp, ocean_salt, mld) as they were uploaded; conc and conc_young of nxs_dyn_get_state; wind.
"""
import json
import os

import numpy as np

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_constants.json")
YEARS_IN_SEC = float.fromhex(json.load(open(_GOLDEN))["members"]["years_in_sec"]["hex"]) if os.path.exists(_GOLDEN) else 365.25 * 86400.

# the variables in id order (nextsim_amd._abi.MEANS_THERMO), each with the key of its source row in `src` (None: computed)
SOURCE = (
    ("sst", "sst"), ("sss", "sss"), ("tsurf_ice", "tice0"), ("meltpond_lid_volume", "lid_volume"), ("meltpond_fraction", "pond_fraction"),   # FE.cpp:8556, 8561, 8566, 8626, 8779
    ("drag_ti", None),                                                                                                                      # :8767-8777
    ("t1", "tice1"), ("t2", "tice2"),                                                                                                       # :8571, 8576
    ("conc_upd", "conc_upd"), ("meltpond_volume", "pond_volume"), ("del_vi_tend", "del_vi_tend"), ("freeze_days", "freeze_days"),           # :8616, 8621, 8656, 8640
    ("freeze_onset", "freeze_onset"), ("conc_summer", "conc_summer"), ("thick_summer", "thick_summer"), ("fyi_fraction", "fyi_fraction"),   # :8652, 8644, 8648, 8601
    ("age_det", "age_det"), ("age", "age"),                                                                                                 # :8606, 8611
    ("Qa", "Qa"), ("Qsw", "Qsw"), ("Qlw", "Qlw"), ("Qsh", "Qsh"), ("Qlh", "Qlh"), ("Qo", "Qo"), ("delS", "delS"), ("evap", "evap"),          # :8697-8725
    ("rain", "rain"), ("sialb", "sialb"), ("albedo", "albedo"),                                                                             # :8729, 8733, 8737
    ("del_vi_young", "del_vi_young"), ("vice_melt", "vice_melt"), ("del_hi", "del_hi"), ("del_hi_young", "del_hi_young"),                   # :8833-8845
    ("newice", "newice"), ("snow2ice", "snow2ice"), ("mlt_top", "mlt_top"), ("mlt_bot", "mlt_bot"),                                         # :8849-8861
    ("dvi_rplnt_myi", "del_vi_rplnt_myi"), ("dci_rplnt_myi", "del_ci_rplnt_myi"), ("dvi_mlt_myi", "del_vi_mlt_myi"), ("dci_mlt_myi", "del_ci_mlt_myi"),   # :8664-8676
    ("fwflux_ice", "fwflux_ice"), ("fwflux", "fwflux"), ("QNoSw", "Qnosun"), ("QSwOcean", "Qsw_ocean"), ("saltflux", "brine"),              # :8829, 8894-8906: -=
    ("tair", "tair"), ("mslp", "mslp"), ("Qsw_in", "Qsw_in"), ("sphuma", "humidity"), ("mixrat", "humidity"), ("d2m", "humidity"),          # :8785-8805
    ("Qlw_in", "longwave"), ("tcc", "longwave"),                                                                                            # :8809, 8813
    ("precip", "precip"), ("snowfall", "snow"), ("snowfr", "snow"), ("ocean_temp", "ocean_temp"), ("ocean_salt", "ocean_salt"), ("mld", "mld"),   # :8825, 8817, 8821, 8873, 8877, 8869
    ("tsurf", None), ("wspeed", None),                                                                                                      # :8551, 8865
)
THERMO = tuple(k for k, _ in SOURCE)
NEGATED = ("fwflux_ice", "fwflux", "QNoSw", "QSwOcean", "saltflux")      # "NB: reversed sign convention!" (FE.cpp:8893)
YEARS = ("age_det", "age")
LIBM = ("wspeed",)                                                       # the variable with a hypot inside
_KEY = dict(SOURCE)


def wind_speed_element(wind, tri):
    """windSpeedElement, FE.cpp:6359-6370: wspd = 0; wspd += hypot(u, v) over the three nodes in order; wspd / 3."""
    Nn = wind.size // 2
    w = np.zeros(tri.shape[0])
    for j in range(3):
        w = w + np.hypot(wind[tri[:, j]], wind[tri[:, j] + Nn])
    return w / 3.


def d_tsurf(src, young):
    """D_tsurf of updateIceDiagnostics, FE.cpp:7872-7883"""
    d_conc = src["conc"].copy()                                       # :7872
    t = src["conc"] * src["tice0"]                                    # :7875
    if young:
        d_conc = d_conc + src["conc_young"]                           # :7878
        t = t + src["conc_young"] * src["tsurf_young"]                # :7881
    return t + (1 - d_conc) * src["sst"]                              # :7883


class ThermoMeansRef:
    """el [Ne, n]: the mesh accumulators of the named variables, columns in the order of `names`; ghost rows (i >= local_nelements) are never touched."""

    def __init__(self, num_elements, local_nelements, young_cat, names):
        self.Ne, self.Neo, self.young, self.names = num_elements, local_nelements, bool(young_cat), tuple(names)
        for k in self.names:
            if k not in _KEY:
                raise KeyError(k)
        self.reset()

    def reset(self):
        self.el = np.zeros((self.Ne, len(self.names)))

    def update(self, tf, src, tri=None):
        n = self.Neo                                                  # FE.cpp:8527: i < M_local_nelements
        with np.errstate(invalid="ignore", divide="ignore"):
            for k, name in enumerate(self.names):
                acc = self.el[:n, k]
                if name == "drag_ti":                                 # FE.cpp:8767-8777
                    drag = src["drag_ti"][:n]
                    if self.young:
                        drag = (src["drag_ti"][:n] * src["conc"][:n] + src["drag_ti_young"][:n] * src["conc_young"][:n]) / (src["conc"][:n] + src["conc_young"][:n])
                    acc += drag * tf
                elif name == "tsurf":
                    acc += d_tsurf(src, self.young)[:n] * tf          # FE.cpp:8551
                elif name == "wspeed":
                    acc += wind_speed_element(src["wind"], tri)[:n] * tf   # FE.cpp:8865
                elif name in YEARS:
                    acc += src[_KEY[name]][:n] * tf / YEARS_IN_SEC    # FE.cpp:8608, 8613
                elif name in NEGATED:
                    acc -= src[_KEY[name]][:n] * tf                   # FE.cpp:8831, 8896, 8900, 8904, 8908
                else:
                    acc += src[_KEY[name]][:n] * tf
