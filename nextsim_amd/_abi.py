"""ctypes mirror of include/nxs_dyn.h (the C ABI of libnxsdyn.so).

Pure declarations: struct layouts, argument types, numpy <-> pointer helpers.  No compute here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint8_p = C.POINTER(C.c_uint8)

NXS_DYN_BBM, NXS_DYN_NO_MOTION, NXS_DYN_FREE_DRIFT, NXS_DYN_EVP, NXS_DYN_MEVP = range(5)
NXS_BASAL_NONE, NXS_BASAL_LEMIEUX = 0, 1
NXS_ICECAT_CLASSIC, NXS_ICECAT_YOUNG_ICE = 0, 1

DYNAMICS_TYPES = {"bbm": NXS_DYN_BBM, "no_motion": NXS_DYN_NO_MOTION, "free_drift": NXS_DYN_FREE_DRIFT,
                  "evp": NXS_DYN_EVP, "mevp": NXS_DYN_MEVP}

ERRORS = {0: "NXS_OK", -1: "NXS_ERR_INVALID", -2: "NXS_ERR_NO_DEVICE", -3: "NXS_ERR_HIP",
          -4: "NXS_ERR_STATE", -5: "NXS_ERR_COMM", -6: "NXS_ERR_NOMEM", -7: "NXS_ERR_INTERNAL"}


class Params(C.Structure):
    _fields_ = [
        ("dtime_step", C.c_double),
        ("substeps", C.c_int32),
        ("dynamics_type", C.c_int32),
        ("basal_stress_type", C.c_int32),
        ("ice_cat_type", C.c_int32),
        ("newice_type", C.c_int32),
        ("equal_ridging", C.c_int32),
        ("use_young_ice_in_myi_reset", C.c_int32),
        ("reserved0", C.c_int32),
        ("young", C.c_double),
        ("nu0", C.c_double),
        ("tan_phi", C.c_double),
        ("compr_strength", C.c_double),
        ("compaction_param", C.c_double),
        ("undamaged_time_relaxation_sigma", C.c_double),
        ("exponent_relaxation_sigma", C.c_double),
        ("compression_factor", C.c_double),
        ("exponent_compression_factor", C.c_double),
        ("min_h", C.c_double),
        ("min_c", C.c_double),
        ("quad_drag_coef_water", C.c_double),
        ("lin_drag_coef_water", C.c_double),
        ("quad_drag_coef_air", C.c_double),
        ("lin_drag_coef_air", C.c_double),
        ("ocean_turning_angle_rad", C.c_double),
        ("basal_k1", C.c_double),
        ("basal_k2", C.c_double),
        ("basal_Cb", C.c_double),
        ("basal_u_0", C.c_double),
        ("evp_e", C.c_double),
        ("evp_Pstar", C.c_double),
        ("evp_C", C.c_double),
        ("evp_dmin", C.c_double),
        ("mevp_alpha", C.c_double),
        ("mevp_beta", C.c_double),
        ("regrid_angle", C.c_double),
    ]

    def copy(self) -> "Params":
        q = Params()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(Params))
        return q


class Mesh(C.Structure):
    _fields_ = [
        ("num_nodes", C.c_int32),
        ("num_elements", C.c_int32),
        ("local_ndof", C.c_int32),
        ("local_nelements", C.c_int32),
        ("indices", c_int32_p),
        ("ghost_nodes", c_uint8_p),
        ("coord_x", c_double_p),
        ("coord_y", c_double_p),
        ("lat", c_double_p),
        ("mask_dirichlet", c_uint8_p),
        ("num_neumann_flags", C.c_int32),
        ("reserved0", C.c_int32),
        ("neumann_flags", c_int32_p),
        ("nodal_element_connectivity", c_double_p),
        ("nodal_connectivity", c_double_p),
        ("nec_width", C.c_int32),
        ("nc_width", C.c_int32),
    ]


class Halo(C.Structure):
    _fields_ = [
        ("rank", C.c_int32),
        ("nranks", C.c_int32),
        ("num_send_procs", C.c_int32),
        ("num_recv_procs", C.c_int32),
        ("send_procs", c_int32_p),
        ("send_offsets", c_int32_p),
        ("send_index", c_int32_p),
        ("recv_procs", c_int32_p),
        ("recv_offsets", c_int32_p),
        ("recv_index", c_int32_p),
    ]


class State(C.Structure):
    _fields_ = [
        ("VT", c_double_p), ("UM", c_double_p), ("UT", c_double_p),
        ("conc", c_double_p), ("thick", c_double_p), ("snow_thick", c_double_p),
        ("damage", c_double_p), ("ridge_ratio", c_double_p),
        ("sigma", c_double_p * 3),
        ("conc_young", c_double_p), ("h_young", c_double_p), ("hs_young", c_double_p),
        ("conc_myi", c_double_p), ("thick_myi", c_double_p),
        ("cohesion", c_double_p), ("time_relaxation_damage", c_double_p),
        ("drag_ui", c_double_p), ("drag_ui_young", c_double_p),
    ]


class Forcing(C.Structure):
    _fields_ = [("wind", c_double_p), ("ocean", c_double_p), ("ssh", c_double_p),
                ("element_depth", c_double_p)]


class Diag(C.Structure):
    _fields_ = [("surface", c_double_p), ("delta_x", c_double_p), ("D_tau_a", c_double_p),
                ("D_tau_w", c_double_p), ("D_del_ci_ridge_myi", c_double_p)]


class Coupled(C.Structure):   # nxs_dyn_coupled
    _fields_ = [("cum_damage", c_double_p), ("conc_fsd", c_double_p), ("num_fsd_bins", C.c_int32), ("reserved0", C.c_int32)]


# ---- the floe-size distribution (include/nxs_dyn.h, nxs_dyn_fsd_*): setup::FSDType, WeldingType, BreakupType of model/enums.hpp:99-116
NXS_FSD_MAX_BINS = 16
NXS_FSD_CONSTANT_SIZE, NXS_FSD_CONSTANT_AREA = 0, 1
NXS_WELDING_NONE, NXS_WELDING_ROACH = 0, 1
NXS_BREAKUP_NONE, NXS_BREAKUP_UNIFORM_SIZE, NXS_BREAKUP_ZHANG, NXS_BREAKUP_DUMONT = range(4)
NXS_FSD_WLBK_ON_DEVICE = 1
FSD_TYPES = {"constant_size": NXS_FSD_CONSTANT_SIZE, "constant_area": NXS_FSD_CONSTANT_AREA}
WELDING_TYPES = {"none": NXS_WELDING_NONE, "roach": NXS_WELDING_ROACH}
BREAKUP_TYPES = {"none": NXS_BREAKUP_NONE, "uniform_size": NXS_BREAKUP_UNIFORM_SIZE, "zhang": NXS_BREAKUP_ZHANG, "dumont": NXS_BREAKUP_DUMONT}
FSD_TABLES = ("bin_widths", "bin_low_limits", "bin_up_limits", "bin_centres", "area_scaled_up", "area_scaled_low", "area_scaled_centered", "area_scaled_binwidth")


class FsdTables(C.Structure):   # nxs_fsd_tables
    _fields_ = [(k, c_double_p) for k in FSD_TABLES] + [("alpha_merge", c_int32_p)]


FSD_CONFIG_INTS = ("num_bins", "breakup_type", "breakup_prob_type", "fsd_damage_type", "welding_type", "distinguish_mech_fsd", "debug_fsd", "breakup_cell_average_thickness")
FSD_CONFIG_REALS = ("breakup_coef1", "breakup_coef2", "breakup_coef3", "breakup_prob_cutoff", "breakup_timescale_tuning", "cpl_time_step", "floes_flex_young",
                    "breakup_thick_min", "fsd_damage_max", "welding_kappa")


class FsdConfig(C.Structure):   # nxs_dyn_fsd_config
    _fields_ = [(k, C.c_int32) for k in FSD_CONFIG_INTS] + [(k, C.c_double) for k in FSD_CONFIG_REALS] + [("tables", FsdTables)]


class FsdState(C.Structure):   # nxs_dyn_fsd_state
    _fields_ = [("conc_mech_fsd", c_double_p), ("cum_wave_damage", c_double_p), ("num_fsd_bins", C.c_int32), ("weld_crash", C.c_int32)]


def fsd_tables_struct(tables: dict) -> FsdTables:
    """nxs_fsd_tables pointing at the arrays of `tables` (float64 [n] each, alpha_merge int32 [n, n]; they must stay alive); a missing key stays NULL."""
    t = FsdTables()
    for k in FSD_TABLES:
        if tables.get(k) is not None:
            setattr(t, k, dptr(tables[k]))
    if tables.get("alpha_merge") is not None:
        t.alpha_merge = iptr(tables["alpha_merge"])
    return t


def fsd_config_struct(num_bins: int, tables: dict, **options) -> FsdConfig:
    """nxs_dyn_fsd_config from keyword options named after its members (breakup_type / welding_type also by the reference's option strings)."""
    c = FsdConfig()
    c.num_bins = int(num_bins)
    for k, v in options.items():
        if k == "breakup_type" and isinstance(v, str):
            v = BREAKUP_TYPES[v]
        if k == "welding_type" and isinstance(v, str):
            v = WELDING_TYPES[v]
        if k not in FSD_CONFIG_INTS + FSD_CONFIG_REALS:
            raise KeyError(f"nxs_dyn_fsd_config has no member {k!r}")
        setattr(c, k, int(v) if k in FSD_CONFIG_INTS else float(v))
    c.tables = fsd_tables_struct(tables)
    return c


# ---- thermo()'s atmospheric bulk fluxes (include/nxs_dyn.h, nxs_dyn_flux_* / nxs_dyn_fluxes)
NXS_FLUX_HUM_DEWPOINT, NXS_FLUX_HUM_SPHUMA, NXS_FLUX_HUM_MIXRAT = range(3)
NXS_FLUX_LW_QLW_IN, NXS_FLUX_LW_TCC = 0, 1
FLUX_HUMIDITY = {"dewpoint": NXS_FLUX_HUM_DEWPOINT, "sphuma": NXS_FLUX_HUM_SPHUMA, "mixrat": NXS_FLUX_HUM_MIXRAT}
FLUX_LONGWAVE = {"Qlw_in": NXS_FLUX_LW_QLW_IN, "tcc": NXS_FLUX_LW_TCC}
FLUX_CONSTANTS = ("tfrwK", "Ra_dry", "Ra_vap", "cpa", "cpv", "Lv0", "eps", "sigma_sb", "vonKarman", "Gamma_d", "rhoa", "Lf", "g")   # NXS_FLUX_CONST_*
FLUX_CONFIG_INTS = ("alb_scheme", "humidity_source", "longwave_source", "force_neutral_atmosphere")
FLUX_CONFIG_REALS = ("alb_ice", "alb_sn", "alb_ponds", "I_0", "ocean_albedo", "drag_ocean_t", "drag_ocean_q", "zref_wind", "zref_temp", "limiting_lengthscale")
FLUX_ATMOSPHERE = ("tair", "mslp", "Qsw_in", "humidity", "longwave")
FLUX_STATE = ("tice0", "tsurf_young", "sst", "sss", "drag_ti", "drag_ti_young", "pond_fraction", "lid_volume")
FLUX_ICE_ROWS = ("Qia", "Qlw", "Qsw", "Qlh", "Qsh", "I", "subl", "dQiadT", "albedo")
FLUX_ROWS = (("Qow", "Qlw_ow", "Qsw_ow", "Qlh_ow", "Qsh_ow", "evap", "tau_ow", "Qia", "Qlwi", "Qswi", "Qlhi", "Qshi", "I", "subl", "dQiadT", "albedo")
             + tuple(k + "_young" for k in FLUX_ICE_ROWS))   # NXS_FLUX_*
NXS_FLUX_ROWS = 25
assert len(FLUX_ROWS) == NXS_FLUX_ROWS


class FluxConfig(C.Structure):   # nxs_dyn_flux_config
    _fields_ = [(k, C.c_int32) for k in FLUX_CONFIG_INTS] + [(k, C.c_double) for k in FLUX_CONFIG_REALS]


class FluxAtmosphere(C.Structure):   # nxs_dyn_flux_atmosphere
    _fields_ = [(k, c_double_p) for k in FLUX_ATMOSPHERE]


class FluxState(C.Structure):   # nxs_dyn_flux_state
    _fields_ = [(k, c_double_p) for k in FLUX_STATE]


class FluxRows(C.Structure):   # nxs_dyn_flux_rows
    _fields_ = [("row", c_double_p * NXS_FLUX_ROWS)]


def flux_config_struct(base: "FluxConfig", **options) -> FluxConfig:
    """A copy of `base` (the defaults of nxs_flux_default_config) with keyword options named after nxs_dyn_flux_config's members; humidity_source /
    longwave_source also by name ("dewpoint" / "sphuma" / "mixrat", "Qlw_in" / "tcc")."""
    c = FluxConfig()
    C.memmove(C.byref(c), C.byref(base), C.sizeof(c))
    for k, v in options.items():
        if k == "humidity_source" and isinstance(v, str):
            v = FLUX_HUMIDITY[v]
        if k == "longwave_source" and isinstance(v, str):
            v = FLUX_LONGWAVE[v]
        if k not in FLUX_CONFIG_INTS + FLUX_CONFIG_REALS:
            raise KeyError(f"nxs_dyn_flux_config has no member {k!r}")
        setattr(c, k, int(v) if k in FLUX_CONFIG_INTS else float(v))
    return c


# ---- thermo()'s ice columns (include/nxs_dyn.h, nxs_col_* / nxs_dyn_column_* / nxs_dyn_column)
COL_THERMO = {"zero_layer": 0, "winton": 1}                 # NXS_COL_THERMO_*: setup::ThermoType
COL_QIO = {"basic": 0, "exchange": 1}                       # NXS_COL_QIO_*: setup::OceanHeatfluxScheme
COL_FREEZINGPOINT = {"linear": 0, "unesco": 1}              # NXS_COL_FREEZINGPOINT_*: setup::FreezingPointType
COL_OCEAN = {"constant": 0, "nudged": 1, "coupled": 7}      # NXS_COL_OCEAN_*: setup::OceanType (coupled is refused)
COL_SNOWFALL = {"precip_snowfr": 0, "snowfall": 1, "precip_tair": 2}   # NXS_COL_SNOWFALL_*
COL_MLD = {"constant": 0, "row": 1}                         # NXS_COL_MLD_*
COL_ENUMS = {"thermo_type": COL_THERMO, "qio_type": COL_QIO, "freezingpoint_type": COL_FREEZINGPOINT, "ocean_type": COL_OCEAN, "snowfall_source": COL_SNOWFALL,
             "mld_source": COL_MLD}
COL_CONSTANTS = ("rhow", "cpw", "rhoi", "rhos", "Lf", "C", "ki", "si", "hmin")   # NXS_COL_CONST_*
COL_CONFIG_INTS = ("thermo_type", "qio_type", "freezingpoint_type", "ocean_type", "snowfall_source", "mld_source", "flooding", "reserved")
COL_CONFIG_REALS = ("freezingpoint_mu", "snow_cond", "Csens_io", "constant_mld", "nudge_timeT", "nudge_timeS", "Qdw_const", "Fdw_const")
COL_FORCING = ("precip", "snow", "ocean_temp", "ocean_salt", "mld")
COL_STATE = ("tice1", "tice2")
COL_ICE_ROWS = ("Qio", "hi", "hs", "hi_old", "del_hi", "del_hs_mlt", "mlt_hi_top", "mlt_hi_bot", "del_hi_s2i")
COL_YOUNG_ROWS = ("Qio_young", "hi_young", "hs_young", "hi_young_old", "del_hi_young", "del_hs_young_mlt", "mlt_hi_top_young", "mlt_hi_bot_young", "del_hi_s2i_young")
COL_ROWS = ("snowfall", "Qdw", "Fdw", "tfrw") + COL_ICE_ROWS + COL_YOUNG_ROWS   # NXS_COL_*
NXS_COL_ROWS = 22
assert len(COL_ROWS) == NXS_COL_ROWS


class ColumnConfig(C.Structure):   # nxs_dyn_column_config
    _fields_ = [(k, C.c_int32) for k in COL_CONFIG_INTS] + [(k, C.c_double) for k in COL_CONFIG_REALS]


class ColumnForcing(C.Structure):   # nxs_dyn_column_forcing
    _fields_ = [(k, c_double_p) for k in COL_FORCING]


class ColumnState(C.Structure):   # nxs_dyn_column_state
    _fields_ = [(k, c_double_p) for k in COL_STATE]


class ColumnRows(C.Structure):   # nxs_dyn_column_rows
    _fields_ = [("row", c_double_p * NXS_COL_ROWS)]


def column_config_struct(base: "ColumnConfig", **options) -> ColumnConfig:
    """A copy of `base` (the defaults of nxs_col_default_config) with keyword options named after nxs_dyn_column_config's members; the enums also by name."""
    c = ColumnConfig()
    C.memmove(C.byref(c), C.byref(base), C.sizeof(c))
    for k, v in options.items():
        if k in COL_ENUMS and isinstance(v, str):
            v = COL_ENUMS[k][v]
        if k not in COL_CONFIG_INTS + COL_CONFIG_REALS or k == "reserved":
            raise KeyError(f"nxs_dyn_column_config has no member {k!r}")
        setattr(c, k, int(v) if k in COL_CONFIG_INTS else float(v))
    return c


# ---- thermo()'s element forcing on the device (include/nxs_dyn.h, nxs_dyn_thermo_forcing_*)
OC_ROWS = ("ocean_temp", "ocean_salt", "qsrml", "mld", "wlbk")   # NXS_OC_*: the rows a coupled ocean delivers (nxs_dyn_ocean_coupled_*)
NXS_OC_ROWS = 5
NXS_GRIDMAP_MAX_RECEIVE = 5
assert len(OC_ROWS) == NXS_OC_ROWS


class OceanCoupledConfig(C.Structure):   # nxs_dyn_ocean_coupled_config
    _fields_ = [("n_fields", C.c_int32), ("row", C.c_int32 * NXS_OC_ROWS), ("a", C.c_double * NXS_OC_ROWS), ("b", C.c_double * NXS_OC_ROWS),
                ("factor", C.c_double * NXS_OC_ROWS), ("bias", C.c_double * NXS_OC_ROWS)]


class OceanCoupledRows(C.Structure):   # nxs_dyn_ocean_coupled_rows
    _fields_ = [("row", c_double_p * NXS_OC_ROWS)]


def ocean_coupled_config_struct(rows, a=None, b=None, factor=None, bias=None) -> OceanCoupledConfig:
    """rows: the names (OC_ROWS) or numbers of the received rows in the order the fields arrive; a, b, factor, bias: per field, a scalar or a sequence (default 1, 0,
    1, 0).  Nothing is checked here: that is nxs_ocean_coupled_config_check's."""
    c = OceanCoupledConfig()
    rows = list(rows)
    c.n_fields = len(rows)
    for k, r in enumerate(rows[:NXS_OC_ROWS]):
        c.row[k] = OC_ROWS.index(r) if isinstance(r, str) else int(r)
    for name, v, dflt in (("a", a, 1.), ("b", b, 0.), ("factor", factor, 1.), ("bias", bias, 0.)):
        vals = np.broadcast_to(np.asarray(dflt if v is None else v, np.float64), (len(rows),)) if len(rows) else np.zeros(0)
        arr = getattr(c, name)
        for k in range(NXS_OC_ROWS):
            arr[k] = float(vals[k]) if k < len(rows) else dflt
    return c


TF_ROWS = FLUX_ATMOSPHERE + COL_FORCING   # NXS_TF_*: tair .. longwave are d_flux_atm's rows, precip .. mld d_col_forcing's
NXS_TF_ROWS = 10
NXS_TF_SETS = 4
NXS_TF_MAX_COLUMNS = 32
NXS_TF_OFF, NXS_TF_LINEAR, NXS_TF_STEP = 0, 1, 2
TF_MODES = {"off": NXS_TF_OFF, "linear": NXS_TF_LINEAR, "step": NXS_TF_STEP}
assert len(TF_ROWS) == NXS_TF_ROWS


class ThermoForcingRows(C.Structure):   # nxs_dyn_thermo_forcing_rows
    _fields_ = [("row", c_double_p * NXS_TF_ROWS)]


class ThermoForcingTime(C.Structure):   # struct nxs_dyn_thermo_forcing_time
    _fields_ = [("mode", C.c_int32 * NXS_TF_ROWS)] + [(k, C.c_double * NXS_TF_ROWS) for k in ("fcoeff0", "fcoeff1", "factor", "bias")]


class ForcingGrid(C.Structure):   # nxs_dyn_forcing_grid
    _fields_ = [("x_in", c_double_p), ("y_in", c_double_p)] + [(k, C.c_int32) for k in ("x_rows", "y_rows", "M", "N", "interp", "row_major")] + [("default_value", C.c_double)]


# ---- the dynamics' nodal forcing on the device (include/nxs_dyn.h, nxs_mapx_* / nxs_dyn_forcing_*)
NF_ROWS = ("wind_u", "wind_v", "ocean_u", "ocean_v", "ssh")   # NXS_NF_*
NF_GROUPS = ("wind", "ocean", "ssh")                          # NXS_NF_GROUP_*
NXS_NF_ROWS, NXS_NF_SETS, NXS_NF_MAX_COLUMNS, NXS_NF_MAX_VECTORS, NXS_NF_GROUPS = 5, 4, 32, 4, 3
MAPX_POLAR_FIELDS = ("lon0", "Rg", "m1", "t1", "eccentricity", "scale", "lat1", "T00", "T01", "T10", "T11", "u0", "v0", "false_easting", "false_northing")


class MapxPolar(C.Structure):   # nxs_mapx_polar
    _fields_ = [(k, C.c_double) for k in MAPX_POLAR_FIELDS]


class ForcingVectors(C.Structure):   # nxs_dyn_forcing_vectors
    _fields_ = ([("n_pairs", C.c_int32)] + [(k, C.c_int32 * NXS_NF_MAX_VECTORS) for k in ("component0", "component1", "east_west_oriented", "is_wav_dir")]
                + [(k, C.c_int32) for k in ("gridded_rotation_angle", "latlon_per_point", "rotate")] + [("lat", c_double_p), ("lon", c_double_p), ("map", MapxPolar),
                                                                                                        ("cos_m_diff_angle", C.c_double), ("sin_m_diff_angle", C.c_double)])


# ---- the coupler's receive of nodal fields (include/nxs_interp.h, nxs_nodemap_*; include/nxs_dyn.h, nxs_dyn_nodes_coupled_*)
NXS_NODEMAP_MAX_RECEIVE = 4
NXS_NODEMAP_GET = 4
NODEMAP_ROTATE = {"none": 0, "uniform": 1, "grid_theta": 2}      # NXS_NODEMAP_ROTATE_*
NC_DATASETS = ("ocean", "wave")                                   # NXS_NC_OCEAN, NXS_NC_WAVE
NC_FIELDS = {"ocean": ("I_Uocn", "I_Vocn", "I_SSH"), "wave": ("I_tauwix", "I_tauwiy")}
NXS_NC_MAX_FIELDS = 3


class NodemapSource(C.Structure):   # nxs_nodemap_source
    _fields_ = [("G", C.c_int32), ("R", C.c_int32), ("reduced", c_int32_p), ("rotation_mode", C.c_int32), ("east_west_oriented", C.c_int32),
                ("cos_m_diff_angle", C.c_double), ("sin_m_diff_angle", C.c_double), ("rotation", C.c_double), ("theta", c_double_p), ("lat", c_double_p),
                ("lon", c_double_p), ("map", C.POINTER(MapxPolar)), ("delta_t", C.c_double)]


NXS_NODEMAP_MAX_LOAD = 8      # columns of nxs_nodemap_load_rows: up to 4 variables x nb_forcing_step (1 or 2)


class NodemapLoad(C.Structure):   # nxs_nodemap_load
    _fields_ = ([("n_var", C.c_int32), ("n_step", C.c_int32), ("fields", C.POINTER(C.c_void_p))]
                + [(k, C.c_double * NXS_NODEMAP_MAX_LOAD) for k in ("scale_factor", "add_offset", "a", "b")] + [("pairs", C.c_int32 * 4)])


class NodesCoupledConfig(C.Structure):   # nxs_dyn_nodes_coupled_config
    _fields_ = [(k, C.c_double * NXS_NC_MAX_FIELDS) for k in ("a", "b", "factor", "bias")]


class ForcingRows(C.Structure):   # nxs_dyn_forcing_rows
    _fields_ = [("row", c_double_p * NXS_NF_ROWS)]


class ForcingTimeRows(C.Structure):   # struct nxs_dyn_forcing_time_rows
    _fields_ = [("mode", C.c_int32 * NXS_NF_GROUPS)] + [(k, C.c_double * NXS_NF_GROUPS) for k in ("fcoeff0", "fcoeff1", "factor", "bias")]


# ---- nesting and the slab ocean's diffusion on the device (include/nxs_dyn.h, nxs_dyn_nesting_* / nxs_dyn_diffuse)
NEST_ELEMENT_ROWS = ("dist", "thick", "conc", "snow_thick", "h_young", "conc_young", "hs_young", "sigma1", "sigma2", "sigma3", "damage", "ridge_ratio")   # NXS_NEST_*
NEST_NODE_ROWS = ("dist_nodes", "VT1", "VT2")
NEST_DATASETS = ("distance_elements", "ice_elements", "dynamics_elements", "distance_nodes", "nodes")   # NXS_NEST_DS_*
NXS_NEST_ELEMENT_ROWS, NXS_NEST_NODE_ROWS, NXS_NEST_DATASETS = 12, 3, 5
NXS_NUDGE_LINEAR, NXS_NUDGE_EXPONENTIAL = 0, 1
NUDGE_FUNCTIONS = {"linear": NXS_NUDGE_LINEAR, "exponential": NXS_NUDGE_EXPONENTIAL}
assert (len(NEST_ELEMENT_ROWS), len(NEST_NODE_ROWS), len(NEST_DATASETS)) == (NXS_NEST_ELEMENT_ROWS, NXS_NEST_NODE_ROWS, NXS_NEST_DATASETS)


class NestingConfig(C.Structure):   # nxs_dyn_nesting_config
    _fields_ = [(k, C.c_int32) for k in ("nudge_function", "nest_dynamic_vars", "time_step", "reserved0")] + [(k, C.c_double) for k in ("nudge_timescale", "nudge_scale", "dtime_step")]


class NestingRows(C.Structure):   # nxs_dyn_nesting_rows
    _fields_ = [("element", c_double_p * NXS_NEST_ELEMENT_ROWS), ("node", c_double_p * NXS_NEST_NODE_ROWS)]


class NestingTime(C.Structure):   # struct nxs_dyn_nesting_time
    _fields_ = [("mode", C.c_int32 * NXS_NEST_DATASETS), ("reserved0", C.c_int32)] + [(k, C.c_double * NXS_NEST_DATASETS) for k in ("fcoeff0", "fcoeff1", "factor", "bias")]


# ---- thermo()'s slab loop from new ice to tracers (include/nxs_dyn.h, nxs_slab_* / nxs_dyn_slab_* / nxs_dyn_slab)
SLAB_CONSTANTS = ("cmin", "hmin", "rhow", "cpw", "rhoi", "rhos", "Lf", "C", "ki", "si", "days_in_sec")   # NXS_SLAB_CONST_*
SLAB_CONFIG_INTS = ("newice_type", "melt_type", "use_assim_flux", "temp_dep_healing", "use_meltponds", "reset_by_date", "include_young_ice", "equal_melting")
SLAB_CONFIG_REALS = ("hnull", "PhiF", "PhiM", "h_young_min", "h_young_max", "assim_flux_exponent", "reset_freeze_days", "meltpond_runoff_fraction",
                     "meltpond_depth_to_fraction", "time_relaxation_damage", "deltaT_relaxation_damage")
SLAB_STATE = ("conc_upd", "pond_volume", "del_vi_tend", "freeze_days", "freeze_onset", "conc_summer", "thick_summer", "fyi_fraction", "age_det", "age")
SLAB_STATE_GET = SLAB_STATE + ("time_relaxation_damage",)   # what nxs_dyn_slab_get_state also returns
SLAB_CLOCK = ("first_step_of_day", "last_step_of_day", "fyi_reset_now", "myi_reset_now", "onset_reset_now")
SLAB_ROWS = ("Qa", "Qsw", "Qlw", "Qsh", "Qlh", "Qo", "Qnosun", "Qsw_ocean", "Qassim", "delS", "fwflux_ice", "fwflux", "brine", "evap", "rain",
             "vice_melt", "del_vi_young", "del_hi", "del_hi_young", "newice", "mlt_top", "mlt_bot", "snow2ice", "albedo", "sialb",
             "del_ci_mlt_myi", "del_vi_mlt_myi", "del_ci_rplnt_myi", "del_vi_rplnt_myi")   # NXS_SLAB_*: D_Qa ... D_del_vi_rplnt_myi
NXS_SLAB_ROWS = 29
assert len(SLAB_ROWS) == NXS_SLAB_ROWS
SLAB_BRANCHES = ("supercooled", "n2_hi_old", "n2_newice", "n3_h0", "n4_young", "n4_not_filled", "n4_sharp", "n4_no_room", "melt", "melt_side", "day_freeze", "day_melt",
                 "conc_ge_cmin", "del_c_neg", "limit", "ridge", "heal_ice", "pond_flushed", "lid_exists", "lid_forms", "lid_removed", "no_ice_tracers", "reset", "old_melt",
                 "assim", "denom_clamp", "sss_below_si", "freeze_days_ge")   # NXS_SLAB_BR_*: bit k of the word of debug array "slab_branches"


SLAB_FSD_BRANCHES = ("melt3", "unbroken", "ctot_break", "limit_rescaled", "limit_mech_rescaled", "limit_zeroed", "lateral", "lat_melting", "fills_lead",
                     "del_c_fsd_ge0", "young_shrinks", "welded", "healed")   # NXS_SLAB_FSD_BR_*: bit k of the word of debug array "slab_fsd_branches"


class SlabCoupledInfo(C.Structure):   # nxs_dyn_slab_coupled_info
    _fields_ = [("thermo_fsd_crash", C.c_int32)]


class SlabConfig(C.Structure):   # nxs_dyn_slab_config
    _fields_ = [(k, C.c_int32) for k in SLAB_CONFIG_INTS] + [(k, C.c_double) for k in SLAB_CONFIG_REALS]


class SlabState(C.Structure):   # nxs_dyn_slab_state
    _fields_ = [(k, c_double_p) for k in SLAB_STATE_GET]


class SlabClock(C.Structure):   # nxs_dyn_slab_clock
    _fields_ = [(k, C.c_int32) for k in SLAB_CLOCK]


class SlabRows(C.Structure):   # nxs_dyn_slab_rows
    _fields_ = [("row", c_double_p * NXS_SLAB_ROWS)]


def slab_config_struct(base: "SlabConfig", **options) -> SlabConfig:
    """A copy of `base` (the defaults of nxs_slab_default_config) with keyword options named after nxs_dyn_slab_config's members."""
    c = SlabConfig()
    C.memmove(C.byref(c), C.byref(base), C.sizeof(c))
    for k, v in options.items():
        if k not in SLAB_CONFIG_INTS + SLAB_CONFIG_REALS:
            raise KeyError(f"nxs_dyn_slab_config has no member {k!r}")
        setattr(c, k, int(v) if k in SLAB_CONFIG_INTS else float(v))
    return c


# nxs_dyn_regrid (include/nxs_dyn.h): ModelVariable::interpTransformation and the flags of nxs_dyn_regrid_var
NXS_TRANSFORM_NONE, NXS_TRANSFORM_CONC, NXS_TRANSFORM_THICK, NXS_TRANSFORM_ENTHALPY = range(4)
TRANSFORMATIONS = {"none": NXS_TRANSFORM_NONE, "conc": NXS_TRANSFORM_CONC, "thick": NXS_TRANSFORM_THICK, "enthalpy": NXS_TRANSFORM_ENTHALPY}
NXS_REGRID_VAR_HAS_MIN, NXS_REGRID_VAR_HAS_MAX, NXS_REGRID_VAR_IS_TICE, NXS_REGRID_VAR_OLD_ON_DEVICE, NXS_REGRID_VAR_NEW_ON_DEVICE = 1, 2, 4, 8, 16


class RegridVar(C.Structure):   # nxs_dyn_regrid_var
    _fields_ = [("old_values", C.c_void_p), ("new_values", C.c_void_p), ("transformation", C.c_int32), ("flags", C.c_int32),
                ("min_val", C.c_double), ("max_val", C.c_double)]


class RegridArgs(C.Structure):   # nxs_dyn_regrid_args
    _fields_ = [("new_mesh", C.POINTER(Mesh)), ("context", C.c_void_p), ("x_old_moved", c_double_p), ("y_old_moved", c_double_p),
                ("previous_numbering", c_double_p), ("n_geom_vertices", C.c_int32), ("num_extra", C.c_int32), ("extra", C.POINTER(RegridVar)),
                ("freezingpoint_mu", C.c_double), ("cohesion", c_double_p), ("time_relaxation_damage", c_double_p), ("drag_ui", c_double_p),
                ("drag_ui_young", c_double_p)]


class RegridInfo(C.Structure):   # nxs_dyn_regrid_info
    _fields_ = [("num_failed", C.c_int32), ("num_exterior", C.c_int32), ("nb_var_element", C.c_int32), ("reserved0", C.c_int32),
                ("collect_ms", C.c_double), ("remap_ms", C.c_double), ("redistribute_ms", C.c_double), ("nodes_ms", C.c_double),
                ("set_mesh_ms", C.c_double), ("total_ms", C.c_double)]


class RegridThermo(C.Structure):   # nxs_dyn_regrid_thermo
    _fields_ = [("carry", C.c_int32), ("reserved", C.c_int32), ("drag_ice_t", C.c_double)]


class RegridThermoInfo(C.Structure):   # nxs_dyn_regrid_thermo_info
    _fields_ = [("flux_carried", C.c_uint32), ("col_carried", C.c_uint32), ("slab_carried", C.c_uint32), ("flux_remade", C.c_uint32),
                ("nb_var_element", C.c_int32), ("tiled", C.c_int32)]


# nxs_dyn_regrid_carry_thermo: the thermodynamic rows as columns of nxs_dyn_regrid, in column order within each kind -- (name, interpTransformation, minVal,
# maxVal, is M_tice) of model/model_variable.cpp (the lines: thermo_carry[] of csrc/nxs_dyn.hip); None = no bound ...
REGRID_THERMO_COLUMNS = (
    ("tice0", "none", None, None, True), ("tsurf_young", "none", None, None, False), ("sst", "none", None, None, False), ("sss", "none", None, None, False),
    ("lid_volume", "none", None, None, False),
    ("conc_upd", "none", -1., 1., False), ("pond_volume", "none", None, None, False), ("del_vi_tend", "none", None, None, False),
    ("freeze_days", "none", 0., None, False), ("freeze_onset", "none", 0., 1., False), ("conc_summer", "none", 0., 1., False),
    ("thick_summer", "none", 0., None, False), ("fyi_fraction", "none", 0., 1., False), ("age_det", "none", 0., None, False), ("age", "none", 0., None, False),
    ("tice2", "thick", None, None, True),
    ("tice1", "enthalpy", None, None, True),
)
# ... and the rows of nxs_dyn_flux_state the reference re-makes instead (FE.cpp:566-571, 3012-3015)
REGRID_THERMO_REMADE = ("drag_ti", "drag_ti_young", "pond_fraction")


# enum nxs_means_var: the Moorings variables nxs_dyn_means_* accumulates, named after GridOutput::variableID
MEANS_ELEMENTAL = ("conc", "thick", "snow", "conc_cons", "damage", "ridge_ratio", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi",
                   "dci_ridge_myi", "sigma_11", "sigma_22", "sigma_12", "sigma_n", "sigma_s", "divergence", "drag_ui", "ice_mask")
MEANS_NODAL = ("VT_x", "VT_y", "wind_x", "wind_y", "tau_ax", "tau_ay", "tauwix", "tauwiy", "taux", "tauy", "taumod")
# the thermodynamic variables, a second elemental range: the rows nxs_dyn_fluxes / nxs_dyn_column / nxs_dyn_slab keep on the handle (C names: upper case)
MEANS_THERMO = ("sst", "sss", "tsurf_ice", "meltpond_lid_volume", "meltpond_fraction", "drag_ti", "t1", "t2",
                "conc_upd", "meltpond_volume", "del_vi_tend", "freeze_days", "freeze_onset", "conc_summer", "thick_summer", "fyi_fraction", "age_det", "age",
                "Qa", "Qsw", "Qlw", "Qsh", "Qlh", "Qo", "delS", "evap", "rain", "sialb", "albedo",
                "del_vi_young", "vice_melt", "del_hi", "del_hi_young", "newice", "snow2ice", "mlt_top", "mlt_bot",
                "dvi_rplnt_myi", "dci_rplnt_myi", "dvi_mlt_myi", "dci_mlt_myi", "fwflux_ice", "fwflux", "QNoSw", "QSwOcean", "saltflux",
                "tair", "mslp", "Qsw_in", "sphuma", "mixrat", "d2m", "Qlw_in", "tcc", "precip", "snowfall", "snowfr", "ocean_temp", "ocean_salt", "mld",
                "tsurf", "wspeed")
NXS_MEANS_NODAL_BEGIN = 64
NXS_MEANS_THERMO_BEGIN = 128
NXS_MEANS_MAX_VARS = 24
MEANS_ID = {k: i for i, k in enumerate(MEANS_ELEMENTAL)}
MEANS_ID.update({k: NXS_MEANS_NODAL_BEGIN + i for i, k in enumerate(MEANS_NODAL)})
MEANS_ID.update({k: NXS_MEANS_THERMO_BEGIN + i for i, k in enumerate(MEANS_THERMO)})
# the floe-size diagnostics of the coupled build (D_dmax, D_dmean: nxs_dyn_fsd_diag_configure), a third elemental range with names of its own
MEANS_FSD = ("dmax", "dmean")
NXS_MEANS_FSD_BEGIN = 192
NXS_MEANS_FSD_END = 194
MEANS_FSD_ID = {k: NXS_MEANS_FSD_BEGIN + i for i, k in enumerate(MEANS_FSD)}
NXS_CPL_OUT_RESET = 1   # nxs_dyn_cpl_out_put: resetMeshMean + resetGridMean behind the copies


class MeansConfig(C.Structure):   # nxs_dyn_means_config
    _fields_ = [("num_elemental", C.c_int32), ("num_nodal", C.c_int32), ("elemental_ids", c_int32_p), ("elemental_mask", c_uint8_p),
                ("nodal_ids", c_int32_p), ("nodal_mask", c_uint8_p)]


class MeansGrid(C.Structure):   # nxs_dyn_means_grid
    _fields_ = [("xmin", C.c_double), ("ymax", C.c_double), ("mooring_spacing", C.c_double), ("miss_val", C.c_double),
                ("ncols", C.c_int32), ("nrows", C.c_int32)]


NXS_MEANS_ROTATE_NONE, NXS_MEANS_ROTATE_NORTH_EAST, NXS_MEANS_ROTATE_GRID_THETA = range(3)   # enum nxs_means_rotation
MEANS_ROTATION = {"none": NXS_MEANS_ROTATE_NONE, "north_east": NXS_MEANS_ROTATE_NORTH_EAST, "grid_theta": NXS_MEANS_ROTATE_GRID_THETA}
NXS_MEANS_MAX_PAIRS = NXS_MEANS_MAX_VARS // 2


class MeansPoints(C.Structure):   # nxs_dyn_means_points
    _fields_ = [("G", C.c_int32), ("rotation", C.c_int32), ("gridX", c_double_p), ("gridY", c_double_p), ("gridLON", c_double_p), ("gridTheta", c_double_p),
                ("rotation_angle", C.c_double), ("miss_val", C.c_double), ("n_pairs", C.c_int32), ("pair_first", C.c_int32 * NXS_MEANS_MAX_PAIRS),
                ("pair_second", C.c_int32 * NXS_MEANS_MAX_PAIRS)]


class MeansRegular(C.Structure):   # nxs_dyn_means_regular
    _fields_ = [("ncols", C.c_int32), ("nrows", C.c_int32), ("xmin", C.c_double), ("ymax", C.c_double), ("mooring_spacing", C.c_double), ("miss_val", C.c_double),
                ("rotation", C.c_int32), ("gridLON", c_double_p), ("rotation_angle", C.c_double), ("n_pairs", C.c_int32),
                ("pair_first", C.c_int32 * NXS_MEANS_MAX_PAIRS), ("pair_second", C.c_int32 * NXS_MEANS_MAX_PAIRS)]


NXS_DRIFTER_SETS = 8   # include/nxs_dyn.h: drifter sets per handle (nxs_dyn_drifters_*)

ICE_DIAG = ("D_conc", "D_thick", "D_snow_thick", "D_sigma0", "D_sigma1", "D_divergence")


class IceDiag(C.Structure):
    _fields_ = [(k, c_double_p) for k in ICE_DIAG]


class Timing(C.Structure):
    _fields_ = [("prep_ms", C.c_double), ("substeps_ms", C.c_double), ("smoother_ms", C.c_double),
                ("update_ms", C.c_double), ("total_ms", C.c_double),
                ("substep_launches", C.c_int32), ("steps_averaged", C.c_int32), ("ring_flush_ms", C.c_double)]


class Traffic(C.Structure):   # nxs_dyn_traffic
    _fields_ = [("substep_kernel", C.c_int32), ("substeps_per_launch", C.c_int32), ("halo_in_kernel", C.c_int32), ("prep_kernel", C.c_int32),
                ("substep_scheme_bytes", C.c_double), ("substep_reread_bytes", C.c_double), ("substep_unique_bytes", C.c_double),
                ("survey_model_bytes", C.c_double), ("move_ring_slots", C.c_int32), ("reserved0", C.c_int32), ("move_ring_bytes", C.c_double),
                ("prep_scheme_bytes", C.c_double), ("prep_unique_bytes", C.c_double), ("update_bytes", C.c_double)]


# ---- numpy helpers --------------------------------------------------------------------------

def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags.c_contiguous, (a.dtype, a.flags)
    return a.ctypes.data_as(c_double_p)


def iptr(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(c_int32_p)


def bptr(a: np.ndarray):
    assert a.dtype == np.uint8 and a.flags.c_contiguous
    return a.ctypes.data_as(c_uint8_p)


# names of the nodal / elemental members of State, in ABI order
STATE_NODAL = ("VT", "UM", "UT")
STATE_ELEMENT = ("conc", "thick", "snow_thick", "damage", "ridge_ratio", "sigma0", "sigma1", "sigma2",
                 "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi")
STATE_INPUT = ("cohesion", "time_relaxation_damage", "drag_ui", "drag_ui_young")


def state_struct(arrays: dict) -> State:
    """Build a State struct pointing at the numpy arrays in `arrays` (which must stay alive)."""
    s = State()
    for k in STATE_NODAL + STATE_INPUT:
        setattr(s, k, dptr(arrays[k]))
    for k in STATE_ELEMENT:
        if k.startswith("sigma"):
            s.sigma[int(k[-1])] = dptr(arrays[k])
        else:
            setattr(s, k, dptr(arrays[k]))
    return s


def forcing_struct(arrays: dict) -> Forcing:
    f = Forcing()
    for k in ("wind", "ocean", "ssh", "element_depth"):
        setattr(f, k, dptr(arrays[k]))
    return f


def mesh_struct(lm, tables=None) -> Mesh:
    """lm: a nextsim_amd.mesh.LocalMesh; tables: optional (nec, nc) bamg-layout double tables."""
    m = Mesh()
    m.num_nodes = lm.num_nodes
    m.num_elements = lm.num_elements
    m.local_ndof = lm.local_ndof
    m.local_nelements = lm.local_nelements
    m.indices = iptr(lm.indices)
    m.ghost_nodes = bptr(lm.ghost_nodes)
    m.coord_x = dptr(lm.coord_x)
    m.coord_y = dptr(lm.coord_y)
    m.lat = dptr(lm.lat)
    m.mask_dirichlet = bptr(lm.mask_dirichlet)
    m.num_neumann_flags = int(lm.neumann_flags.size)
    m.neumann_flags = iptr(lm.neumann_flags)
    if tables is not None:
        nec, nc = tables
        m.nodal_element_connectivity = dptr(nec)
        m.nodal_connectivity = dptr(nc)
        m.nec_width = nec.shape[1]
        m.nc_width = nc.shape[1]
    return m


def halo_struct(lm) -> Halo:
    h = Halo()
    h.rank, h.nranks = lm.rank, lm.nranks
    h.num_send_procs = int(lm.send_procs.size)
    h.num_recv_procs = int(lm.recv_procs.size)
    h.send_procs = iptr(lm.send_procs)
    h.send_offsets = iptr(lm.send_offsets)
    h.send_index = iptr(lm.send_index)
    h.recv_procs = iptr(lm.recv_procs)
    h.recv_offsets = iptr(lm.recv_offsets)
    h.recv_index = iptr(lm.recv_index)
    return h


def repo_root() -> str:
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
