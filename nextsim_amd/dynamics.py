"""Host-side mirror of the reference's call surface for the dynamics path, over the C ABI.

`FiniteElementDynamics` keeps the names of FiniteElement's methods on this path
(model/finiteelement.hpp:162-164 and FE.cpp:8197-8214): `explicitSolve()`, `update()`, `step()`,
`checkRegridding()`, `checkFieldsFast()`, `updateGhosts` happens inside.  Every call goes through
libnxsdyn.so (include/nxs_dyn.h); there is no Python or CPU compute path here, and a missing
library or GPU is an error, never a fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

from . import _abi

_LIB = None
# NXS_DYN_LIBRARY: another build of the same library (kernel experiments); never a different implementation
_LIB_PATH = os.environ.get("NXS_DYN_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libnxsdyn.so")


class NxsError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{_abi.ERRORS.get(code, code)}: {what}")
        self.code = code


def build_library(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of nextsim_amd/csrc (cross-compiles without a GPU)."""
    src_dir = os.path.dirname(_LIB_PATH)
    args = ["make", "-s", "-C", src_dir]
    if force:
        args.insert(1, "-B")
    subprocess.check_call(args)
    return _LIB_PATH


def load_library():
    """dlopen libnxsdyn.so and declare every symbol of include/nxs_dyn.h.  Raises if absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise NxsError(-2, f"{_LIB_PATH} is missing: build it with __graft_entry__.build() "
                           "(there is no CPU fallback for the dynamics path)")
    L = C.CDLL(_LIB_PATH)
    P = C.POINTER
    H = C.c_void_p
    L.nxs_dyn_abi_version.restype = C.c_int
    L.nxs_dyn_last_error.restype = C.c_char_p
    L.nxs_dyn_last_error.argtypes = [H]
    L.nxs_dyn_default_params.argtypes = [P(_abi.Params)]
    L.nxs_dyn_create.argtypes = [P(_abi.Params), C.c_int, P(H)]
    L.nxs_dyn_destroy.argtypes = [H]
    L.nxs_dyn_set_params.argtypes = [H, P(_abi.Params)]
    L.nxs_dyn_set_mesh.argtypes = [H, P(_abi.Mesh)]
    L.nxs_dyn_set_halo.argtypes = [H, P(_abi.Halo)]
    L.nxs_dyn_comm_unique_id.argtypes = [C.c_void_p]
    L.nxs_dyn_comm_init.argtypes = [H, C.c_void_p, C.c_int, C.c_int]
    L.nxs_dyn_comm_selftest.argtypes = [H, P(C.c_int32)]
    L.nxs_dyn_set_halo_exchange_fn.argtypes = [H, HALO_FN, C.c_void_p]
    L.nxs_dyn_ipc_export.argtypes = [H, C.c_void_p]
    L.nxs_dyn_ipc_connect.argtypes = [H, C.c_void_p, _abi.c_int32_p, _abi.c_int32_p, _abi.c_int32_p]
    L.nxs_dyn_ipc_selftest.argtypes = [H, C.c_int, P(C.c_int32)]
    L.nxs_dyn_ipc_record_bytes.argtypes = [H, P(C.c_int32)]
    L.nxs_dyn_ipc_export_record.argtypes = [H, C.c_void_p, C.c_int32]
    L.nxs_dyn_ipc_connect_records.argtypes = [H, C.c_void_p, C.c_int64, C.c_int32]
    L.nxs_dyn_ipc_loopback.argtypes = [H]
    L.nxs_dyn_put_state.argtypes = [H, P(_abi.State)]
    L.nxs_dyn_get_state.argtypes = [H, P(_abi.State)]
    L.nxs_dyn_set_forcing.argtypes = [H, P(_abi.Forcing)]
    L.nxs_dyn_get_diag.argtypes = [H, P(_abi.Diag)]
    L.nxs_dyn_set_wave_stress.argtypes = [H, _abi.c_double_p]
    L.nxs_dyn_put_coupled.argtypes = [H, P(_abi.Coupled)]
    L.nxs_dyn_get_coupled.argtypes = [H, P(_abi.Coupled)]
    L.nxs_fsd_bins.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, P(_abi.FsdTables)]
    L.nxs_fsd_config_check.argtypes = [P(_abi.FsdConfig), C.c_int32]
    L.nxs_dyn_fsd_configure.argtypes = [H, P(_abi.FsdConfig)]
    L.nxs_dyn_fsd_put.argtypes = [H, P(_abi.FsdState)]
    L.nxs_dyn_fsd_get.argtypes = [H, P(_abi.FsdState)]
    L.nxs_dyn_fsd_init.argtypes = [H]
    L.nxs_dyn_fsd_update.argtypes = [H]
    L.nxs_dyn_fsd_breakup.argtypes = [H, C.c_void_p, C.c_int32, P(C.c_int32), P(C.c_int32)]
    L.nxs_dyn_fsd_weld.argtypes = [H, C.c_double, _abi.c_uint8_p]
    L.nxs_flux_default_config.argtypes = [P(_abi.FluxConfig)]
    L.nxs_flux_config_check.argtypes = [P(_abi.FluxConfig)]
    L.nxs_flux_constants.argtypes = [P(C.c_double), C.c_int32]
    L.nxs_dyn_flux_configure.argtypes = [H, P(_abi.FluxConfig)]
    L.nxs_dyn_flux_set_atmosphere.argtypes = [H, P(_abi.FluxAtmosphere)]
    L.nxs_dyn_flux_put.argtypes = [H, P(_abi.FluxState)]
    L.nxs_dyn_flux_get.argtypes = [H, P(_abi.FluxState)]
    L.nxs_dyn_fluxes.argtypes = [H]
    L.nxs_dyn_fluxes_get.argtypes = [H, P(_abi.FluxRows), P(C.c_void_p)]
    L.nxs_col_default_config.argtypes = [P(_abi.ColumnConfig)]
    L.nxs_col_config_check.argtypes = [P(_abi.ColumnConfig)]
    L.nxs_col_constants.argtypes = [P(C.c_double), C.c_int32]
    L.nxs_dyn_column_configure.argtypes = [H, P(_abi.ColumnConfig)]
    L.nxs_dyn_column_set_forcing.argtypes = [H, P(_abi.ColumnForcing)]
    L.nxs_dyn_column_put.argtypes = [H, P(_abi.ColumnState)]
    L.nxs_dyn_column_get_state.argtypes = [H, P(_abi.ColumnState)]
    L.nxs_dyn_column.argtypes = [H, C.c_int32]
    L.nxs_dyn_column_get.argtypes = [H, P(_abi.ColumnRows), P(C.c_void_p)]
    L.nxs_dyn_thermo_forcing_pair.argtypes = [H, P(_abi.ThermoForcingRows), P(_abi.ThermoForcingRows)]
    L.nxs_dyn_thermo_forcing_time.argtypes = [H, P(_abi.ThermoForcingTime)]
    L.nxs_dyn_thermo_forcing_targets.argtypes = [H, C.c_int32, _abi.c_double_p, _abi.c_double_p]
    L.nxs_dyn_thermo_forcing_ingest.argtypes = [H, C.c_int32, P(_abi.ForcingGrid), _abi.c_double_p, C.c_int32, _abi.c_int32_p, _abi.c_int32_p]
    L.nxs_dyn_thermo_forcing_get.argtypes = [H, C.c_int32, P(_abi.ThermoForcingRows)]
    L.nxs_mapx_constants.argtypes = [P(C.c_double), C.c_int32]
    L.nxs_mapx_polar_north.argtypes = [C.c_double] * 9 + [P(_abi.MapxPolar)]
    L.nxs_mapx_forward.argtypes = [P(_abi.MapxPolar), C.c_int64, _abi.c_double_p, _abi.c_double_p, _abi.c_double_p, _abi.c_double_p, C.c_int32]
    L.nxs_dyn_forcing_targets.argtypes = [H, C.c_int32, _abi.c_double_p, _abi.c_double_p]
    L.nxs_dyn_forcing_ingest.argtypes = [H, C.c_int32, P(_abi.ForcingGrid), C.c_int32, C.c_int32, _abi.c_double_p, C.c_int32, _abi.c_int32_p, _abi.c_int32_p, P(_abi.ForcingVectors)]
    L.nxs_dyn_set_forcing_time_rows.argtypes = [H, P(_abi.ForcingTimeRows)]
    L.nxs_dyn_set_element_depth.argtypes = [H, _abi.c_double_p]
    L.nxs_dyn_forcing_get.argtypes = [H, C.c_int32, P(_abi.ForcingRows)]
    L.nxs_nesting_config_check.argtypes = [P(_abi.NestingConfig)]
    L.nxs_dyn_nesting_configure.argtypes = [H, P(_abi.NestingConfig)]
    L.nxs_dyn_nesting_pair.argtypes = [H, P(_abi.NestingRows), P(_abi.NestingRows)]
    L.nxs_dyn_nesting_time.argtypes = [H, P(_abi.NestingTime)]
    L.nxs_dyn_nesting_ice.argtypes = [H]
    L.nxs_dyn_nesting_dynamics.argtypes = [H]
    L.nxs_dyn_nesting_get.argtypes = [H, C.c_int32, P(_abi.NestingRows)]
    L.nxs_dyn_diffusion_configure.argtypes = [H, C.c_double, C.c_double, C.c_double, C.c_double]
    L.nxs_dyn_diffuse.argtypes = [H]
    L.nxs_dyn_flux_device_rows.argtypes = [H, P(C.c_void_p)]
    L.nxs_ocean_coupled_default_config.argtypes = [P(_abi.OceanCoupledConfig)]
    L.nxs_ocean_coupled_config_check.argtypes = [P(_abi.OceanCoupledConfig)]
    L.nxs_dyn_ocean_coupled_attach.argtypes = [H, C.c_void_p, P(_abi.OceanCoupledConfig)]
    L.nxs_dyn_ocean_coupled_receive.argtypes = [H, P(C.c_void_p), C.c_int32]
    L.nxs_dyn_ocean_coupled_put_rows.argtypes = [H, P(_abi.OceanCoupledRows)]
    L.nxs_dyn_ocean_coupled_get.argtypes = [H, P(_abi.OceanCoupledRows), P(C.c_void_p)]
    L.nxs_nodes_coupled_default_config.argtypes = [P(_abi.NodesCoupledConfig)]
    L.nxs_dyn_nodes_coupled_attach.argtypes = [H, C.c_int32, C.c_void_p, P(_abi.NodesCoupledConfig)]
    L.nxs_dyn_nodes_coupled_receive.argtypes = [H, C.c_int32, P(C.c_void_p), C.c_int32, C.c_int32]
    L.nxs_dyn_nodes_coupled_get.argtypes = [H, C.c_int32, P(C.c_void_p), P(C.c_void_p)]
    for _n in ("nxs_dyn_forcing_attach_mesh", "nxs_dyn_thermo_forcing_attach_mesh"):
        getattr(L, _n).argtypes = [H, C.c_int32, C.c_void_p]
    for _n in ("nxs_dyn_forcing_ingest_mesh", "nxs_dyn_thermo_forcing_ingest_mesh"):
        getattr(L, _n).argtypes = [H, C.c_int32, P(_abi.NodemapLoad), P(C.c_int32), C.c_int32]
    L.nxs_slab_default_config.argtypes = [P(_abi.SlabConfig)]
    L.nxs_slab_config_check.argtypes = [P(_abi.SlabConfig)]
    L.nxs_slab_constants.argtypes = [P(C.c_double), C.c_int32]
    L.nxs_dyn_slab_configure.argtypes = [H, P(_abi.SlabConfig)]
    L.nxs_dyn_slab_put.argtypes = [H, P(_abi.SlabState)]
    L.nxs_dyn_slab_get_state.argtypes = [H, P(_abi.SlabState)]
    L.nxs_dyn_slab.argtypes = [H, C.c_int32, P(_abi.SlabClock)]
    L.nxs_dyn_slab_get.argtypes = [H, P(_abi.SlabRows), P(C.c_void_p)]
    L.nxs_slab_coupled_config_check.argtypes = [P(_abi.SlabConfig), C.c_int32, C.c_int32]
    L.nxs_dyn_slab_coupled_configure.argtypes = [H, C.c_int32]
    L.nxs_dyn_slab_coupled.argtypes = [H, C.c_int32, P(_abi.SlabClock)]
    L.nxs_dyn_slab_coupled_info.argtypes = [H, P(_abi.SlabCoupledInfo)]
    L.nxs_dyn_ice_diagnostics.argtypes = [H, P(_abi.IceDiag), P(C.c_void_p)]
    L.nxs_dyn_means_configure.argtypes = [H, P(_abi.MeansConfig)]
    L.nxs_dyn_means_set_tau_ow.argtypes = [H, _abi.c_double_p]
    L.nxs_dyn_means_update.argtypes = [H, C.c_double]
    L.nxs_dyn_means_get.argtypes = [H, _abi.c_double_p, _abi.c_double_p, P(C.c_void_p), P(C.c_void_p)]
    L.nxs_dyn_means_to_grid.argtypes = [H, P(_abi.MeansGrid), _abi.c_double_p, _abi.c_double_p]
    L.nxs_dyn_means_to_grid_conservative.argtypes = [H, C.c_void_p, C.c_double, _abi.c_double_p]
    L.nxs_dyn_means_reset.argtypes = [H]
    L.nxs_dyn_means_points_set.argtypes = [H, P(_abi.MeansPoints)]
    L.nxs_dyn_means_points_lsm.argtypes = [H, _abi.c_int32_p, _abi.c_int32_p]
    L.nxs_dyn_means_points_update.argtypes = [H]
    L.nxs_dyn_means_points_get.argtypes = [H, C.c_int32, _abi.c_double_p, _abi.c_double_p, P(C.c_void_p), P(C.c_void_p)]
    L.nxs_dyn_means_points_reset.argtypes = [H]
    L.nxs_dyn_means_regular_set.argtypes = [H, P(_abi.MeansRegular)]
    L.nxs_dyn_means_regular_lsm.argtypes = [H, _abi.c_int32_p, _abi.c_int32_p]
    L.nxs_dyn_means_regular_update.argtypes = [H]
    L.nxs_dyn_means_regular_get.argtypes = [H, C.c_int32, _abi.c_double_p, _abi.c_double_p, P(C.c_void_p), P(C.c_void_p)]
    L.nxs_dyn_means_regular_reset.argtypes = [H]
    L.nxs_dyn_cpl_out_configure.argtypes = [H, P(_abi.MeansConfig)]
    L.nxs_dyn_cpl_out_update.argtypes = [H, C.c_double]
    L.nxs_dyn_cpl_out_get.argtypes = [H, _abi.c_double_p, _abi.c_double_p, P(C.c_void_p), P(C.c_void_p)]
    L.nxs_dyn_cpl_out_reset.argtypes = [H]
    L.nxs_dyn_cpl_out_attach_grid.argtypes = [H, C.c_void_p, P(_abi.MeansPoints)]
    L.nxs_dyn_cpl_out_put.argtypes = [H, _abi.c_double_p, _abi.c_double_p, P(C.c_void_p), P(C.c_void_p), C.c_int32]
    L.nxs_dyn_cpl_out_reset_grid.argtypes = [H]
    L.nxs_dyn_fsd_diag_configure.argtypes = [H, C.c_double, C.c_double, C.c_double]
    L.nxs_dyn_drifters_set.argtypes = [H, C.c_int32, C.c_int32, _abi.c_double_p, _abi.c_double_p, _abi.c_int32_p]
    L.nxs_dyn_drifters_clear.argtypes = [H, C.c_int32]
    L.nxs_dyn_drifters_mesh_bbox.argtypes = [H, C.c_int32, _abi.c_double_p]
    L.nxs_dyn_drifters_move.argtypes = [H, _abi.c_double_p]
    L.nxs_dyn_drifters_conc.argtypes = [H, C.c_int32, _abi.c_double_p, _abi.c_double_p]
    L.nxs_dyn_drifters_mask.argtypes = [H, C.c_int32, C.c_double, _abi.c_int32_p, C.c_int32, P(C.c_int32)]
    L.nxs_dyn_drifters_get.argtypes = [H, C.c_int32, P(C.c_int32), _abi.c_double_p, _abi.c_double_p, _abi.c_int32_p, _abi.c_double_p, _abi.c_int32_p]
    L.nxs_dyn_regrid.argtypes = [H, P(_abi.RegridArgs), P(_abi.RegridInfo)]
    L.nxs_dyn_regrid_carry_thermo.argtypes = [H, P(_abi.RegridThermo)]
    L.nxs_dyn_regrid_thermo_info_get.argtypes = [H, P(_abi.RegridThermoInfo)]
    L.nxs_dyn_step.argtypes = [H]
    L.nxs_dyn_explicit_solve.argtypes = [H]
    L.nxs_dyn_update.argtypes = [H]
    L.nxs_dyn_synchronize.argtypes = [H]
    L.nxs_dyn_step_host.argtypes = [H, P(_abi.State), P(_abi.Forcing)]
    L.nxs_dyn_set_forcing_pair.argtypes = [H, P(_abi.Forcing), P(_abi.Forcing)]
    L.nxs_dyn_set_forcing_time.argtypes = [H, C.c_double, C.c_double, P(C.c_double), P(C.c_double)]
    L.nxs_dyn_check_regridding.argtypes = [H, P(C.c_double), P(C.c_int32), P(C.c_int32)]
    L.nxs_dyn_check_fields_fast.argtypes = [H, P(C.c_int32)]
    L.nxs_dyn_get_timing.argtypes = [H, P(_abi.Timing)]
    L.nxs_dyn_get_step_times.argtypes = [H, _abi.c_double_p, C.c_int32, P(C.c_int32)]
    L.nxs_dyn_get_traffic_model.argtypes = [H, P(_abi.Traffic)]
    L.nxs_dyn_physical_constants.argtypes = [P(C.c_double), C.c_int32]
    L.nxs_dyn_selftest_quotients.argtypes = [C.c_int32, C.c_int64, C.c_uint64, C.c_int32, P(C.c_int64)]
    L.nxs_dyn_set_option.argtypes = [H, C.c_char_p, C.c_int64]
    L.nxs_dyn_debug_array.argtypes = [H, C.c_char_p, _abi.c_double_p, C.c_int64]
    L.nxs_dyn_get_branch_trace.argtypes = [H, C.POINTER(C.c_uint64), C.c_int64]
    L.nxs_mesh_connectivity.argtypes = [_abi.c_int32_p, C.c_int32, C.c_int32, P(C.c_int32), _abi.c_double_p,
                                        P(C.c_int32), _abi.c_double_p]
    L.nxs_mesh_element_connectivity.argtypes = [_abi.c_int32_p, C.c_int32, C.c_int32, _abi.c_double_p]
    L.nxs_calc_cohesion.argtypes = [C.c_double, C.c_double, _abi.c_int32_p, C.c_int64, C.c_int64, _abi.c_double_p]
    for name in EXPORTS:
        getattr(L, name)  # raises AttributeError if a declared symbol is not exported
        if name not in ("nxs_dyn_last_error",):
            getattr(L, name).restype = C.c_int
    L.nxs_dyn_last_error.restype = C.c_char_p
    if L.nxs_dyn_abi_version() != 2:
        raise NxsError(-1, "libnxsdyn.so ABI version mismatch")
    _LIB = L
    return L


def mapx_constants() -> dict:
    """nxs_mapx_constants: mapx_Re_km and PI of contrib/mapx/include/mapx.h as the kernels hold them."""
    out = (C.c_double * 2)()
    rc = load_library().nxs_mapx_constants(out, 2)
    if rc:
        raise NxsError(rc, "nxs_mapx_constants")
    return {"Re_km": out[0], "PI": out[1]}


def mapx_polar_north(lat0=90., lon0=0., lat1=60., rotation=-45., scale=0.001, center_lat=90., center_lon=135., equatorial_radius=6378.273, eccentricity=0.081816153) -> "_abi.MapxPolar":
    """nxs_mapx_polar_north: the constants of forward_mapx from what an .mpp file holds (the defaults are the model's own map, rotation -45)."""
    L = load_library()
    m = _abi.MapxPolar()
    rc = L.nxs_mapx_polar_north(lat0, lon0, lat1, rotation, scale, center_lat, center_lon, equatorial_radius, eccentricity, C.byref(m))
    if rc:
        raise NxsError(rc, (L.nxs_dyn_last_error(None) or b"").decode())
    return m


def mapx_forward(m, lat, lon, device: int = -1):
    """nxs_mapx_forward: forward_mapx of every (lat, lon) in degrees; device < 0 runs the same source on the host."""
    L = load_library()
    lat, lon = np.ascontiguousarray(lat, np.float64).ravel(), np.ascontiguousarray(lon, np.float64).ravel()
    if lat.shape != lon.shape:
        raise ValueError("lat and lon differ in length")
    x, y = np.empty(lat.size), np.empty(lat.size)
    rc = L.nxs_mapx_forward(C.byref(m), lat.size, _abi.dptr(lat), _abi.dptr(lon), _abi.dptr(x), _abi.dptr(y), int(device))
    if rc:
        raise NxsError(rc, (L.nxs_dyn_last_error(None) or b"").decode())
    return x, y


def forcing_vectors(pairs=(), lat=None, lon=None, map=None, rotation_angle=0., per_point=False, is_wav_dir=(), gridded_rotation_angle=False):
    """nxs_dyn_forcing_vectors from pairs = [(column0, column1, east_west_oriented), ...]; cos / sin(-rotation_angle) are taken here, as transformData takes them.
    Returns the struct and what must outlive the call."""
    v = _abi.ForcingVectors()
    v.n_pairs = len(pairs)
    for k, (j0, j1, ew) in enumerate(pairs[:_abi.NXS_NF_MAX_VECTORS]):
        v.component0[k], v.component1[k], v.east_west_oriented[k] = int(j0), int(j1), int(bool(ew))
    for k in is_wav_dir:
        v.is_wav_dir[k] = 1
    v.gridded_rotation_angle, v.latlon_per_point, v.rotate = int(bool(gridded_rotation_angle)), int(bool(per_point)), int(rotation_angle != 0.)
    keep = [None if a is None else np.ascontiguousarray(a, np.float64).ravel() for a in (lat, lon)]
    if keep[0] is not None:
        v.lat = _abi.dptr(keep[0])
    if keep[1] is not None:
        v.lon = _abi.dptr(keep[1])
    if map is not None:
        v.map = map
    v.cos_m_diff_angle, v.sin_m_diff_angle = math.cos(-rotation_angle), math.sin(-rotation_angle)
    return v, keep


HALO_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _abi.c_double_p, _abi.c_double_p)

# every symbol include/nxs_dyn.h declares
IPC_BLOB_BYTES = 128

EXPORTS = (
    "nxs_dyn_set_halo_exchange_fn", "nxs_dyn_ipc_export", "nxs_dyn_ipc_connect", "nxs_dyn_ipc_selftest",
    "nxs_dyn_ipc_record_bytes", "nxs_dyn_ipc_export_record", "nxs_dyn_ipc_connect_records", "nxs_dyn_ipc_loopback",
    "nxs_dyn_abi_version", "nxs_dyn_last_error", "nxs_dyn_default_params", "nxs_dyn_physical_constants", "nxs_dyn_selftest_quotients", "nxs_dyn_create", "nxs_dyn_destroy",
    "nxs_dyn_set_params", "nxs_dyn_set_mesh", "nxs_dyn_set_halo", "nxs_dyn_comm_unique_id", "nxs_dyn_comm_init", "nxs_dyn_comm_selftest",
    "nxs_dyn_put_state", "nxs_dyn_get_state", "nxs_dyn_set_forcing", "nxs_dyn_set_forcing_pair", "nxs_dyn_set_forcing_time",
    "nxs_dyn_get_diag", "nxs_dyn_ice_diagnostics", "nxs_dyn_step",
    "nxs_dyn_set_wave_stress", "nxs_dyn_put_coupled", "nxs_dyn_get_coupled",
    "nxs_fsd_bins", "nxs_fsd_config_check", "nxs_dyn_fsd_configure", "nxs_dyn_fsd_put", "nxs_dyn_fsd_get", "nxs_dyn_fsd_init", "nxs_dyn_fsd_update", "nxs_dyn_fsd_breakup",
    "nxs_dyn_fsd_weld",
    "nxs_flux_default_config", "nxs_flux_config_check", "nxs_flux_constants", "nxs_dyn_flux_configure", "nxs_dyn_flux_set_atmosphere", "nxs_dyn_flux_put", "nxs_dyn_flux_get",
    "nxs_dyn_fluxes", "nxs_dyn_fluxes_get",
    "nxs_col_default_config", "nxs_col_config_check", "nxs_col_constants", "nxs_dyn_column_configure", "nxs_dyn_column_set_forcing", "nxs_dyn_column_put",
    "nxs_dyn_column_get_state", "nxs_dyn_column", "nxs_dyn_column_get",
    "nxs_dyn_thermo_forcing_pair", "nxs_dyn_thermo_forcing_time", "nxs_dyn_thermo_forcing_targets", "nxs_dyn_thermo_forcing_ingest", "nxs_dyn_thermo_forcing_get",
    "nxs_mapx_constants", "nxs_mapx_polar_north", "nxs_mapx_forward", "nxs_dyn_forcing_targets", "nxs_dyn_forcing_ingest", "nxs_dyn_set_forcing_time_rows", "nxs_dyn_set_element_depth",
    "nxs_dyn_forcing_get",
    "nxs_nesting_config_check", "nxs_dyn_nesting_configure", "nxs_dyn_nesting_pair", "nxs_dyn_nesting_time", "nxs_dyn_nesting_ice", "nxs_dyn_nesting_dynamics",
    "nxs_dyn_nesting_get", "nxs_dyn_diffusion_configure", "nxs_dyn_diffuse", "nxs_dyn_flux_device_rows",
    "nxs_ocean_coupled_default_config", "nxs_ocean_coupled_config_check", "nxs_dyn_ocean_coupled_attach", "nxs_dyn_ocean_coupled_receive", "nxs_dyn_ocean_coupled_put_rows",
    "nxs_dyn_ocean_coupled_get", "nxs_nodes_coupled_default_config", "nxs_dyn_nodes_coupled_attach", "nxs_dyn_nodes_coupled_receive", "nxs_dyn_nodes_coupled_get",
    "nxs_dyn_forcing_attach_mesh", "nxs_dyn_forcing_ingest_mesh", "nxs_dyn_thermo_forcing_attach_mesh", "nxs_dyn_thermo_forcing_ingest_mesh",
    "nxs_slab_default_config", "nxs_slab_config_check", "nxs_slab_constants", "nxs_dyn_slab_configure", "nxs_dyn_slab_put", "nxs_dyn_slab_get_state", "nxs_dyn_slab",
    "nxs_dyn_slab_get", "nxs_slab_coupled_config_check", "nxs_dyn_slab_coupled_configure", "nxs_dyn_slab_coupled", "nxs_dyn_slab_coupled_info",
    "nxs_dyn_means_configure", "nxs_dyn_means_set_tau_ow", "nxs_dyn_means_update", "nxs_dyn_means_get", "nxs_dyn_means_to_grid", "nxs_dyn_means_to_grid_conservative", "nxs_dyn_means_reset",
    "nxs_dyn_means_points_set", "nxs_dyn_means_points_lsm", "nxs_dyn_means_points_update", "nxs_dyn_means_points_get", "nxs_dyn_means_points_reset",
    "nxs_dyn_means_regular_set", "nxs_dyn_means_regular_lsm", "nxs_dyn_means_regular_update", "nxs_dyn_means_regular_get", "nxs_dyn_means_regular_reset",
    "nxs_dyn_cpl_out_configure", "nxs_dyn_cpl_out_update", "nxs_dyn_cpl_out_get", "nxs_dyn_cpl_out_reset", "nxs_dyn_cpl_out_attach_grid", "nxs_dyn_cpl_out_put",
    "nxs_dyn_cpl_out_reset_grid", "nxs_dyn_fsd_diag_configure",
    "nxs_dyn_drifters_set", "nxs_dyn_drifters_clear", "nxs_dyn_drifters_mesh_bbox", "nxs_dyn_drifters_move", "nxs_dyn_drifters_conc", "nxs_dyn_drifters_mask",
    "nxs_dyn_drifters_get", "nxs_dyn_regrid", "nxs_dyn_regrid_carry_thermo", "nxs_dyn_regrid_thermo_info_get",
    "nxs_dyn_explicit_solve", "nxs_dyn_update", "nxs_dyn_synchronize", "nxs_dyn_step_host",
    "nxs_dyn_check_regridding", "nxs_dyn_check_fields_fast", "nxs_dyn_get_timing", "nxs_dyn_get_step_times", "nxs_dyn_get_traffic_model", "nxs_dyn_set_option",
    "nxs_dyn_debug_array", "nxs_dyn_get_branch_trace", "nxs_mesh_connectivity", "nxs_mesh_element_connectivity", "nxs_calc_cohesion",
)
INTERP_EXPORTS = ("nxs_interp_mesh_to_mesh_2d", "nxs_interp_mesh_to_grid", "nxs_interp_mesh_to_grid_device", "nxs_interp_conservative_remap", "nxs_interp_grid_to_mesh",
                  "nxs_interp_last_error", "nxs_interp_last_info", "nxs_mesh_convex_completion", "nxs_mesh_convex_completion_mode", "nxs_regrid_create", "nxs_regrid_destroy",
                  "nxs_regrid_interp_nodes", "nxs_regrid_remap_elements", "nxs_interp_last_timing", "nxs_regrid_debug_tables", "nxs_gridmap_create", "nxs_gridmap_destroy",
                  "nxs_gridmap_info", "nxs_gridmap_mesh_to_grid", "nxs_gridmap_grid_to_mesh", "nxs_gridmap_export", "nxs_gridmap_import", "nxs_gridmap_restrict",
                  "nxs_gridmap_debug_chunk", "nxs_gridmap_receive_rows", "nxs_gridmap_debug_receive_lists", "nxs_gridmap_send_rows", "nxs_nodemap_create", "nxs_nodemap_destroy",
                  "nxs_nodemap_info", "nxs_nodemap_device", "nxs_nodemap_export", "nxs_nodemap_import", "nxs_nodemap_set_source", "nxs_nodemap_receive_rows", "nxs_nodemap_debug_source",
                  "nxs_nodemap_load_rows", "nxs_nodemap_debug_load")


def selftest_quotients(n: int, seed: int = 1, mode: int = 0, device: int = 0) -> int:
    """nxs_dyn_selftest_quotients: n sextuples of numerators over one divisor computed with the shared reciprocal and with six divisions on `device`;
    the number of quotients whose bits differ."""
    L = load_library()
    bad = C.c_int64(-1)
    rc = L.nxs_dyn_selftest_quotients(device, n, seed, mode, C.byref(bad))
    if rc != 0:
        raise NxsError(rc, (L.nxs_dyn_last_error(None) or b"").decode(errors="replace"))
    return bad.value


def mesh_connectivity(indices: np.ndarray, num_nodes: int):
    """(NodalElementConnectivity, NodalConnectivity) in bamg's layout and row order (host code of the
    product library; the stand-in for BamgConvertMeshx at FE.cpp:77-80)."""
    L = load_library()
    ne = indices.size // 3
    w1, w2 = C.c_int32(), C.c_int32()
    rc = L.nxs_mesh_connectivity(_abi.iptr(indices), num_nodes, ne, C.byref(w1), None, C.byref(w2), None)
    if rc:
        raise NxsError(rc, "nxs_mesh_connectivity")
    nec = np.empty((num_nodes, w1.value))
    nc = np.empty((num_nodes, w2.value))
    rc = L.nxs_mesh_connectivity(_abi.iptr(indices), num_nodes, ne, C.byref(w1), _abi.dptr(nec), C.byref(w2), _abi.dptr(nc))
    if rc:
        raise NxsError(rc, "nxs_mesh_connectivity")
    return nec, nc


def calc_cohesion(C_fix: float, C_alea: float, global_element_id: np.ndarray, num_global_elements: int) -> np.ndarray:
    """calcCohesion() (FE.cpp:3909-3914): C_fix + C_alea * (the reference's minstd/uniform_01 draw of each global element)."""
    L = load_library()
    ids = np.ascontiguousarray(global_element_id, np.int32)
    out = np.empty(ids.size)
    rc = L.nxs_calc_cohesion(float(C_fix), float(C_alea), _abi.iptr(ids), ids.size, int(num_global_elements), _abi.dptr(out))
    if rc:
        raise NxsError(rc, "nxs_calc_cohesion")
    return out


def mesh_element_connectivity(indices: np.ndarray, num_nodes: int) -> np.ndarray:
    """bamgmesh->ElementConnectivity ([Ne,3] doubles, 1-based, NaN on the boundary), bamg's column order."""
    L = load_library()
    indices = np.ascontiguousarray(indices, np.int32)
    ec = np.empty((indices.size // 3, 3))
    rc = L.nxs_mesh_element_connectivity(_abi.iptr(indices), num_nodes, indices.size // 3, _abi.dptr(ec))
    if rc:
        raise NxsError(rc, "nxs_mesh_element_connectivity")
    return ec


_HIP = None


def hip_runtime():
    """The HIP runtime libnxsdyn.so itself is linked against (one runtime in the process), with the few prototypes a caller needs to hand the library a plain
    device buffer (an `old_values` of nxs_dyn_regrid_var, the M_wlbk of nxs_dyn_fsd_breakup) without another GPU framework."""
    global _HIP
    if _HIP is None:
        import re
        load_library()
        out = subprocess.check_output(["readelf", "-d", _LIB_PATH], text=True)
        name = [n for n in re.findall(r"NEEDED.*\[(.*)\]", out) if "amdhip64" in n][0]
        hip = C.CDLL(name)
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipDeviceGetName.argtypes = [C.c_char_p, C.c_int, C.c_int]
        _HIP = hip
    return _HIP


def device_put(a: np.ndarray) -> int:
    """A new device buffer holding the C-contiguous array `a`; returns its address (free it with device_free)."""
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    if hip_runtime().hipMalloc(C.byref(p), a.nbytes) != 0 or hip_runtime().hipMemcpy(p, a.ctypes.data, a.nbytes, 1) != 0:
        raise NxsError(-3, "hipMalloc / hipMemcpy of a device buffer failed")
    return p.value


def device_free(address: int):
    hip_runtime().hipFree(C.c_void_p(int(address)))


def device_name(device: int = 0) -> str:
    """hipDeviceGetName of `device`."""
    buf = C.create_string_buffer(256)
    if hip_runtime().hipDeviceGetName(buf, 256, int(device)) != 0:
        raise NxsError(-3, "hipDeviceGetName failed")
    return buf.value.decode(errors="replace")


def fsd_bins(fsd_type, num_bins: int, min_floe_size: float, bin_cst_width: float, welding_use_scaled_area: bool = True) -> dict:
    """The tables of initFsd() (FE.cpp:7408-7533; nxs_fsd_bins, host only): bin_widths, bin_low_limits, bin_up_limits, bin_centres, area_scaled_up / _low /
    _centered / _binwidth ([num_bins] each) and alpha_merge ([num_bins, num_bins] int32, -999 where no bin matches).  fsd_type: "constant_size" / "constant_area"."""
    L = load_library()
    n = int(num_bins)
    if n < 1:
        raise NxsError(-1, f"fsd_bins: num_bins = {n}")
    out = {k: np.empty(n) for k in _abi.FSD_TABLES}
    out["alpha_merge"] = np.empty((n, n), np.int32)
    t = _abi.fsd_tables_struct(out)
    ft = _abi.FSD_TYPES[fsd_type] if isinstance(fsd_type, str) else int(fsd_type)
    rc = L.nxs_fsd_bins(ft, n, float(min_floe_size), float(bin_cst_width), int(bool(welding_use_scaled_area)), C.byref(t))
    if rc:
        raise NxsError(rc, "nxs_fsd_bins")
    return out


def flux_default_config() -> dict:
    """The thermo.* defaults of model/options.cpp:388-438 the bulk fluxes read (nxs_flux_default_config, host only), keyed like nxs_dyn_flux_config."""
    L = load_library()
    c = _abi.FluxConfig()
    rc = L.nxs_flux_default_config(C.byref(c))
    if rc:
        raise NxsError(rc, "nxs_flux_default_config")
    return {k: getattr(c, k) for k, _ in _abi.FluxConfig._fields_}


def _flux_config(options: dict) -> "_abi.FluxConfig":
    L = load_library()
    base = _abi.FluxConfig()
    L.nxs_flux_default_config(C.byref(base))
    return _abi.flux_config_struct(base, **options)


def flux_config_check(**options) -> int:
    """What flux_configure would answer for the defaults changed by `options` (nxs_flux_config_check, host only): 0 or NXS_ERR_INVALID."""
    c = _flux_config(options)
    return load_library().nxs_flux_config_check(C.byref(c))


def column_default_config() -> dict:
    """The defaults of model/options.cpp:112, 291-293, 383-420 the ice columns read (nxs_col_default_config, host only), keyed like nxs_dyn_column_config."""
    L = load_library()
    c = _abi.ColumnConfig()
    rc = L.nxs_col_default_config(C.byref(c))
    if rc != 0:
        raise NxsError(rc, "nxs_col_default_config")
    return {k: getattr(c, k) for k, _ in _abi.ColumnConfig._fields_ if k != "reserved"}


def _column_config(options: dict) -> "_abi.ColumnConfig":
    L = load_library()
    base = _abi.ColumnConfig()
    L.nxs_col_default_config(C.byref(base))
    return _abi.column_config_struct(base, **options)


def column_config_check(**options) -> int:
    """What column_configure would answer for the defaults changed by `options` (nxs_col_config_check, host only): 0 or NXS_ERR_INVALID."""
    c = _column_config(options)
    return load_library().nxs_col_config_check(C.byref(c))


def column_constants() -> dict:
    """The physical:: constants compiled into the column kernel (nxs_col_constants, host only)."""
    out = (C.c_double * len(_abi.COL_CONSTANTS))()
    rc = load_library().nxs_col_constants(out, len(_abi.COL_CONSTANTS))
    if rc != 0:
        raise NxsError(rc, "nxs_col_constants")
    return dict(zip(_abi.COL_CONSTANTS, out))


def slab_default_config() -> dict:
    """The defaults of model/options.cpp:329-331, 397-403, 428-449, 543-548 the slab loop reads (nxs_slab_default_config, host only), keyed like nxs_dyn_slab_config."""
    c = _abi.SlabConfig()
    rc = load_library().nxs_slab_default_config(C.byref(c))
    if rc != 0:
        raise NxsError(rc, "nxs_slab_default_config")
    return {k: getattr(c, k) for k, _ in _abi.SlabConfig._fields_}


def _slab_config(options: dict) -> "_abi.SlabConfig":
    base = _abi.SlabConfig()
    load_library().nxs_slab_default_config(C.byref(base))
    return _abi.slab_config_struct(base, **options)


def slab_config_check(**options) -> int:
    """What slab_configure would answer for the defaults changed by `options` (nxs_slab_config_check, host only): 0 or NXS_ERR_INVALID."""
    c = _slab_config(options)
    return load_library().nxs_slab_config_check(C.byref(c))


def _nesting_config(nudge_function="linear", nudge_timescale=86400., nudge_scale=1., nest_dynamic_vars=False, time_step=0, dtime_step=None) -> "_abi.NestingConfig":
    c = _abi.NestingConfig()
    c.nudge_function = _abi.NUDGE_FUNCTIONS[nudge_function] if isinstance(nudge_function, str) else int(nudge_function)
    c.nest_dynamic_vars, c.time_step = int(bool(nest_dynamic_vars)), int(time_step)
    c.nudge_timescale, c.nudge_scale = float(nudge_timescale), float(nudge_scale)
    c.dtime_step = float(time_step if dtime_step is None else dtime_step)
    return c


def nesting_config_check(**options):
    """What nesting_configure would answer for `options` (nxs_nesting_config_check, host only): (0 or NXS_ERR_INVALID, the message)."""
    L = load_library()
    rc = L.nxs_nesting_config_check(C.byref(_nesting_config(**options)))
    return rc, (L.nxs_dyn_last_error(None) or b"").decode() if rc else ""


def ocean_coupled_default_config() -> dict:
    """nxs_ocean_coupled_default_config: the rows of the reference's receive (coupler.rcv_first_layer_depth off, no wave model) and their coefficients."""
    c = _abi.OceanCoupledConfig()
    rc = load_library().nxs_ocean_coupled_default_config(C.byref(c))
    if rc:
        raise NxsError(rc, "nxs_ocean_coupled_default_config")
    n = c.n_fields
    return {"rows": tuple(_abi.OC_ROWS[c.row[k]] for k in range(n)), "a": list(c.a[:n]), "b": list(c.b[:n]), "factor": list(c.factor[:n]), "bias": list(c.bias[:n])}


def ocean_coupled_config_check(rows, **coef) -> int:
    """nxs_ocean_coupled_config_check: 0, or the status nxs_dyn_ocean_coupled_attach would return for this configuration (the text: nxs_dyn_last_error(NULL))."""
    c = _abi.ocean_coupled_config_struct(rows, **coef)
    return load_library().nxs_ocean_coupled_config_check(C.byref(c))


def slab_coupled_config_check(coupled_melt_type: int, attached_bins: int, **options) -> int:
    """What slab_coupled_configure(coupled_melt_type) would answer on a slab configured with the defaults changed by `options` (its own melt_type among them) and
    `attached_bins` floe-size bins attached (nxs_slab_coupled_config_check, host only): 0 or NXS_ERR_INVALID."""
    c = _slab_config(options)
    return load_library().nxs_slab_coupled_config_check(C.byref(c), int(coupled_melt_type), int(attached_bins))


def slab_constants() -> dict:
    """The constants compiled into the slab kernel (nxs_slab_constants, host only)."""
    out = (C.c_double * len(_abi.SLAB_CONSTANTS))()
    rc = load_library().nxs_slab_constants(out, len(_abi.SLAB_CONSTANTS))
    if rc != 0:
        raise NxsError(rc, "nxs_slab_constants")
    return dict(zip(_abi.SLAB_CONSTANTS, out))


def slab_clock(current_time: float, dt: float, reset_date: str = "0915") -> dict:
    """The five flags of nxs_dyn_slab_clock as thermo() derives them from M_current_time (FE.cpp:5653-5655, 5208, 5999, 6028, 6044).  current_time is a day number
    in the epoch of the reference's core/include/date.hpp (days since 1900-01-01, fractions are the time of day); dt is dtime_step in seconds."""
    import math
    days_in_sec = 86400.
    t = float(current_time)
    frac = math.fmod(t, 1.)
    num_steps_in_day = int(_c_round(days_in_sec / float(dt)))
    step_in_day = 1 + int(_c_round(num_steps_in_day * frac))
    import datetime
    day = datetime.date(1900, 1, 1) + datetime.timedelta(days=int(t))   # date.hpp:24-26, 89-92: getEpoch() + static_cast<long>(date_time) days
    md = f"{day.month:02d}{day.day:02d}"
    midnight = frac == 0.
    return {"first_step_of_day": int(step_in_day == 1), "last_step_of_day": int(step_in_day == num_steps_in_day), "fyi_reset_now": int(md == "0915" and midnight),
            "myi_reset_now": int(md == str(reset_date) and midnight), "onset_reset_now": int(md == "0801" and midnight)}


def _c_round(x: float) -> float:
    """std::round: halves away from zero"""
    import math
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def flux_constants() -> dict:
    """The physical:: constants compiled into the flux kernel (nxs_flux_constants, host only)."""
    out = (C.c_double * len(_abi.FLUX_CONSTANTS))()
    rc = load_library().nxs_flux_constants(out, len(_abi.FLUX_CONSTANTS))
    if rc:
        raise NxsError(rc, "nxs_flux_constants")
    return dict(zip(_abi.FLUX_CONSTANTS, out))


def fsd_config_check(num_bins: int, tables: dict, attached_bins: int, **options) -> int:
    """What fsd_configure would answer for this configuration on a handle whose conc_fsd has `attached_bins` bins (nxs_fsd_config_check, host only): 0 or
    NXS_ERR_INVALID (-1)."""
    L = load_library()
    c = _abi.fsd_config_struct(num_bins, tables, **options)
    return L.nxs_fsd_config_check(C.byref(c), int(attached_bins))


REGRID_INPUTS = ("cohesion", "time_relaxation_damage", "drag_ui", "drag_ui_young")
# FiniteElementDynamics.regrid_carry_thermo: the thermodynamic rows as columns of a regrid, (name, kind, min, max, is_tice) in column order within each kind, and the
# flux rows that are re-made instead
REGRID_THERMO_COLUMNS = _abi.REGRID_THERMO_COLUMNS
REGRID_THERMO_REMADE = _abi.REGRID_THERMO_REMADE


def regrid_args(lm_new, previous_numbering, n_geom_vertices, inputs, extras=(), context=None, moved=None, num_nodes_old=None, num_elements_old=None,
                freezingpoint_mu=0.055, validate=True):
    """nxs_dyn_regrid_args for FiniteElementDynamics.regrid, and everything it points to: (args, keep-alive list, extras' result arrays).  Pure host code: with
    `validate` the arguments nxs_dyn_regrid would refuse raise ValueError here, before any library call.
    extras: dicts {"old": [Ne_old] array or device address (int), "new": [Ne_new] array to fill, device address, or absent (one is made and put into the
    dict), "transformation": "none" | "conc" | "thick" | "enthalpy" (or NXS_TRANSFORM_*), "min": float or None, "max": float or None, "is_tice": bool}.
    context: an interp.Regrid of the old mesh at x0 + M_UM, or None with moved = (x, y) of those coordinates."""
    keep = []
    a = _abi.RegridArgs()
    Ne_new, Nn_new = lm_new.num_elements, lm_new.num_nodes

    def bad(what):
        if validate:
            raise ValueError("regrid: " + what)

    m = _abi.mesh_struct(lm_new)
    keep.append(m)
    a.new_mesh = C.pointer(m)
    for k in REGRID_INPUTS:
        v = None if inputs is None else inputs.get(k)
        if v is None:
            bad(f"inputs['{k}'] of the new mesh is required (re-made after a regrid, not interpolated)")
            continue
        v = np.ascontiguousarray(v, np.float64)
        if v.shape != (Ne_new,):
            raise ValueError(f"regrid: inputs['{k}'] has shape {v.shape}, expected ({Ne_new},)")
        keep.append(v)
        setattr(a, k, _abi.dptr(v))
    if context is not None:
        a.context = context.h if hasattr(context, "h") else C.c_void_p(int(context))
        keep.append(context)
    elif moved is not None:
        x, y = (np.ascontiguousarray(q, np.float64) for q in moved)
        if num_nodes_old is not None and (x.shape != (num_nodes_old,) or y.shape != (num_nodes_old,)):
            raise ValueError(f"regrid: moved coordinates have shapes {x.shape}, {y.shape}, expected ({num_nodes_old},)")
        keep += [x, y]
        a.x_old_moved, a.y_old_moved = _abi.dptr(x), _abi.dptr(y)
    else:
        bad("neither a context nor the moved coordinates of the old mesh")
    if previous_numbering is not None:
        pn = np.ascontiguousarray(previous_numbering, np.float64)
        if pn.shape != (Nn_new,):
            raise ValueError(f"regrid: previous_numbering has shape {pn.shape}, expected ({Nn_new},)")
        keep.append(pn)
        a.previous_numbering = _abi.dptr(pn)
    a.n_geom_vertices = int(n_geom_vertices)
    a.freezingpoint_mu = float(freezingpoint_mu)
    extras = list(extras) if not isinstance(extras, int) else extras
    if isinstance(extras, int):           # (a bare count: only to show that a negative one is refused)
        if extras < 0:
            bad(f"num_extra = {extras}")
        a.num_extra = extras
        return a, keep, []
    arr = (_abi.RegridVar * max(len(extras), 1))()
    keep.append(arr)
    results = []
    for k, x in enumerate(extras):
        v = arr[k]
        t = x.get("transformation", "none")
        t = _abi.TRANSFORMATIONS.get(t, t) if isinstance(t, str) else int(t)
        if not isinstance(t, int) or not (_abi.NXS_TRANSFORM_NONE <= t <= _abi.NXS_TRANSFORM_ENTHALPY):
            bad(f"extras[{k}] has the unknown transformation {x.get('transformation')!r}")
            t = t if isinstance(t, int) else -1
        v.transformation = t
        flags = 0
        old = x.get("old")
        if old is None:
            bad(f"extras[{k}] has no 'old' values")
        elif isinstance(old, (int, np.integer)):
            v.old_values = int(old); flags |= _abi.NXS_REGRID_VAR_OLD_ON_DEVICE
        else:
            old = np.ascontiguousarray(old, np.float64)
            if num_elements_old is not None and old.shape != (num_elements_old,):
                raise ValueError(f"regrid: extras[{k}]['old'] has shape {old.shape}, expected ({num_elements_old},)")
            keep.append(old)
            v.old_values = old.ctypes.data
        new = x.get("new")
        if isinstance(new, (int, np.integer)):
            v.new_values = int(new); flags |= _abi.NXS_REGRID_VAR_NEW_ON_DEVICE
            results.append(None)
        else:
            if new is None:
                new = x["new"] = np.empty(Ne_new)
            if not (isinstance(new, np.ndarray) and new.dtype == np.float64 and new.flags.c_contiguous and new.flags.writeable and new.shape == (Ne_new,)):
                raise ValueError(f"regrid: extras[{k}]['new'] must be a writeable C-contiguous float64 array of shape ({Ne_new},)")
            keep.append(new)
            v.new_values = new.ctypes.data
            results.append(new)
        if x.get("min") is not None:
            flags |= _abi.NXS_REGRID_VAR_HAS_MIN; v.min_val = float(x["min"])
        if x.get("max") is not None:
            flags |= _abi.NXS_REGRID_VAR_HAS_MAX; v.max_val = float(x["max"])
        if x.get("is_tice"):
            flags |= _abi.NXS_REGRID_VAR_IS_TICE
        v.flags = flags
    a.num_extra = len(extras)
    a.extra = arr
    return a, keep, results


class FiniteElementDynamics:
    """The dynamics part of FiniteElement on one GPU (one MPI-rank equivalent)."""

    def __init__(self, params: _abi.Params, device: int = 0):
        self.L = load_library()
        self.h = C.c_void_p()
        self.params = params.copy()
        rc = self.L.nxs_dyn_create(C.byref(self.params), device, C.byref(self.h))
        if rc:
            raise NxsError(rc, (self.L.nxs_dyn_last_error(None) or b"").decode())
        self.lm = None
        self._keep = []

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.nxs_dyn_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc:
            raise NxsError(rc, (self.L.nxs_dyn_last_error(self.h) or b"").decode())

    # ---- setup (distributedMeshProcessing / initUpdateGhosts) ----
    def set_params(self, params: _abi.Params):
        self.params = params.copy()
        self._chk(self.L.nxs_dyn_set_params(self.h, C.byref(self.params)))

    def set_mesh(self, lm, tables=None):
        m = _abi.mesh_struct(lm, tables)
        self._chk(self.L.nxs_dyn_set_mesh(self.h, C.byref(m)))
        self.lm = lm
        if lm.nranks > 1:
            hs = _abi.halo_struct(lm)
            self._chk(self.L.nxs_dyn_set_halo(self.h, C.byref(hs)))

    def comm_init(self, unique_id: bytes, rank: int, nranks: int):
        buf = C.create_string_buffer(unique_id, 128)
        self._chk(self.L.nxs_dyn_comm_init(self.h, buf, rank, nranks))

    def comm_selftest(self) -> int:
        """Coded payloads through the RCCL communicator (self send/recv + the halo segments); returns the number of wrong values."""
        err = C.c_int32(-1)
        self._chk(self.L.nxs_dyn_comm_selftest(self.h, C.byref(err)))
        return err.value

    def set_halo_exchange(self, fn):
        """fn(send: np.ndarray, recv: np.ndarray) -> None : host-staged updateGhosts through the caller's
        communicator (send/recv are views laid out per neighbour as [u-block | v-block])."""
        lm = self.lm
        ns, nr = 2 * int(lm.send_offsets[-1]), 2 * int(lm.recv_offsets[-1])

        def tramp(ctx, send, recv):
            try:
                sv = np.ctypeslib.as_array(send, shape=(max(ns, 1),))[:ns]
                rv = np.ctypeslib.as_array(recv, shape=(max(nr, 1),))[:nr]
                fn(sv, rv)
                return 0
            except Exception:  # noqa: BLE001 -- never unwind through the C ABI
                import traceback
                traceback.print_exc()
                return 1
        self._halo_cb = HALO_FN(tramp)
        self._chk(self.L.nxs_dyn_set_halo_exchange_fn(self.h, self._halo_cb, None))

    def ipc_setup(self, all_gather, selftest_rounds: int = 64, low_level: bool = False) -> bool:
        """Collective setup of the device-direct halo transport (peer-mapped mailboxes).
        all_gather(obj) -> list of every rank's obj (the launcher's communicator, e.g.
        torch.distributed.all_gather_object).  Returns True when the transport is connected and its
        self-test passed on EVERY rank; otherwise the handle is left on its previous transport.
        Default: the record form (nxs_dyn_ipc_export_record / nxs_dyn_ipc_connect_records) -- the library finds every neighbour's segment, totals and
        flag slot itself, also for the directions nxs_dyn_set_halo added on a ragged partition.  low_level: the caller's own bookkeeping through
        nxs_dyn_ipc_connect (tables for the caller's send neighbours; refused by the library where a neighbour exists in one direction only)."""
        lm = self.lm
        ok = 1
        self._ipc_error = ""
        if low_level:
            blob = C.create_string_buffer(IPC_BLOB_BYTES)
            try:
                self._chk(self.L.nxs_dyn_ipc_export(self.h, blob))
            except NxsError as e:
                self._ipc_error = f"rank {lm.rank}: export: {e}"
                ok = 0
            infos = all_gather({"ok": ok, "blob": blob.raw, "recv_procs": lm.recv_procs.tolist(),
                                "recv_offsets": lm.recv_offsets.tolist(), "err": self._ipc_error})
        else:
            n = C.c_int32(0)
            rec = b""
            try:
                self._chk(self.L.nxs_dyn_ipc_record_bytes(self.h, C.byref(n)))
            except NxsError as e:
                self._ipc_error = f"rank {lm.rank}: record: {e}"
                ok = 0
            stride = max(all_gather(int(n.value)))       # (the launcher's MPI_Allreduce(MAX))
            if ok:
                buf = C.create_string_buffer(stride)
                try:
                    self._chk(self.L.nxs_dyn_ipc_export_record(self.h, buf, stride))
                    rec = buf.raw
                except NxsError as e:
                    self._ipc_error = f"rank {lm.rank}: export: {e}"
                    ok = 0
            infos = all_gather({"ok": ok, "rec": rec if ok else bytes(stride), "err": self._ipc_error})
        if not all(i["ok"] for i in infos):
            self._ipc_error = "; ".join(i["err"] for i in infos if i["err"])   # (every rank reports what any rank saw)
            return False
        ok = 1
        try:
            if low_level:
                blobs, off, tot, slot = b"", [], [], []
                for q in lm.send_procs.tolist():
                    inf = infos[q]
                    k = inf["recv_procs"].index(lm.rank)
                    blobs += inf["blob"]
                    off.append(inf["recv_offsets"][k]); tot.append(inf["recv_offsets"][-1]); slot.append(k)
                a_off, a_tot, a_slot = (np.ascontiguousarray(np.asarray(v, np.int32)) for v in (off, tot, slot))
                bbuf = C.create_string_buffer(blobs, max(len(blobs), 1))
                self._chk(self.L.nxs_dyn_ipc_connect(self.h, bbuf, _abi.iptr(a_off), _abi.iptr(a_tot), _abi.iptr(a_slot)))
            else:
                recs = b"".join(i["rec"] for i in infos)
                self._chk(self.L.nxs_dyn_ipc_connect_records(self.h, C.create_string_buffer(recs, len(recs)), stride, len(infos)))
        except NxsError as e:
            self._ipc_error = f"rank {lm.rank}: connect: {e}"
            ok = 0
        oks = all_gather((ok, self._ipc_error))
        if not all(o for o, _ in oks):
            self._ipc_error = "; ".join(m for _, m in oks if m)
            self.L.nxs_dyn_set_halo(self.h, C.byref(_abi.halo_struct(lm)))  # drops the half-made transport
            return False
        err = C.c_int32(0)
        try:
            self._chk(self.L.nxs_dyn_ipc_selftest(self.h, selftest_rounds, C.byref(err)))
        except NxsError as e:   # still take part in the gather below: the other ranks are waiting in it
            self._ipc_error = f"rank {lm.rank}: self-test: {e}"
            err.value = err.value or -1
        if err.value and not self._ipc_error:
            self._ipc_error = f"rank {lm.rank}: self-test: {err.value} payload(s) wrong"
        errs = all_gather((int(err.value), self._ipc_error))
        good = all(e == 0 for e, _ in errs)
        if not good:
            self._ipc_error = "; ".join(m for _, m in errs if m)
            self.L.nxs_dyn_set_halo(self.h, C.byref(_abi.halo_struct(lm)))
        return good

    def ipc_loopback(self) -> bool:
        """Profiling aid (nxs_dyn_ipc_loopback): the device-direct mailboxes of this handle connected to THEMSELVES, so that a rank's partition can be stepped
        alone on a device with the exchange inside its kernels.  The ghosts receive meaningless velocities (results are NOT the model's); the launches walk
        the same tables and move the same bytes.  False when the partition's lists do not allow it (no neighbour)."""
        rc = self.L.nxs_dyn_ipc_loopback(self.h)
        if rc == -1:
            return False
        self._chk(rc)
        return True

    @staticmethod
    def comm_unique_id() -> bytes:
        L = load_library()
        buf = C.create_string_buffer(128)
        rc = L.nxs_dyn_comm_unique_id(buf)
        if rc:
            raise NxsError(rc, (L.nxs_dyn_last_error(None) or b"").decode())
        return buf.raw

    def set_option(self, key: str, value: int):
        self._chk(self.L.nxs_dyn_set_option(self.h, key.encode(), int(value)))

    # ---- data movement ----
    def put_state(self, arrays: dict):
        s = _abi.state_struct(arrays)
        self._chk(self.L.nxs_dyn_put_state(self.h, C.byref(s)))

    def set_forcing(self, arrays: dict):
        f = _abi.forcing_struct(arrays)
        self._chk(self.L.nxs_dyn_set_forcing(self.h, C.byref(f)))

    def set_forcing_pair(self, arrays0: dict, arrays1: dict):
        """The two snapshots of a forcing interval become resident (ExternalData's interpolated_data[0], [1])."""
        f0, f1 = _abi.forcing_struct(arrays0), _abi.forcing_struct(arrays1)
        self._keep_forcing = (arrays0, arrays1)
        self._chk(self.L.nxs_dyn_set_forcing_pair(self.h, C.byref(f0), C.byref(f1)))

    def set_forcing_time(self, fcoeff0: float, fcoeff1: float, factor=None, bias=None):
        """Per step: M_factor*(fcoeff0*d0 + fcoeff1*d1) + M_bias_correction on the device (externaldata.cpp:360-401)."""
        fa = (C.c_double * 3)(*factor) if factor is not None else None
        bi = (C.c_double * 3)(*bias) if bias is not None else None
        self._chk(self.L.nxs_dyn_set_forcing_time(self.h, float(fcoeff0), float(fcoeff1), fa, bi))

    # ---- the coupled build's terms (#ifdef OASIS in the reference) ----
    def set_wave_stress(self, tau_wi):
        """M_tau_wi ([2*Nn], u then v): the wave radiation stress explicitSolve() adds to the wind stress (FE.cpp:10509-10518).  None detaches it."""
        if tau_wi is None:
            self._chk(self.L.nxs_dyn_set_wave_stress(self.h, None))
            return
        a = np.ascontiguousarray(tau_wi, np.float64)
        if a.shape != (2 * self.lm.num_nodes,):
            raise ValueError(f"tau_wi has shape {a.shape}, expected ({2 * self.lm.num_nodes},)")
        self._chk(self.L.nxs_dyn_set_wave_stress(self.h, _abi.dptr(a)))

    def put_coupled(self, cum_damage=None, conc_fsd=None):
        """M_cum_damage ([Ne]) and M_conc_fsd ([num_fsd_bins, Ne], bin-major) to the device; what is given is carried by the following steps
        (FE.cpp:4233-4238, 3991-3994), what is None is detached."""
        c = _abi.Coupled()
        Ne = self.lm.num_elements
        if cum_damage is not None:
            cd = np.ascontiguousarray(cum_damage, np.float64)
            if cd.shape != (Ne,):
                raise ValueError(f"cum_damage has shape {cd.shape}, expected ({Ne},)")
            c.cum_damage = _abi.dptr(cd)
        if conc_fsd is not None:
            cf = np.ascontiguousarray(conc_fsd, np.float64)
            if cf.ndim != 2 or cf.shape[1] != Ne:
                raise ValueError(f"conc_fsd has shape {cf.shape}, expected (num_fsd_bins, {Ne})")
            c.conc_fsd = _abi.dptr(cf)
            c.num_fsd_bins = cf.shape[0]
        self._chk(self.L.nxs_dyn_put_coupled(self.h, C.byref(c)))

    def get_coupled(self, cum_damage: bool = True, num_fsd_bins: int = 0) -> dict:
        """{'cum_damage': [Ne]} and / or {'conc_fsd': [num_fsd_bins, Ne]} from the device; asking for a member that is not attached is an error."""
        c = _abi.Coupled()
        out = {}
        Ne = self.lm.num_elements
        if cum_damage:
            out["cum_damage"] = np.empty(Ne)
            c.cum_damage = _abi.dptr(out["cum_damage"])
        if num_fsd_bins > 0:
            out["conc_fsd"] = np.empty((num_fsd_bins, Ne))
            c.conc_fsd = _abi.dptr(out["conc_fsd"])
            c.num_fsd_bins = num_fsd_bins
        self._chk(self.L.nxs_dyn_get_coupled(self.h, C.byref(c)))
        return out

    # ---- the floe-size distribution: initFsd / updateFSD / redistributeFSD / weldingRoach (FE.cpp:7562-7576, 4674-4732, 4268-4483, 4737-4870, 5888-5896) ----
    def fsd_configure(self, tables: dict, **options):
        """nxs_dyn_fsd_configure: the tables of fsd_bins (or the caller's own) and the options of the loops, keywords named after nxs_dyn_fsd_config
        (breakup_type / welding_type also as the reference's strings).  The number of bins is the tables'; it must be the attached conc_fsd's."""
        tables = {k: np.ascontiguousarray(v, np.int32 if k == "alpha_merge" else np.float64) for k, v in tables.items() if v is not None}
        n = int(options.pop("num_bins", tables["bin_centres"].size if "bin_centres" in tables else 0))
        c = _abi.fsd_config_struct(n, tables, **options)
        self._chk(self.L.nxs_dyn_fsd_configure(self.h, C.byref(c)))
        self._fsd_bins = n

    def fsd_put(self, conc_mech_fsd=None, cum_wave_damage=None):
        """M_conc_mech_fsd ([num_fsd_bins, Ne], bin-major) and M_cum_wave_damage ([Ne]) to the device; what is None is detached."""
        s = _abi.FsdState()
        Ne = self.lm.num_elements
        if conc_mech_fsd is not None:
            m = np.ascontiguousarray(conc_mech_fsd, np.float64)
            if m.ndim != 2 or m.shape[1] != Ne:
                raise ValueError(f"conc_mech_fsd has shape {m.shape}, expected (num_fsd_bins, {Ne})")
            s.conc_mech_fsd = _abi.dptr(m)
            s.num_fsd_bins = m.shape[0]
        if cum_wave_damage is not None:
            w = np.ascontiguousarray(cum_wave_damage, np.float64)
            if w.shape != (Ne,):
                raise ValueError(f"cum_wave_damage has shape {w.shape}, expected ({Ne},)")
            s.cum_wave_damage = _abi.dptr(w)
        self._chk(self.L.nxs_dyn_fsd_put(self.h, C.byref(s)))

    def fsd_get(self, num_fsd_bins: int = 0, cum_wave_damage: bool = False) -> dict:
        """{'conc_mech_fsd': [num_fsd_bins, Ne]} and / or {'cum_wave_damage': [Ne]} from the device, and 'weld_crash': whether a crash condition of
        weldingRoach was met since the last fsd_get."""
        s = _abi.FsdState()
        out = {}
        Ne = self.lm.num_elements
        if num_fsd_bins > 0:
            out["conc_mech_fsd"] = np.empty((num_fsd_bins, Ne))
            s.conc_mech_fsd = _abi.dptr(out["conc_mech_fsd"])
            s.num_fsd_bins = num_fsd_bins
        if cum_wave_damage:
            out["cum_wave_damage"] = np.empty(Ne)
            s.cum_wave_damage = _abi.dptr(out["cum_wave_damage"])
        self._chk(self.L.nxs_dyn_fsd_get(self.h, C.byref(s)))
        out["weld_crash"] = int(s.weld_crash)
        return out

    def fsd_init(self):
        """The distribution at the end of initFsd(): all the ice in the highest bin.  Asynchronous."""
        self._chk(self.L.nxs_dyn_fsd_init(self.h))

    def fsd_update(self):
        """updateFSD(): the bins rescaled to the total concentration.  Asynchronous."""
        self._chk(self.L.nxs_dyn_fsd_update(self.h))

    def fsd_breakup(self, wlbk, want_flags: bool = True):
        """redistributeFSD() with M_wlbk = wlbk ([Ne] array, or an int: a device address).  Returns (M_breakup_in_dt, crash) -- or None, the call staying
        asynchronous, with want_flags False."""
        flags = 0
        if isinstance(wlbk, (int, np.integer)):
            ptr, flags = C.c_void_p(int(wlbk)), _abi.NXS_FSD_WLBK_ON_DEVICE
        else:
            w = np.ascontiguousarray(wlbk, np.float64)
            if w.shape != (self.lm.num_elements,):
                raise ValueError(f"wlbk has shape {w.shape}, expected ({self.lm.num_elements},)")
            ptr = C.c_void_p(w.ctypes.data)
        if not want_flags:
            self._chk(self.L.nxs_dyn_fsd_breakup(self.h, ptr, flags, None, None))
            return None
        b, c = C.c_int32(-1), C.c_int32(-1)
        self._chk(self.L.nxs_dyn_fsd_breakup(self.h, ptr, flags, C.byref(b), C.byref(c)))
        return bool(b.value), bool(c.value)

    def fsd_weld(self, ddt: float, freezing):
        """weldingRoach(i, ddt) and the mechanical healing where freezing[i] (thermo's del_hi > 0).  The kernel is asynchronous."""
        f = np.ascontiguousarray(np.asarray(freezing) != 0, np.uint8)
        if f.shape != (self.lm.num_elements,):
            raise ValueError(f"freezing has shape {f.shape}, expected ({self.lm.num_elements},)")
        self._chk(self.L.nxs_dyn_fsd_weld(self.h, float(ddt), _abi.bptr(f)))

    # ---- thermo()'s atmospheric bulk fluxes: OWBulkFluxes + IABulkFluxes (FE.cpp:5214-5277) ----
    def _element_rows(self, struct, names, rows: dict, what: str):
        keep = []
        for k, v in rows.items():
            if k not in names:
                raise KeyError(f"{what} has no row {k!r}")
            if v is None:
                continue
            a = np.ascontiguousarray(v, np.float64)
            if a.shape != (self.lm.num_elements,):
                raise ValueError(f"{k} has shape {a.shape}, expected ({self.lm.num_elements},)")
            setattr(struct, k, _abi.dptr(a))
            keep.append(a)
        return keep

    def flux_configure(self, **options):
        """nxs_dyn_flux_configure: the defaults of flux_default_config() changed by keywords named after nxs_dyn_flux_config's members.  Survives set_mesh."""
        c = _flux_config(options)
        self._chk(self.L.nxs_dyn_flux_configure(self.h, C.byref(c)))

    def flux_set_atmosphere(self, **rows):
        """tair, mslp, Qsw_in, humidity (dew point, specific humidity or mixing ratio, as configured), longwave (Qlw_in or tcc): [Ne] each; a row left out or
        None keeps the device copy."""
        a = _abi.FluxAtmosphere()
        keep = self._element_rows(a, _abi.FLUX_ATMOSPHERE, rows, "nxs_dyn_flux_atmosphere")
        self._chk(self.L.nxs_dyn_flux_set_atmosphere(self.h, C.byref(a)))
        del keep

    def flux_put(self, **rows):
        """tice0, tsurf_young, sst, sss, drag_ti, drag_ti_young, pond_fraction, lid_volume: [Ne] each; a row left out or None keeps the device copy."""
        s = _abi.FluxState()
        keep = self._element_rows(s, _abi.FLUX_STATE, rows, "nxs_dyn_flux_state")
        self._chk(self.L.nxs_dyn_flux_put(self.h, C.byref(s)))
        del keep

    def flux_get(self, names=_abi.FLUX_STATE) -> dict:
        """The named rows of nxs_dyn_flux_state from the device (all of them by default)."""
        out = {k: np.empty(self.lm.num_elements) for k in names}
        s = _abi.FluxState()
        self._element_rows(s, _abi.FLUX_STATE, out, "nxs_dyn_flux_state")
        self._chk(self.L.nxs_dyn_flux_get(self.h, C.byref(s)))
        return out

    def fluxes(self):
        """nxs_dyn_fluxes: one launch; D_tau_ow, M_drag_ui / M_drag_ti and their _young twins are updated on the device.  Asynchronous on the handle's stream."""
        self._chk(self.L.nxs_dyn_fluxes(self.h))

    def fluxes_get(self, names=_abi.FLUX_ROWS, want_device: bool = False):
        """The named rows of _abi.FLUX_ROWS as host arrays; with want_device also {name: device pointer} of all 25 rows."""
        out = {k: np.empty(self.lm.num_elements) for k in names}
        r = _abi.FluxRows()
        for k, v in out.items():
            r.row[_abi.FLUX_ROWS.index(k)] = _abi.dptr(v)
        dev = (C.c_void_p * _abi.NXS_FLUX_ROWS)()
        self._chk(self.L.nxs_dyn_fluxes_get(self.h, C.byref(r), dev if want_device else None))
        if want_device:
            return out, dict(zip(_abi.FLUX_ROWS, (int(p or 0) for p in dev)))
        return out

    # ---- thermo()'s ice columns: sections 3.2 to 5 of the slab loop, thermoWinton / thermoIce0 (FE.cpp:5306-5411) ----
    def column_configure(self, **options):
        """nxs_dyn_column_configure: the defaults of column_default_config() changed by keywords named after nxs_dyn_column_config's members.  Survives set_mesh."""
        c = _column_config(options)
        self._chk(self.L.nxs_dyn_column_configure(self.h, C.byref(c)))

    def column_set_forcing(self, **rows):
        """precip, snow (snowfr or snowfall, as configured), ocean_temp, ocean_salt, mld: [Ne] each; a row left out or None keeps the device copy."""
        f = _abi.ColumnForcing()
        keep = self._element_rows(f, _abi.COL_FORCING, rows, "nxs_dyn_column_forcing")
        self._chk(self.L.nxs_dyn_column_set_forcing(self.h, C.byref(f)))
        del keep

    def column_put(self, **rows):
        """tice1, tice2: [Ne] each (tice0, tsurf_young, sst and sss are flux_put's); a row left out or None keeps the device copy."""
        s = _abi.ColumnState()
        keep = self._element_rows(s, _abi.COL_STATE, rows, "nxs_dyn_column_state")
        self._chk(self.L.nxs_dyn_column_put(self.h, C.byref(s)))
        del keep

    def column_get(self, names=_abi.COL_STATE) -> dict:
        """The named rows of nxs_dyn_column_state from the device (nxs_dyn_column_get_state; both by default)."""
        out = {k: np.empty(self.lm.num_elements) for k in names}
        s = _abi.ColumnState()
        self._element_rows(s, _abi.COL_STATE, out, "nxs_dyn_column_state")
        self._chk(self.L.nxs_dyn_column_get_state(self.h, C.byref(s)))
        return out

    def column(self, dt: int):
        """nxs_dyn_column: one launch; dt is thermo()'s integer argument.  M_tice, M_tsurf_young, M_h_young and M_hs_young are updated on the device.  Asynchronous."""
        self._chk(self.L.nxs_dyn_column(self.h, int(dt)))

    def column_rows(self, names=_abi.COL_ROWS, want_device: bool = False):
        """The named rows of _abi.COL_ROWS as host arrays (nxs_dyn_column_get); with want_device also {name: device pointer} of all 22 rows."""
        out = {k: np.empty(self.lm.num_elements) for k in names}
        r = _abi.ColumnRows()
        for k, v in out.items():
            r.row[_abi.COL_ROWS.index(k)] = _abi.dptr(v)
        dev = (C.c_void_p * _abi.NXS_COL_ROWS)()
        self._chk(self.L.nxs_dyn_column_get(self.h, C.byref(r), dev if want_device else None))
        if want_device:
            return out, dict(zip(_abi.COL_ROWS, (int(p or 0) for p in dev)))
        return out

    # ---- thermo()'s element forcing: both snapshots resident, ExternalData::get per step on the device (model/externaldata.cpp:324-439, 1436) ----
    def _thermo_forcing_rows(self, rows, what: str):
        r, keep = _abi.ThermoForcingRows(), []
        for k, v in (rows or {}).items():
            if k not in _abi.TF_ROWS:
                raise KeyError(f"{what} has no row {k!r}")
            if v is None:
                continue
            a = np.ascontiguousarray(v, np.float64)
            if a.shape != (self.lm.num_elements,):
                raise ValueError(f"{k} has shape {a.shape}, expected ({self.lm.num_elements},)")
            r.row[_abi.TF_ROWS.index(k)] = _abi.dptr(a)
            keep.append(a)
        return r, keep

    def thermo_forcing_pair(self, snapshot0: dict, snapshot1: dict = None):
        """nxs_dyn_thermo_forcing_pair: {row name of _abi.TF_ROWS: [Ne]} of snapshot 0 and (optionally) 1; a row left out or None keeps that snapshot's device copy."""
        r0, keep0 = self._thermo_forcing_rows(snapshot0, "nxs_dyn_thermo_forcing_rows")
        r1, keep1 = self._thermo_forcing_rows(snapshot1, "nxs_dyn_thermo_forcing_rows")
        self._chk(self.L.nxs_dyn_thermo_forcing_pair(self.h, C.byref(r0), C.byref(r1) if snapshot1 is not None else None))
        del keep0, keep1

    def thermo_forcing_time(self, rows: dict):
        """nxs_dyn_thermo_forcing_time: {row name: dict(mode="off" | "linear" | "step" or NXS_TF_*, fcoeff0=, fcoeff1=, factor=1, bias=0)}; a row left out is OFF.
        One asynchronous launch writes the rows nxs_dyn_fluxes / nxs_dyn_column / nxs_dyn_slab read."""
        t = _abi.ThermoForcingTime()
        for k in range(_abi.NXS_TF_ROWS):
            t.factor[k] = 1.
        for name, spec in rows.items():
            if name not in _abi.TF_ROWS:
                raise KeyError(f"nxs_dyn_thermo_forcing_time has no row {name!r}")
            k = _abi.TF_ROWS.index(name)
            mode = spec.get("mode", "linear")
            t.mode[k] = _abi.TF_MODES[mode] if isinstance(mode, str) else int(mode)
            t.fcoeff0[k], t.fcoeff1[k] = float(spec.get("fcoeff0", 1.)), float(spec.get("fcoeff1", 0.))
            t.factor[k], t.bias[k] = float(spec.get("factor", 1.)), float(spec.get("bias", 0.))
        self._chk(self.L.nxs_dyn_thermo_forcing_time(self.h, C.byref(t)))

    def thermo_forcing_targets(self, set: int, RX, RY):
        """nxs_dyn_thermo_forcing_targets: the [Ne] element barycentres in the coordinates of dataset `set` (0 .. NXS_TF_SETS - 1), resident until the mesh changes."""
        rx, ry = np.ascontiguousarray(RX, np.float64), np.ascontiguousarray(RY, np.float64)
        if rx.shape != (self.lm.num_elements,) or ry.shape != rx.shape:
            raise ValueError(f"targets have shapes {rx.shape}, {ry.shape}, expected ({self.lm.num_elements},)")
        self._chk(self.L.nxs_dyn_thermo_forcing_targets(self.h, int(set), _abi.dptr(rx), _abi.dptr(ry)))

    def thermo_forcing_ingest(self, set: int, x_in, y_in, data, row, snapshot, default_value=1e8, interp=1, row_major=False):
        """nxs_dyn_thermo_forcing_ingest: InterpFromGridToMeshx at the targets of `set`, arguments as interp.InterpFromGridToMeshx (data [M, N, N_data], or
        [N, M, N_data] when row_major; x_in / y_in centres or contours).  Column j goes to snapshot[j] of row[j] (a name of _abi.TF_ROWS, NXS_TF_*, or -1 / None:
        skipped).  The launch is asynchronous."""
        f64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
        x_in, y_in, data = f64(x_in), f64(y_in), f64(data)
        if data.ndim == 2:
            data = data[:, :, None]
        M, N = (data.shape[1], data.shape[0]) if row_major else (data.shape[0], data.shape[1])
        rows = np.array([-1 if r is None else _abi.TF_ROWS.index(r) if isinstance(r, str) else int(r) for r in row], np.int32)
        snaps = np.ascontiguousarray(snapshot, np.int32)
        if rows.shape != (data.shape[2],) or snaps.shape != rows.shape:
            raise ValueError(f"row and snapshot must name the {data.shape[2]} columns of data")
        g = _abi.ForcingGrid(_abi.dptr(x_in), _abi.dptr(y_in), x_in.size, y_in.size, M, N, int(interp), int(bool(row_major)), float(default_value))
        self._chk(self.L.nxs_dyn_thermo_forcing_ingest(self.h, int(set), C.byref(g), _abi.dptr(data), data.shape[2], _abi.iptr(rows), _abi.iptr(snaps)))

    def thermo_forcing_attach_mesh(self, set: int, nodemap):
        """nxs_dyn_thermo_forcing_attach_mesh: an interp.NodeMap whose targets are this mesh's element barycentres (borrowed: keep it alive); None detaches."""
        self._chk(self.L.nxs_dyn_thermo_forcing_attach_mesh(self.h, int(set), nodemap.h if nodemap is not None else None))
        self._mf_elem_maps = getattr(self, "_mf_elem_maps", {})
        self._mf_elem_maps[int(set)] = nodemap

    def thermo_forcing_ingest_mesh(self, set: int, fields, row, n_step=2, scale_factor=1., add_offset=0., a=1., b=0., pairs=(), device: bool = False):
        """nxs_dyn_thermo_forcing_ingest_mesh: one loadDataset of a dataset on a triangulated source (interp.NodeMap.load_rows' arguments: n_step*n_var fields in
        the order fstep*n_var + j).  Variable j goes to row[j] (a name of _abi.TF_ROWS, NXS_TF_*, or -1 / None: skipped), forcing step fstep to snapshot fstep.
        The launches are asynchronous."""
        self._ingest_mesh(self.L.nxs_dyn_thermo_forcing_ingest_mesh, getattr(self, "_mf_elem_maps", {}).get(int(set)), _abi.TF_ROWS, set, fields, row, n_step,
                          scale_factor, add_offset, a, b, pairs, device)

    def thermo_forcing_get(self, which: int, names=_abi.TF_ROWS) -> dict:
        """nxs_dyn_thermo_forcing_get: the named rows of snapshot 0 / 1 (which = 0 / 1) or as the launches will read them (which = 2)."""
        out = {k: np.empty(self.lm.num_elements) for k in names}
        r, _ = self._thermo_forcing_rows(out, "nxs_dyn_thermo_forcing_rows")
        self._chk(self.L.nxs_dyn_thermo_forcing_get(self.h, int(which), C.byref(r)))
        return out

    # ---- the dynamics' nodal forcing: both snapshots of M_wind, M_ocean, M_ssh made on the device from the source grid (model/externaldata.cpp:461-940) ----
    def forcing_targets(self, set: int, RX, RY):
        """nxs_dyn_forcing_targets: the [Nn] node positions in the coordinates of dataset `set` (0 .. NXS_NF_SETS - 1), resident until the mesh changes."""
        rx, ry = np.ascontiguousarray(RX, np.float64), np.ascontiguousarray(RY, np.float64)
        if rx.shape != (self.lm.num_nodes,) or ry.shape != rx.shape:
            raise ValueError(f"targets have shapes {rx.shape}, {ry.shape}, expected ({self.lm.num_nodes},)")
        self._chk(self.L.nxs_dyn_forcing_targets(self.h, int(set), _abi.dptr(rx), _abi.dptr(ry)))

    def forcing_ingest(self, set: int, x_in, y_in, data, row, snapshot, default_value=1e8, interp=1, row_major=False, cyclic_x=False, cyclic_y=False, vectors=None):
        """nxs_dyn_forcing_ingest: transformData, the cyclic wrap and InterpFromGridToMeshx at the targets of `set` on the device.  data [M, N, N_data] (or
        [N, M, N_data] when row_major) untransformed and without the wrap; column j goes to snapshot[j] of row[j] (a name of _abi.NF_ROWS, NXS_NF_*, or -1 / None:
        skipped).  vectors: None, or a dict as forcing_vectors() takes it.  The launches are asynchronous."""
        f64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
        x_in, y_in, data = f64(x_in), f64(y_in), f64(data)
        if data.ndim == 2:
            data = data[:, :, None]
        M, N = (data.shape[1], data.shape[0]) if row_major else (data.shape[0], data.shape[1])
        rows = np.array([-1 if r is None else _abi.NF_ROWS.index(r) if isinstance(r, str) else int(r) for r in row], np.int32)
        snaps = np.ascontiguousarray(snapshot, np.int32)
        if rows.shape != (data.shape[2],) or snaps.shape != rows.shape:
            raise ValueError(f"row and snapshot must name the {data.shape[2]} columns of data")
        g = _abi.ForcingGrid(_abi.dptr(x_in), _abi.dptr(y_in), x_in.size, y_in.size, M, N, int(interp), int(bool(row_major)), float(default_value))
        v, keep = forcing_vectors(**vectors) if vectors is not None else (None, None)
        self._chk(self.L.nxs_dyn_forcing_ingest(self.h, int(set), C.byref(g), int(bool(cyclic_x)), int(bool(cyclic_y)), _abi.dptr(data), data.shape[2], _abi.iptr(rows),
                                                _abi.iptr(snaps), C.byref(v) if v is not None else None))
        self._nf_grid_shape = (M + int(bool(cyclic_y)), N + int(bool(cyclic_x)), data.shape[2])
        del keep

    def forcing_attach_mesh(self, set: int, nodemap):
        """nxs_dyn_forcing_attach_mesh: an interp.NodeMap with this mesh's nodes as targets (borrowed: keep it alive); None detaches."""
        self._chk(self.L.nxs_dyn_forcing_attach_mesh(self.h, int(set), nodemap.h if nodemap is not None else None))
        self._mf_node_maps = getattr(self, "_mf_node_maps", {})
        self._mf_node_maps[int(set)] = nodemap

    def forcing_ingest_mesh(self, set: int, fields, row, n_step=2, scale_factor=1., add_offset=0., a=1., b=0., pairs=(), device: bool = False):
        """nxs_dyn_forcing_ingest_mesh: one loadDataset of a dataset on a triangulated source (interp.NodeMap.load_rows' arguments: n_step*n_var fields in the order
        fstep*n_var + j).  Variable j goes to the half-row row[j] (a name of _abi.NF_ROWS, NXS_NF_*, or -1 / None: skipped), forcing step fstep to snapshot fstep.
        The launches are asynchronous."""
        self._ingest_mesh(self.L.nxs_dyn_forcing_ingest_mesh, getattr(self, "_mf_node_maps", {}).get(int(set)), _abi.NF_ROWS, set, fields, row, n_step,
                          scale_factor, add_offset, a, b, pairs, device)

    def _ingest_mesh(self, entry, nodemap, names, set, fields, row, n_step, scale_factor, add_offset, a, b, pairs, device):
        from . import interp
        l, keep = interp.NodeMap._load_struct(nodemap, fields, n_step, scale_factor, add_offset, a, b, pairs, device)   # (without a map: the library refuses the call)
        rows = np.array([-1 if r is None else names.index(r) if isinstance(r, str) else int(r) for r in row], np.int32)
        if rows.shape != (l.n_var,):
            raise ValueError(f"row must name the {l.n_var} variables")
        self._chk(entry(self.h, int(set), C.byref(l), _abi.iptr(rows), 1 if device else 0))   # NXS_REGRID_IN_DEVICE
        del keep

    def set_forcing_time_rows(self, groups: dict):
        """nxs_dyn_set_forcing_time_rows: {"wind" | "ocean" | "ssh": dict(mode="linear" | "step" | "off" or NXS_TF_*, fcoeff0=, fcoeff1=, factor=1, bias=0)}; a group
        left out is OFF.  One asynchronous launch writes M_wind / M_ocean / M_ssh as the step reads them."""
        t = _abi.ForcingTimeRows()
        for k in range(_abi.NXS_NF_GROUPS):
            t.factor[k] = 1.
        for name, spec in groups.items():
            if name not in _abi.NF_GROUPS:
                raise KeyError(f"nxs_dyn_set_forcing_time_rows has no group {name!r}")
            k = _abi.NF_GROUPS.index(name)
            mode = spec.get("mode", "linear")
            t.mode[k] = _abi.TF_MODES[mode] if isinstance(mode, str) else int(mode)
            t.fcoeff0[k], t.fcoeff1[k] = float(spec.get("fcoeff0", 1.)), float(spec.get("fcoeff1", 0.))
            t.factor[k], t.bias[k] = float(spec.get("factor", 1.)), float(spec.get("bias", 0.))
        self._chk(self.L.nxs_dyn_set_forcing_time_rows(self.h, C.byref(t)))

    def set_element_depth(self, depth):
        """nxs_dyn_set_element_depth: M_element_depth ([Ne], a constant dataset) alone."""
        a = np.ascontiguousarray(depth, np.float64)
        if a.shape != (self.lm.num_elements,):
            raise ValueError(f"element_depth has shape {a.shape}, expected ({self.lm.num_elements},)")
        self._chk(self.L.nxs_dyn_set_element_depth(self.h, _abi.dptr(a)))

    def forcing_get(self, which: int, names=_abi.NF_ROWS) -> dict:
        """nxs_dyn_forcing_get: the named [Nn] half-rows of snapshot 0 / 1."""
        out = {k: np.empty(self.lm.num_nodes) for k in names}
        r = _abi.ForcingRows()
        for k, a in out.items():
            r.row[_abi.NF_ROWS.index(k)] = _abi.dptr(a)
        self._chk(self.L.nxs_dyn_forcing_get(self.h, int(which), C.byref(r)))
        return out

    def forcing_grid(self) -> np.ndarray:
        """debug array "nf_grid": the last forcing_ingest's grid data after transformData and the wrap, [cM, cN, N_data]."""
        shape = getattr(self, "_nf_grid_shape", None)
        if shape is None:
            raise NxsError(-2, "forcing_grid before forcing_ingest")
        out = np.empty(shape)
        self._chk(self.L.nxs_dyn_debug_array(self.h, b"nf_grid", _abi.dptr(out), out.size))
        return out

    # ---- nesting: nestingIce / nestingDynamics on the device (FE.cpp:4878-4958), both snapshots of a nesting interval resident ----
    def nesting_configure(self, **options):
        """nxs_dyn_nesting_configure: nudge_function ("linear" | "exponential"), nudge_timescale (s), nudge_scale (= M_nudge_lengthscale * M_res_root_mesh),
        nest_dynamic_vars, time_step (the model's int) and dtime_step (its double; time_step by default).  Survives set_mesh."""
        self._chk(self.L.nxs_dyn_nesting_configure(self.h, C.byref(_nesting_config(**options))))

    def _nesting_rows(self, rows):
        r, keep = _abi.NestingRows(), []
        for k, v in (rows or {}).items():
            if k not in _abi.NEST_ELEMENT_ROWS + _abi.NEST_NODE_ROWS:
                raise KeyError(f"nxs_dyn_nesting_rows has no row {k!r}")
            if v is None:
                continue
            nodal = k in _abi.NEST_NODE_ROWS
            n = self.lm.num_nodes if nodal else self.lm.num_elements
            a = np.ascontiguousarray(v, np.float64)
            if a.shape != (n,):
                raise ValueError(f"{k} has shape {a.shape}, expected ({n},)")
            if nodal:
                r.node[_abi.NEST_NODE_ROWS.index(k)] = _abi.dptr(a)
            else:
                r.element[_abi.NEST_ELEMENT_ROWS.index(k)] = _abi.dptr(a)
            keep.append(a)
        return r, keep

    def nesting_pair(self, snapshot0: dict, snapshot1: dict = None):
        """nxs_dyn_nesting_pair: {row name of _abi.NEST_ELEMENT_ROWS ([Ne]) or _abi.NEST_NODE_ROWS ([Nn])} of snapshot 0 and (optionally) 1; a row left out or None
        is not given.  The rows go with the mesh."""
        r0, keep0 = self._nesting_rows(snapshot0)
        r1, keep1 = self._nesting_rows(snapshot1)
        self._chk(self.L.nxs_dyn_nesting_pair(self.h, C.byref(r0), C.byref(r1) if snapshot1 is not None else None))
        del keep0, keep1

    def nesting_time(self, datasets: dict):
        """nxs_dyn_nesting_time: {dataset name of _abi.NEST_DATASETS: dict(mode="linear" | "step" | "off" or NXS_TF_*, fcoeff0=, fcoeff1=, factor=1, bias=0)}; a dataset
        left out is OFF.  No launch: nesting_ice / nesting_dynamics evaluate the targets."""
        t = _abi.NestingTime()
        for k in range(_abi.NXS_NEST_DATASETS):
            t.factor[k] = 1.
        for name, spec in datasets.items():
            if name not in _abi.NEST_DATASETS:
                raise KeyError(f"nxs_dyn_nesting_time has no dataset {name!r}")
            k = _abi.NEST_DATASETS.index(name)
            mode = spec.get("mode", "linear")
            t.mode[k] = _abi.TF_MODES[mode] if isinstance(mode, str) else int(mode)
            t.fcoeff0[k], t.fcoeff1[k] = float(spec.get("fcoeff0", 1.)), float(spec.get("fcoeff1", 0.))
            t.factor[k], t.bias[k] = float(spec.get("factor", 1.)), float(spec.get("bias", 0.))
        self._chk(self.L.nxs_dyn_nesting_time(self.h, C.byref(t)))

    def nesting_ice(self):
        """nxs_dyn_nesting_ice: one launch; M_conc, M_thick, M_snow_thick (and the young-ice trio) relaxed towards the outer model.  Asynchronous."""
        self._chk(self.L.nxs_dyn_nesting_ice(self.h))

    def nesting_dynamics(self):
        """nxs_dyn_nesting_dynamics: one launch; M_sigma, M_damage, M_ridge_ratio and M_VT, where they are current on the device.  Asynchronous."""
        self._chk(self.L.nxs_dyn_nesting_dynamics(self.h))

    def nesting_get(self, which: int, names=_abi.NEST_ELEMENT_ROWS + _abi.NEST_NODE_ROWS) -> dict:
        """nxs_dyn_nesting_get: the named rows of snapshot 0 / 1."""
        out = {k: np.empty(self.lm.num_nodes if k in _abi.NEST_NODE_ROWS else self.lm.num_elements) for k in names}
        r, _ = self._nesting_rows(out)
        self._chk(self.L.nxs_dyn_nesting_get(self.h, int(which), C.byref(r)))
        return out

    # ---- the slab ocean's horizontal diffusion: diffuse() for M_sst and M_sss (FE.cpp:2760-2815) ----
    def diffusion_configure(self, diffusivity_sst: float, diffusivity_sss: float, dx: float, dtime_step: float):
        """nxs_dyn_diffusion_configure: a diffusivity <= 0 switches that field off.  Survives set_mesh."""
        self._chk(self.L.nxs_dyn_diffusion_configure(self.h, float(diffusivity_sst), float(diffusivity_sss), float(dx), float(dtime_step)))

    def diffuse(self):
        """nxs_dyn_diffuse: one Jacobi step on the sst / sss rows of flux_put, in place; call it right before step().  Asynchronous."""
        self._chk(self.L.nxs_dyn_diffuse(self.h))

    # ---- a coupled ocean: thermo() under OceanType::COUPLED, and the receive of its element fields (include/nxs_dyn.h, nxs_dyn_ocean_coupled_*) ----
    def ocean_coupled_attach(self, gridmap=None, rows=None, **coef):
        """nxs_dyn_ocean_coupled_attach.  gridmap: an interp.GridMap of this handle's mesh (borrowed: keep it alive), or None for a host that only uses
        ocean_coupled_put_rows.  rows: the received rows in the order the fields arrive (names of _abi.OC_ROWS; default: ocean_coupled_default_config()); a, b,
        factor, bias: per field.  While attached with ocean_temp, ocean_salt and qsrml, fluxes / column / slab / slab_coupled run the COUPLED branch."""
        if rows is None:
            d = ocean_coupled_default_config()
            rows = d.pop("rows")
            coef = dict(d, **coef)
        c = _abi.ocean_coupled_config_struct(rows, **coef)
        self._chk(self.L.nxs_dyn_ocean_coupled_attach(self.h, gridmap.h if gridmap is not None else None, C.byref(c)))
        self._oc_map, self._oc_fields = gridmap, c.n_fields

    def ocean_coupled_detach(self):
        """nxs_dyn_ocean_coupled_attach(h, NULL, NULL): the handle is again the library without a coupled ocean."""
        self._chk(self.L.nxs_dyn_ocean_coupled_attach(self.h, None, None))
        self._oc_map = None

    def ocean_coupled_receive(self, fields, device: bool = False):
        """nxs_dyn_ocean_coupled_receive: fields = one [G] array per configured row, in the configured order -- or, with device=True, one device address each.  One
        launch on the handle's stream."""
        n = len(fields)
        ptrs = (C.c_void_p * max(n, 1))()
        keep = []
        for k, f in enumerate(fields):
            if device:
                ptrs[k] = int(f)
            else:
                a = np.ascontiguousarray(f, np.float64).ravel()
                G = self._oc_map.info()["grid_size"] if getattr(self, "_oc_map", None) is not None else a.size
                if a.size != G:
                    raise ValueError(f"field {k} has {a.size} cells, the map's grid has {G}")
                keep.append(a)
                ptrs[k] = a.ctypes.data
        if n != getattr(self, "_oc_fields", n):
            raise ValueError(f"{n} fields given, the attached configuration receives {self._oc_fields}")
        self._chk(self.L.nxs_dyn_ocean_coupled_receive(self.h, ptrs, 1 if device else 0))   # NXS_REGRID_IN_DEVICE
        del keep

    def ocean_coupled_put_rows(self, **rows):
        """ocean_temp, ocean_salt, qsrml, mld, wlbk: [Ne] host rows; a row left out or None is skipped."""
        r = _abi.OceanCoupledRows()
        keep = []
        for k, v in rows.items():
            if k not in _abi.OC_ROWS:
                raise KeyError(f"nxs_dyn_ocean_coupled_rows has no row {k!r}")
            if v is None:
                continue
            a = np.ascontiguousarray(v, np.float64)
            if a.shape != (self.lm.num_elements,):
                raise ValueError(f"{k} has shape {a.shape}, expected ({self.lm.num_elements},)")
            r.row[_abi.OC_ROWS.index(k)] = _abi.dptr(a)
            keep.append(a)
        self._chk(self.L.nxs_dyn_ocean_coupled_put_rows(self.h, C.byref(r)))
        del keep

    def ocean_coupled_get(self, names=(), want_device: bool = False):
        """The named rows of _abi.OC_ROWS as host arrays (synchronised); with want_device also {name: device pointer} of the five rows, 0 for a missing one."""
        out = {k: np.empty(self.lm.num_elements) for k in names}
        r = _abi.OceanCoupledRows()
        for k, v in out.items():
            r.row[_abi.OC_ROWS.index(k)] = _abi.dptr(v)
        dev = (C.c_void_p * _abi.NXS_OC_ROWS)()
        self._chk(self.L.nxs_dyn_ocean_coupled_get(self.h, C.byref(r), dev if want_device else None))
        if want_device:
            return out, dict(zip(_abi.OC_ROWS, (int(p or 0) for p in dev)))
        return out

    # ---- the nodal half of a coupled run's receive (include/nxs_dyn.h, nxs_dyn_nodes_coupled_*) ----
    def nodes_coupled_attach(self, which, nodemap, a=1., b=0., factor=1., bias=0.):
        """nxs_dyn_nodes_coupled_attach.  which: "ocean" (I_Uocn, I_Vocn, I_SSH) or "wave" (I_tauwix, I_tauwiy); nodemap: an interp.NodeMap with this mesh's nodes as
        targets and a source set (borrowed: keep it alive); a, b, factor, bias per field (scalars are broadcast)."""
        w = _abi.NC_DATASETS.index(which)
        c = _abi.NodesCoupledConfig()
        n = len(_abi.NC_FIELDS[which])
        for name, v, dflt in (("a", a, 1.), ("b", b, 0.), ("factor", factor, 1.), ("bias", bias, 0.)):
            vals = np.broadcast_to(np.asarray(v, np.float64), (n,))
            for k in range(_abi.NXS_NC_MAX_FIELDS):
                getattr(c, name)[k] = float(vals[k]) if k < n else dflt
        self._chk(self.L.nxs_dyn_nodes_coupled_attach(self.h, w, nodemap.h if nodemap is not None else None, C.byref(c)))
        if not hasattr(self, "_nc_maps"):
            self._nc_maps = {}
        self._nc_maps[which] = nodemap

    def nodes_coupled_detach(self, which):
        """nxs_dyn_nodes_coupled_attach(h, which, NULL, NULL)"""
        self._chk(self.L.nxs_dyn_nodes_coupled_attach(self.h, _abi.NC_DATASETS.index(which), None, None))
        getattr(self, "_nc_maps", {}).pop(which, None)

    def nodes_coupled_receive(self, which, fields, device: bool = False):
        """nxs_dyn_nodes_coupled_receive: fields = one [G] array per field of the dataset, in order -- or, with device=True, one device address each.  Two launches on
        the handle's stream."""
        n = len(fields)
        ptrs = (C.c_void_p * max(n, 1))()
        keep = []
        for k, f in enumerate(fields):
            if device:
                ptrs[k] = int(f) if f is not None else None
            elif f is not None:
                arr = np.ascontiguousarray(f, np.float64).ravel()
                keep.append(arr)
                ptrs[k] = arr.ctypes.data
        self._chk(self.L.nxs_dyn_nodes_coupled_receive(self.h, _abi.NC_DATASETS.index(which), ptrs, n, 1 if device else 0))   # NXS_REGRID_IN_DEVICE
        del keep

    def nodes_coupled_get(self, which, want_device: bool = False):
        """The received rows [n_fields, Nn] (synchronised); with want_device also their device addresses."""
        n = len(_abi.NC_FIELDS[which])
        out = np.empty((n, self.lm.num_nodes))
        ptrs, dev = (C.c_void_p * _abi.NXS_NC_MAX_FIELDS)(), (C.c_void_p * _abi.NXS_NC_MAX_FIELDS)()
        for k in range(n):
            ptrs[k] = out[k].ctypes.data
        self._chk(self.L.nxs_dyn_nodes_coupled_get(self.h, _abi.NC_DATASETS.index(which), ptrs, dev if want_device else None))
        if want_device:
            return out, [int(p or 0) for p in dev[:n]]
        return out

    def flux_device_rows(self) -> dict:
        """nxs_dyn_flux_device_rows: {row name of _abi.FLUX_STATE: device address, 0 for a row never put on this mesh}."""
        dev = (C.c_void_p * len(_abi.FLUX_STATE))()
        self._chk(self.L.nxs_dyn_flux_device_rows(self.h, dev))
        return dict(zip(_abi.FLUX_STATE, (int(p or 0) for p in dev)))

    # ---- thermo()'s slab loop from new ice to tracers: sections 6 to 10 (FE.cpp:5413-6133) ----
    def slab_configure(self, **options):
        """nxs_dyn_slab_configure: the defaults of slab_default_config() changed by keywords named after nxs_dyn_slab_config's members.  Survives set_mesh."""
        c = _slab_config(options)
        self._chk(self.L.nxs_dyn_slab_configure(self.h, C.byref(c)))

    def slab_put(self, **rows):
        """conc_upd, pond_volume, del_vi_tend, freeze_days, freeze_onset, conc_summer, thick_summer, fyi_fraction, age_det, age: [Ne] each; a row left out or None
        keeps the device copy."""
        s = _abi.SlabState()
        keep = self._element_rows(s, _abi.SLAB_STATE, rows, "nxs_dyn_slab_state")
        self._chk(self.L.nxs_dyn_slab_put(self.h, C.byref(s)))
        del keep

    def slab_get(self, names=_abi.SLAB_STATE_GET) -> dict:
        """The named rows of nxs_dyn_slab_state from the device (nxs_dyn_slab_get_state), time_relaxation_damage among them."""
        out = {k: np.empty(self.lm.num_elements) for k in names}
        s = _abi.SlabState()
        self._element_rows(s, _abi.SLAB_STATE_GET, out, "nxs_dyn_slab_state")
        self._chk(self.L.nxs_dyn_slab_get_state(self.h, C.byref(s)))
        return out

    def slab(self, dt: int, clock: dict):
        """nxs_dyn_slab: one launch; dt is thermo()'s integer argument, clock the five flags of slab_clock().  The ice state, the slab ocean, the ice temperatures
        and the tracers are updated on the device.  Asynchronous."""
        k = _abi.SlabClock()
        for name, v in clock.items():
            if name not in _abi.SLAB_CLOCK:
                raise KeyError(f"nxs_dyn_slab_clock has no member {name!r}")
            setattr(k, name, int(bool(v)))
        self._chk(self.L.nxs_dyn_slab(self.h, int(dt), C.byref(k)))

    def slab_coupled_configure(self, melt_type: int):
        """nxs_dyn_slab_coupled_configure: the melt type (1, 2, 3) of slab_coupled(), on top of slab_configure().  Survives set_mesh."""
        self._chk(self.L.nxs_dyn_slab_coupled_configure(self.h, int(melt_type)))

    def slab_coupled(self, dt: int, clock: dict):
        """nxs_dyn_slab_coupled: slab() as a wave-coupled build compiles it, on the attached floe-size bins (put_coupled, fsd_put): melt_type 3, the FSD branches
        of the limit block, redistributeThermoFSD, the in-loop welding and the mechanical healing.  Two launches; everything else as slab()."""
        k = _abi.SlabClock()
        for name, v in clock.items():
            if name not in _abi.SLAB_CLOCK:
                raise KeyError(f"nxs_dyn_slab_clock has no member {name!r}")
            setattr(k, name, int(v))
        self._chk(self.L.nxs_dyn_slab_coupled(self.h, int(dt), C.byref(k)))

    def slab_coupled_info(self) -> dict:
        """nxs_dyn_slab_coupled_info: thermo_fsd_crash, the debug_fsd conditions of redistributeThermoFSD since the last call (cleared by it)."""
        i = _abi.SlabCoupledInfo()
        self._chk(self.L.nxs_dyn_slab_coupled_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in _abi.SlabCoupledInfo._fields_}

    def slab_rows(self, names=_abi.SLAB_ROWS, want_device: bool = False):
        """The named rows of _abi.SLAB_ROWS as host arrays (nxs_dyn_slab_get); with want_device also {name: device pointer} of all 29 rows."""
        out = {k: np.empty(self.lm.num_elements) for k in names}
        r = _abi.SlabRows()
        for k, v in out.items():
            r.row[_abi.SLAB_ROWS.index(k)] = _abi.dptr(v)
        dev = (C.c_void_p * _abi.NXS_SLAB_ROWS)()
        self._chk(self.L.nxs_dyn_slab_get(self.h, C.byref(r), dev if want_device else None))
        if want_device:
            return out, dict(zip(_abi.SLAB_ROWS, (int(p or 0) for p in dev)))
        return out

    def get_state(self) -> dict:
        Nn, Ne = self.lm.num_nodes, self.lm.num_elements
        out = {k: np.empty(2 * Nn) for k in _abi.STATE_NODAL}
        out.update({k: np.empty(Ne) for k in _abi.STATE_ELEMENT})
        s = _abi.State()
        for k in _abi.STATE_NODAL:
            setattr(s, k, _abi.dptr(out[k]))
        for k in _abi.STATE_ELEMENT:
            if k.startswith("sigma"):
                s.sigma[int(k[-1])] = _abi.dptr(out[k])
            else:
                setattr(s, k, _abi.dptr(out[k]))
        self._chk(self.L.nxs_dyn_get_state(self.h, C.byref(s)))
        return out

    def get_diag(self) -> dict:
        Nn, Ne = self.lm.num_nodes, self.lm.num_elements
        out = {"surface": np.empty(Ne), "delta_x": np.empty(Ne), "D_tau_a": np.empty(2 * Nn),
               "D_tau_w": np.empty(2 * Nn), "D_del_ci_ridge_myi": np.empty(Ne)}
        d = _abi.Diag()
        for k, v in out.items():
            setattr(d, k, _abi.dptr(v))
        self._chk(self.L.nxs_dyn_get_diag(self.h, C.byref(d)))
        return out

    def updateIceDiagnostics(self, want_host: bool = True):
        """updateIceDiagnostics() (FE.cpp:7860-7905) on the device-resident state.  Returns (dict of host arrays or None, device pointer of the
        [Ne][6] interleaved rows D_conc, D_thick, D_snow_thick, D_sigma0, D_sigma1, D_divergence -- what interp.InterpFromMeshToGridx_device samples)."""
        Ne = self.lm.num_elements
        out, d = None, None
        if want_host:
            out = {k: np.empty(Ne) for k in _abi.ICE_DIAG}
            d = _abi.IceDiag()
            for k in _abi.ICE_DIAG:
                setattr(d, k, _abi.dptr(out[k]))
        dev = C.c_void_p()
        self._chk(self.L.nxs_dyn_ice_diagnostics(self.h, C.byref(d) if d is not None else None, C.byref(dev)))
        return out, dev.value

    # ---- regrid: interpFields() + assignVariables() (FE.cpp:3071-3154, 553-572) without the state leaving the device ----
    def regrid(self, lm_new, previous_numbering, n_geom_vertices, inputs, extras=(), context=None, moved=None, freezingpoint_mu=0.055, validate=True):
        """nxs_dyn_regrid: the prognostic state moves onto the adapted mesh `lm_new` on the device -- collectVariables, the conservative remapping,
        redistributeVariables (bounds, no_old_ice, the young-ice cap), the six nodal columns, M_UM = M_UT = 0 -- and the handle goes on with lm_new.
        inputs: cohesion, time_relaxation_damage, drag_ui, drag_ui_young of the new mesh.  extras / context / moved: see regrid_args; host 'new' arrays of
        the extras are filled in place.  Forcing is the next set_forcing.  Returns nxs_dyn_regrid_info as a dict."""
        a, keep, _ = regrid_args(lm_new, previous_numbering, n_geom_vertices, inputs, extras, context, moved,
                                 None if self.lm is None else self.lm.num_nodes, None if self.lm is None else self.lm.num_elements, freezingpoint_mu, validate)
        info = _abi.RegridInfo()
        self._chk(self.L.nxs_dyn_regrid(self.h, C.byref(a), C.byref(info)))
        del keep
        self.lm = lm_new
        return {k: getattr(info, k) for k, _ in _abi.RegridInfo._fields_ if k != "reserved0"}

    def regrid_carry_thermo(self, carry: bool = True, drag_ice_t: float = 0.0013):
        """nxs_dyn_regrid_carry_thermo: from now on regrid() carries every row of flux_put / column_put / slab_put that is present on the old mesh (the columns of
        REGRID_THERMO_COLUMNS) and re-makes drag_ti = drag_ti_young = drag_ice_t, pond_fraction = 0; only the forcing is given again on the new mesh.  Survives
        set_mesh; carry=False restores the default (every thermodynamic row missing after a regrid)."""
        o = _abi.RegridThermo(int(bool(carry)), 0, float(drag_ice_t))
        self._chk(self.L.nxs_dyn_regrid_carry_thermo(self.h, C.byref(o)))

    def regrid_thermo_info(self) -> dict:
        """nxs_dyn_regrid_thermo_info_get: what the last regrid() did -- the bit masks flux_carried / col_carried / slab_carried / flux_remade (bit k: row k of
        _abi.FLUX_STATE / COL_STATE / SLAB_STATE), the same as tuples of row names under *_names, nb_var_element, tiled."""
        i = _abi.RegridThermoInfo()
        self._chk(self.L.nxs_dyn_regrid_thermo_info_get(self.h, C.byref(i)))
        out = {k: getattr(i, k) for k, _ in _abi.RegridThermoInfo._fields_}
        for k, rows in (("flux_carried", _abi.FLUX_STATE), ("col_carried", _abi.COL_STATE), ("slab_carried", _abi.SLAB_STATE), ("flux_remade", _abi.FLUX_STATE)):
            out[k + "_names"] = tuple(name for b, name in enumerate(rows) if out[k] & (1 << b))
        return out

    # ---- the Moorings time means: updateMeans / updateGridMean / resetMeshMean (FE.cpp:8518-9024, gridoutput.cpp:387-550) ----
    @staticmethod
    def _means_list(variables, first, last):
        """[(name or id, mask)] or [name or id] -> (ids, masks) as int32 / uint8 arrays"""
        ids, masks = [], []
        for v in variables or ():
            name, mask = v if isinstance(v, (tuple, list)) else (v, False)
            ids.append((_abi.MEANS_FSD_ID[name] if name in _abi.MEANS_FSD_ID else _abi.MEANS_ID[name]) if isinstance(name, str) else int(name))
            masks.append(1 if mask else 0)
        return np.asarray(ids, np.int32), np.asarray(masks, np.uint8)

    def means_configure(self, elemental=(), nodal=()):
        """The output variables of the Moorings (GridOutput's M_elemental_variables / M_nodal_variables): names of _abi.MEANS_ELEMENTAL and MEANS_THERMO (the
        elemental list takes both, mixed) / MEANS_NODAL (or NXS_MEANS_* numbers), each optionally as (name, mask) for Variable::mask.  Two empty lists switch the
        feature off.  Survives set_mesh.  A thermodynamic variable reads the row fluxes() / column() / slab() left on the handle: means_update refuses while it is
        missing."""
        c, keep = self._means_config(elemental, nodal)
        self._chk(self.L.nxs_dyn_means_configure(self.h, C.byref(c)))
        self._means_n = (int(keep[0].size), int(keep[2].size))

    def _means_config(self, elemental, nodal):
        ei, em = self._means_list(elemental, 0, len(_abi.MEANS_ELEMENTAL))
        ni, nm = self._means_list(nodal, _abi.NXS_MEANS_NODAL_BEGIN, _abi.NXS_MEANS_NODAL_BEGIN + len(_abi.MEANS_NODAL))
        c = _abi.MeansConfig()
        c.num_elemental, c.num_nodal = ei.size, ni.size
        if ei.size:
            c.elemental_ids, c.elemental_mask = _abi.iptr(ei), _abi.bptr(em)
        if ni.size:
            c.nodal_ids, c.nodal_mask = _abi.iptr(ni), _abi.bptr(nm)
        return c, (ei, em, ni, nm)

    def means_set_tau_ow(self, tau_ow):
        """D_tau_ow ([Ne], written by the thermodynamics): the input of taux / tauy / taumod that is not the handle's.  None detaches it."""
        if tau_ow is None:
            self._chk(self.L.nxs_dyn_means_set_tau_ow(self.h, None))
            return
        a = np.ascontiguousarray(tau_ow, np.float64)
        if a.shape != (self.lm.num_elements,):
            raise ValueError(f"tau_ow has shape {a.shape}, expected ({self.lm.num_elements},)")
        self._chk(self.L.nxs_dyn_means_set_tau_ow(self.h, _abi.dptr(a)))

    def means_update(self, time_factor: float):
        """updateMeans(means, time_factor) on the device-resident state; asynchronous on the handle's stream."""
        self._chk(self.L.nxs_dyn_means_update(self.h, float(time_factor)))

    def means_get(self, want_host: bool = True):
        """(elemental [Ne, n_el] or None, nodal [Nn, n_nod] or None, device pointer of the elemental rows, of the nodal rows)."""
        n_el, n_nod = getattr(self, "_means_n", (0, 0))
        el = np.empty((self.lm.num_elements, n_el)) if want_host and n_el else None
        nod = np.empty((self.lm.num_nodes, n_nod)) if want_host and n_nod else None
        de, dn = C.c_void_p(), C.c_void_p()
        self._chk(self.L.nxs_dyn_means_get(self.h, _abi.dptr(el) if el is not None else None, _abi.dptr(nod) if nod is not None else None,
                                           C.byref(de), C.byref(dn)))
        return el, nod, de.value, dn.value

    def means_to_grid(self, xmin, ymax, mooring_spacing, ncols, nrows, miss_val=-1e14, grid_elemental=None, grid_nodal=None):
        """updateGridMean() on the regular grid: samples the accumulators and ADDS them to grid_elemental [n_el, ncols * nrows] / grid_nodal
        [n_nod, ncols * nrows] (made of zeros when None); returns the two arrays (None for an empty list)."""
        n_el, n_nod = getattr(self, "_means_n", (0, 0))
        G = int(ncols) * int(nrows)
        if grid_elemental is None and n_el:
            grid_elemental = np.zeros((n_el, G))
        if grid_nodal is None and n_nod:
            grid_nodal = np.zeros((n_nod, G))
        for a, n in ((grid_elemental, n_el), (grid_nodal, n_nod)):
            if n and a.shape != (n, G):
                raise ValueError(f"grid array has shape {a.shape}, expected ({n}, {G})")
        g = _abi.MeansGrid(float(xmin), float(ymax), float(mooring_spacing), float(miss_val), int(ncols), int(nrows))
        self._chk(self.L.nxs_dyn_means_to_grid(self.h, C.byref(g), _abi.dptr(grid_elemental) if n_el else None, _abi.dptr(grid_nodal) if n_nod else None))
        return (grid_elemental if n_el else None), (grid_nodal if n_nod else None)

    def means_to_grid_conservative(self, gridmap, miss_val=-1e14, grid_elemental=None):
        """updateGridMean()'s elemental leg on a loaded grid with conservative remapping: the accumulator rows through `gridmap` (interp.GridMap of this
        mesh) with missing value 0., ADDED to grid_elemental [n_el, G] (made of zeros when None) without transposition, then the ice-mask rule."""
        n_el = getattr(self, "_means_n", (0, 0))[0]
        G = gridmap.info()["grid_size"]
        if grid_elemental is None:
            grid_elemental = np.zeros((max(n_el, 1), G))
        if n_el and (grid_elemental.shape != (n_el, G) or grid_elemental.dtype != np.float64 or not grid_elemental.flags.c_contiguous):
            raise ValueError(f"grid array has shape {grid_elemental.shape}, expected a C-contiguous float64 ({n_el}, {G})")
        self._chk(self.L.nxs_dyn_means_to_grid_conservative(self.h, gridmap.h, float(miss_val), _abi.dptr(grid_elemental)))
        return grid_elemental

    def means_reset(self):
        """resetMeshMean(bamgmesh): both accumulators to zero, on the stream."""
        self._chk(self.L.nxs_dyn_means_reset(self.h))

    # ---- what the three output grids of the handle (means_points_*, means_regular_*, cpl_out_attach_grid / _put) share ----
    @staticmethod
    def _grid_pairs(p, pairs):
        """the vectorial variables of a grid descriptor: pairs of columns of the configured nodal list"""
        pairs = list(pairs)
        p.n_pairs = len(pairs)
        for k, (first, second) in enumerate(pairs[:_abi.NXS_MEANS_MAX_PAIRS]):
            p.pair_first[k], p.pair_second[k] = int(first), int(second)

    def _grid_points(self, gridX, gridY, miss_val, rotation, gridLON, gridTheta, rotation_angle, pairs):
        """(the _abi.MeansPoints of a set of points, the arrays it points into), or (None, []) without coordinates"""
        if gridX is None or np.size(gridX) == 0:
            return None, []
        x, y = np.ascontiguousarray(gridX, np.float64).ravel(), np.ascontiguousarray(gridY, np.float64).ravel()
        if x.shape != y.shape:
            raise ValueError("gridX and gridY differ in length")
        p = _abi.MeansPoints()
        p.G, p.rotation = x.size, _abi.MEANS_ROTATION[rotation] if isinstance(rotation, str) else int(rotation)
        p.gridX, p.gridY = _abi.dptr(x), _abi.dptr(y)
        keep = [x, y]
        for name, a in (("gridLON", gridLON), ("gridTheta", gridTheta)):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64).ravel()
                if a.shape != x.shape:
                    raise ValueError(f"{name} has {a.size} entries, the grid {x.size}")
                keep.append(a)
                setattr(p, name, _abi.dptr(a))
        p.rotation_angle, p.miss_val = float(rotation_angle), float(miss_val)
        self._grid_pairs(p, pairs)
        return p, keep

    def _grid_lsm(self, entry, G, lsm) -> np.ndarray:
        """setLSM of a grid of G points through `entry`: computed (lsm None) or taken over; returns it"""
        out = np.empty(G, np.int32)
        given = None if lsm is None else np.ascontiguousarray(lsm, np.int32).ravel()
        if given is not None and given.size != G:
            raise ValueError(f"lsm has {given.size} entries, the grid {G}")
        self._chk(entry(self.h, _abi.iptr(given) if given is not None else None, _abi.iptr(out)))
        return out

    def _grid_rows(self, n, G, want_host, call):
        """([n_el, G] or None, [n_nod, G] or None, the two device pointers) of a grid's accumulators: call(elemental, nodal, elemental_dev, nodal_dev) is the entry"""
        n_el, n_nod = n
        el = np.empty((n_el, G)) if want_host and n_el else None
        nod = np.empty((n_nod, G)) if want_host and n_nod else None
        de, dn = C.c_void_p(), C.c_void_p()
        self._chk(call(_abi.dptr(el) if el is not None else None, _abi.dptr(nod) if nod is not None else None, C.byref(de), C.byref(dn)))
        return el, nod, de.value, dn.value

    # ---- the Moorings means on a loaded grid: updateGridMean / setLSM / applyLSM / rotateVectors / resetGridMean (gridoutput.cpp:387-415, 470-485, 558-651) ----
    def means_points_set(self, gridX=None, gridY=None, miss_val=-1e14, rotation="none", gridLON=None, gridTheta=None, rotation_angle=0., pairs=()):
        """The loaded grid of the Moorings on the handle: projected coordinates gridX / gridY [G], the rotation mode ("none", "north_east" with gridLON in
        degrees, "grid_theta" with gridTheta in radians) with rotation_angle in radians, and the vectorial variables as pairs of columns of the configured nodal
        list.  Everything is copied; the grid, its mask and its accumulators survive set_mesh and regrid.  No coordinates (or empty ones) remove the object."""
        p, keep = self._grid_points(gridX, gridY, miss_val, rotation, gridLON, gridTheta, rotation_angle, pairs)
        self._chk(self.L.nxs_dyn_means_points_set(self.h, C.byref(p) if p is not None else None))
        self._points_G = int(p.G) if p is not None else 0

    def means_points_lsm(self, lsm=None) -> np.ndarray:
        """setLSM: computed on the handle's own mesh at rest (1 where a grid point lies in any triangle, ghosts included) or, given, uploaded.  Returns it."""
        return self._grid_lsm(self.L.nxs_dyn_means_points_lsm, getattr(self, "_points_G", 0), lsm)

    def means_points_update(self):
        """updateGridMean() on the loaded grid: one launch on the handle's stream that locates every grid point once in the mesh displaced by M_UM."""
        self._chk(self.L.nxs_dyn_means_points_update(self.h))

    def means_points_get(self, apply_lsm: bool = False, want_host: bool = True):
        """(elemental [n_el, G] or None, nodal [n_nod, G] or None, device pointer of the elemental rows, of the nodal rows); apply_lsm: applyLSM on the copy."""
        return self._grid_rows(getattr(self, "_means_n", (0, 0)), getattr(self, "_points_G", 0), want_host,
                               lambda el, nod, de, dn: self.L.nxs_dyn_means_points_get(self.h, int(bool(apply_lsm)), el, nod, de, dn))

    def means_points_reset(self):
        """resetGridMean(): the grid accumulators to zero, on the stream."""
        self._chk(self.L.nxs_dyn_means_points_reset(self.h))

    # ---- the Moorings means on the regular grid: the same five on the M_is_regular_grid branch (gridoutput.cpp:486-538, InterpFromMeshToGridx) ----
    def means_regular_set(self, xmin=0., ymax=0., mooring_spacing=0., ncols=0, nrows=0, miss_val=-1e14, rotation="none", gridLON=None, rotation_angle=0., pairs=()):
        """The regular grid of the Moorings on the handle: M_xmin, M_ymax, M_mooring_spacing, M_ncols (along x), M_nrows (along y), the rotation mode ("none", or
        "north_east" with gridLON [ncols * nrows] in degrees, in grid order) with rotation_angle in radians, and the vectorial variables as pairs of columns of the
        configured nodal list.  Everything is copied; the grid, its mask and its accumulators survive set_mesh and regrid.  ncols or nrows 0 removes the object."""
        if not ncols or not nrows:
            self._chk(self.L.nxs_dyn_means_regular_set(self.h, None))
            self._regular_G = 0
            return
        p = _abi.MeansRegular()
        p.ncols, p.nrows = int(ncols), int(nrows)
        p.xmin, p.ymax, p.mooring_spacing, p.miss_val = float(xmin), float(ymax), float(mooring_spacing), float(miss_val)
        p.rotation = _abi.MEANS_ROTATION[rotation] if isinstance(rotation, str) else int(rotation)
        if gridLON is not None:
            lon = np.ascontiguousarray(gridLON, np.float64).ravel()
            if lon.size != int(ncols) * int(nrows):
                raise ValueError(f"gridLON has {lon.size} entries, the grid {int(ncols) * int(nrows)}")
            p.gridLON = _abi.dptr(lon)
        p.rotation_angle = float(rotation_angle)
        self._grid_pairs(p, pairs)
        self._chk(self.L.nxs_dyn_means_regular_set(self.h, C.byref(p)))
        self._regular_G = int(ncols) * int(nrows)

    def means_regular_lsm(self, lsm=None) -> np.ndarray:
        """setLSM: computed on the handle's own mesh at rest (1 where any triangle, ghosts included, holds the grid point) or, given, taken over.  Returns it."""
        return self._grid_lsm(self.L.nxs_dyn_means_regular_lsm, getattr(self, "_regular_G", 0), lsm)

    def means_regular_update(self):
        """updateGridMean() on the regular grid: two launches on the handle's stream, nothing crosses to the host."""
        self._chk(self.L.nxs_dyn_means_regular_update(self.h))

    def means_regular_get(self, apply_lsm: bool = False, want_host: bool = True):
        """(elemental [n_el, ncols * nrows] or None, nodal [n_nod, ncols * nrows] or None, device pointer of the elemental rows, of the nodal rows), grid order;
        apply_lsm: applyLSM on the copy."""
        return self._grid_rows(getattr(self, "_means_n", (0, 0)), getattr(self, "_regular_G", 0), want_host,
                               lambda el, nod, de, dn: self.L.nxs_dyn_means_regular_get(self.h, int(bool(apply_lsm)), el, nod, de, dn))

    def means_regular_reset(self):
        """resetGridMean(): the grid accumulators to zero, on the stream."""
        self._chk(self.L.nxs_dyn_means_regular_reset(self.h))

    # ---- the coupler's outgoing fields: M_cpl_out, the "coupler put" of step() (FE.cpp:8226-8266) and the put in front of a regrid (FE.cpp:8012-8052) ----
    def cpl_out_configure(self, elemental=(), nodal=()):
        """The variables of M_cpl_out, a second accumulator set beside the Moorings': the names (or numbers) means_configure takes, `dmax` / `dmean` among them;
        a mask flag is refused.  Two empty lists switch the set off and free it, the attached grid included.  Survives set_mesh / regrid."""
        c, keep = self._means_config(elemental, nodal)
        self._chk(self.L.nxs_dyn_cpl_out_configure(self.h, C.byref(c)))
        self._cpl_n = (int(keep[0].size), int(keep[2].size))
        if self._cpl_n == (0, 0):
            self._cpl_map, self._cpl_G = None, 0

    def cpl_out_update(self, time_factor: float):
        """updateMeans(M_cpl_out, cpl_time_factor): the kernels of means_update on this set; asynchronous on the handle's stream."""
        self._chk(self.L.nxs_dyn_cpl_out_update(self.h, float(time_factor)))

    def cpl_out_get(self, want_host: bool = True):
        """(elemental [Ne, n_el] or None, nodal [Nn, n_nod] or None, device pointer of the elemental rows, of the nodal rows) of the mesh accumulators."""
        n_el, n_nod = getattr(self, "_cpl_n", (0, 0))
        el = np.empty((self.lm.num_elements, n_el)) if want_host and n_el else None
        nod = np.empty((self.lm.num_nodes, n_nod)) if want_host and n_nod else None
        de, dn = C.c_void_p(), C.c_void_p()
        self._chk(self.L.nxs_dyn_cpl_out_get(self.h, _abi.dptr(el) if el is not None else None, _abi.dptr(nod) if nod is not None else None, C.byref(de), C.byref(dn)))
        return el, nod, de.value, dn.value

    def cpl_out_reset(self):
        """resetMeshMean(bamgmesh) of M_cpl_out: both mesh accumulators to zero, on the stream."""
        self._chk(self.L.nxs_dyn_cpl_out_reset(self.h))

    def cpl_out_attach_grid(self, gridmap, gridX=None, gridY=None, miss_val=-1e14, rotation="none", gridLON=None, gridTheta=None, rotation_angle=0., pairs=()):
        """The exchange grid of M_cpl_out: `gridmap` is the interp.GridMap of THIS mesh (borrowed: keep it alive; dropped by set_mesh / regrid, attach the new one
        again), the P-points with their rotation and pairs as means_points_set takes them (needed only with nodal variables).  The grid accumulators survive
        set_mesh / regrid and a new attach on a grid of the same size."""
        p, keep = self._grid_points(gridX, gridY, miss_val, rotation, gridLON, gridTheta, rotation_angle, pairs)
        self._chk(self.L.nxs_dyn_cpl_out_attach_grid(self.h, gridmap.h if gridmap is not None else None, C.byref(p) if p is not None else None))
        self._cpl_map, self._cpl_G = gridmap, gridmap.info()["grid_size"]

    def cpl_out_put(self, want_host: bool = True, reset: bool = False):
        """M_cpl_out.updateGridMean() on the handle's stream: (grid_elemental [n_el, G] or None, grid_nodal [n_nod, G] or None, device pointer of the elemental
        grid rows, of the nodal ones).  want_host False: asynchronous, nothing is copied.  reset: resetMeshMean + resetGridMean behind the copies."""
        return self._grid_rows(getattr(self, "_cpl_n", (0, 0)), getattr(self, "_cpl_G", 0), want_host,
                               lambda el, nod, de, dn: self.L.nxs_dyn_cpl_out_put(self.h, el, nod, de, dn, _abi.NXS_CPL_OUT_RESET if reset else 0))

    def cpl_out_reset_grid(self):
        """resetGridMean() of M_cpl_out: the grid accumulators to zero, on the stream."""
        self._chk(self.L.nxs_dyn_cpl_out_reset_grid(self.h))

    def fsd_diag_configure(self, dmax_c_threshold=0.1, fsd_unbroken_floe_size=1000., fsd_min_floe_size=10.):
        """The three options of D_dmax / D_dmean (wave_coupling.dmax_c_threshold, fsd_unbroken_floe_size, fsd_min_floe_size; the defaults of options.cpp:510-518):
        what the means `dmax` / `dmean` of either set read beside fsd_configure's bin limits and centres."""
        self._chk(self.L.nxs_dyn_fsd_diag_configure(self.h, float(dmax_c_threshold), float(fsd_unbroken_floe_size), float(fsd_min_floe_size)))

    # ---- the drifters: checkMoveDrifters / checkUpdateDrifters (FE.cpp:8375-8437), Drifters::move / updateConc / maskXY (drifters.cpp:468-579) ----
    @staticmethod
    def _bbox(bbox):
        if bbox is None:
            return None, None
        b = np.ascontiguousarray(bbox, np.float64)
        if b.shape != (4,):
            raise ValueError("bbox is xmin, xmax, ymin, ymax")
        return b, _abi.dptr(b)

    def drifters_set(self, set: int, x, y, id):
        """Replace drifter set `set` (0 .. NXS_DRIFTER_SETS - 1) by the positions x, y and ids (M_X, M_Y, M_i); empty arrays make an empty set."""
        x = np.ascontiguousarray(x, np.float64); y = np.ascontiguousarray(y, np.float64); id = np.ascontiguousarray(id, np.int32)
        if not (x.ndim == y.ndim == id.ndim == 1 and x.size == y.size == id.size):
            raise ValueError("x, y and id must be vectors of one length")
        self._chk(self.L.nxs_dyn_drifters_set(self.h, int(set), int(x.size), _abi.dptr(x), _abi.dptr(y), _abi.iptr(id)))

    def drifters_clear(self, set: int):
        self._chk(self.L.nxs_dyn_drifters_clear(self.h, int(set)))

    def drifters_mesh_bbox(self, displaced: bool = False) -> np.ndarray:
        """xmin, xmax, ymin, ymax of this handle's nodes (displaced by M_UM when asked): several ranks reduce it with min / max and pass the result as `bbox`."""
        out = np.empty(4)
        self._chk(self.L.nxs_dyn_drifters_mesh_bbox(self.h, int(bool(displaced)), _abi.dptr(out)))
        return out

    def drifters_move(self, bbox=None):
        """checkMoveDrifters(): every set moved by M_UT interpolated in the undisplaced mesh, then M_UT = 0; nothing at all without a set.  Asynchronous."""
        keep, ptr = self._bbox(bbox)
        self._chk(self.L.nxs_dyn_drifters_move(self.h, ptr))

    def drifters_conc(self, set: int, bbox=None, want_host: bool = True):
        """Drifters::updateConc on the mesh displaced by M_UM; returns the concentrations (None when want_host is False: they stay in the set)."""
        keep, ptr = self._bbox(bbox)
        out = None
        if want_host:
            out = np.empty(self.drifters_count(set))
        self._chk(self.L.nxs_dyn_drifters_conc(self.h, int(set), ptr, _abi.dptr(out) if out is not None else None))
        return out

    def drifters_mask(self, set: int, conc_lim: float, keepers=None) -> int:
        """Drifters::maskXY: keeps the drifters with conc > conc_lim whose id is among `keepers` (None: every id), in their order; returns how many are left."""
        left = C.c_int32(-1)
        k = None if keepers is None else np.ascontiguousarray(keepers, np.int32)
        self._chk(self.L.nxs_dyn_drifters_mask(self.h, int(set), float(conc_lim), _abi.iptr(k) if k is not None else None, 0 if k is None else int(k.size), C.byref(left)))
        return left.value

    def drifters_count(self, set: int) -> int:
        n = C.c_int32(-1)
        self._chk(self.L.nxs_dyn_drifters_get(self.h, int(set), C.byref(n), None, None, None, None, None))
        return n.value

    def drifters_get(self, set: int) -> dict:
        """The set as it is now: x, y, id, conc, found (0 = in no triangle at the last move / conc, 1 = in an owned element, 2 = in a ghost element)."""
        n = self.drifters_count(set)
        out = {"x": np.empty(n), "y": np.empty(n), "id": np.empty(n, np.int32), "conc": np.empty(n), "found": np.empty(n, np.int32)}
        m = C.c_int32(-1)
        self._chk(self.L.nxs_dyn_drifters_get(self.h, int(set), C.byref(m), _abi.dptr(out["x"]), _abi.dptr(out["y"]), _abi.iptr(out["id"]), _abi.dptr(out["conc"]),
                                              _abi.iptr(out["found"])))
        assert m.value == n
        return out

    def drifters_update(self, set: int, conc_lim: float, keepers=None, bbox=None) -> int:
        """updateConc + maskXY, as Drifters::updateDrifters chains them at an output time; returns how many drifters are left."""
        self.drifters_conc(set, bbox, want_host=False)
        return self.drifters_mask(set, conc_lim, keepers)

    def branch_trace(self) -> dict:
        """The record option "trace_branches" keeps (include/nxs_dyn.h): {'hash', 'damage_substeps', 'flags', 'substeps'}."""
        t = np.zeros((self.lm.num_elements, 4), np.uint64)
        self._chk(self.L.nxs_dyn_get_branch_trace(self.h, t.ctypes.data_as(C.POINTER(C.c_uint64)), t.size))
        return {"hash": t[:, 0], "damage_substeps": t[:, 1], "flags": t[:, 2], "substeps": t[:, 3]}

    def debug_array(self, name: str) -> np.ndarray:
        Nn, Ne = self.lm.num_nodes, self.lm.num_elements
        n = {"rlmass": Nn, "node_mass": Nn, "C_bu": Nn, "grad_ssh": 2 * Nn, "fcor": Nn, "VTM": 2 * Nn,
             "shape": 6 * Ne, "emass": Ne, "ecbu": Ne, "force": 6 * Ne, "volume": Ne, "expC": Ne,
             "erec": 6 * Ne, "nrec": 10 * Nn, "xy": 2 * Nn, "delta_x": Ne, "surface": Ne, "tau_a": 2 * Nn, "drag_ui": Ne, "drag_ui_young": Ne, "slab_branches": Ne, "slab_fsd_branches": Ne,
             "means_update_ms": 2, "means_points_ms": 2, "means_regular_ms": 2, "slab_coupled_ms": 2, "drifters_ms": 4, "phase_times": 8 * 8192, "phase_times_prep": 8 * 8192, "shape_range": 1, "guard_launch": 2, "update_launch": 3, "diffuse_table": 3 * Ne}[name]
        out = np.empty(n)
        self._chk(self.L.nxs_dyn_debug_array(self.h, name.encode(), _abi.dptr(out), n))
        return out

    # ---- the reference's call surface ----
    def step(self):
        """FE.cpp:8197-8214: UM_P = M_UM; explicitSolve(); update(UM_P) (or free drift / no motion)."""
        self._chk(self.L.nxs_dyn_step(self.h))

    def explicitSolve(self):
        self._chk(self.L.nxs_dyn_explicit_solve(self.h))

    def update(self):
        self._chk(self.L.nxs_dyn_update(self.h))

    def synchronize(self):
        self._chk(self.L.nxs_dyn_synchronize(self.h))

    def checkRegridding(self):
        ang, flip, rg = C.c_double(), C.c_int32(), C.c_int32()
        self._chk(self.L.nxs_dyn_check_regridding(self.h, C.byref(ang), C.byref(flip), C.byref(rg)))
        return ang.value, flip.value, rg.value

    def checkFieldsFast(self) -> int:
        c = C.c_int32()
        self._chk(self.L.nxs_dyn_check_fields_fast(self.h, C.byref(c)))
        return c.value

    def timing(self) -> dict:
        t = _abi.Timing()
        self._chk(self.L.nxs_dyn_get_timing(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _abi.Timing._fields_}

    def step_times(self) -> np.ndarray:
        """Device milliseconds of every step since the last "timing_reset" (nxs_dyn_get_step_times)."""
        n = C.c_int32()
        self._chk(self.L.nxs_dyn_get_step_times(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.float64)
        self._chk(self.L.nxs_dyn_get_step_times(self.h, _abi.dptr(out), n.value, C.byref(n)))
        return out[:n.value]

    KERNEL_NAMES = {0: "none", 1: "k_sigma + k_solve_move", 2: "k_substep_fused", 3: "k_substep_multi", 4: "k_substep_pair",
                    5: "k_substep_resident", 6: "k_substep_resident_big", 7: "k_substep_flow"}
    PREP_NAMES = {0: "none", 1: "k_prep_elements + k_prep_nodes (work arrays)", 2: "k_prep_elements + k_prep_nodes", 3: "k_prep_fused"}

    def traffic_model(self) -> dict:
        """Bytes per launch the kernels of the last step had to move (nxs_dyn_get_traffic_model; include/nxs_dyn.h says what each figure counts)."""
        t = _abi.Traffic()
        self._chk(self.L.nxs_dyn_get_traffic_model(self.h, C.byref(t)))
        d = {k: getattr(t, k) for k, _ in _abi.Traffic._fields_ if k != "reserved0"}
        d["substep_kernel_name"] = self.KERNEL_NAMES.get(t.substep_kernel, "?")
        d["prep_kernel_name"] = self.PREP_NAMES.get(t.prep_kernel, "?")
        return d


Dynamics = FiniteElementDynamics
