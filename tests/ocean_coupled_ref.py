"""A line-by-line restatement of what a coupled ocean (OceanType::COUPLED, the reference's #ifdef OASIS) adds to a step, for include/nxs_dyn.h's
nxs_dyn_ocean_coupled_* and include/nxs_interp.h's nxs_gridmap_receive_rows.  FE.cpp = model/finiteelement.cpp.

1. The receive of the element fields, ExternalData::check_and_reload for ocean_cpl_elements / wave_cpl_elements:
     receiveCouplingData (externaldata.cpp:461-514)         t = f_v[c]; t *= a_v; t += b_v, every cell of the field (reduced_nodes_ind is empty)
     interpolateDataset  (externaldata.cpp:1291-1493)       the variables interleaved [G][nb_var], ConservativeRemappingGridToMesh
                         (contrib/bamg/src/ConservativeRemapping.cpp:138-171): from 0, += in * w in the order of the scatter over (cell row, position),
                         triangle_area summed alongside, times 1. / triangle_area -- 0 * (1 / 0.), a NaN, on a triangle no wet cell touches
     ExternalData::get   (externaldata.cpp:434, 438)        M_factor * interpolated_data[0][i] + M_bias_correction, always evaluated
2. The three guarded sites of thermo().  Where the coupled loop is the same statement sequence the restatements of tests/fluxes_ref.py, column_ref.py,
   slab_ref.py and slab_fsd_ref.py are used UNCHANGED:
     FE.cpp:5149-5157   Qow = Qlw + Qsh + Qlh; Qow += Qsw * M_qsrml                                           qow()
     FE.cpp:5348-5358   Qdw = Fdw = 0, M_sst = M_ocean_temp, M_sss = M_ocean_salt before iceOceanHeatflux     column(): column_ref.column as the CONSTANT
                        column with Qdw_const = Fdw_const = 0 on the reset rows
     FE.cpp:5826-5841   M_sst, M_sss not advanced; FE.cpp:5859 Tbot = freezingPoint(M_sss) sees the received salinity   slab(), slab_coupled(): the loops of
                        slab_ref.slab / slab_fsd_ref.slab_coupled with exactly the three statements below restated (the source of the unchanged function with
                        those lines replaced; every replacement is asserted to match once, so a change of the restatement cannot slip by)
Planted mistakes (tests/test_ocean_coupled_ref.py shows that each changes a bit): MISTAKES.  Like the restatements it stands on, its parity with a binary of the
reference is NOT pinned (model/ cannot be compiled here); the receive is pinned to the real bamg through tests/golden/bamg_grid_remap.npz."""
from __future__ import annotations

import inspect
import re

import numpy as np

import column_ref as CR
import slab_fsd_ref as SFR
import slab_ref as SR

F = np.float64
ROWS = ("ocean_temp", "ocean_salt", "qsrml", "mld", "wlbk")          # NXS_OC_*
MISTAKES = ("qsw_kept", "reset_after_qio", "tbot_advanced", "transform_after", "no_get")


# ---- 1. the receive ---------------------------------------------------------------------------------------------------------------------------------------
def receive(lists, fields, a, b, factor, bias, drop=()):
    """lists: gridP [rows], off [rows + 1], tris, w [entries], nels (GridMap.export(), or a golden case); fields: n_var arrays [G].  Returns [n_var, nels]."""
    gridP, off, tris, w, nels = lists["gridP"], lists["off"], lists["tris"], lists["w"], int(lists["nels"])
    nb_var = len(fields)
    co = [np.broadcast_to(np.asarray(v, F), (nb_var,)) for v in (a, b, factor, bias)]
    G = np.asarray(fields[0]).size
    with np.errstate(all="ignore"):
        # receiveCouplingData: one get_2d per variable, then per cell t = f; t *= a; t += b -- into the interleaved [G][nb_var] array interpolateDataset hands on
        data_in = np.empty((G, nb_var))
        for v in range(nb_var):
            t = np.array(fields[v], F).ravel()
            if "transform_after" not in drop:
                t = t * co[0][v]
                t = t + co[1][v]
            data_in[:, v] = t
        # ConservativeRemappingGridToMesh, ConservativeRemapping.cpp:145-170
        interp_out = np.zeros((nels, nb_var))
        triangle_area = np.zeros(nels)
        for i in range(gridP.size):
            cell = int(gridP[i])
            for k in range(int(off[i]), int(off[i + 1])):
                tr = int(tris[k])
                triangle_area[tr] = triangle_area[tr] + w[k]
                interp_out[tr, :] = interp_out[tr, :] + data_in[cell, :] * w[k]
        r_triangle_area = F(1.) / triangle_area
        interp_out = interp_out * r_triangle_area[:, None]
        out = np.empty((nb_var, nels))
        for v in range(nb_var):
            x = interp_out[:, v]
            if "transform_after" in drop:
                x = x * co[0][v]
                x = x + co[1][v]
            out[v] = x if "no_get" in drop else co[2][v] * x + co[3][v]          # ExternalData::get, externaldata.cpp:434, 438
    return out


def interleaved(fields, a, b):
    """the array nxs_gridmap_grid_to_mesh takes for the same receive: [G][n_var], transformed"""
    co = [np.broadcast_to(np.asarray(v, F), (len(fields),)) for v in (a, b)]
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.stack([np.array(f, F).ravel() * co[0][v] + co[1][v] for v, f in enumerate(fields)], axis=1))


def lists_of(case):
    """the lists of a golden case of tests/grid_remap_ref.py in the shape receive() takes"""
    return {"gridP": case["gridP"], "off": case["off"], "tris": case["tris"], "w": case["w"], "nels": case["tri"].shape[0]}


def awkward_fields(G, n_var, seed=11):
    """n_var fields [G] with a -0., a NaN cell and an Inf cell among them, and coefficients with a = 2, b != 0, factor != 1, bias != 0"""
    rng = np.random.default_rng(seed)
    fields = [rng.standard_normal(G) * (10. ** (v - 1)) for v in range(n_var)]
    fields[0][0] = -0.
    if G > 2:
        fields[0][G // 2] = np.nan
        fields[n_var - 1][G - 1] = np.inf
    a = np.array([1., 2., 1., 0.5, 2.][:n_var])
    b = np.array([0., 0.25, -273.15, 0., 1e-3][:n_var])
    factor = np.array([1., 1., 0.01, 3., 1.][:n_var])
    bias = np.array([0., -1.5, 0., 0.125, 0.][:n_var])
    return fields, a, b, factor, bias


# ---- 2. the three guarded sites ---------------------------------------------------------------------------------------------------------------------------
def qow(flux_rows, qsrml, drop=()):
    """FE.cpp:5149-5157 from the rows OWBulkFluxes made: Qow = Qlw + Qsh + Qlh, then += Qsw * M_qsrml"""
    Qow = flux_rows["Qlw_ow"] + flux_rows["Qsh_ow"] + flux_rows["Qlh_ow"]
    if "qsw_kept" in drop:
        return Qow + flux_rows["Qsw_ow"]
    return Qow + flux_rows["Qsw_ow"] * qsrml


def column(inp, cfg, tri, young, dt, drop=()):
    """thermo(), FE.cpp:5306-5411 under OceanType::COUPLED: inp["sst"], inp["sss"] are reset to inp["ocean_temp"], inp["ocean_salt"] IN PLACE before
    iceOceanHeatflux and freezingPoint read them; then the CONSTANT column with Qdw_const = Fdw_const = 0.  cfg["freezingpoint_type"] must be "unesco"
    (FE.cpp:1244-1248)."""
    assert cfg["freezingpoint_type"] == "unesco", "FE.cpp:1246: a coupled ocean forces FreezingPointType::UNESCO"
    c = dict(cfg, ocean_type="constant", Qdw_const=0., Fdw_const=0.)
    if "reset_after_qio" not in drop:
        inp["sst"], inp["sss"] = inp["ocean_temp"].copy(), inp["ocean_salt"].copy()      # FE.cpp:5355-5356
    rows, rec = CR.column(inp, c, tri, young, dt)
    if "reset_after_qio" in drop:
        inp["sst"], inp["sss"] = inp["ocean_temp"].copy(), inp["ocean_salt"].copy()
    return rows, rec


_GUARDS = (
    # FE.cpp:5826-5829: the heat flux into the slab ocean is not applied
    (r"M_sst = M_sst - ddt \* \(Qio_mean \+ Qow_mean - Qdw \+ Qassm\) / \(rhow \* cpw \* mld\)", "pass"),
    # FE.cpp:5838-5841: delsss is computed (it feeds D_delS, FE.cpp:5930) and not added
    (r"M_sss = M_sss \+ delsss", "M_sss_advanced = M_sss + delsss"),
    # FE.cpp:5859: freezingPoint(M_sss) therefore sees the received salinity
    (r"Tbot = F\(CR\.freezing_point\(ccfg, M_sss\)\)", 'Tbot = F(CR.freezing_point(ccfg, M_sss_advanced if "tbot_advanced" in drop else M_sss))'),
)


def _coupled_loop(module, name):
    src = inspect.getsource(getattr(module, name))
    for pat, new in _GUARDS:
        src, n = re.subn(r"(?m)^(\s*)" + pat + r"\s*$", lambda m: m.group(1) + new, src)
        assert n == 1, (name, pat, n)
    ns = dict(vars(module))
    exec(compile(src, f"<{module.__name__}.{name} under OceanType::COUPLED>", "exec"), ns)
    return ns[name]


slab = _coupled_loop(SR, "slab")                     # slab_ref.slab's arguments; inp["sst"], inp["sss"] come back unchanged
slab_coupled = _coupled_loop(SFR, "slab_coupled")    # slab_fsd_ref.slab_coupled's arguments


# ---- designed inputs ----------------------------------------------------------------------------------------------------------------------------------------
def received_rows(inp, seed=23):
    """ocean_temp / ocean_salt distinct from inp's sst / sss on every element (within 0.2 K and 1 %: the strata of the designed inputs keep their side of si), qsrml in
    (0, 1), mld, wlbk"""
    rng = np.random.default_rng(seed)
    Ne = inp["sst"].size
    d = rng.uniform(0.02, 0.2, Ne) * np.where(rng.random(Ne) < 0.5, -1., 1.)
    out = {"ocean_temp": inp["sst"] + d, "ocean_salt": inp["sss"] * (1. + rng.uniform(1e-3, 1e-2, Ne) * np.where(rng.random(Ne) < 0.5, -1., 1.)),
           "qsrml": rng.uniform(0.05, 0.95, Ne), "mld": rng.uniform(5., 40., Ne), "wlbk": rng.uniform(0., 300., Ne)}
    assert (out["ocean_temp"] != inp["sst"]).all() and (out["ocean_salt"] != inp["sss"]).all()
    return {k: np.ascontiguousarray(v, F) for k, v in out.items()}
