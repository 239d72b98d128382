"""A line-by-line restatement of the coupler's outgoing side (M_cpl_out, the reference's #ifdef OASIS) for include/nxs_dyn.h's nxs_dyn_cpl_out_* /
nxs_dyn_fsd_diag_configure and include/nxs_interp.h's nxs_gridmap_send_rows.  FE.cpp = model/finiteelement.cpp.

1. The put, M_cpl_out.updateGridMean(bamgmesh, M_local_nelements, M_UM) (model/gridoutput.cpp:387-415) with interpMethod::conservative:
     elemental leg   ConservativeRemappingMeshToGrid(interp_out, interp_in, nb_var, grid_size, 0., gridP, cornerX, cornerY, triangles, weights) (:473;
                     contrib/bamg/src/ConservativeRemapping.cpp:103-135): every cell 0. (the missing value the reference passes THERE), a wet cell
                     v = 0; v += in[tri * nb_var + var] * w in list order; v *= r_cell_area -- then data_grid[var][c] += interp_out[nb_var * c + var] (:545)
     nodal leg       InterpFromMeshToMesh2dx on the mesh displaced by M_UM (isdefault = true, 0.), rotateVectors, data_grid += interp_out * proc_mask (:478-485,
                     511-543): tests/means_points_ref.py, used unchanged.  No ice-mask rule: initOASIS sets no mask flag (FE.cpp:7596-7684).
   r_cell_area is restated from ConservativeRemapping.cpp:116-122, 556-645 (the corners on the clockwise tour around their mean, the shoelace sum); the elemental
   leg is pinned to the real bamg through tests/golden/bamg_grid_remap.npz, the nodal leg through tests/golden/means_points.npz (tests/test_cpl_out_ref.py).
2. The two sets: M_moorings and M_cpl_out are two GridOutput objects, each with its own data_mesh / data_grid; updateMeans(set, time_factor) adds to ONE of them
   (tests/means_ref.MeansRef per set), resetMeshMean / resetGridMean zero one of them.  TwoSets keeps that book.
3. D_dmax / D_dmean, the "FSD relative parameters" block of updateIceDiagnostics (FE.cpp:7902-7951), and their accumulation (FE.cpp:8883-8889).
Planted mistakes (tests/test_cpl_out_ref.py shows that each changes a bit): MISTAKES."""
from __future__ import annotations

import numpy as np

import means_points_ref as P
import means_ref as MR

F = np.float64
MISTAKES = ("area_before_sum", "plain_store", "no_proc_mask", "strict_threshold", "last_bin_centre")
DEFAULTS = {"dmax_c_threshold": 0.1, "fsd_unbroken_floe_size": 1000., "fsd_min_floe_size": 10.}   # options.cpp:510-518 (tests/golden/cpl_out_options.json)


# ---- 1. the put ---------------------------------------------------------------------------------------------------------------------------------------------
def _quadrant(x, y):
    return (0 if x > 0 else 1) if y > 0 else (3 if x > 0 else 2)


def _cw_less(a, b):          # ConservativeRemapping.cpp:614-645
    ka, kb = _quadrant(*a), _quadrant(*b)
    return ka < kb if ka != kb else b[0] * a[1] < b[1] * a[0]


def polygon_area(pts):
    """ConservativeRemapping.cpp:556-611 on python floats (IEEE doubles, one rounding per operation): the mean subtracted, libstdc++'s insertion sort along the
    clockwise tour, the mean added back, the shoelace sum."""
    n = len(pts)
    mx = my = 0.
    for x, y in pts:
        mx += x; my += y
    inv_n = 1. / float(n)
    mx *= inv_n; my *= inv_n
    p = [(x - mx, y - my) for x, y in pts]
    for k in range(1, n):
        moving, hole = p[k], k
        if _cw_less(moving, p[0]):
            while hole > 0:
                p[hole] = p[hole - 1]; hole -= 1
        else:
            while _cw_less(moving, p[hole - 1]):
                p[hole] = p[hole - 1]; hole -= 1
        p[hole] = moving
    p = [(x + mx, y + my) for x, y in p]
    twice = 0.
    for k in range(n):
        before = p[k - 1]
        twice += (before[0] + p[k][0]) * (before[1] - p[k][1])
    return abs(twice) * 0.5


def r_cell_area(cornerX, cornerY, cell):
    return 1. / polygon_area([(float(cornerX[cell][k]), float(cornerY[cell][k])) for k in range(4)])


def lists_of(c):
    """the lists of a golden case (or of GridMap.export()) with the corners as [G, 4]"""
    G = np.asarray(c["cornerX"]).size // 4
    return {"gridP": np.asarray(c["gridP"]), "off": np.asarray(c["off"]), "tris": np.asarray(c["tris"]), "w": np.asarray(c["w"], F),
            "cornerX": np.asarray(c["cornerX"], F).reshape(G, 4), "cornerY": np.asarray(c["cornerY"], F).reshape(G, 4), "G": G}


def send_rows(lists, data_mesh, data_grid, drop=()):
    """the elemental leg: data_mesh [nels, n_el] (the interleaved mesh accumulators), data_grid [n_el, G] added to IN PLACE.  A list may name a triangle twice."""
    gridP, off, tris, w, G = lists["gridP"], lists["off"], lists["tris"], lists["w"], lists["G"]
    data_mesh = np.asarray(data_mesh, F)
    nb_var = data_mesh.shape[1]
    with np.errstate(all="ignore"):
        interp_out = np.zeros((G, nb_var))                       # ConservativeRemapping.cpp:109-110: miss_val = 0.
        for i in range(gridP.size):
            cell = int(gridP[i])
            r = F(r_cell_area(lists["cornerX"], lists["cornerY"], cell))
            v = np.zeros(nb_var)
            for k in range(int(off[i]), int(off[i + 1])):
                term = data_mesh[int(tris[k])] * w[k]
                v = v + (term * r if "area_before_sum" in drop else term)
            if "area_before_sum" not in drop:
                v = v * r
            interp_out[cell] = v
        for nv in range(nb_var):                                 # gridoutput.cpp:545
            if "plain_store" in drop:
                data_grid[nv] = interp_out[:, nv]
            else:
                data_grid[nv] += interp_out[:, nv]
    return data_grid


def nodal_leg(gn, x, y, tri, n_owned, nod, gx, gy, pairs=(), cosang=None, sinang=None, miss_val=-1e14, drop=(), interp=P.interp):
    """gn [n_nod, G] added to IN PLACE; x, y = the DISPLACED nodes.  means_points_ref.update_grid_mean's nodal statements with no elemental list and no ice mask."""
    if "no_proc_mask" in drop:
        with np.errstate(invalid="ignore"):
            out = np.array(interp(x, y, tri, nod, gx, gy, True))
            P.rotate(out, pairs, cosang, sinang, miss_val)
            for nv in range(gn.shape[0]):
                gn[nv] += out[:, nv]
        return gn
    P.update_grid_mean(None, gn, x, y, tri, n_owned, None, nod, gx, gy, pairs, cosang, sinang, miss_val, -1, (), (), interp)
    return gn


def put(ge, gn, lists, el, x, y, tri, n_owned, nod, gx, gy, pairs=(), cosang=None, sinang=None, miss_val=-1e14, drop=()):
    """M_cpl_out.updateGridMean(): ge [n_el, G] / gn [n_nod, G] (either None for an empty list) added to IN PLACE"""
    if ge is not None:
        send_rows(lists, el, ge, drop)
    if gn is not None:
        nodal_leg(gn, x, y, tri, n_owned, nod, gx, gy, pairs, cosang, sinang, miss_val, drop)
    return ge, gn


# ---- 2. the two sets ----------------------------------------------------------------------------------------------------------------------------------------
class TwoSets:
    """M_moorings and M_cpl_out side by side: one MeansRef each (None: not configured); what is done to one leaves the other alone."""

    def __init__(self, num_nodes, num_elements, local_nelements, young_cat):
        self.shape = (num_nodes, num_elements, local_nelements, young_cat)
        self.sets = {"moorings": None, "cpl_out": None}

    def configure(self, which, elemental=(), nodal=()):
        self.sets[which] = MR.MeansRef(*self.shape, elemental, nodal) if (elemental or nodal) else None

    def update(self, which, tf, state, **kw):                    # updateMeans(set, time_factor)
        self.sets[which].update(tf, state, **kw)

    def reset(self, which):                                      # resetMeshMean(bamgmesh)
        self.sets[which].reset()

    def rows(self, which):
        s = self.sets[which]
        return (None, None) if s is None else (s.el if s.elemental else None, s.nod if s.nodal else None)


# ---- 3. D_dmax / D_dmean --------------------------------------------------------------------------------------------------------------------------------------
def fsd_diag(mech, D_conc, up, centres, dmax_c_threshold=DEFAULTS["dmax_c_threshold"], fsd_unbroken_floe_size=DEFAULTS["fsd_unbroken_floe_size"],
             fsd_min_floe_size=DEFAULTS["fsd_min_floe_size"], drop=()):
    """FE.cpp:7902-7951 element by element on python floats.  mech [nb, n] = M_conc_mech_fsd (nb == 0: no bins attached), D_conc [n].  Returns (D_dmax, D_dmean)."""
    mech = np.asarray(mech, F).reshape(-1, len(D_conc))
    nb, n = mech.shape
    D_dmax, D_dmean = np.zeros(n), np.zeros(n)
    thr, unbroken, dmin = float(dmax_c_threshold), float(fsd_unbroken_floe_size), float(fsd_min_floe_size)
    std_min = lambda a, b: b if b < a else a                      # noqa: E731  std::min / std::max as libstdc++ defines them (a NaN falls as there)
    std_max = lambda a, b: b if a < b else a                      # noqa: E731
    for i in range(n):
        dmean = dmax = 0.
        dc = float(D_conc[i])
        if nb > 0:
            if dc > 0:
                dmax = dmean = 1000.
                m = [float(v) for v in mech[:, i]]
                broken = m[nb - 1] < thr * dc if "strict_threshold" in drop else m[nb - 1] <= thr * dc
                if broken:
                    ctot_fsd = m[nb - 1]
                    for j in range(nb - 2, -1, -1):
                        ctot_fsd += m[j]
                        if ctot_fsd > thr * dc:
                            dmax = float(up[j])
                            break
                    dmean = 0.
                    for j in range(nb):
                        dmean += m[j] * float(centres[j]) / dc
                else:
                    dmax = (m[nb - 1] / dc - thr) / (1. - thr) * (unbroken - float(up[nb - 1])) + float(up[nb - 1])
                    dmax = std_min(dmax, unbroken)
                    dmean = 0.
                    for j in range(nb - 1):
                        dmean += m[j] * float(centres[j]) / dc
                    dmean += m[nb - 1] * (float(centres[nb - 1]) if "last_bin_centre" in drop else dmax) / dc
                dmax = std_min(dmax, unbroken)
                dmax = std_max(dmax, dmin)
                dmean = std_min(dmax, dmean)
                dmean = std_max(dmean, dmin)
            else:
                dmax = dmean = 0.
        D_dmax[i], D_dmean[i] = dmax, dmean
    return D_dmax, D_dmean


def fsd_means(acc_dmax, acc_dmean, D_dmax, D_dmean, n_owned, tf):
    """FE.cpp:8883-8889: data_mesh[i] += D_dmax[i] * time_factor over the owned elements"""
    acc_dmax[:n_owned] += D_dmax[:n_owned] * tf
    acc_dmean[:n_owned] += D_dmean[:n_owned] * tf
