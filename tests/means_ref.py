"""numpy restatement of FiniteElement::updateMeans (model/finiteelement.cpp:8518-9024, "FE.cpp" below) for the variables nxs_dyn_means_* covers, and of
GridOutput::updateGridMean's transposition, proc mask and ice mask on the regular grid (model/gridoutput.cpp:387-550).

Every statement is `data_mesh[i] += field[i] * time_factor`: a rounded product and a rounded sum in fp64, which is what numpy does element by element,
so the device's accumulators can be compared with these bit for bit.  Only hypot (taux, tauy, taumod: FE.cpp:8980, 8996) goes through a math library.

Inputs are the host's vectors: the state members of nxs_dyn_get_state, the side outputs of nxs_dyn_get_diag (surface, D_tau_a, D_tau_w,
D_del_ci_ridge_myi), the six vectors of nxs_dyn_ice_diagnostics, M_wind, M_tau_wi, D_tau_ow, M_drag_ui, M_drag_ui_young.
"""
import numpy as np

ELEMENTAL = ("conc", "thick", "snow", "conc_cons", "damage", "ridge_ratio", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi",
             "dci_ridge_myi", "sigma_11", "sigma_22", "sigma_12", "sigma_n", "sigma_s", "divergence", "drag_ui", "ice_mask")
NODAL = ("VT_x", "VT_y", "wind_x", "wind_y", "tau_ax", "tau_ay", "tauwix", "tauwiy", "taux", "tauy", "taumod")
LIBM = ("taux", "tauy", "taumod")          # the variables with a hypot inside


def stress_gather(nec, tau_ow, surface, conc):
    """FE.cpp:9000-9016: per node, sums over j = 0 .. NodalElementConnectivitySize[1] - 1 in that order of D_tau_ow * M_surface, M_conc * M_surface and
    M_surface, entries with elt_num = NodalElementConnectivity - 1 < 0 skipped (NaN padding converts to a negative int), then the two quotients.
    nec: [Nn, W] doubles, 1-based, as bamg leaves the table."""
    Nn, W = nec.shape
    tau_a = np.zeros(Nn); c = np.zeros(Nn); s = np.zeros(Nn)
    for j in range(W):
        col = nec[:, j]
        ok = ~np.isnan(col)
        elt = np.where(ok, col, 0.).astype(np.int64) - 1
        ok &= elt >= 0
        e = elt[ok]
        tau_a[ok] += tau_ow[e] * surface[e]
        c[ok] += conc[e] * surface[e]
        s[ok] += surface[e]
    with np.errstate(invalid="ignore", divide="ignore"):
        return tau_a / s, c / s


class MeansRef:
    """The mesh accumulators of a GridOutput: el [Ne, n_el], nod [Nn, n_nod], columns in the order of the two lists."""

    def __init__(self, num_nodes, num_elements, local_nelements, young_cat, elemental=(), nodal=(), nec=None):
        self.Nn, self.Ne, self.Neo, self.young = num_nodes, num_elements, local_nelements, bool(young_cat)
        self.elemental, self.nodal, self.nec = tuple(elemental), tuple(nodal), nec
        self.reset()

    def reset(self):                       # resetMeshMean
        self.el = np.zeros((self.Ne, len(self.elemental)))
        self.nod = np.zeros((self.Nn, len(self.nodal)))
        self.nod_terms = np.zeros((self.Nn, len(self.nodal)))   # taux / tauy / taumod: sum over the calls of (|tau_i conc| + |tau_a wind2 (1 - conc)|) time_factor

    def update(self, tf, state, diag=None, ice_diag=None, wind=None, tau_wi=None, tau_ow=None, drag_ui=None, drag_ui_young=None):
        n, Nn = self.Neo, self.Nn          # FE.cpp:8527: i < M_local_nelements -- ghost rows are never touched
        s = {k: (v[:n] if v.shape[0] == self.Ne else v) for k, v in state.items()}
        with np.errstate(invalid="ignore", divide="ignore"):
            for k, name in enumerate(self.elemental):
                acc = self.el[:n, k]
                if name == "conc": acc += ice_diag["D_conc"][:n] * tf                     # FE.cpp:8526
                elif name == "thick": acc += ice_diag["D_thick"][:n] * tf                 # :8531
                elif name == "snow": acc += ice_diag["D_snow_thick"][:n] * tf             # :8546
                elif name == "conc_cons": acc += s["conc"] * tf                           # :8586
                elif name in ("damage", "ridge_ratio", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi"):
                    acc += s[name] * tf                                                   # :8536, 8541, 8581, 8591, 8596, 8632, 8636
                elif name == "dci_ridge_myi": acc += diag["D_del_ci_ridge_myi"][:n] * tf  # :8660
                elif name in ("sigma_11", "sigma_22", "sigma_12"):
                    acc += s["sigma" + str(("sigma_11", "sigma_22", "sigma_12").index(name))] * tf   # :8682-8693
                elif name == "sigma_n": acc += ice_diag["D_sigma0"][:n] * tf              # :8741
                elif name == "sigma_s": acc += ice_diag["D_sigma1"][:n] * tf              # :8746
                elif name == "divergence": acc += ice_diag["D_divergence"][:n] * tf       # :8751
                elif name == "drag_ui":                                                   # :8756-8766
                    drag = drag_ui[:n]
                    if self.young:
                        drag = (drag_ui[:n] * s["conc"] + drag_ui_young[:n] * s["conc_young"]) / (s["conc"] + s["conc_young"])
                    acc += drag * tf
                elif name == "ice_mask":                                                  # :8912-8920 -- no time_factor
                    h = s["thick"] + s["h_young"] if self.young else s["thick"]
                    acc += np.where(h > 0., 1., 0.)
                else:
                    raise KeyError(name)
            gather = None
            for k, name in enumerate(self.nodal):
                acc = self.nod[:, k]                                                      # :8932: i < M_num_nodes, ghosts included
                if name == "VT_x": acc += state["VT"][:Nn] * tf
                elif name == "VT_y": acc += state["VT"][Nn:] * tf
                elif name == "wind_x": acc += wind[:Nn] * tf
                elif name == "wind_y": acc += wind[Nn:] * tf
                elif name == "tau_ax": acc += diag["D_tau_a"][:Nn] * tf
                elif name == "tau_ay": acc += diag["D_tau_a"][Nn:] * tf
                elif name == "tauwix": acc += tau_wi[:Nn] * tf
                elif name == "tauwiy": acc += tau_wi[Nn:] * tf
                elif name in LIBM:                                                        # :8974-9020
                    wind2 = np.hypot(wind[:Nn], wind[Nn:])
                    if name == "taux": tau_i = diag["D_tau_w"][:Nn]; wind2 = wind2 * wind[:Nn]
                    elif name == "tauy": tau_i = diag["D_tau_w"][Nn:]; wind2 = wind2 * wind[Nn:]
                    else: tau_i = np.hypot(diag["D_tau_w"][:Nn], diag["D_tau_w"][Nn:]); wind2 = wind2 * wind2
                    if gather is None:
                        gather = stress_gather(self.nec, tau_ow, diag["surface"], state["conc"])
                    tau_a, conc = gather
                    acc += (tau_i * conc + tau_a * wind2 * (1. - conc)) * tf
                    self.nod_terms[:, k] += (np.abs(tau_i * conc) + np.abs(tau_a * wind2 * (1. - conc))) * tf
                else:
                    raise KeyError(name)


def grid_mean(sample, n_elemental, n_nodal, local_proc_column, el_rows, nod_rows, ncols, nrows, miss_val, ice_mask_col, el_mask, nod_mask,
              grid_el=None, grid_nod=None):
    """GridOutput::updateGridMean on the regular grid (gridoutput.cpp:387-415, 517-537).  sample(rows) -> [ncols, nrows, nvar]: InterpFromMeshToGridx with
    M_ncols "lines" along x, M_nrows along y and default value 0 (:496-504) on the displaced mesh.  Adds into grid_el [n_el, ncols * nrows] and
    grid_nod [n_nod, ncols * nrows] (zeros when None) and returns them."""
    G = ncols * nrows
    grid_el = np.zeros((n_elemental, G)) if grid_el is None else grid_el
    grid_nod = np.zeros((n_nodal, G)) if grid_nod is None else grid_nod

    def transposed(a):                      # bamg_ind = i * nrows + j  ->  grid_ind = i + ncols * j  (:526-537)
        return np.ascontiguousarray(a.reshape(ncols, nrows).T).ravel()
    pm = None
    if n_nodal:                             # setProcMask (:360-378): 0 + interp_out
        pm = np.zeros(G) + transposed(sample(local_proc_column[:, None])[..., 0])
    if n_elemental:
        out = sample(el_rows)
        for nv in range(n_elemental):
            grid_el[nv] += transposed(out[..., nv])
    if n_nodal:
        out = sample(nod_rows)
        for nv in range(n_nodal):
            grid_nod[nv] += transposed(out[..., nv]) * pm
    if ice_mask_col is not None and ice_mask_col >= 0:   # :404-414: nodal variables first, then the elemental ones in their order
        for nv in range(n_nodal):
            if nod_mask[nv]:
                grid_nod[nv][(grid_el[ice_mask_col] <= 0.) & (grid_nod[nv] != miss_val)] = 0.
        for nv in range(n_elemental):
            if el_mask[nv]:
                grid_el[nv][(grid_el[ice_mask_col] <= 0.) & (grid_el[nv] != miss_val)] = 0.
    return grid_el, grid_nod
