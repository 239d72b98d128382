"""Host reference of nxs_dyn_regrid: the part of FiniteElement::interpFields + assignVariables that lies between the member vectors and the two
interpolation routines, in plain numpy float64, written from the reference's lines and in their operand order:

  collect       collectVariables          FE.cpp:2120-2151 (column order: sortPrognosticVars, FE.cpp:2087-2111)
  redistribute  redistributeVariables     FE.cpp:2196-2258 (apply_maxima = true)
  nodes         gatherFieldsNode          FE.cpp:3174-3198
  scatter       scatterFieldsNode + assignVariables   FE.cpp:3280-3293, 553-561

Every operation is one IEEE multiply, divide, square root, max or min on doubles, so the device is expected to give the same bits.  The two interpolations of
`chain` are passed in: the repository's own (pinned bit for bit to the real bamg by tests/test_remap.py and tests/test_interp.py) or the real bamg's."""
import numpy as np

NONE, CONC, THICK, ENTHALPY = range(4)
KINDS = {"none": NONE, "conc": CONC, "thick": THICK, "enthalpy": ENTHALPY}
# physical::si, Lf, C (model/constants.hpp:68, 44, 17)
SI, LF, HEAT_C = 5., 333.55e3, 2100.

STATE_ELEMENT = ("conc", "thick", "snow_thick", "damage", "ridge_ratio", "sigma0", "sigma1", "sigma2", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi")
# minVal / maxVal of model_variable.cpp for the handle's own variables: name -> (min or None, max or None)
BOUNDS = {"conc": (0., 1.), "thick": (0., None), "snow_thick": (0., None), "damage": (0., 1. - 1e-10), "ridge_ratio": (0., 1.),
          "sigma0": (None, None), "sigma1": (None, None), "sigma2": (None, None), "conc_young": (0., 1.), "h_young": (0., None), "hs_young": (0., None),
          "conc_myi": (0., 1.), "thick_myi": (0., None), "cum_damage": (0., None), "conc_fsd": (0., 1.)}


def columns(extras=(), cum_damage=False, num_fsd_bins=0):
    """The column table after sortPrognosticVars: a list of dicts {name, kind, min, max, is_tice, extra (index into extras or None)}."""
    cols = [dict(name=k, kind=NONE, min=BOUNDS[k][0], max=BOUNDS[k][1], is_tice=False, extra=None) for k in STATE_ELEMENT]
    if cum_damage:
        cols.append(dict(name="cum_damage", kind=NONE, min=0., max=None, is_tice=False, extra=None))
    for b in range(num_fsd_bins):
        cols.append(dict(name=f"conc_fsd{b}", kind=NONE, min=0., max=1., is_tice=False, extra=None))
    for kind in (NONE, CONC, THICK, ENTHALPY):
        for i, x in enumerate(extras):
            t = x.get("transformation", "none")
            t = KINDS[t] if isinstance(t, str) else int(t)
            if t == kind:
                cols.append(dict(name=f"extra{i}", kind=kind, min=x.get("min"), max=x.get("max"), is_tice=bool(x.get("is_tice")), extra=i))
    return cols


def collect(state, cols, extras_old=(), coupled=None, mu=0.055):
    """[Ne_old, nb_var] rows.  state: the handle's element vectors; extras_old: the old values of the extras; coupled: {'cum_damage', 'conc_fsd' [bins, Ne]}."""
    Ne = state["conc"].size
    out = np.empty((Ne, len(cols)))
    M_conc, M_thick = state["conc"], state["thick"]
    for j, c in enumerate(cols):
        if c["extra"] is not None:
            val = np.array(extras_old[c["extra"]], np.float64)
        elif c["name"] == "cum_damage":
            val = coupled["cum_damage"].copy()
        elif c["name"].startswith("conc_fsd"):
            val = coupled["conc_fsd"][int(c["name"][8:])].copy()
        else:
            val = state[c["name"]].copy()
        if c["kind"] == CONC:
            val = val * M_conc                                                       # FE.cpp:2139
        elif c["kind"] == THICK:
            val = val * M_thick                                                      # FE.cpp:2142
        elif c["kind"] == ENTHALPY:
            with np.errstate(divide="ignore", invalid="ignore"):
                val = (val - mu * SI * LF / (HEAT_C * val)) * M_thick                # FE.cpp:2145
        out[:, j] = val
    return out


def _std_max(a, b):   # std::max(a, b) = (a < b) ? b : a
    return np.where(a < b, b, a)


def _std_min(a, b):   # std::min(a, b) = (b < a) ? b : a
    return np.where(b < a, b, a)


def redistribute(rows, cols, young_ice, mu=0.055):
    """The variables on the new mesh: {name: [Ne_new]} (extras as 'extra<i>').  A row the remapping left NaN stays NaN in every variable (the reference
    asserts before it gets here; the library hands the NaN to the caller)."""
    out = {}
    failed = np.isnan(rows[:, 0])
    for j, c in enumerate(cols):
        raw = rows[:, j]
        val = raw.copy()
        no_old_ice = np.zeros(raw.size, bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            if c["kind"] == CONC:                                                    # FE.cpp:2217-2223
                ok = out["conc"] > 0
                val = np.where(ok, raw / out["conc"], raw); no_old_ice = ~ok
            elif c["kind"] == THICK:                                                 # FE.cpp:2224-2230
                ok = out["thick"] > 0
                val = np.where(ok, raw / out["thick"], raw); no_old_ice = ~ok
            elif c["kind"] == ENTHALPY:                                              # FE.cpp:2231-2241
                ok = out["thick"] > 0
                enth = raw / out["thick"]
                val = np.where(ok, 0.5 * (enth - np.sqrt(enth * enth + 4 * mu * SI * LF / HEAT_C)), raw); no_old_ice = ~ok
        if c["is_tice"]:
            val = np.where(no_old_ice, -mu * SI, val)                                # FE.cpp:2243-2245
        if c["min"] is not None:
            val = _std_max(np.float64(c["min"]), val)                                # FE.cpp:2247
        if c["max"] is not None:
            val = _std_min(np.float64(c["max"]), val)                                # FE.cpp:2249
        out[c["name"]] = np.where(failed, raw, val)
    if young_ice:                                                                    # FE.cpp:2253-2256
        over = ~failed & ((out["conc"] + out["conc_young"]) > 1.)
        out["conc_young"] = np.where(over, 1. - out["conc"], out["conc_young"])
    return out


def nodes(VT, UM, UT):
    """[Nn_old, 6] = VT.u, VT.v, UM.u, UM.v, UT.u, UT.v (FE.cpp:3174-3198)."""
    Nn = VT.size // 2
    return np.column_stack([VT[:Nn], VT[Nn:], UM[:Nn], UM[Nn:], UT[:Nn], UT[Nn:]])


def scatter(nod_out):
    """M_VT from columns 0, 1 (FE.cpp:3280-3285); M_UM = M_UT = 0 (assignVariables, FE.cpp:553-560, after the unpacking of FE.cpp:3286-3292)."""
    n = nod_out.shape[0]
    return {"VT": np.concatenate([nod_out[:, 0], nod_out[:, 1]]), "UM": np.zeros(2 * n), "UT": np.zeros(2 * n)}


def chain(state, old_mesh, new_mesh, previous_numbering, n_geom, young_ice, remap, interp, extras=(), coupled=None, mu=0.055):
    """interpFields on the host.  old_mesh = (tri0 0-based, x moved, y moved), new_mesh = (tri0, x, y); remap(index_old1, xo, yo, index_new1, xn, yn, prev, ngeom, rows)
    and interp(index_old1, xo, yo, nod_rows, xn, yn) are the two interpolations.  Returns (state on the new mesh incl. VT / UM / UT, extras' new values, nb_var)."""
    to, xo, yo = old_mesh
    tn, xn, yn = new_mesh
    coupled = coupled or {}
    cols = columns(extras, "cum_damage" in coupled, coupled["conc_fsd"].shape[0] if "conc_fsd" in coupled else 0)
    rows = collect(state, cols, [x["old"] for x in extras], coupled, mu)
    rows_new = remap(to + 1, xo, yo, tn + 1, xn, yn, previous_numbering, n_geom, rows)
    out = redistribute(rows_new, cols, young_ice, mu)
    nod = interp(to + 1, xo, yo, nodes(state["VT"], state["UM"], state["UT"]), xn, yn)
    out.update(scatter(nod))
    new_extras = [out.pop(f"extra{i}") for i in range(len(extras))]
    return out, new_extras, len(cols)
