"""Host reference of update() (FE.cpp:3946-4131; oracle/dyn_ref.c ref_update, the kernel k_update) in plain Python float64, one element after the other, written
from the reference's lines and in their operand order -- and the table of inputs that drives every branch of it (rows(), table()).

Every operation is one IEEE add, subtract, multiply, divide or comparison on doubles and there is no libm call, so the oracle and the device are expected to
give the same BITS, NaN payloads and the sign of zero included.  min and max are the selections std::min / std::max make (STD_MIN / STD_MAX of the oracle and
of the kernels): they return their FIRST argument whenever the comparison is false, hence also when either argument is NaN -- fmin / fmax do not.

update() returns, next to the arrays, one uint64 per element with one bit per decision taken (BITS): the coverage tests of tests/test_update_ref.py ask every
bit to be set in block 0, in the ragged last block and in every displacement zone in which it can be set at all.

`mutate` plants one deliberate mistake (MUTATIONS); tests/test_update_ref.py shows that the comparison with the oracle notices each of them on the table."""
import numpy as np

DAYS_IN_SEC = 86400.
ELEMENT = ("conc", "thick", "snow_thick", "ridge_ratio", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi")     # what the table sets
SIGMA = ("sigma0", "sigma1", "sigma2")
BLOCK = 256

BITS = ("SCALED", "GATE_NEUMANN", "GATE_CONC", "MIN1_BINDS", "EQUAL_RIDGING", "MYI_CAPPED_AT_1", "MYI_BELOW_1", "OW_BELOW_0", "OW_ABOVE_1", "YOUNG_POS",
        "YOUNG_NONPOS", "YOUNG_ZEROED", "RIDGING", "FAIL_MIN_C", "FAIL_MIN_H", "FAIL_NCY", "CONC_ABOVE_1", "CONC_BELOW_0", "NCY_LIMITED", "HAS_ICE", "CAP_50",
        "ONE_MINUS_NCY_BINDS", "ICE_FREE", "ICE_FREE_LEFTOVER", "LB_CONC", "LB_THICK", "LB_THICK_MYI", "LB_SNOW", "MYI_ABOVE_BOUND", "MYI_BELOW_0",
        "MYI_BOUND_WITH_YOUNG", "NAN_IN", "NEG_ZERO_IN")
BIT = {k: np.uint64(1) << np.uint64(i) for i, k in enumerate(BITS)}
assert len(BITS) <= 64

MUTATIONS = ("min_c_ge", "min_h_ge", "ncy_le", "no_cap_50", "fmin_fmax", "myi_bound_without_young", "d_del_of_the_first_block", "neumann_one_corner")


def std_min(a, b):
    return b if b < a else a


def std_max(a, b):
    return b if a < b else a


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return b if b < a else a


def _fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return b if a < b else a


def params_of(p):
    """The members of nxs_dyn_params update() reads."""
    return dict(young=int(p.ice_cat_type) == 1, equal_ridging=int(p.equal_ridging), newice_type=int(p.newice_type),
                use_young_ice_in_myi_reset=int(p.use_young_ice_in_myi_reset), min_c=float(p.min_c), min_h=float(p.min_h), dtime_step=float(p.dtime_step))


def neumann_corners(lm):
    """[Ne, 3] bool: the corner is in M_neumann_flags (FE.cpp:3957-3961 looks the three of them up)."""
    return np.isin(lm.indices.reshape(-1, 3) - 1, lm.neumann_flags)


def surface(lm, um):
    """measure(element, mesh, UM) (FE.cpp:1929-1933) of every element: vertices = coordinates + 1. * UM, half the absolute Jacobian (FE.cpp:1613-1618)."""
    Nn = lm.num_nodes
    nd = lm.indices.reshape(-1, 3) - 1
    vx = lm.coord_x[nd] + 1. * um[nd]
    vy = lm.coord_y[nd] + 1. * um[nd + Nn]
    jac = (vx[:, 1] - vx[:, 0]) * (vy[:, 2] - vy[:, 0])
    jac = jac - (vx[:, 2] - vx[:, 0]) * (vy[:, 1] - vy[:, 0])
    return (1. / 2) * np.abs(jac), jac


def update(arr, surface_old, surface_new, corners, prm, mutate=None):
    """arr: the element vectors before update() (ELEMENT + SIGMA; not changed); surface_old: M_surface as prep left it; surface_new: measure() with the M_UM
    update() sees; corners: neumann_corners(); prm: params_of().  Returns (arrays after, D_del_ci_ridge_myi, branch mask)."""
    assert mutate is None or mutate in MUTATIONS
    Ne = surface_old.size
    out = {k: np.array(arr[k], np.float64, copy=True) for k in ELEMENT + SIGMA}
    D = np.zeros(Ne)
    branch = np.zeros(Ne, np.uint64)
    young, equal_ridging = prm["young"], prm["equal_ridging"]
    min_c, min_h = prm["min_c"], prm["min_h"]
    smin, smax = (_fmin, _fmax) if mutate == "fmin_fmax" else (std_min, std_max)
    for e in range(Ne):
        b = 0
        to_be_updated = True
        if mutate == "neumann_one_corner":
            if corners[e, 0]:
                to_be_updated = False
        elif corners[e, 0] or corners[e, 1] or corners[e, 2]:
            to_be_updated = False
        D_del = 0.
        conc, thick, snow, tmyi, cmyi = (float(out[k][e]) for k in ("conc", "thick", "snow_thick", "thick_myi", "conc_myi"))
        ridge = float(out["ridge_ratio"][e])
        cy, hy, hsy = (float(out[k][e]) for k in ("conc_young", "h_young", "hs_young"))
        s0, s1, s2 = (float(out[k][e]) for k in SIGMA)
        if any(v != v for v in (conc, thick, snow, tmyi, cmyi, ridge, cy, hy, hsy)):
            b |= int(BIT["NAN_IN"])
        if conc == 0. and np.signbit(conc):
            b |= int(BIT["NEG_ZERO_IN"])
        so, sn = float(surface_old[e]), float(surface_new[e])
        old_conc = conc
        if (conc > 0.) and to_be_updated:
            b |= int(BIT["SCALED"])
            surf_ratio = so / sn
            conc *= surf_ratio
            thick *= surf_ratio
            snow *= surf_ratio
            tmyi *= surf_ratio
            s0 *= surf_ratio; s1 *= surf_ratio; s2 *= surf_ratio
            if 1. < conc:
                b |= int(BIT["MIN1_BINDS"])
            ridge = 1. - (1. - ridge) * smin(1., conc) / (old_conc * surf_ratio)
            if young:
                hy *= surf_ratio
                cy *= surf_ratio
                hsy *= surf_ratio
            if equal_ridging:
                b |= int(BIT["EQUAL_RIDGING"])
                conc_ratio = smin(1., conc) / old_conc
                cmyi *= conc_ratio
                D_del = 0.
            else:
                cmyi *= surf_ratio
                D_del = -cmyi
                b |= int(BIT["MYI_CAPPED_AT_1"] if 1. < cmyi else BIT["MYI_BELOW_1"])
                cmyi = smin(cmyi, 1.)
                D_del += cmyi
            D_del *= DAYS_IN_SEC / prm["dtime_step"]
        else:
            b |= int(BIT["GATE_NEUMANN"] if conc > 0. else BIT["GATE_CONC"])

        ow = 1. - conc
        if young:
            ow -= cy
        if ow < 0.:
            b |= int(BIT["OW_BELOW_0"])
            ow = 0.
        if ow > 1.:
            b |= int(BIT["OW_ABOVE_1"])
            ow = 1.

        ncy = 0.
        del_c = 0.
        if young:
            if cy > 0.:
                b |= int(BIT["YOUNG_POS"])
                ncy = smin(1., smax(0., 1. - conc - ow))
                c1 = (conc >= min_c) if mutate == "min_c_ge" else (conc > min_c)
                c2 = (thick >= min_h) if mutate == "min_h_ge" else (thick > min_h)
                c3 = (ncy <= cy) if mutate == "ncy_le" else (ncy < cy)
                if c1 and c2 and c3:
                    b |= int(BIT["RIDGING"])
                    new_h_young = ncy * hy / cy
                    new_hs_young = ncy * hsy / cy
                    newice = hy - new_h_young
                    del_c = (cy - ncy) / 10.
                    newsnow = hsy - new_hs_young
                    hy = new_h_young
                    hsy = new_hs_young
                    ridge = 1. - (1. - ridge) * thick / (thick + newice)
                    thick += newice
                    snow += newsnow
                elif not c1:
                    b |= int(BIT["FAIL_MIN_C"])
                elif not c2:
                    b |= int(BIT["FAIL_MIN_H"])
                else:
                    b |= int(BIT["FAIL_NCY"])
            else:
                b |= int(BIT["YOUNG_NONPOS"])
                if hy != 0. or hsy != 0.:
                    b |= int(BIT["YOUNG_ZEROED"])
                hy = 0.
                hsy = 0.

        x = 1. - ncy - ow + del_c
        if x > 1.:
            b |= int(BIT["CONC_ABOVE_1"])
        if x < 0.:
            b |= int(BIT["CONC_BELOW_0"])
        conc = smin(1., smax(0., x))
        if young:
            if (1. - conc) < ncy:
                b |= int(BIT["NCY_LIMITED"])
            ncy = smax(0., smin(ncy, 1. - conc))
            cy = ncy

        if conc > 0.:
            b |= int(BIT["HAS_ICE"])
            test_h = thick / conc
            if test_h > 50.:
                b |= int(BIT["CAP_50"])
                if mutate != "no_cap_50":
                    test_h = 50.
            if (thick / test_h) < (1. - ncy):
                pass
            else:
                b |= int(BIT["ONE_MINUS_NCY_BINDS"])
            conc = smin(1. - ncy, thick / test_h)
        else:
            b |= int(BIT["ICE_FREE"])
            if ridge != 0. or thick != 0. or snow != 0.:
                b |= int(BIT["ICE_FREE_LEFTOVER"])
            ridge = 0.
            thick = 0.
            snow = 0.

        if not (conc > 0.) and (conc != 0. or np.signbit(conc)):
            b |= int(BIT["LB_CONC"])
        if not (thick > 0.) and (thick != 0. or np.signbit(thick)):
            b |= int(BIT["LB_THICK"])
        if not (tmyi > 0.) and (tmyi != 0. or np.signbit(tmyi)):
            b |= int(BIT["LB_THICK_MYI"])
        if not (snow > 0.) and (snow != 0. or np.signbit(snow)):
            b |= int(BIT["LB_SNOW"])
        conc = conc if conc > 0. else 0.
        thick = thick if thick > 0. else 0.
        tmyi = tmyi if tmyi > 0. else 0.
        snow = snow if snow > 0. else 0.
        if mutate == "d_del_of_the_first_block":
            D_del += -cmyi
        else:
            D_del = -cmyi
        if prm["newice_type"] == 4 and prm["use_young_ice_in_myi_reset"]:
            b |= int(BIT["MYI_BOUND_WITH_YOUNG"])
            # M_conc_young as it stands, whatever the category (FE.cpp:4126-4128): the classic one has left the array alone
            bound = conc if mutate == "myi_bound_without_young" else conc + (cy if young else float(out["conc_young"][e]))
        else:
            bound = conc
        if bound < cmyi:
            b |= int(BIT["MYI_ABOVE_BOUND"])
        if smin(cmyi, bound) < 0.:
            b |= int(BIT["MYI_BELOW_0"])
        cmyi = smax(0., smin(cmyi, bound))
        D_del += cmyi

        out["conc"][e], out["thick"][e], out["snow_thick"][e], out["thick_myi"][e], out["conc_myi"][e] = conc, thick, snow, tmyi, cmyi
        out["ridge_ratio"][e] = ridge
        if young:
            out["conc_young"][e], out["h_young"][e], out["hs_young"][e] = cy, hy, hsy
        out["sigma0"][e], out["sigma1"][e], out["sigma2"][e] = s0, s1, s2
        D[e] = D_del
        branch[e] = b
    return out, D, branch


# ---- the two displacement fields and their zones -------------------------------------------------------------------------------------------------------------

STILL, CONVERGING, DIVERGING, BETWEEN = 0, 1, 2, 3
ZONE_NAMES = ("still", "converging", "diverging")
T_STILL, T_CONV = 0.36, 0.68      # the zones along x, as fractions of the mesh's width


def displacements(lm):
    """(UM_A, UM_B).  UM_A: a smooth field of a few per cent of an edge, there when prep records M_surface.  UM_B = UM_A + (g, 0.3 g) with g a function of x alone:
    0 up to T_STILL of the width (UM_B is UM_A bit for bit there), then compressing by 7 % rising to 17 % (dg/dx = -0.07 .. -0.17: surf_ratio 1.075 .. 1.205), then
    stretching by 8 % rising to 20 % (surf_ratio 0.926 .. 0.833).  1 + dg/dx > 0 everywhere and the shear 0.3 g leaves areas alone: no triangle flips."""
    Nn = lm.num_nodes
    x, y = lm.coord_x, lm.coord_y
    L, H = np.ptp(x), np.ptp(y)
    t = (x - x.min()) / L
    s = (y - y.min()) / H
    edge = np.sqrt(L * H / lm.num_elements)
    um_a = np.concatenate([0.04 * edge * np.sin(4.1 * t + 0.3) * np.cos(3.3 * s), 0.03 * edge * np.cos(2.7 * t) * np.sin(5.2 * s + 0.4)])
    w = 1. - T_CONV
    u = np.clip(t - T_STILL, 0., T_CONV - T_STILL)
    v = np.clip(t - T_CONV, 0., None)
    g = L * (-(0.07 * u + 0.10 * u * u / (2. * (T_CONV - T_STILL))) + (0.08 * v + 0.12 * v * v / (2. * w)))
    moved = t > T_STILL
    um_b = um_a.copy()
    um_b[:Nn] = np.where(moved, um_a[:Nn] + g, um_a[:Nn])
    um_b[Nn:] = np.where(moved, um_a[Nn:] + 0.3 * g, um_a[Nn:])
    return um_a, um_b


def zones(lm, um_a, um_b):
    """(zone of every element, surface with UM_A, surface with UM_B, the two Jacobians).  still: every corner has UM_B == UM_A, bit for bit; converging /
    diverging: every corner lies in that stretch of x; BETWEEN: the triangles that straddle two stretches."""
    Nn = lm.num_nodes
    nd = lm.indices.reshape(-1, 3) - 1
    same = (um_a[:Nn].view(np.uint64) == um_b[:Nn].view(np.uint64)) & (um_a[Nn:].view(np.uint64) == um_b[Nn:].view(np.uint64))
    t = (lm.coord_x - lm.coord_x.min()) / np.ptp(lm.coord_x)
    conv = (t > T_STILL) & (t <= T_CONV)
    div = t > T_CONV
    z = np.full(nd.shape[0], BETWEEN)
    z[same[nd].all(1)] = STILL
    z[conv[nd].all(1)] = CONVERGING
    z[div[nd].all(1)] = DIVERGING
    sa, ja = surface(lm, um_a)
    sb, jb = surface(lm, um_b)
    return z, sa, sb, ja, jb


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------------------

BASE = dict(conc=0.3, thick=0.6, snow_thick=0.1, ridge_ratio=0.2, conc_young=0.1, h_young=0.02, hs_young=0.005, conc_myi=0.1, thick_myi=0.2)


NAN_SIGN = np.uint64(1) << np.uint64(63)
NAN_PAYLOAD = (np.uint64(1) << np.uint64(51)) - np.uint64(1)


def nan_with_payload(payload):
    """The quiet NaN with `payload` in its low 51 bits, as a Python float."""
    return float(np.array([0x7ff8000000000000 | int(payload)], np.uint64).view(np.float64)[0])


def rows(min_c, min_h):
    """[(name, the members that differ from BASE)].  Rows that sit exactly on a threshold only do so where nothing scales them: in the still zone."""
    up = lambda v: float(np.nextafter(v, np.inf))    # noqa: E731
    left = dict(thick=0.5, snow_thick=0.1, ridge_ratio=0.3, conc_young=0., h_young=0., hs_young=0.)     # what an ice-free element must lose
    ridging = dict(conc_young=1.2, h_young=0.3, hs_young=0.05)     # conc + conc_young > 1: new_conc_young < conc_young whatever the zone
    nan = [nan_with_payload(0x5a5a00 + k) for k in range(6)]     # a payload of its own each: a NaN that comes out is the one that went in
    return [
        # the scaling gate: (conc > 0) && to_be_updated
        ("gate conc 0", dict(left, conc=0.)), ("gate conc -0", dict(left, conc=-0.)), ("gate conc -1e-18", dict(left, conc=-1e-18)),
        ("gate conc 1e-300", dict(left, conc=1e-300)), ("base conc 0.3", {}), ("conc 1 ridge 0", dict(conc=1., thick=2., ridge_ratio=0.)),
        # the ridge ratio: STD_MIN(1, conc) binds where the zone converges (and everywhere from 1.3)
        ("conc 1 ridge 0.5", dict(conc=1., thick=2., ridge_ratio=0.5)), ("conc 1 ridge 1", dict(conc=1., thick=2., ridge_ratio=1.)),
        ("conc 1.3 ridge 0.5", dict(conc=1.3, thick=2., ridge_ratio=0.5)),
        # the multi-year concentration
        ("myi 0.2 stays below 1", dict(conc=0.9, thick=1.8, conc_myi=0.2)), ("myi 0.95 above 1 where converging", dict(conc=1., thick=2., conc_myi=0.95)),
        ("myi 1.3 above 1", dict(conc=1., thick=2., conc_myi=1.3)), ("myi above conc", dict(conc_myi=0.6)), ("myi negative", dict(conc_myi=-0.1)),
        ("myi equals conc", dict(conc_myi=0.3)), ("myi -0", dict(conc_myi=-0.)),
        # the open-water clamp
        ("conc + young above 1", dict(conc=0.8, thick=1.6, conc_young=0.5, h_young=0.1, hs_young=0.02)), ("conc negative", dict(conc=-0.2)),
        ("conc + young exactly 1", dict(conc=0.75, thick=1.5, conc_young=0.25)),
        # the young-ice ridging condition, each conjunct failing alone
        ("conc at min_c", dict(ridging, conc=min_c, thick=0.2)), ("conc one ulp above min_c", dict(ridging, conc=up(min_c), thick=0.2)),
        ("thick at min_h", dict(ridging, conc=0.5, thick=min_h)), ("thick one ulp above min_h", dict(ridging, conc=0.5, thick=up(min_h))),
        ("new young equals young", dict(conc=0.5, thick=1., conc_young=0.25, h_young=0.05)), ("thick below min_h", dict(ridging, conc=0.5, thick=min_h / 2.)),
        ("young 0 with thickness", dict(conc_young=0., h_young=0.05, hs_young=0.01)), ("young negative", dict(conc_young=-0.1, h_young=0.05)),
        ("young -0", dict(conc_young=-0., h_young=0.05)),
        # the final clamps
        ("del_c above 1 from conc 1", dict(conc=1., thick=2., conc_young=0.5, h_young=0.1, hs_young=0.02)),
        ("del_c above 1 from conc 1.3", dict(conc=1.3, thick=2., conc_young=0.5, h_young=0.1, hs_young=0.02)),
        # the 50 m cap
        ("true thickness 120", dict(conc=0.5, thick=60.)), ("true thickness 60", dict(conc=0.5, thick=30.)), ("true thickness exactly 50", dict(conc=0.5, thick=25.)),
        # the lower bounds
        ("thick negative", dict(thick=-0.5)), ("thick_myi negative", dict(thick_myi=-0.2)), ("snow negative", dict(snow_thick=-0.1)),
        # NaN, one member at a time
        ("NaN conc", dict(conc=nan[0])), ("NaN thick", dict(thick=nan[1])), ("NaN conc_young", dict(conc_young=nan[2])), ("NaN conc_myi", dict(conc_myi=nan[3])),
        ("NaN ridge_ratio", dict(ridge_ratio=nan[4])), ("NaN h_young", dict(h_young=nan[5])),
    ]


def deal(lm, zone):
    """The row of every element.  Block 0 and the ragged last block get the rows in order, element after element; the other elements get them round-robin
    within their group: the on-Neumann elements, then each zone, then the triangles between two zones."""
    Ne = lm.num_elements
    on_neumann = neumann_corners(lm).any(1)
    last = (Ne // BLOCK) * BLOCK
    group = np.where(on_neumann, 4, zone)
    e = np.arange(Ne)
    group = np.where(e < BLOCK, 5, np.where(e >= last, 6, group))
    row = np.zeros(Ne, np.int64)
    for gid in range(7):
        idx = np.flatnonzero(group == gid)
        row[idx] = np.arange(idx.size)
    return row, group


def table(lm, min_c, min_h, zone):
    """({name: [Ne]} of ELEMENT, row index of every element, the rows)."""
    R = rows(min_c, min_h)
    row, group = deal(lm, zone)
    row = row % len(R)
    cols = {k: np.array([dict(BASE, **over)[k] for _, over in R]) for k in ELEMENT}
    return {k: np.ascontiguousarray(cols[k][row]) for k in ELEMENT}, row, R


def expected_bits(prm):
    """The decisions update() can take at all with these parameters."""
    young_only = {"YOUNG_POS", "YOUNG_NONPOS", "YOUNG_ZEROED", "RIDGING", "FAIL_MIN_C", "FAIL_MIN_H", "FAIL_NCY", "CONC_ABOVE_1", "CONC_BELOW_0", "NCY_LIMITED", "OW_BELOW_0"}
    # LB_CONC cannot be taken: conc arrives at its lower bound as STD_MIN(1 - ncy, thick / test_h) with 0 <= ncy <= 1 and test_h = thick / conc of thick's sign
    # (conc > 0 there), so neither argument is negative, and a NaN second argument is not selected
    want = set(BITS) - {"LB_CONC"}
    if not prm["young"]:
        want -= young_only         # (without the young ice 1 - conc - ow is 0 or conc again: neither clamp of the final conc can bind, and ow < 0 needs conc > 1,
        want |= {"OW_BELOW_0"}     #  which the rows with conc 1.3 give)
    want -= {"MYI_CAPPED_AT_1", "MYI_BELOW_1"} if prm["equal_ridging"] else {"EQUAL_RIDGING"}
    if not (prm["newice_type"] == 4 and prm["use_young_ice_in_myi_reset"]):
        want -= {"MYI_BOUND_WITH_YOUNG"}
    return want


# the decisions that read surf_ratio, and the zones in which the table can take them (every zone, thanks to the rows with conc and conc_myi of 1.3)
RATIO_BITS = ("SCALED", "MIN1_BINDS", "EQUAL_RIDGING", "MYI_CAPPED_AT_1", "MYI_BELOW_1")


# ---- the case both test files run: the toy mesh, the two displacement fields, the table --------------------------------------------------------------------

MESH = "toy"      # the smallest mesh of tests/cases.py with on-Neumann elements (126), at least three blocks of 256 elements and a ragged last one (2368 =
#                   9 * 256 + 64); "tiny" has 84 elements, "small" (2836) is larger and has no on-Neumann element in block 0 or in its last block
COMBINATIONS = {
    "young": {},
    "young equal_ridging": {"equal_ridging": 1},
    "young newice 4 without young ice in the myi reset": {"use_young_ice_in_myi_reset": 0},
    "classic": {"ice_cat_type": 0, "newice_type": 1},
    "classic equal_ridging": {"ice_cat_type": 0, "newice_type": 1, "equal_ridging": 1},
    "classic newice 4": {"ice_cat_type": 0},      # not a configuration of the reference (FE.cpp:1212-1215 ties newice_type 4 to the young category); the line
    #                                               FE.cpp:4126-4128 reads M_conc_young whatever the category, and so do the oracle and the kernel
}


class Setup:
    """The inputs of one parameter combination: the case with M_UM = UM_A, UM_B, the zones, the surfaces of both fields and the table."""

    def __init__(self, over, substeps=1):
        import cases
        gm, p, g, lms, fields = cases.make_case(MESH, substeps=substeps, dtime_step=substeps * 200. / 120., **over)
        self.lm, self.p = lms[0], p
        self.Ne, self.Nn = self.lm.num_elements, self.lm.num_nodes
        self.um_a, self.um_b = displacements(self.lm)
        self.f = dict(fields[0], UM=self.um_a.copy())
        self.zone, self.s_a, self.s_b, self.jac_a, self.jac_b = zones(self.lm, self.um_a, self.um_b)
        self.tab, self.row, self.rows = table(self.lm, p.min_c, p.min_h, self.zone)
        self.corners = neumann_corners(self.lm)
        self.on_neumann = self.corners.any(1)
        self.prm = params_of(p)

    def row_name(self, e):
        return self.rows[self.row[e]][0]


def bits_differ(a, b, nan_sign=True):
    """The indices at which two float64 vectors differ in their bits.  nan_sign=False: where both hold a NaN its sign bit is left out of the comparison (the
    payload and the quiet bit still count) -- IEEE 754 (6.3) leaves the sign of a NaN result of an arithmetic operation open, and two processors use that."""
    ua = np.ascontiguousarray(a, np.float64).view(np.uint64)
    ub = np.ascontiguousarray(b, np.float64).view(np.uint64)
    if not nan_sign:
        both = np.isnan(a) & np.isnan(b)
        ua = np.where(both, ua & ~NAN_SIGN, ua)
        ub = np.where(both, ub & ~NAN_SIGN, ub)
    return np.flatnonzero(ua != ub)
