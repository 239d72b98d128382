"""tests/cpl_out_ref.py pinned (CPU): its elemental leg to the real bamg's ConservativeRemappingMeshToGrid (tests/golden/bamg_grid_remap.npz), its nodal leg to the
real bamg's InterpFromMeshToMesh2dx chained as updateGridMean chains it (tests/golden/means_points.npz), its options to the reference's defaults, and every planted
mistake shown to change at least one bit.  No device."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import cpl_out_ref as CO  # noqa: E402
import grid_remap_ref as G  # noqa: E402
import make_means_points_golden as MG  # noqa: E402
import means_points_ref as P  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", G.CASES)
def test_the_elemental_leg_is_the_real_bamgs_on_the_wet_rows(name):
    c = G.case(name)
    lists = CO.lists_of(c)
    wet = np.zeros(lists["G"], bool)
    wet[lists["gridP"]] = True
    for nv in (1, 7):
        got = CO.send_rows(lists, c[f"m2g_in{nv}"], np.zeros((nv, lists["G"])))
        want = c[f"m2g_out{nv}"]
        assert G.same_bits(got.T[wet] + 0., want[wet] + 0.), (name, nv)          # (the += onto the zeroed accumulator makes a -0. a +0.)
        assert (want[~wet] == G.MISS).all() and not got.T[~wet].any()             # the fixture's own missing value there; the put passes 0.
        twice = CO.send_rows(lists, c[f"m2g_in{nv}"], got.copy())                # a second put without a reset adds again
        assert G.same_bits(twice, got + got)


@pytest.fixture(scope="module")
def points():
    c = MG.means_points_case()
    c["z"] = dict(np.load(os.path.join(GOLD, "means_points.npz")))
    return c


def _nodal(c, rotation, drop=()):
    nn = c["x"].size
    cs, sn = P.cos_sin(rotation, MG.ROTATION_ANGLE, c["lon"], c["theta"])
    gn = np.zeros((len(MG.NODAL), c["gx"].size))
    out = []
    for UM in (c["UM1"], c["UM2"]):
        CO.nodal_leg(gn, c["x"] + UM[:nn], c["y"] + UM[nn:], c["tri"], c["n_owned"], c["nod"], c["gx"], c["gy"], MG.PAIRS, cs, sn, MG.MISS, drop)
        out.append(gn.copy())
    return out


def test_the_nodal_leg_is_the_real_bamgs_in_the_unmasked_columns(points):
    c, z = points, points["z"]
    assert MG.ties(c) == (0, 0, 0)
    free = [k for k, m in enumerate(MG.NOD_MASK) if not m]                        # this set has no ice-mask rule: the fixture's masked columns are not its
    assert free == [0, 2, 3]
    g1, g2 = _nodal(c, "north_east")
    assert P.equal(g1[free], z["gn1"][free]) and P.equal(g2[free], z["gn2"][free])
    _, t2 = _nodal(c, "grid_theta")
    assert P.equal(t2[free], z["gn2_theta"][free])
    assert np.isnan(g2).any()                                                      # the fixture's NaN node is seen


def test_the_defaults_are_the_references():
    d = json.load(open(os.path.join(GOLD, "cpl_out_options.json")))
    assert {k: d[k] for k in CO.DEFAULTS} == CO.DEFAULTS == {"dmax_c_threshold": 0.1, "fsd_unbroken_floe_size": 1000., "fsd_min_floe_size": 10.}


def fsd_case(nb, n=40, seed=5, at=0, negative=True, D_conc=None):
    """mech [nb, n], D_conc [n], up, centres with every branch of FE.cpp:7902-7951 at the elements at .. at + 8: no ice, the last bin at, one ulp below and one ulp
    above threshold * D_conc, all broken bins empty (D_dmax keeps 1000 and is clipped), dmean > dmax, values below the minimum floe size, an unbroken share beyond
    the cap, D_conc < 0; everywhere else broken and unbroken elements alternate.  D_conc given (the state's M_conc + M_conc_young): used as it is -- it holds 0 at
    `at` and one value at at + 1 .. at + 3"""
    rng = np.random.default_rng(seed + nb)
    low = 10. + 20. * np.arange(nb)
    up, centres = low + 20., low + 10.
    given = D_conc is not None
    D_conc = np.array(D_conc, np.float64) if given else rng.uniform(0.2, 1., n)
    n = D_conc.size
    mech = rng.uniform(0., 1., (nb, n))
    mech *= D_conc / mech.sum(0)
    mech[nb - 1, ::2] *= 0.05                                    # broken: the last bin under the threshold
    k = at
    if given:
        assert D_conc[k] == 0. and D_conc[k + 1] == D_conc[k + 2] == D_conc[k + 3] and not negative
    else:
        D_conc[k] = 0.; D_conc[k + 2] = D_conc[k + 3] = D_conc[k + 1]
    mech[:, k] = 0.                                              # no ice
    thr = CO.DEFAULTS["dmax_c_threshold"]
    edge = thr * D_conc[k + 1]
    mech[nb - 1, k + 1], mech[nb - 1, k + 2], mech[nb - 1, k + 3] = edge, np.nextafter(edge, 0.), np.nextafter(edge, 1.)
    mech[:nb - 1, k + 4] = 0.; mech[nb - 1, k + 4] = 0.01 * D_conc[k + 4]    # all broken bins empty and the last one under the threshold: D_dmax stays 1000
    mech[:, k + 5] = 0.; mech[0, k + 5] = 3. * D_conc[k + 5]     # dmean > dmax
    mech[:, k + 6] = 1e-6 * D_conc[k + 6]                        # below fsd_min_floe_size
    mech[nb - 1, k + 7] = 5. * D_conc[k + 7]                     # unbroken beyond the cap
    if negative:
        D_conc[k + 8] = -0.1                                     # D_conc < 0: the else branch
    return mech, D_conc, up, centres


@pytest.mark.parametrize("nb", [1, 2, 12, 16])
def test_dmax_dmean_branches_and_bounds(nb):
    mech, D_conc, up, centres = fsd_case(nb)
    dmax, dmean = CO.fsd_diag(mech, D_conc, up, centres)
    ice = D_conc > 0
    assert not dmax[~ice].any() and not dmean[~ice].any()
    assert (dmax[ice] >= 10.).all() and (dmax[ice] <= 1000.).all() and (dmean[ice] >= 10.).all() and (dmean[ice] <= dmax[ice]).all()
    assert dmax[4] == 1000. and dmean[6] == 10.
    z0, z1 = CO.fsd_diag(np.zeros((0, D_conc.size)), D_conc, up, centres)          # M_num_fsd_bins == 0
    assert not z0.any() and not z1.any()


def test_every_planted_mistake_changes_a_bit(points):
    c = G.case("coarse")
    lists = CO.lists_of(c)
    seeded = np.full((7, lists["G"]), 0.25)
    right = CO.send_rows(lists, c["m2g_in7"], seeded.copy())
    for m in ("area_before_sum", "plain_store"):
        assert not G.same_bits(CO.send_rows(lists, c["m2g_in7"], seeded.copy(), drop=(m,)), right), m
    assert not P.equal(_nodal(points, "north_east", drop=("no_proc_mask",))[1], _nodal(points, "north_east")[1])
    mech, D_conc, up, centres = fsd_case(12)
    right = CO.fsd_diag(mech, D_conc, up, centres)
    for m in ("strict_threshold", "last_bin_centre"):
        wrong = CO.fsd_diag(mech, D_conc, up, centres, drop=(m,))
        assert not (G.same_bits(wrong[0], right[0]) and G.same_bits(wrong[1], right[1])), m
    assert set(CO.MISTAKES) == {"area_before_sum", "plain_store", "no_proc_mask", "strict_threshold", "last_bin_centre"}
