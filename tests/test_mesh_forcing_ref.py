"""tests/mesh_forcing_ref.py (the tail of loadDataset, transformData per forcing step, the column order of interpolateDataset, the gather) pinned to
tests/golden/mesh_forcing.npz, which the REAL bamg made from the restated load: both sources, node and element targets, bit for bit.  Each planted mistake changes
a bit of the result.  No device, no library."""
import numpy as np
import pytest

import mesh_forcing_ref as MF
import nodal_receive_ref as R


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(MF.GOLD))


def chain(name, kind, mistake=None):
    src = R.source(name)
    v, w = MF.weights(name, kind)
    return MF.ingest(MF.raw_fields(src["G"], src["reduced"]), src["reduced"], MF.N_VAR, MF.N_STEP, v, w, mistake=mistake, pairs=MF.PAIRS, rotate=R.uniform_rotation(), **MF.coef())


@pytest.mark.parametrize("kind", MF.KINDS)
@pytest.mark.parametrize("name", MF.SOURCES)
def test_the_restated_chain_gives_the_fixtures_bits(gold, name, kind):
    Y = gold[f"Y_{kind}_{name}"]
    got = chain(name, kind)
    assert got.shape == (6, Y.shape[0]) and R.equal(got, Y.T)


def test_the_fixture_holds_what_the_issue_asks_of_it(gold):
    nodal = np.load(R.GOLD)
    for name in MF.SOURCES:
        src = R.source(name)
        f = MF.raw_fields(src["G"], src["reduced"])
        assert f.shape == (6, 63) and not np.isinf(f).any()
        wet_nan = np.isnan(f[:, src["reduced"]])
        assert wet_nan.sum() >= 6 and wet_nan[0].any() and wet_nan[1].any() and wet_nan[2].any() and wet_nan[3:].any()      # NaN at several wet points, both steps, pair and scalar
        for kind, n in (("nodes", 1464), ("elements", 2732)):
            px, py = MF.targets(src, kind)
            Y = gold[f"Y_{kind}_{name}"]
            assert px.size == n and Y.shape == (n, 6) and np.isfinite(Y).all()
            assert R.ties(src, px, py) == 0 and R.in_fill(src, px, py).size == 0
            W = nodal["W_" + name] if kind == "nodes" else gold["Wb_" + name]
            it, _ = R.D.locate(src["x"], src["y"], src["tri"], px, py)
            nnz = (W != 0).sum(1)
            assert (it >= 0).any() and ((it < 0) & (nnz == 1)).any() and ((it < 0) & (nnz >= 2)).any()      # inside, a hull vertex's cone, beyond a hull edge
            assert (np.abs(px - src["x"].mean()) > 0.5 * np.ptp(src["x"])).any()                             # beyond the source's box
        assert np.array_equal(gold["bx_" + name], MF.targets(src, "elements")[0]) and np.array_equal(gold["by_" + name], MF.targets(src, "elements")[1])
    c = MF.coef()
    assert c["scale_factor"][2] != 1. and c["add_offset"][2] != 0. and c["a"][1] != 1. and c["b"][1] != 0. and MF.PAIRS == [(0, 1)]
    assert (c["scale_factor"][:3] != c["scale_factor"][3:]).any()      # two forcing steps, two files


@pytest.mark.parametrize("mistake", MF.MISTAKES)
def test_every_planted_mistake_changes_a_bit(gold, mistake):
    """NaN zeroed after the rotation, (d*a + b)*scale_factor + add_offset, the snapshots swapped, column index j*n_step + fstep, the rotation in the first forcing
    step only, reduced ignored"""
    name = "strip" if mistake == "reduced_ignored" else "full"      # (reduced is the identity in the full case)
    for kind in MF.KINDS:
        Y = gold[f"Y_{kind}_{name}"]
        assert R.equal(chain(name, kind), Y.T) and not R.equal(chain(name, kind, mistake), Y.T), (mistake, kind)


def test_the_load_is_four_roundings_and_nan_becomes_zero_before_the_pair_turns():
    src = R.source("strip")
    f = MF.raw_fields(src["G"], src["reduced"])
    c = MF.coef()
    plain = MF.loaded_data(f, src["reduced"], 3, 2, **c)
    assert np.isfinite(plain).all() and np.abs(plain).max() < 1e3                       # neither NaN nor the land value reaches loaded_data
    d, k = f[5][src["reduced"]], 5
    with np.errstate(invalid="ignore"):
        want = (d * c["scale_factor"][k] + c["add_offset"][k]) * c["a"][k] + c["b"][k]
    assert R.equal(plain[k], np.where(np.isnan(want), 0., want))
    i = int(np.flatnonzero(np.isnan(f[0][src["reduced"]]))[0])
    turned = MF.loaded_data(f, src["reduced"], 3, 2, pairs=MF.PAIRS, rotate=R.uniform_rotation(), **c)
    cs, sn = R.uniform_rotation()
    assert plain[0, i] == 0. and turned[0, i] == cs * 0. + sn * plain[1, i] and turned[1, i] == -sn * 0. + cs * plain[1, i]
    assert R.equal(turned[2], plain[2]) and R.equal(turned[5], plain[5]) and not R.equal(turned[3:5], plain[3:5])      # the scalars stay, BOTH steps' pairs turn
    one = MF.loaded_data(f[:3], src["reduced"], 3, 1, pairs=MF.PAIRS, rotate=R.uniform_rotation(), **MF.coef(3, 1))
    assert R.equal(one, turned[:3])                                                                                      # n_step = 1 is the first snapshot
