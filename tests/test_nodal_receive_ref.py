"""The restatement of the coupler's nodal receive (tests/nodal_receive_ref.py) pinned to tests/golden/nodal_receive.npz, which the REAL bamg made, and shown to be
sensitive: each planted mistake changes a bit.  No device, no library."""
import numpy as np
import pytest

import nodal_receive_ref as R


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLD)


def test_the_fixture_is_the_one_the_generator_describes(gold):
    for name in R.CASES:
        src = R.source(name)
        px, py = R.targets(src)
        assert np.array_equal(px, gold["px_" + name]) and np.array_equal(py, gold["py_" + name])
        assert R.ties(src, px, py) == 0                                   # the condition: no target is left out, none sits on an edge
        box = (px < src["x"].min()) | (px > src["x"].max()) | (py < src["y"].min()) | (py > src["y"].max())
        assert box.any() and (~box).any()
    assert R.source("full")["reduced"].size == 63 and np.array_equal(R.source("full")["reduced"], np.arange(63))
    strip = R.source("strip")["reduced"]
    assert strip.size == 56 and strip[0] != 0 and (np.diff(strip) > 1).any()      # a strict subset, not 0 .. R - 1
    assert np.array_equal(R.in_fill(R.source("notch"), gold["px_notch"], gold["py_notch"]), gold["fill_notch"]) and gold["fill_notch"].size > 0
    for name in ("full", "strip"):
        assert R.in_fill(R.source(name), gold["px_" + name], gold["py_" + name]).size == 0
        W = gold["W_" + name]
        nnz = (W != 0).sum(1)
        it, _ = R.D.locate(R.source(name)["x"], R.source(name)["y"], R.source(name)["tri"], gold["px_" + name], gold["py_" + name])
        assert (it >= 0).any() and ((it < 0) & (nnz == 1)).any() and ((it < 0) & (nnz >= 2)).any()      # inside, the cone of a hull vertex, beyond an edge
        assert (np.abs(W.sum(1) - 1.) < 1e-14).all()


@pytest.mark.parametrize("name", ["full", "strip"])
def test_the_restated_apply_gives_the_real_librarys_bits(gold, name):
    src = R.source(name)
    v, a = R.weights_from_dense(gold["W_" + name], src["tri"])
    assert np.array_equal(R.dense(v, a, src["x"].size).view(np.uint64), gold["W_" + name].view(np.uint64))
    d, Y = R.awkward_data(src), gold["Y_" + name]
    assert (d < 0).any() and (d == 0).all(1).any() and np.isnan(d).all(1).sum() == 1
    for k in range(2):
        assert R.equal(R.apply(v, a, d[:, k]), Y[:, k])
    assert np.isnan(Y).any() and not np.isnan(Y).all()
    # inside a triangle the weights are the integer area coordinates over their sum, as _weights.cpp:79-81 divides them
    it, dd = R.D.locate(src["x"], src["y"], src["tri"], gold["px_" + name], gold["py_" + name])
    ins = it >= 0
    assert np.array_equal(v[ins], src["tri"][it[ins]])
    assert np.array_equal(a[ins], dd[ins].astype(np.float64) / dd[ins].sum(1).astype(np.float64)[:, None])


def chain(gold, name, mistake=None, per_point=True):
    src = R.source(name)
    v, w = R.weights_from_dense(gold["W_" + name], src["tri"])
    f = R.fields_case(src["G"], 3)
    rot = R.cos_sin_theta(R.MAP_ROTATION, src["theta"]) if per_point else R.uniform_rotation()
    return R.receive(f, src["reduced"], [2., 1.5, -0.5], [0.25, -1., 0.125], v, w, [(0, 1)], rot, None, [1.5, -2., 3.], [0.5, 0.25, -1.], mistake=mistake)


@pytest.mark.parametrize("per_point", [False, True])
@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_each_planted_mistake_changes_a_bit(gold, mistake, per_point):
    good = chain(gold, "strip", None, per_point)
    assert np.isfinite(good).all() and R.equal(good, chain(gold, "strip", None, per_point))
    bad = chain(gold, "strip", mistake, per_point)
    assert not R.equal(good, bad), mistake
    if mistake in ("rotation_sign", "rotate_after_gather"):
        assert R.equal(good[2], bad[2])                                   # the scalar never sees the rotation


def test_the_order_of_the_chain(gold):
    """a, b before the rotation; the rotation before the gather; factor, bias after it: what the restatement states, spelled out once more on one target"""
    src = R.source("strip")
    v, w = R.weights_from_dense(gold["W_strip"], src["tri"])
    f = R.fields_case(src["G"], 2)
    c, s = R.uniform_rotation()
    out = R.receive(f, src["reduced"], [2., 3.], [0.5, -0.5], v, w, [(0, 1)], (c, s), None, [1.5, 2.5], [1., -1.])
    i = 17
    t0 = f[0][src["reduced"]] * 2. + 0.5
    t1 = f[1][src["reduced"]] * 3. + -0.5
    n0, n1 = c * t0 + s * t1, -s * t0 + c * t1
    x0 = w[i, 0] * n0[v[i, 0]] + w[i, 1] * n0[v[i, 1]] + w[i, 2] * n0[v[i, 2]]
    x1 = w[i, 0] * n1[v[i, 0]] + w[i, 1] * n1[v[i, 1]] + w[i, 2] * n1[v[i, 2]]
    assert out[0, i] == 1.5 * x0 + 1. and out[1, i] == 2.5 * x1 + -1.
