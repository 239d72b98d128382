"""The host references of tests/krylov_ref.py, checked on their own (no GPU): what tests/test_gpu_krylov_edges.py holds the
Krylov kernels against has to be right first, and the meshes have to have the shapes those tests are there for."""
from fractions import Fraction

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import krylov_ref as R
from test_krylov import unit_square


def _row_lengths(tri, n):
    A, _ = R.p1_poisson(tri, np.zeros(n) + np.arange(n), np.arange(n) ** 2.0, np.zeros(n), np.ones(tri.shape[0]), eliminate=False)
    return np.diff(A.indptr)


def test_p1_poisson_is_symmetric_with_zero_row_sums_before_the_dirichlet_step():
    tri, x, y, bnd, _, _ = R.hub_mesh()
    for mesh in ((tri, x, y, bnd), R.rect_grid(7, 15), R.fan_mesh(70)):
        t, xx, yy, d = mesh
        A, b = R.p1_poisson(t, xx, yy, d, np.ones(t.shape[0]), eliminate=False)
        assert abs(A - A.T).max() == 0.0
        assert np.all(np.abs(np.asarray(A.sum(1)).ravel()) <= 1e-12 * A.diagonal())
        assert np.all(A.diagonal() > 0) and np.all(b > 0)
        xs, ys = xx[t - 1], yy[t - 1]
        area = 0.5 * np.abs((xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (xs[:, 2] - xs[:, 0]) * (ys[:, 1] - ys[:, 0]))
        assert abs(b.sum() - area.sum()) <= 1e-13 * area.sum()          # f = 1: the load is the area
        # after it: identity rows and columns on the flagged nodes, the rest untouched
        E, be = R.p1_poisson(t, xx, yy, d, np.ones(t.shape[0]))
        dn = np.flatnonzero(d)
        assert np.all(be[dn] == 0) and abs(E - E.T).max() == 0.0
        assert np.array_equal(E[dn].toarray(), np.eye(xx.size)[dn])
        free = np.flatnonzero(d == 0)
        assert np.array_equal(E[free][:, free].toarray(), A[free][:, free].toarray()) and np.array_equal(be[free], b[free])


def test_p1_poisson_reproduces_the_known_answer():
    tri, x, y, bnd = unit_square(32)
    xb = x[tri - 1].mean(1); yb = y[tri - 1].mean(1)
    f = 2 * np.pi ** 2 * np.sin(np.pi * xb) * np.sin(np.pi * yb)
    A, b = R.p1_poisson(tri, x, y, bnd, f)
    u = spla.spsolve(A.tocsc(), b)
    assert np.abs(u - np.sin(np.pi * x) * np.sin(np.pi * y)).max() < 5e-3
    t2, x2, y2, b2 = R.rect_grid(32, 32)
    assert np.array_equal(t2, tri) and np.array_equal(x2, x) and np.array_equal(y2, y) and np.array_equal(b2, bnd)


def test_p1_poisson_keeps_an_unreferenced_node_as_an_explicit_row():
    tri, x, y, bnd = R.rect_grid(8, 8)
    x = np.append(x, 2.0); y = np.append(y, 2.0)
    A, b = R.p1_poisson(tri, x, y, np.append(bnd, 1), np.ones(tri.shape[0]))
    assert A[81, 81] == 1.0 and b[81] == 0.0 and A[81].nnz == 1
    A, b = R.p1_poisson(tri, x, y, np.append(bnd, 0), np.ones(tri.shape[0]))
    assert A[81, 81] == 0.0 and A.indptr[82] - A.indptr[81] == 1


def test_sell_order_matvec_is_the_sequential_row_loop_bit_for_bit():
    for n in (1, 64, 65):
        rp, ci, va = R.ragged_matrix(n, seed=11)
        cnt = np.diff(rp)
        assert cnt.min() >= 1 and cnt.max() <= min(n, 40)
        x = np.random.default_rng(n).normal(size=n)
        seq = np.zeros(n)
        for r in range(n):
            cols = ci[rp[r]:rp[r + 1]]
            assert np.unique(cols).size == cols.size and r in cols
            acc = 0.0
            for q in range(rp[r], rp[r + 1]):
                acc += va[q] * x[ci[q]]
            seq[r] = acc
        assert np.array_equal(R.sell_order_matvec(rp, ci, va, x), seq)
    rp, ci, va = R.ragged_matrix(4097, seed=3)
    assert np.any(np.diff(ci[rp[5]:rp[6]]) < 0) or np.any(np.diff(ci[rp[6]:rp[7]]) < 0) or np.any(np.diff(ci[rp[7]:rp[8]]) < 0)   # shuffled
    x = np.random.default_rng(0).normal(size=4097)
    A = sp.csr_matrix((va, ci, rp), shape=(4097, 4097))
    assert np.abs(R.sell_order_matvec(rp, ci, va, x) - A @ x).max() <= 1e-13 * np.abs(A @ x).max()


def test_first_iterations_match_a_hand_computation_on_a_2x2_system():
    # A = [[4, 1], [1, 3]], b = (1, 2), in rationals
    F = Fraction
    a = [[F(4), F(1)], [F(1), F(3)]]; b = [F(1), F(2)]
    mv = lambda v: [a[0][0] * v[0] + a[0][1] * v[1], a[1][0] * v[0] + a[1][1] * v[1]]   # noqa: E731
    dot = lambda p, q: p[0] * q[0] + p[1] * q[1]                                          # noqa: E731
    z = [b[0] / 4, b[1] / 3]
    q = mv(z)
    alpha = dot(b, z) / dot(z, q)
    assert alpha == F(19, 23)
    x1 = [alpha * z[0], alpha * z[1]]; r1 = [b[0] - alpha * q[0], b[1] - alpha * q[1]]
    A = sp.csr_matrix(np.array([[4.0, 1.0], [1.0, 3.0]]))
    got = R.cg_first_iteration(A, np.array([1.0, 2.0]))
    assert abs(got["alpha"] - 19 / 23) <= 2e-16
    assert np.abs(got["x1"] - np.array([float(v) for v in x1])).max() <= 2e-16
    assert abs(got["rel_residual"] - float(dot(r1, r1) / dot(b, b)) ** 0.5) <= 4e-16
    assert 0 < got["rel_alpha"] < 1e-15 and got["rel_residual_err"] < 1e-14
    # BiCGStab: y = D^-1 b, v = A y, alpha = (b,b)/(b,v), s = b - alpha v, z = D^-1 s, t = A z, omega = (t,s)/(t,t)
    v = mv(z)
    alpha = dot(b, b) / dot(b, v)
    s = [b[0] - alpha * v[0], b[1] - alpha * v[1]]
    zz = [s[0] / 4, s[1] / 3]
    t = mv(zz)
    omega = dot(t, s) / dot(t, t)
    x1 = [alpha * z[0] + omega * zz[0], alpha * z[1] + omega * zz[1]]
    r1 = [s[0] - omega * t[0], s[1] - omega * t[1]]
    got = R.bicgstab_first_iteration(A, np.array([1.0, 2.0]))
    assert abs(got["alpha"] - float(alpha)) <= 4e-16 and abs(got["omega"] - float(omega)) <= 1e-14 * abs(float(omega))
    assert np.abs(got["x1"] - np.array([float(v) for v in x1])).max() <= 1e-15
    assert abs(got["rel_residual"] - float(dot(r1, r1) / dot(b, b)) ** 0.5) <= 1e-15
    assert np.all(got["x1_err"] < 1e-13)


def test_the_bound_holds_for_another_order_and_a_lost_row_breaks_it():
    """numpy's pairwise sums are one more summation order: they must sit inside the bound; a dot that loses ONE row (or, at
    the largest size, the rows of one block) must sit far outside."""
    for n, lost in ((4097, 1), (524288 + 321, 256)):
        A, b = R.pentadiagonal(n, seed=n)
        ref = R.cg_first_iteration(A, b)
        assert all(s == abs(v) for v, s in ref["dots"].values())             # positive terms throughout
        z = b / A.diagonal()
        q = A @ z
        alpha = np.sum(b * z) / np.sum(z * q)
        assert abs(alpha - ref["alpha"]) <= ref["rel_alpha"] * ref["alpha"]
        r1 = b - alpha * q
        assert abs(np.sqrt(np.sum(r1 * r1) / np.sum(b * b)) - ref["rel_residual"]) <= ref["rel_residual_err"]
        assert ref["rel_residual_err"] <= 100 * R.gamma(n + 1) * ref["rel_residual"]
        for name in ("rz", "pAp"):
            t = (b * z) if name == "rz" else (z * q)
            hole = np.sum(t) - np.sum(t[1000:1000 + lost])
            moved = abs(hole / ref["dots"][name][0] - 1.0)
            assert moved > 1e3 * ref["rel_alpha"], (n, name, moved, ref["rel_alpha"])
        bi = R.bicgstab_first_iteration(A, b)
        assert np.isfinite(bi["rel_omega"]) and bi["rel_omega"] <= 1e3 * R.gamma(n + 1)
        assert bi["rel_residual_err"] <= 1e4 * R.gamma(n + 1) * bi["rel_residual"]
        for name in ("ts", "tt", "rhat_v"):
            v, s = bi["dots"][name]
            assert abs(v) >= 0.2 * s                                           # no dot lives on cancellation: a lost block shows
    assert 1.0e-10 < R.cg_first_iteration(*R.pentadiagonal(524288 + 321, seed=524288 + 321))["rel_alpha"] < 1.3e-10


def test_bicgstab_reference_where_the_first_half_step_solves_the_system():
    A, b = R.pentadiagonal(1, seed=1)
    got = R.bicgstab_first_iteration(A, b)
    assert np.abs(got["x1"] - b / A.diagonal()).max() <= 2e-16 and np.all(got["x1_err"] <= 1e-15)
    assert got["rel_residual"] <= 1e-15 and got["rel_residual_err"] <= 1e-7   # (sqrt of a sum at round-off level)


def test_meshes_have_the_shapes_the_gpu_tests_are_there_for():
    tri, x, y, bnd, hubs, sizes = R.hub_mesh()
    n = x.size
    assert 1100 <= n <= 1500 and tri.min() == 1 and tri.max() == n and np.unique(tri).size == n
    assert len(sizes) == 3 and all(14 <= k <= 20 for k in sizes)
    rows = _row_lengths(tri, n)
    assert sorted(rows[hubs] - 1) == sorted(sizes)                               # valence = ring size
    # the element loop of the assembly: one round per patch in the mesh as numbered, a second round once it is shuffled
    assert R.elements_per_patch(tri, n).max() <= 512
    ts, xs, ys, bs, perm = R.permute_nodes(tri, x, y, bnd, seed=5)
    assert R.elements_per_patch(ts, n).max() > 512
    assert np.array_equal(xs[perm], x) and np.array_equal(bs[perm], bnd) and np.array_equal(xs[ts - 1], x[tri - 1])
    # elements_per_patch against the plain count
    want = np.zeros((n + 127) // 128, int)
    for e in ts - 1:
        for p in set(e // 128):
            want[p] += 1
    assert np.array_equal(R.elements_per_patch(ts, n), want)
    # the grids: Nn <= 64 (one slice) and Nn % 128 in {1, 64, 65, 127}
    sizes = {(6, 6): 49, (7, 7): 64, (4, 12): 65, (8, 8): 81, (10, 10): 121, (7, 15): 128, (2, 42): 129}
    for (nx, ny), nn in sizes.items():
        t, xx, yy, d = R.rect_grid(nx, ny)
        assert xx.size == nn and np.unique(t).size == nn and d.sum() < nn
    t, xx, yy, d = R.drop_last_node(*R.rect_grid(7, 15))
    assert xx.size == 127 and np.unique(t).size == 127 and t.shape[0] == 2 * 7 * 15 - 2
    # the fans.  Valence 70: more than 64 element colours, but slices 71, 6 and 5 wide stay far below 64 KiB of LDS
    t, xx, yy, d = R.fan_mesh(70)
    rows = _row_lengths(t, xx.size)
    assert xx.size == 141 and rows[0] == 71 and rows[1:].max() <= 7 and d[0] == 0 and d.sum() == 70
    assert np.array_equal(rows, R.row_lengths(t, xx.size))
    assert R.patch_lds_bytes(t, xx.size) == 8 * (64 * 71 + 64 * 6 + 128) < 64 * 1024
    # valence 130: one slice of 64 x 131 doubles, past the 64 KiB a launch gets unasked, within the 160 KiB of a workgroup
    t, xx, yy, d = R.fan_mesh(130)
    rows = _row_lengths(t, xx.size)
    assert rows[0] == 131 and rows[1:].max() <= 7 and np.array_equal(rows, R.row_lengths(t, xx.size))
    assert 64 * 1024 < R.patch_lds_bytes(t, xx.size) == 8 * (64 * 131 + 64 * 6 + 128) <= 160 * 1024
    # two hubs of valence 160, one in each slice of the first patch: past 160 KiB, yet within the 256 colours and 65535 entries
    t, xx, yy, d = R.two_fans(160)
    rows = _row_lengths(t, xx.size)
    assert rows[0] == 161 and rows[64] == 161 and np.sort(rows)[-3] <= 4 and np.unique(t).size == xx.size == 322
    assert R.patch_lds_bytes(t, xx.size) == 8 * (2 * 64 * 161 + 128) > 160 * 1024 and 2 * 64 * 161 <= 0xFFFF
    assert np.array_equal(R.row_lengths(np.array([[1, 2, 3]]), 4), [3, 3, 3, 1])
