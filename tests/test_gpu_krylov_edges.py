"""The kernels of nextsim_amd/csrc/nxs_krylov.hip against the host references of tests/krylov_ref.py at the shapes where
they take another path: the reductions (grid_sum's ticket groups, the second stride of its last-block pass, the MAXG cap
and the grid-stride loops), the SpMV's slices, the patch assembly (second round of the element loop, hubs, a single slice,
ragged last patches, an unreferenced node, more than 64 element colours, patches past the default and past the whole LDS) and systems that converge exactly.
The dots are read through the public ABI: Solver.solve(..., max_iter=1) returns x1 and the residual of the first iteration."""
import functools

import numpy as np
import pytest
import scipy.sparse.linalg as spla

import krylov_ref as R
from nextsim_amd import krylov
from nextsim_amd.dynamics import NxsError

pytestmark = pytest.mark.gpu

BLOCK = 256
N_BLOCKS = 524288 + 321           # > MAXG * BLOCK rows and > 8192 slices: every grid-stride loop runs twice, ragged last slice
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 65793, N_BLOCKS)


@functools.lru_cache(maxsize=None)
def _system(n):
    A, b = R.pentadiagonal(n, seed=n)
    A.data.flags.writeable = False; b.flags.writeable = False
    return A, b


@functools.lru_cache(maxsize=None)
def _first_iteration(n, method):
    A, b = _system(n)
    return R.cg_first_iteration(A, b) if method == krylov.CG else R.bicgstab_first_iteration(A, b)


@pytest.mark.parametrize("method", [krylov.CG, krylov.BICGSTAB], ids=["cg", "bicgstab"])
@pytest.mark.parametrize("n", SIZES)
def test_first_iteration_pins_every_dot(n, method):
    """x1 carries alpha = (b,z)/(p,Ap) (CG: k_cg_init, k_spmv_sell<1>) resp. alpha and omega (BiCGStab: k_bicg_init,
    k_spmv_sell<1>, k_spmv_sell<2>), the returned residual carries (r1,r1)/(b,b) (k_cg_xr resp. k_bicg_x): each within the
    bound derived in tests/krylov_ref.py ("the bound on |device - this reference|") -- 1.2e-10 relative for alpha at the
    largest size, where one lost row is 2e-6 and one lost block 5e-4."""
    A, b = _system(n)
    ref = _first_iteration(n, method)
    s = krylov.Solver()
    try:
        s.set_matrix(A.indptr, A.indices, A.data)
        x1, info = s.solve(b, method=method, rtol=1e-30, max_iter=1)
    finally:
        s.close()
    assert info["iterations"] == 1
    worst = float(np.max(np.abs(x1 - ref["x1"]) / ref["x1_err"]))
    d_rel = abs(info["rel_residual"] - ref["rel_residual"])
    print(f"n={n} method={method}: rel_alpha bound {ref['rel_alpha']:.3e}, max |x1 - ref| / bound = {worst:.3e}, "
          f"max rel |x1 - ref| = {np.max(np.abs(x1 - ref['x1']) / np.abs(ref['x1'])):.3e}, rel_residual {info['rel_residual']:.17g} "
          f"ref {ref['rel_residual']:.17g} diff {d_rel:.3e} bound {ref['rel_residual_err']:.3e}")
    assert np.all(np.isfinite(x1)) and np.all(ref["x1_err"] > 0)
    assert np.all(np.abs(x1 - ref["x1"]) <= ref["x1_err"])
    assert d_rel <= ref["rel_residual_err"]


def _spmv_check(rp, ci, va, x):
    s = krylov.Solver()
    try:
        s.set_matrix(rp, ci, va)
        got, _ = s.spmv(x)
        inf = s.info()
    finally:
        s.close()
    n = x.size
    assert np.array_equal(got, R.sell_order_matvec(rp, ci, va, x))
    assert inf["nnz"] == rp[-1] and inf["stored_entries"] >= inf["nnz"] and inf["spmv_bytes"] == 12 * int(rp[-1]) + 16 * n
    cnt = np.diff(np.asarray(rp, np.int64))
    widths = np.maximum.reduceat(cnt, np.arange(0, n, 64))              # a slice is as wide as its longest row
    assert inf["stored_entries"] == 64 * int(widths.sum())


@pytest.mark.parametrize("n", [65793, N_BLOCKS])
def test_spmv_beyond_one_pass_of_the_grid_is_bit_identical(n):
    A, _ = _system(n)
    x = np.random.default_rng(n).normal(size=n)
    _spmv_check(A.indptr, A.indices, A.data, x)


def test_spmv_ragged_rows_beyond_one_pass_of_the_grid_is_bit_identical():
    """Rows of 1 .. 40 entries in shuffled column order: slices of every width, more than 8192 of them, the last one ragged."""
    rp, ci, va = R.ragged_matrix(N_BLOCKS, seed=7)
    _spmv_check(rp, ci, va, np.random.default_rng(8).normal(size=N_BLOCKS))


# ---- the assembly ---------------------------------------------------------------------------------------------------------------

RTOL = 1e-10


def _load(tri, x, y):
    xb = x[tri - 1].mean(1); yb = y[tri - 1].mean(1)
    return 1.0 + xb + 2.0 * yb * yb


def _check_poisson(tri, x, y, bnd):
    """poisson_solve against the reference SYSTEM (not the solver's own): residual, distance from the direct solve of the
    reference system by the condition number, run-to-run bits."""
    assert x.size <= 1500
    f = _load(tri, x, y)
    A, b = R.p1_poisson(tri, x, y, bnd, f)
    u, info = krylov.poisson_solve(tri, x, y, bnd, f, rtol=RTOL)
    u2, info2 = krylov.poisson_solve(tri, x, y, bnd, f, rtol=RTOL)
    assert np.array_equal(u, u2) and info["iterations"] == info2["iterations"] and info["rel_residual"] == info2["rel_residual"]
    assert np.all(np.isfinite(u)) and info["rel_residual"] <= RTOL
    res = np.linalg.norm(b - A @ u)
    u_ref = spla.spsolve(A.tocsc(), b)
    kappa = np.linalg.cond(A.toarray())
    err = np.linalg.norm(u - u_ref)
    print(f"Nn={x.size} Ne={tri.shape[0]}: iterations {info['iterations']}, |b - A_ref u| / |b| = {res / np.linalg.norm(b):.3e}, "
          f"|u - u_ref| / |u_ref| = {err / np.linalg.norm(u_ref):.3e}, kappa = {kappa:.3e}")
    assert res <= 10 * RTOL * np.linalg.norm(b)
    assert err <= kappa * 10 * RTOL * np.linalg.norm(u_ref)
    assert np.all(u[np.asarray(bnd).astype(bool)] == 0.0)
    return u


@functools.lru_cache(maxsize=None)
def _hub_mesh():
    return R.hub_mesh()


def test_assembly_on_a_mesh_with_hubs():
    tri, x, y, bnd, hubs, sizes = _hub_mesh()
    assert R.elements_per_patch(tri, x.size).max() <= 512
    u = _check_poisson(tri, x, y, bnd)
    assert u.min() >= 0.0 and np.all(u[hubs] > 0)                      # f > 0: maximum principle (Delaunay: an M-matrix)


def test_assembly_with_a_second_round_of_the_element_loop():
    """The same mesh, nodes renumbered at random: every patch of 128 rows is touched by more than 512 elements."""
    tri, x, y, bnd, hubs, _ = _hub_mesh()
    ts, xs, ys, bs, perm = R.permute_nodes(tri, x, y, bnd, seed=5)
    assert R.elements_per_patch(ts, xs.size).max() > 512
    u = _check_poisson(ts, xs, ys, bs)
    assert u.min() >= 0.0 and np.all(u[perm[hubs]] > 0)


@pytest.mark.parametrize("nx,ny,drop,nn", [(6, 6, False, 49), (7, 7, False, 64), (4, 12, False, 65), (8, 8, False, 81), (10, 10, False, 121),
                                           (7, 15, True, 127), (7, 15, False, 128), (2, 42, False, 129)])
def test_assembly_at_the_slice_and_patch_edges(nx, ny, drop, nn):
    """Nn <= 64: one slice, the patch's second slice is the clamp; Nn % 128 in {1, 64, 65, 127}: a last patch of one row, of
    exactly one slice, of one slice and a row, of one row short of full."""
    mesh = R.rect_grid(nx, ny)
    if drop:
        mesh = R.drop_last_node(*mesh)
    assert mesh[1].size == nn
    _check_poisson(*mesh)


def test_assembly_with_a_node_no_element_references():
    tri, x, y, bnd = R.rect_grid(8, 8)
    x = np.append(x, 2.0); y = np.append(y, 2.0)
    u = _check_poisson(tri, x, y, np.append(bnd, 1).astype(np.uint8))   # flagged: an identity row, u = 0 there
    assert u[81] == 0.0
    with pytest.raises(NxsError, match=r"row 81\b") as ei:              # not flagged: a zero row, refused by name
        krylov.poisson_solve(tri, x, y, np.append(bnd, 0).astype(np.uint8), _load(tri, x, y), rtol=RTOL)
    assert ei.value.code == -1


def test_assembly_around_a_vertex_of_valence_70():
    """The hub's 70 elements share a node, so they want 70 colours -- more than one 64-bit mask of them.  (Its slices are 71, 6
    and 5 wide: 40 KB of LDS, no more than any launch gets.)  The solve must be right."""
    tri, x, y, bnd = R.fan_mesh(70)
    assert R.patch_lds_bytes(tri, x.size) < 64 * 1024
    _check_poisson(tri, x, y, bnd)


def _lds_per_workgroup():
    """hipDeviceGetAttribute(hipDeviceAttributeMaxSharedMemoryPerBlock) of device 0, from the HIP runtime the library runs on."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    value = ctypes.c_int(0)
    MAX_SHARED_MEMORY_PER_BLOCK = 74                                   # hip_runtime_api.h, hipDeviceAttribute_t (HIP 6 and 7)
    assert hip.hipDeviceGetAttribute(ctypes.byref(value), MAX_SHARED_MEMORY_PER_BLOCK, 0) == 0
    assert 32 * 1024 <= value.value <= 1024 * 1024 and value.value % 1024 == 0, value.value
    return value.value


def _solves_or_is_refused_by_lds(tri, x, y, bnd):
    """What the device can hold decides: a patch that fits a workgroup's LDS is solved to the bars of every other mesh, one
    that does not is refused as NXS_ERR_INVALID with a message about the LDS -- never a misleading 'no diagonal', never a
    wrong answer."""
    need, have = R.patch_lds_bytes(tri, x.size), _lds_per_workgroup()
    print(f"patch assembly wants {need} B of LDS, a workgroup has {have} B")
    if need <= have:
        _check_poisson(tri, x, y, bnd)
    else:
        with pytest.raises(NxsError, match=r"patch.*LDS") as ei:
            krylov.poisson_solve(tri, x, y, bnd, _load(tri, x, y), rtol=RTOL)
        assert ei.value.code == -1 and "diagonal" not in str(ei.value)   # NXS_ERR_INVALID
    return need, have


def test_assembly_with_a_patch_beyond_the_default_lds():
    """A hub of valence 130: its slice alone is 64 x 131 doubles, the launch asks for 71 168 B -- past the 64 KiB a launch gets
    unasked, so the limit has to be raised first; a gfx950 workgroup has 160 KiB and solves it."""
    tri, x, y, bnd = R.fan_mesh(130)
    need, have = _solves_or_is_refused_by_lds(tri, x, y, bnd)
    assert need == 71168 > 64 * 1024


def test_assembly_with_a_patch_beyond_a_workgroups_lds():
    """Hubs of valence 160 in both slices of one patch: 165 888 B, more than the 160 KiB of a gfx950 workgroup (and within
    256 colours and 65 535 entries, so nothing else refuses it first)."""
    tri, x, y, bnd = R.two_fans(160)
    need, have = _solves_or_is_refused_by_lds(tri, x, y, bnd)
    assert need == 165888 > 160 * 1024


# ---- exact convergence and trivial systems ------------------------------------------------------------------------------------------

def _diag_system(kind, n):
    d = np.ones(n) if kind == "identity" else 2.0 ** ((np.arange(n) % 7) - 3)
    b = ((np.arange(n) * 5 + 3) % 17 - 8).astype(np.float64)             # small integers, some of them 0
    if n == 1:
        b[:] = 3.0
    return np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), d, b


@pytest.mark.parametrize("method", [krylov.CG, krylov.BICGSTAB], ids=["cg", "bicgstab"])
@pytest.mark.parametrize("kind", ["identity", "pow2"])
@pytest.mark.parametrize("n", [1, 64, 1000])
def test_exact_convergence_stays_finite(n, kind, method):
    """r becomes 0 exactly in the first iteration; the residual is looked at every 10th only, and the iterations in between
    must leave x alone (they used to form 0 / 0)."""
    rp, ci, d, b = _diag_system(kind, n)
    s = krylov.Solver()
    try:
        s.set_matrix(rp, ci, d)
        x, info = s.solve(b, method=method, rtol=1e-12, max_iter=500)
    finally:
        s.close()
    assert np.all(np.isfinite(x))
    assert np.array_equal(x, b / d)
    assert info["rel_residual"] == 0.0 and info["iterations"] <= 10


@pytest.mark.parametrize("method", [krylov.CG, krylov.BICGSTAB], ids=["cg", "bicgstab"])
def test_trivial_solves_and_the_handle_after_them(method):
    n = 4097
    A, b = _system(n)
    fresh = krylov.Solver()
    s = krylov.Solver()
    try:
        fresh.set_matrix(A.indptr, A.indices, A.data)
        want, winfo = fresh.solve(b, method=method, rtol=1e-12)
        assert winfo["rel_residual"] <= 1e-12 and np.linalg.norm(A @ want - b) <= 1e-11 * np.linalg.norm(b)
        s.set_matrix(A.indptr, A.indices, A.data)

        def again():
            x, info = s.solve(b, method=method, rtol=1e-12)
            assert np.array_equal(x, want) and info["iterations"] == winfo["iterations"] and info["rel_residual"] == winfo["rel_residual"]

        x, info = s.solve(np.zeros(n), method=method)
        assert np.all(x == 0.0) and info["iterations"] == 0 and info["rel_residual"] == 0.0
        again()
        x, info = s.solve(b, method=method, max_iter=0)
        assert np.all(x == 0.0) and info["iterations"] == 0 and info["rel_residual"] == 1.0
        again()
        # a system that converges exactly, on the same handle, and the first one back again
        rp, ci, d, bd = _diag_system("pow2", 1000)
        s.set_matrix(rp, ci, d)
        x, info = s.solve(bd, method=method)
        assert np.array_equal(x, bd / d) and info["rel_residual"] == 0.0
        s.set_matrix(A.indptr, A.indices, A.data)
        again()
    finally:
        s.close(); fresh.close()
