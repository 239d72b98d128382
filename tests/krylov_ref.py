"""Plain host references for the Krylov extension (nextsim_amd/csrc/nxs_krylov.hip): numpy, scipy and math.fsum only --
no GPU and none of the code under test.  The P1 Poisson system of k_assemble_patches + k_apply_dirichlet, the row sums of
k_spmv_sell in their order, the first iteration of run_solver's CG and BiCGStab with a bound on how far a device that sums
in another order may be from it, and the meshes the edge tests need."""
import math

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53          # unit round-off of binary64


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): k roundings in a row change a result by at most this, relatively."""
    return k * U / (1.0 - k * U)


# ---- the P1 Poisson system ---------------------------------------------------------------------------------------------------

def p1_poisson(tri, x, y, dirichlet, f, eliminate=True):
    """CSR A_ref (sorted columns) and b_ref of -laplace(u) = f, P1 elements, f constant per element, homogeneous Dirichlet
    on the flagged nodes.  tri is 1-based.  The formulas of k_assemble_patches -- area = 1/2 |(x1-x0)(y2-y0) - (x2-x0)(y1-y0)|,
    m_jk = (dy_j dy_k + dx_j dx_k) / (4 area) with d._j the edge opposite vertex j, f area / 3 per vertex -- in np.longdouble,
    rounded to double once, after the sum over the elements.  Then the elimination of k_apply_dirichlet: row and column
    zeroed, diagonal 1, rhs 0.  A node no element references keeps an (explicit) zero row; flagged, it becomes the row of
    the identity.  eliminate=False returns the system before that step."""
    LD = np.longdouble
    t = np.asarray(tri, np.int64) - 1
    n = int(np.asarray(x).size)
    xs, ys = np.asarray(x, LD)[t], np.asarray(y, LD)[t]
    area = LD(0.5) * np.abs((xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (xs[:, 2] - xs[:, 0]) * (ys[:, 1] - ys[:, 0]))
    rows, cols, vals = [], [], []
    for j in range(3):
        jp1, jp2 = (j + 1) % 3, (j + 2) % 3
        for k in range(3):
            kp1, kp2 = (k + 1) % 3, (k + 2) % 3
            m = ((ys[:, jp1] - ys[:, jp2]) * (ys[:, kp1] - ys[:, kp2]) + (xs[:, jp1] - xs[:, jp2]) * (xs[:, kp1] - xs[:, kp2])) / (LD(4.0) * area)
            rows.append(t[:, j]); cols.append(t[:, k]); vals.append(m)
    rows.append(np.arange(n)); cols.append(np.arange(n)); vals.append(np.zeros(n, LD))      # every row has its diagonal
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    key = rows * n + cols
    order = np.argsort(key, kind="stable")
    key, vals = key[order], vals[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    summed = np.add.reduceat(vals, first)                                                   # long double sums, one per entry
    r, c = key[first] // n, key[first] % n
    b = np.zeros(n, LD)
    fa = np.asarray(f, LD) * area / LD(3.0)
    for j in range(3):
        np.add.at(b, t[:, j], fa)
    val, b = summed.astype(np.float64), b.astype(np.float64)
    if eliminate:
        d = np.asarray(dirichlet).astype(bool)
        off_diag = r != c
        val[(d[r] | d[c]) & off_diag] = 0.0
        val[d[r] & ~off_diag] = 1.0
        b[d] = 0.0
    A = sp.csr_matrix((val, (r, c)), shape=(n, n))          # (explicit zeros stay: the pattern is the kernel's)
    A.sort_indices()
    return A, b


# ---- SpMV in the kernel's order -------------------------------------------------------------------------------------------------

def sell_order_matvec(rowptr, colidx, val, x):
    """Row sums in CSR entry order, acc = acc + (val_j * x[col_j]) for j = 0, 1, ... with the product rounded before the
    sum (no FMA): what a sequential loop over the row gives, vectorised over the rows."""
    rowptr = np.asarray(rowptr, np.int64); colidx = np.asarray(colidx); val = np.asarray(val, np.float64); x = np.asarray(x, np.float64)
    cnt = np.diff(rowptr)
    acc = np.zeros(cnt.size)
    rows = np.arange(cnt.size)
    for j in range(int(cnt.max()) if cnt.size else 0):
        rows = rows[cnt[rows] > j]
        q = rowptr[rows] + j
        prod = val[q] * x[colidx[q]]
        acc[rows] = acc[rows] + prod
    return acc


def _abs_matvec(A, v):
    B = A.copy(); B.data = np.abs(B.data)
    return B @ np.abs(v)


def _fdot(a, b):
    """(sum of the rounded products, exactly rounded; sum of their moduli)."""
    t = a * b
    return math.fsum(t), math.fsum(np.abs(t))


# ---- the bound on |device - this reference| ---------------------------------------------------------------------------------------
# The device and this module form every element-wise quantity with the same IEEE operations (the library is built without
# FMA contraction and without fast-math), so quantities built from bit-identical inputs are bit-identical: dinv, z = dinv b,
# A z (the order of sell_order_matvec) and the products inside the first dots.  What differs is the ORDER of the sums.
#   dot:      any order of adding n terms t_i errs by at most gamma_{n-1} sum|t_i| (Higham, Accuracy and Stability, 4.2);
#             fsum here errs by u |sum|.  Both together stay below gamma_{n+1} sum|t_i|  =: _dot_err.
#   quotient: a = p / q of two such dots: relative bounds add, plus u for the division on either side:
#             rel(a) = _dot_err(p)/|p| + _dot_err(q)/|q| + 2u.
# From the first quotient on, the two sides carry DIFFERENT scalars, and what is built from them differs by propagated
# error e(.) (first order, moduli everywhere) plus roundings that no longer cancel; an expression that the compiler may or
# may not contract is charged both roundings:
#   v = a w (scalar a):    e(v) <= rel(a) |a w| + e(w) |a| + 2u |a w|
#   v = w1 - w2:           e(v) <= e(w1) + e(w2) + 2u |v|
#   v = A w:               e(v) <= |A| e(w) + 2 gamma_{L} |A||w|,  L = longest row (each side's own row-sum roundings)
#   dot of such vectors:   sum_i e(t_i) + _dot_err,  e(a_i b_i) <= |a_i| e(b_i) + |b_i| e(a_i) + e(a_i) e(b_i) + 2u |a_i b_i|
#   sqrt(p / q):           |sqrt a - sqrt a'| <= |a - a'| / sqrt a  and  <= sqrt|a - a'|; the smaller of the two, + 2u.
# Second-order terms are kept where a product of two errors appears and are otherwise below 1e-20 of the result.
# Sizes: at n = 524 609 gamma_{n+1} = 5.8e-11, so alpha is pinned to 1.2e-10; one row missing from a dot moves it by
# 1/n = 2e-6, one block of 256 rows by 5e-4.

def _dot_err(n, sum_abs):
    return gamma(n + 1) * sum_abs


def _rel_quot(n, p, sp_, q, sq_, ep=0.0, eq=0.0):
    if p == 0.0 and sp_ == 0.0 and ep == 0.0:
        return 0.0                                      # 0 / q on both sides
    if p == 0.0 or q == 0.0:
        return math.inf
    return (_dot_err(n, sp_) + ep) / abs(p) + (_dot_err(n, sq_) + eq) / abs(q) + 2 * U


def _sqrt_ratio(n, rr, e_rr, bb):
    """sqrt(rr / bb) as run_solver forms it and the bound on the device's distance from it."""
    ratio = rr / bb
    e_ratio = (e_rr + _dot_err(n, rr)) / bb + ratio * (_dot_err(n, bb) / bb + 2 * U)
    val = math.sqrt(ratio)
    e = math.sqrt(e_ratio) if ratio == 0.0 else min(e_ratio / val, math.sqrt(e_ratio))
    return val, e + 2 * U * val


def cg_first_iteration(A, b):
    """One iteration of Jacobi-preconditioned CG from x0 = 0 in run_solver's order (k_cg_init, k_spmv_sell<1>, k_cg_xr):
    z = D^-1 b, p = z, q = A p, alpha = (b,z)/(p,q), x1 = alpha p, r1 = b - alpha q, rel = sqrt((r1,r1)/(b,b)).
    Dots by math.fsum.  Returns alpha, x1, rel_residual, the dots with the sums of their terms' moduli, and the bounds of
    the comment above: rel_alpha, x1_err (per entry, absolute) and rel_residual_err (absolute)."""
    A = sp.csr_matrix(A); b = np.asarray(b, np.float64)
    n = b.size
    dinv = 1.0 / A.diagonal()
    z = dinv * b
    rz, s_rz = _fdot(b, z)
    bb, s_bb = _fdot(b, b)
    q = sell_order_matvec(A.indptr, A.indices, A.data, z)
    pq, s_pq = _fdot(z, q)
    alpha = rz / pq
    rel_alpha = _rel_quot(n, rz, s_rz, pq, s_pq)
    x1 = alpha * z
    x1_err = (rel_alpha + 2 * U) * np.abs(x1)
    aq = alpha * q
    r1 = b - aq
    e_r1 = (rel_alpha + 2 * U) * np.abs(aq) + 2 * U * np.abs(r1)
    rr, _ = _fdot(r1, r1)
    e_rr = math.fsum(2 * np.abs(r1) * e_r1 + e_r1 * e_r1 + 2 * U * r1 * r1)
    rel, e_rel = _sqrt_ratio(n, rr, e_rr, bb)
    return {"alpha": alpha, "rel_alpha": rel_alpha, "x1": x1, "x1_err": x1_err, "rel_residual": rel, "rel_residual_err": e_rel, "z": z,
            "dots": {"rz": (rz, s_rz), "bb": (bb, s_bb), "pAp": (pq, s_pq), "rr1": (rr, rr)}}


def bicgstab_first_iteration(A, b):
    """One iteration of right-Jacobi-preconditioned BiCGStab from x0 = 0 in run_solver's order (k_bicg_init, k_bicg_p,
    k_spmv_sell<1>, k_bicg_s, k_spmv_sell<2>, k_bicg_x): rhat = r = p = b, y = D^-1 p, v = A y, alpha = (b,b)/(rhat,v),
    s = r - alpha v, z = D^-1 s, t = A z, omega = (t,s)/(t,t) (0 where (t,t) = 0), x1 = alpha y + omega z, r1 = s - omega t.
    Same returns as cg_first_iteration, with omega and rel_omega."""
    A = sp.csr_matrix(A); b = np.asarray(b, np.float64)
    n = b.size
    L = int(np.diff(A.indptr).max())
    d = A.diagonal()
    dinv = 1.0 / d
    y = dinv * b
    bb, s_bb = _fdot(b, b)
    v = sell_order_matvec(A.indptr, A.indices, A.data, y)
    rv, s_rv = _fdot(b, v)
    alpha = bb / rv
    rel_alpha = _rel_quot(n, bb, s_bb, rv, s_rv)
    av = alpha * v
    s = b - av
    e_s = (rel_alpha + 2 * U) * np.abs(av) + 2 * U * np.abs(s)
    z = dinv * s
    e_z = dinv * e_s + 2 * U * np.abs(z)
    t = sell_order_matvec(A.indptr, A.indices, A.data, z)
    e_t = _abs_matvec(A, e_z) + 2 * gamma(L) * _abs_matvec(A, z)
    ts, s_ts = _fdot(t, s)
    tt, s_tt = _fdot(t, t)
    e_ts = math.fsum(np.abs(t) * e_s + np.abs(s) * e_t + e_s * e_t + 2 * U * np.abs(t * s))
    e_tt = math.fsum(2 * np.abs(t) * e_t + e_t * e_t + 2 * U * t * t)
    omega = ts / tt if tt != 0.0 else 0.0
    rel_omega = _rel_quot(n, ts, s_ts, tt, s_tt, e_ts, e_tt) if tt != 0.0 else math.inf
    # Where the two dots drown in their own error (s = 0 up to rounding: the first half step has solved the system) omega is
    # noise on both sides, but bounded noise: t = (I - N) s with N = -(A - D) D^-1, so |(t,s)| / (t,t) <= |s| / |t| <=
    # 1 / (1 - |N|_2), |N|_2 <= sqrt(|N|_1 |N|_inf), and a computed dot obeys Cauchy-Schwarz up to (1 + gamma_n)/(1 - gamma_n).
    N = sp.csr_matrix(A - sp.diags(d)) @ sp.diags(dinv)
    N.data = np.abs(N.data)
    nu = math.sqrt(float(N.sum(0).max()) * float(N.sum(1).max())) if N.nnz else 0.0
    omega_cap = (1.0 + 3 * gamma(n + 1)) / (1.0 - nu) if nu < 1.0 else math.inf
    d_omega = min(rel_omega * abs(omega) if math.isfinite(rel_omega) else math.inf, 2 * omega_cap)     # |omega_dev - omega_ref|
    ay, oz, ot = alpha * y, omega * z, omega * t
    x1 = ay + oz
    e_oz = d_omega * (np.abs(z) + e_z) + abs(omega) * e_z + 2 * U * np.abs(oz)
    x1_err = (rel_alpha + 2 * U) * np.abs(ay) + e_oz + 2 * U * np.abs(x1)
    r1 = s - ot
    e_r1 = e_s + d_omega * (np.abs(t) + e_t) + abs(omega) * e_t + 2 * U * np.abs(ot) + 2 * U * np.abs(r1)
    rr, _ = _fdot(r1, r1)
    e_rr = math.fsum(2 * np.abs(r1) * e_r1 + e_r1 * e_r1 + 2 * U * r1 * r1)
    rel, e_rel = _sqrt_ratio(n, rr, e_rr, bb)
    return {"alpha": alpha, "rel_alpha": rel_alpha, "omega": omega, "rel_omega": rel_omega, "x1": x1, "x1_err": x1_err,
            "rel_residual": rel, "rel_residual_err": e_rel,
            "dots": {"bb": (bb, s_bb), "rhat_v": (rv, s_rv), "ts": (ts, s_ts), "tt": (tt, s_tt), "rr1": (rr, rr)}}


# ---- matrices -----------------------------------------------------------------------------------------------------------------------

def pentadiagonal(n, seed=0):
    """SPD pentadiagonal M-matrix (strictly diagonally dominant: diagonal 5 .. 6 against -1, -1, -1/2, -1/2) from
    scipy.sparse.diags, and a right-hand side with 1 <= b_i < 1.5.  Then z = D^-1 b lies in (1/6, 0.3), (A z)_i >= 1 - 3 * 0.3
    > 0, and every term of every dot of the first CG iteration is positive: a partial sum that went missing cannot hide
    behind cancellation."""
    rng = np.random.default_rng(seed)
    bands = [(0, 5.0 + rng.random(n))] + [(k, np.full(n - abs(k), w)) for k, w in ((-2, -0.5), (-1, -1.0), (1, -1.0), (2, -0.5)) if abs(k) < n]
    A = sp.diags([v for _, v in bands], [k for k, _ in bands], shape=(n, n), format="csr")
    A.sort_indices()
    return A, 1.0 + 0.5 * rng.random(n)


def ragged_matrix(n, seed=0, longest=40):
    """Rows of 1 .. `longest` entries (the diagonal among them, distinct columns), in shuffled order inside every row."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, min(n, longest) + 1, n)
    rp = np.zeros(n + 1, np.int64); np.cumsum(cnt, out=rp[1:])
    row = np.repeat(np.arange(n), cnt)
    j = np.arange(rp[-1]) - rp[row]                                         # position inside the row
    step = rng.integers(1, max(2, (n - 1) // max(1, min(n, longest)) + 1), rp[-1])
    step[rp[:-1]] = 0                                                       # entry 0 is the diagonal
    off = np.cumsum(step); off -= off[rp[row]]                              # distinct offsets < n inside a row
    col = (row + off) % n
    val = rng.normal(size=rp[-1]) + 3.0 * (j == 0)
    order = np.argsort(row + rng.random(rp[-1]), kind="stable")             # shuffle inside the rows
    return rp.astype(np.int32), col[order].astype(np.int32), val[order]


# ---- meshes (tri is 1-based, as the ABI takes it) -------------------------------------------------------------------------------

def rect_grid(nx, ny):
    """(nx + 1) x (ny + 1) nodes on the unit square, two triangles per cell, boundary flagged: tests/test_krylov.py's
    unit_square for nx = ny."""
    X, Y = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 1, ny + 1), indexing="ij")
    nid = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a = nid[:-1, :-1].ravel(); b = nid[1:, :-1].ravel(); c = nid[1:, 1:].ravel(); d = nid[:-1, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]) + 1
    x, y = X.ravel(), Y.ravel()
    bnd = (x == 0) | (x == 1) | (y == 0) | (y == 1)
    return tri.astype(np.int32), x, y, bnd.astype(np.uint8)


def drop_last_node(tri, x, y, bnd):
    """The mesh without its last node and that node's triangles (the far corner of a rect_grid: two triangles)."""
    n = x.size
    keep = ~(tri == n).any(1)
    return np.ascontiguousarray(tri[keep]), x[:-1].copy(), y[:-1].copy(), bnd[:-1].copy()


def hub_mesh(n_pts=1150, hubs=3, ring=(14, 21), seed=0):
    """Delaunay mesh (cases._delaunay) of random points in a 600 x 450 km box, as tests/test_gpu_fuzz.py::random_mesh, with
    `hubs` vertices that own a ring of ring[0] <= k < ring[1] close neighbours (valence k).  Unlike random_mesh the nodes are
    numbered with locality (three bands in y, by x inside a band), as a mesh generator would; coordinates are returned
    scaled to the unit box.  Returns tri, x, y, dirichlet (the box's boundary), hub_nodes (0-based), ring_sizes."""
    import cases
    rng = np.random.default_rng(seed)
    L, H, nb = 600e3, 450e3, 14
    s = np.arange(nb) / nb
    bx = np.concatenate([L * s, np.full(nb, L), L * (1 - s), np.zeros(nb)])
    by = np.concatenate([np.zeros(nb), H * s, np.full(nb, H), H * (1 - s)])
    px = L * rng.uniform(0.04, 0.96, n_pts); py = H * rng.uniform(0.04, 0.96, n_pts)
    hx, hy, is_hub, sizes = [], [], [], []
    centres = [(0.3, 0.3), (0.7, 0.45), (0.4, 0.72), (0.62, 0.2), (0.2, 0.6)]
    for i in range(hubs):
        cx, cy = L * centres[i % len(centres)][0], H * centres[i % len(centres)][1]
        k = int(rng.integers(ring[0], ring[1])); rad = rng.uniform(9e3, 14e3)
        keep = np.hypot(px - cx, py - cy) > 2.2 * rad                      # clear the neighbourhood: the ring owns the hub
        px, py = px[keep], py[keep]
        ang = 2 * np.pi * (np.arange(k) + rng.uniform(0, 1)) / k
        hx += [cx] + list(cx + rad * np.cos(ang)); hy += [cy] + list(cy + rad * np.sin(ang))
        is_hub += [True] + [False] * k; sizes.append(k)
    x = np.concatenate([bx, px, hx]); y = np.concatenate([by, py, hy])
    on_b = np.zeros(x.size, bool); on_b[:4 * nb] = True
    hub = np.zeros(x.size, bool); hub[x.size - len(is_hub):] = is_hub
    order = np.lexsort((x, np.minimum((3 * y / H).astype(int), 2)))         # new id -> old id
    x, y, on_b, hub = x[order], y[order], on_b[order], hub[order]
    tri = cases._delaunay(x, y) + 1
    return tri.astype(np.int32), x / L, y / L, on_b.astype(np.uint8), np.flatnonzero(hub), sizes


def permute_nodes(tri, x, y, flags, seed=0):
    """The same mesh with its nodes renumbered at random: node i becomes node perm[i].  Returns tri, x, y, flags, perm."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(x.size)
    xn, yn, fn = np.empty_like(x), np.empty_like(y), np.empty_like(flags)
    xn[perm], yn[perm], fn[perm] = x, y, flags
    return (perm[np.asarray(tri) - 1] + 1).astype(np.int32), xn, yn, fn, perm


def fan_mesh(k, outer=True):
    """One vertex (node 0, the centre) of valence k: k triangles around it, and (outer) a second ring of k nodes joined
    to the first by 2k triangles, so that the first ring is interior too.  The outermost ring is the boundary."""
    ang = 2 * np.pi * np.arange(k) / k
    x = [np.zeros(1), 0.5 * np.cos(ang)]; y = [np.zeros(1), 0.5 * np.sin(ang)]
    r1 = 1 + np.arange(k); r1n = 1 + (np.arange(k) + 1) % k
    tris = [np.stack([np.zeros(k, np.int64), r1, r1n], 1)]
    bnd = np.concatenate([[0], np.ones(k, np.uint8)])
    if outer:
        x.append(np.cos(ang + np.pi / k)); y.append(np.sin(ang + np.pi / k))
        r2 = 1 + k + np.arange(k); r2n = 1 + k + (np.arange(k) + 1) % k
        tris += [np.stack([r1, r2, r1n], 1), np.stack([r1n, r2, r2n], 1)]
        bnd = np.concatenate([[0], np.zeros(k, np.uint8), np.ones(k, np.uint8)])
    tri = np.concatenate(tris) + 1
    return tri.astype(np.int32), np.concatenate(x), np.concatenate(y), bnd.astype(np.uint8)


def two_fans(k):
    """Two fan_mesh(k, outer=False) side by side, numbered so that the hubs are nodes 0 and 64: one long row in EACH of the
    two 64-row slices of the first patch."""
    tri, x, y, bnd = fan_mesh(k, outer=False)
    n = x.size
    tri = np.concatenate([tri, tri + n]); x = np.concatenate([x, x + 2.0]); y = np.concatenate([y, y]); bnd = np.concatenate([bnd, bnd])
    new = np.arange(2 * n); new[n], new[64] = 64, n                         # old id -> new id: the second hub and node 64 swap
    xn, yn, fn = np.empty_like(x), np.empty_like(y), np.empty_like(bnd)
    xn[new], yn[new], fn[new] = x, y, bnd
    return (new[tri - 1] + 1).astype(np.int32), xn, yn, fn


def row_lengths(tri, num_nodes):
    """Entries per row of the P1 pattern: the node and its neighbours (a node no element references: its diagonal)."""
    t = np.asarray(tri, np.int64) - 1
    r = np.concatenate([t[:, j] for j in range(3) for _ in range(3)] + [np.arange(num_nodes)])
    c = np.concatenate([t[:, k] for _ in range(3) for k in range(3)] + [np.arange(num_nodes)])
    return np.bincount(np.unique(r * num_nodes + c) // num_nodes, minlength=num_nodes)


def patch_lds_bytes(tri, num_nodes):
    """Dynamic LDS the patch assembly asks for, as the host code sizes it: a slice of 64 rows is as wide as its longest row,
    a patch is two consecutive slices, the launch gets the largest patch plus the 128 rhs entries, in doubles."""
    cnt = row_lengths(tri, num_nodes)
    size = 64 * np.maximum.reduceat(cnt, np.arange(0, num_nodes, 64))
    if size.size % 2:
        size = np.append(size, 0)
    return 8 * (int(size.reshape(-1, 2).sum(1).max()) + 128)


def elements_per_patch(tri, num_nodes, patch_rows=128):
    """How many elements touch each patch of `patch_rows` consecutive rows (an element counts once per patch it touches):
    the trip count of k_assemble_patches' element loop is ceil(this / 512)."""
    p = (np.asarray(tri, np.int64) - 1) // patch_rows
    npatch = (num_nodes + patch_rows - 1) // patch_rows
    cnt = np.zeros(npatch, np.int64)
    for k in range(3):
        new = np.ones(p.shape[0], bool)
        for j in range(k):
            new &= p[:, k] != p[:, j]
        np.add.at(cnt, p[new, k], 1)
    return cnt
