"""The device-built regrid tables (nextsim_amd/csrc/nxs_regrid_tables.inl) at the sizes and shapes the other tests do not reach: the exclusive
scan with one, two (a one-entry tail), five blocks and with a THIRD level (more than 1024 * 1024 entries: the bucket grid of every mesh beyond
524 288 triangles), triangles on both sides of the wide threshold (a box of NXS_GRID_WIDE = 64 cells gets a workgroup, 63 cells a thread),
cells listed by a wide AND a narrow triangle (the two fill kernels share the cell's cursor; the sort behind them makes the list ascending) and
a triangle in the last column / row of the grid.

The bucket grid is compared with the numpy restatement of its definition that tests/test_remap.py states (bamg's integer plane: bounding box
+ 5 %, 2^30 - 1 units, truncation; G x G cells, G doubling while 2 G^2 < triangles; every triangle listed in the cells its bounding box touches,
ascending): ALL offsets and ALL lists, not a sample.  The connectivity tables are compared with dynamics.mesh_connectivity /
mesh_element_connectivity."""
import time

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

WIDE = 64                          # NXS_GRID_WIDE
SCAN_BLOCK = 1024                  # entries per block of k_scan_blocks
BIG = "h9200"                      # the coarsest disc (edge a multiple of 100 m) with more than 524 288 triangles: 524 394 (h9300: 513 306)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------

def grid_size(nels):
    G = 1
    while 2 * G * G < nels and G < 4096:
        G <<= 1
    return G


def cell_boxes(x, y, tri, G):
    """cx0, cx1, cy0, cy1 of every triangle (tests/test_remap.py:272-279)."""
    px0, px1, py0, py1 = x.min(), x.max(), y.min(), y.max()
    dx, dy = (px1 - px0) * 0.05, (py1 - py0) * 0.05
    px0 -= dx; py0 -= dy; px1 += dx; py1 += dy
    coef = 1073741823. / max(px1 - px0, py1 - py0)
    ix = (coef * (x - px0)).astype(np.int64); iy = (coef * (y - py0)).astype(np.int64)
    shift = 30 - int(np.log2(G))
    cx0 = np.clip(ix[tri].min(1) >> shift, 0, G - 1); cx1 = np.clip(ix[tri].max(1) >> shift, 0, G - 1)
    cy0 = np.clip(iy[tri].min(1) >> shift, 0, G - 1); cy1 = np.clip(iy[tri].max(1) >> shift, 0, G - 1)
    return cx0, cx1, cy0, cy1


def grid_tables(boxes, G):
    """(off, lst, pair_tri, pair_cell): the offsets (prefix sums of the cells' counts: one np.add.at, one cumsum), every cell's list ascending,
    and the (triangle, cell) pairs they were made from."""
    cx0, cx1, cy0, cy1 = boxes
    w = cx1 - cx0 + 1
    n = w * (cy1 - cy0 + 1)
    t = np.repeat(np.arange(n.size), n)
    k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
    cell = (cy0[t] + k // w[t]) * G + cx0[t] + k % w[t]
    cnt = np.zeros(G * G, np.int64)
    np.add.at(cnt, cell, 1)
    off = np.concatenate([[0], np.cumsum(cnt)])
    lst = t[np.lexsort((t, cell))]
    return off, lst, t, cell


def cell_list(boxes, G, c):
    """The definition itself for ONE cell (tests/test_remap.py:283-284), independent of grid_tables' bookkeeping."""
    cx0, cx1, cy0, cy1 = boxes
    cy, cx = divmod(int(c), G)
    return np.flatnonzero((cx0 <= cx) & (cx <= cx1) & (cy0 <= cy) & (cy <= cy1))


def check_grid(rg, x, y, tri, cells=()):
    """The whole bucket grid of the context against the restatement; `cells` are compared once more against the one-cell definition."""
    off, lst = rg.debug_table(0).astype(np.int64), rg.debug_table(1).astype(np.int64)
    G = int(round(np.sqrt(off.size - 1)))
    assert G * G + 1 == off.size and G == grid_size(tri.shape[0])
    boxes = cell_boxes(x, y, tri, G)
    want_off, want_lst, pt, pc = grid_tables(boxes, G)
    assert off[0] == 0 and np.all(np.diff(off) >= 0) and off[-1] == lst.size == want_off[-1] == int(((boxes[1] - boxes[0] + 1) * (boxes[3] - boxes[2] + 1)).sum())
    bad = np.flatnonzero(off != want_off)
    assert bad.size == 0, f"{bad.size} offsets differ, the first at entry {bad[0]} (scan block {bad[0] // SCAN_BLOCK}, entry {bad[0] % SCAN_BLOCK} of it): {off[bad[0]]} != {want_off[bad[0]]}"
    bad = np.flatnonzero(lst != want_lst)
    assert bad.size == 0, f"{bad.size} list entries differ, the first in cell {np.searchsorted(off, bad[0], 'right') - 1}"
    for c in cells:
        assert np.array_equal(lst[off[c]:off[c + 1]], cell_list(boxes, G, c)), c
    return G, boxes, off, lst, pt, pc


def check_connectivity(rg, x, tri):
    from nextsim_amd import dynamics
    nods, nels = x.size, tri.shape[0]
    idx = np.ascontiguousarray((tri + 1).ravel(), np.int32)
    nec, _ = dynamics.mesh_connectivity(idx, nods)
    assert np.array_equal(rg.debug_table(2).reshape(nods, -1), np.where(np.isnan(nec), 0, nec).astype(np.int32) - 1)
    ec = dynamics.mesh_element_connectivity(idx, nods)
    assert np.array_equal(rg.debug_table(3).reshape(nels, 3), np.where(np.isnan(ec), 0, ec).astype(np.int32) - 1)


def scan_boundary_cells(n_entries):
    """The entries on both sides of every block boundary of the scan's second level (a block of it covers 1024 blocks of 1024 entries), of the
    first boundaries of the first level, and the last entries."""
    c = {0, 1, n_entries - 3, n_entries - 2}
    for b in (SCAN_BLOCK, 2 * SCAN_BLOCK):
        c |= {b - 1, b, b + 1}
    for b in range(SCAN_BLOCK * SCAN_BLOCK, n_entries, SCAN_BLOCK * SCAN_BLOCK):
        c |= {b - SCAN_BLOCK - 1, b - SCAN_BLOCK, b - 1, b, b + 1, b + SCAN_BLOCK - 1, b + SCAN_BLOCK}
    return sorted(i for i in c if 0 <= i < n_entries - 1)          # (entry n - 1 is the total, not a cell)


def _regrid(x, y, tri):
    from nextsim_amd import interp
    return interp.Regrid(np.ascontiguousarray((tri + 1).ravel(), np.int32), x, y)


# ---- B1: three scan levels ---------------------------------------------------------------------------------------------------------------------

def test_bucket_grid_beyond_a_million_cells_scans_on_three_levels():
    """nels > 524 288: G = 1024, 1 048 577 entries = 1025 blocks, whose sums are scanned by two blocks (the second holds one entry), whose sums by one."""
    from nextsim_amd import interp
    t0 = time.time()
    gm = cases.global_mesh(BIG)
    x, y, tri = gm.x, gm.y, gm.tri
    nods, nels = x.size, tri.shape[0]
    assert 524288 < nels < 1.01 * 524288 and grid_size(nels) == 1024
    t1 = time.time()
    rg = _regrid(x, y, tri)
    n_entries = 1024 * 1024 + 1
    assert -(-n_entries // SCAN_BLOCK) == 1025 and -(-1025 // SCAN_BLOCK) == 2
    rng = np.random.default_rng(0)
    cells = scan_boundary_cells(n_entries) + rng.integers(0, 1024 * 1024, 400).tolist()
    assert {1023, 1024, 1025, 1024 * 1024 - 1} <= set(cells)
    G, boxes, off, lst, _, _ = check_grid(rg, x, y, tri, cells)
    assert G == 1024 and off.size == n_entries
    assert 0 < off[SCAN_BLOCK * 512] < off[-1], "lists on both sides of the middle of the scan"
    check_connectivity(rg, x, tri)
    t2 = time.time()
    # one context, both calls of a regrid, against the one-shot calls
    idx = np.ascontiguousarray((tri + 1).ravel(), np.int32)
    xn, yn, trin, ng = cases.rect_mesh(9, 3, L=0.5 * np.ptp(x), H=0.4 * np.ptp(y), x0=x.mean() - 0.25 * np.ptp(x), y0=y.mean() - 0.2 * np.ptp(y))
    elem = rng.random((nels, 2)); nodal = rng.standard_normal((nods, 2))
    a1 = rg.remap_elements(elem, trin + 1, xn, yn, np.zeros(xn.size), ng)
    a2 = rg.interp_nodes(nodal, xn, yn, False, 0.0)
    b1 = interp.ConservativeRemappingMeshToMesh(elem, idx, x, y, trin + 1, xn, yn, np.zeros(xn.size), ng)
    b2 = interp.InterpFromMeshToMesh2dx(idx, x, y, nodal, xn, yn, False, 0.0)
    assert np.array_equal(a1, b1, equal_nan=True) and np.array_equal(a2, b2)
    assert np.all(np.isfinite(a1)) and np.all(np.isfinite(a2))
    rg.close()
    print(f"{BIG}: {nels} triangles, G = {G}, {off[-1]} list entries, {len(cells)} cells compared one by one; mesh {t1 - t0:.1f} s, tables {t2 - t1:.1f} s, "
          f"the two regrid calls twice {time.time() - t2:.1f} s")


# ---- B2: the scan's block edges at small sizes -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,G_want,blocks", [(10, 16, 1), (20, 32, 2), (32, 64, 5)])
def test_bucket_grid_at_the_scan_block_edges(n, G_want, blocks):
    """257 entries: one block; 1025: two, the second holding one entry; 4097: five, the last holding one."""
    from nextsim_amd import mesh as M
    gm = M.make_toy_mesh(n)
    x, y, tri = gm.x, gm.y, gm.tri
    rg = _regrid(x, y, tri)
    G = grid_size(tri.shape[0])
    assert G == G_want and -(-(G * G + 1) // SCAN_BLOCK) == blocks
    G, boxes, off, lst, _, _ = check_grid(rg, x, y, tri, range(G * G))
    check_connectivity(rg, x, tri)
    rg.close()
    print(f"toy mesh {n}: {tri.shape[0]} triangles, G = {G}, {G * G + 1} entries in {blocks} scan block(s), {off[-1]} list entries, every cell compared")


# ---- B3, B4: wide triangles ---------------------------------------------------------------------------------------------------------------------

def _lattice_and_quad(overlap):
    """A fine lattice (cases.rect_mesh, 400 km x 300 km) and, as a second component, a quad of two large triangles: beside the lattice, or lying
    across it (the two components then overlap in the plane; the tables do not mind, only bamg's convex completion, which is not asked for)."""
    x, y, tri, _ = cases.rect_mesh(32, 11)
    x0, y0 = (-100e3, -850e3) if overlap else (300e3, -900e3)
    qx = np.array([x0, x0 + 300e3, x0 + 300e3, x0]); qy = np.array([y0, y0, y0 + 280e3, y0 + 280e3])
    n = x.size
    quad = np.array([[n, n + 1, n + 2], [n, n + 2, n + 3]], np.int32)
    return np.concatenate([x, qx]), np.concatenate([y, qy]), np.ascontiguousarray(np.vstack([tri, quad]), np.int32)


@pytest.mark.parametrize("overlap", [False, True], ids=["beside", "across"])
def test_bucket_grid_with_wide_and_narrow_triangles(overlap):
    x, y, tri = _lattice_and_quad(overlap)
    rg = _regrid(x, y, tri)
    G, boxes, off, lst, pt, pc = check_grid(rg, x, y, tri)
    ncell = (boxes[1] - boxes[0] + 1) * (boxes[3] - boxes[2] + 1)
    wide = ncell >= WIDE
    assert wide.sum() >= 1 and (~wide).sum() >= 1 and wide[-2:].all() and not wide[:-2].any()
    has_wide = np.zeros(G * G, bool); has_wide[pc[wide[pt]]] = True
    has_narrow = np.zeros(G * G, bool); has_narrow[pc[~wide[pt]]] = True
    shared = np.flatnonzero(has_wide & has_narrow)
    print(f"{'across' if overlap else 'beside'}: G = {G}, {int(wide.sum())} wide triangles of {ncell[wide].tolist()} cells, the widest narrow one {int(ncell[~wide].max())} cells, "
          f"{shared.size} cells listed by both kinds")
    if overlap:
        assert shared.size >= 20
    for c in shared:
        got = lst[off[c]:off[c + 1]]
        assert np.array_equal(got, cell_list(boxes, G, c)) and np.all(np.diff(got) > 0), c
        assert wide[got].any() and not wide[got].all()
    for c in np.flatnonzero(has_wide)[::7]:
        assert np.array_equal(lst[off[c]:off[c + 1]], cell_list(boxes, G, c)), c
    check_connectivity(rg, x, tri)
    rg.close()


def _threshold_mesh():
    """G = 16.  In units of a cell (u, v; the bounding box of the mesh is 0.727 .. 15.27 in both): a triangle whose box is cells 0..7 x 0..7 (64 cells: the
    wide way), one of 9..15 x 0..8 (7 x 9 = 63: the narrow way, and it reaches column G - 1), and a band of 132 small triangles over rows 9 .. 15
    (its top row is row G - 1) that makes the mesh large enough for G = 16."""
    S, G = 100e3, 16
    at = lambda u: (np.asarray(u, float) * 1.1 / G - 0.05) * S          # noqa: E731   cell units -> metres (the box is [0, S]^2 plus 5 % each side)
    lo, hi = 0.05 * G / 1.1, 1.05 * G / 1.1                               # the box's corners in cell units
    px = [lo, 7.5, lo, 9.5, hi, 9.5]; py = [lo, lo, 7.5, lo, lo, 8.5]
    tris = [[0, 1, 2], [3, 4, 5]]
    nx, ny = 12, 7
    gu, gv = np.meshgrid(np.linspace(lo, hi, nx), np.linspace(9.5, hi, ny))
    base = len(px)
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = base + j * nx + i
            tris += [[a, a + 1, a + nx + 1], [a, a + nx + 1, a + nx]]
    x = at(np.concatenate([px, gu.ravel()])); y = at(np.concatenate([py, gv.ravel()]))
    x[[0, 2]] = 0.; y[[0, 1, 3, 4]] = 0.; x[4] = S                         # the corners exactly
    x[base:][gu.ravel() == lo] = 0.; x[base:][gu.ravel() == hi] = S; y[base:][gv.ravel() == hi] = S
    return x - 2e5, y + 3e5, np.array(tris, np.int32)


def test_bucket_grid_at_the_wide_threshold_and_at_the_rim():
    x, y, tri = _threshold_mesh()
    rg = _regrid(x, y, tri)
    G = grid_size(tri.shape[0])
    assert G == 16
    G, boxes, off, lst, pt, pc = check_grid(rg, x, y, tri, range(G * G))
    w, h = boxes[1] - boxes[0] + 1, boxes[3] - boxes[2] + 1
    assert (w[0], h[0]) == (8, 8) and (w[1], h[1]) == (7, 9) and w[0] * h[0] == WIDE and w[1] * h[1] == WIDE - 1
    assert ((w * h) >= WIDE).sum() == 1
    assert boxes[1][1] == G - 1 and boxes[3][2:].max() == G - 1 and boxes[1].max() == G - 1       # column G - 1 and row G - 1 are in use
    last_col = np.flatnonzero(np.diff(off)[G - 1::G]); last_row = np.flatnonzero(np.diff(off)[(G - 1) * G:])
    assert last_col.size >= 9 and last_row.size == G
    check_connectivity(rg, x, tri)
    rg.close()
    print(f"G = {G}: boxes of 8 x 8 = 64 (wide) and 7 x 9 = 63 (narrow) cells, {last_col.size} cells of column {G - 1} and {last_row.size} of row {G - 1} hold triangles; every cell compared")
