"""Conservative remapping between the mesh and a grid of quadrilateral cells on the device (include/nxs_interp.h: nxs_gridmap_*; include/nxs_dyn.h:
nxs_dyn_means_to_grid_conservative) against the REAL contrib/bamg as tests/golden/bamg_grid_remap.npz holds it, and -- on grids and meshes the golden
file does not hold -- against tests/native/gridmap_host.cpp, the host build of the same per-cell code, which tests/test_grid_remap_host.py pins to
the golden file.  Bar: lists, weights and both applications bit for bit (NaNs by position: the sign of a generated NaN differs between x86 and gfx950)."""
import ctypes as C

import numpy as np
import pytest

import cases
import grid_remap_ref as R

pytestmark = pytest.mark.gpu

H2D, D2H = 1, 2
NXS_ERR_INVALID, NXS_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def host_binary(tmp_path_factory):
    return R.build_host(str(tmp_path_factory.mktemp("gridmap") / "gridmap_host"))


def _hip():
    from nextsim_amd import dynamics
    L = dynamics.load_library()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipFree.argtypes = [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    return L


class Dev:
    """a device array of doubles for the pointer variants"""

    def __init__(self, shape, src=None):
        self.L, self.shape, self.p = _hip(), shape, C.c_void_p()
        self.nbytes = int(np.prod(shape)) * 8
        assert self.L.hipMalloc(C.byref(self.p), max(self.nbytes, 8)) == 0
        if src is not None:
            src = np.ascontiguousarray(src, np.float64)
            assert self.L.hipMemcpy(self.p, src.ctypes.data, src.nbytes, H2D) == 0

    def get(self):
        out = np.empty(self.shape)
        assert self.L.hipMemcpy(out.ctypes.data, self.p, out.nbytes, D2H) == 0
        return out

    def free(self):
        self.L.hipFree(self.p)


def _make(x, y, tri, gx, gy, cx, cy):
    from nextsim_amd import interp
    rg = interp.Regrid(np.ascontiguousarray((tri + 1).ravel(), np.int32), x, y)
    return rg, interp.GridMap.weights(rg, gx, gy, cx, cy)


def _case_map(name):
    c = R.case(name)
    rg, gm = _make(c["x"], c["y"], c["tri"], c["gridX"], c["gridY"], c["cornerX"], c["cornerY"])
    return c, rg, gm


def _lists_equal(e, want, prefix=""):
    for k in ("gridP", "off", "tris"):
        assert np.array_equal(e[k], want[prefix + k]), k
    assert np.array_equal(R.bits(e["w"]), R.bits(want[prefix + "w"]))


@pytest.mark.parametrize("name", R.CASES)
def test_weights_of_every_golden_case_are_the_real_bamgs(name):
    c, rg, gm = _case_map(name)
    info = gm.info()
    wet, entries, longest = R.COUNTS[name]
    assert info == {"wet": wet, "entries": entries, "longest": longest, "failed": 0, "nels": c["tri"].shape[0], "grid_size": c["gridX"].size}
    assert (c["gridP"].size, c["tris"].size) == (wet, entries)          # the golden's own counts: no cell is left out
    e = gm.export()
    _lists_equal(e, c)
    assert np.array_equal(R.bits(e["cornerX"]), R.bits(c["cornerX"])) and np.array_equal(R.bits(e["cornerY"]), R.bits(c["cornerY"]))
    gm.close(); rg.close()


@pytest.mark.parametrize("nv", [1, 7])
@pytest.mark.parametrize("name", R.CASES)
def test_both_applications_bit_for_bit_host_and_device_pointers_and_miss_values(name, nv):
    c, rg, gm = _case_map(name)
    G, nels = c["gridX"].size, c["tri"].shape[0]
    wet = np.zeros(G, bool); wet[c["gridP"]] = True
    m_in, m_want = c[f"m2g_in{nv}"], c[f"m2g_out{nv}"]
    g_in, g_want = c[f"g2m_in{nv}"], c[f"g2m_out{nv}"]
    d_min, d_gin = Dev((nels, nv), m_in), Dev((G, nv), g_in)
    for in_dev in (False, True):
        for out_dev in (False, True):
            d_mout, d_gout = Dev((G, nv)), Dev((nels, nv))
            kw_m = dict(in_device=(d_min.p.value, nv) if in_dev else None, out_device=d_mout.p.value if out_dev else None)
            kw_g = dict(in_device=(d_gin.p.value, nv) if in_dev else None, out_device=d_gout.p.value if out_dev else None)
            got = gm.mesh_to_grid(None if in_dev else m_in, R.MISS, **kw_m)
            got = d_mout.get() if out_dev else got
            assert R.same_bits(got, m_want), (in_dev, out_dev)
            got = gm.grid_to_mesh(None if in_dev else g_in, **kw_g)
            got = d_gout.get() if out_dev else got
            assert R.same_bits(got, g_want), (in_dev, out_dev)
            d_mout.free(); d_gout.free()
    for miss in (0., -0., 1e14):
        got = gm.mesh_to_grid(m_in, miss)
        assert R.same_bits(got[wet], m_want[wet])
        assert np.array_equal(R.bits(got[~wet]), np.full(got[~wet].shape, miss).view(np.uint64))      # its bits preserved on land cells
    untouched = np.ones(nels, bool); untouched[c["tris"]] = False
    if wet.any():
        assert np.isnan(g_want[untouched]).all()                       # 0 * (1 / 0.), as in the reference
    d_min.free(); d_gin.free(); gm.close(); rg.close()


@pytest.mark.parametrize("name", ["coarse", "long_rows", "fine", "aligned", "one_cell"])
def test_restrict_gives_the_filtered_lists_and_export_import_the_same_results(name):
    from nextsim_amd import interp
    c, rg, gm = _case_map(name)
    nloc = int((c["local"] >= 0).sum())
    r = gm.restrict(c["local"], nloc)
    _lists_equal(r.export(), c, "r_")
    i = r.info()
    assert (i["wet"], i["entries"], i["nels"], i["grid_size"], i["failed"]) == (c["r_gridP"].size, c["r_tris"].size, nloc, c["gridX"].size, 0)
    # the restricted map applied to the local rows: the partition's share of every sum.  The full map on rows that are 0. outside the partition adds only
    # +-0. terms in between, so wherever both are finite and not zero the two agree bit for bit.
    keep = c["local"] >= 0
    local_in = c["m2g_in7"][keep]
    got = r.mesh_to_grid(local_in, 0.)
    full = gm.mesh_to_grid(np.where(keep[:, None], c["m2g_in7"], 0.), 0.)
    rows = c["r_gridP"]
    cmp = np.isfinite(full[rows]) & np.isfinite(got[rows]) & (full[rows] != 0.)
    assert cmp.any() and np.array_equal(R.bits(got[rows][cmp]), R.bits(full[rows][cmp]))
    again = interp.GridMap.import_(r.export())
    assert R.same_bits(again.mesh_to_grid(local_in, 0.), got)
    # export -> import: the same lists and the same results
    e = gm.export()
    twin = interp.GridMap.import_(e)
    _lists_equal(twin.export(), c)
    for nv in (1, 7):
        assert R.same_bits(twin.mesh_to_grid(c[f"m2g_in{nv}"], R.MISS), c[f"m2g_out{nv}"])
        assert R.same_bits(twin.grid_to_mesh(c[f"g2m_in{nv}"]), c[f"g2m_out{nv}"])
    for m in (r, again, twin, gm):
        m.close()
    rg.close()


@pytest.mark.parametrize("n_wet", [1, 63, 64, 65, 257])
def test_sizes_at_the_launch_edges(host_binary, tmp_path, n_wet):
    """`fine`'s grid cut (and, beyond its 97 wet cells, repeated) to n_wet wet cells with a land cell after every 16th: the walk's blocks of 64 cells, the
    compaction's of 4, the 256 lanes of the row kernel and of the two applications."""
    c = R.case("fine")
    wet = c["gridP"]
    land = np.setdiff1d(np.arange(c["gridX"].size), wet)
    sel = []
    for k in range(n_wet):
        sel.append(wet[k % wet.size])
        if k % 16 == 15:
            sel.append(land[(k // 16) % land.size])
    sel = np.array(sel)
    gx, gy, cx, cy = c["gridX"][sel], c["gridY"][sel], c["cornerX"][sel], c["cornerY"][sel]
    rng = np.random.default_rng(n_wet)
    m_in, g_in = rng.standard_normal((c["tri"].shape[0], 3)), rng.standard_normal((sel.size, 3))
    want = R.run_host(host_binary, tmp_path, c["x"], c["y"], c["tri"], gx, gy, cx.ravel(), cy.ravel(), m_in, g_in, miss=-7.)
    rg, gm = _make(c["x"], c["y"], c["tri"], gx, gy, cx, cy)
    i = gm.info()
    assert (i["wet"], i["failed"], i["entries"], i["longest"]) == (n_wet, 0, want["tris"].size, want["longest"]) and want["failed"] == 0
    # the rows are the golden's rows of the chosen cells
    for row in (0, n_wet - 1):
        src = int(np.flatnonzero(wet == sel[want["gridP"][row]])[0])
        lo, hi = want["off"][row], want["off"][row + 1]
        assert np.array_equal(want["tris"][lo:hi], c["tris"][c["off"][src]:c["off"][src + 1]])
        assert np.array_equal(R.bits(want["w"][lo:hi]), R.bits(c["w"][c["off"][src]:c["off"][src + 1]]))
    _lists_equal(gm.export(), want)
    assert R.same_bits(gm.mesh_to_grid(m_in, -7.), want["m2g_out"])
    assert R.same_bits(gm.grid_to_mesh(g_in), want["g2m_out"])
    gm.close(); rg.close()


def test_long_rows_built_in_chunks_of_four_cells():
    """more than one chunk: the arena is reused and the offsets run on across the chunks"""
    from nextsim_amd import interp
    interp.gridmap_debug_chunk(4)
    try:
        c, rg, gm = _case_map("long_rows")
        assert interp.gridmap_debug_chunk(4) == 2          # 6 wet cells
        assert gm.info()["failed"] == 0 and gm.info()["longest"] == 373 > 96
        _lists_equal(gm.export(), c)
        assert R.same_bits(gm.grid_to_mesh(c["g2m_in7"]), c["g2m_out7"])
        gm.close(); rg.close()
    finally:
        interp.gridmap_debug_chunk(0)
    c, rg, gm = _case_map("long_rows")
    assert interp.gridmap_debug_chunk(0) == 1
    gm.close(); rg.close()


def test_create_destroy_cycles_return_the_device_memory():
    """Two create / destroy cycles (context, map, restricted map, both applications) leave no less free device memory than there was.  The grid is `fine`'s
    wet cells repeated to 257, so that the walk's arena alone is 257 x 82 KB = 21 MB a cycle: what a cycle kept would show far above the 2 MiB blocks in
    which the runtime takes and returns memory (which is why the value may come back LARGER than it was)."""
    L = _hip()
    c = R.case("fine")
    sel = np.resize(c["gridP"], 257)
    gx, gy, cx, cy = c["gridX"][sel], c["gridY"][sel], c["cornerX"][sel], c["cornerY"][sel]
    g_in = np.ones((sel.size, 7))

    def free_bytes():
        a, b = C.c_size_t(), C.c_size_t()
        assert L.hipMemGetInfo(C.byref(a), C.byref(b)) == 0
        return a.value

    def cycle():
        rg, gm = _make(c["x"], c["y"], c["tri"], gx, gy, cx, cy)
        assert gm.info()["wet"] == 257
        r = gm.restrict(c["local"], int((c["local"] >= 0).sum()))
        gm.mesh_to_grid(c["m2g_in7"]); gm.grid_to_mesh(g_in)
        r.close(); gm.close(); rg.close()
    cycle(); cycle()
    start = free_bytes()
    cycle(); cycle()
    end = free_bytes()
    print(f"free device memory: {start} before, {end} after two cycles")
    assert end >= start


def test_argument_checks_on_the_device():
    from nextsim_amd import interp
    from nextsim_amd.interp import NxsError
    c, rg, gm = _case_map("one_cell")
    with pytest.raises(NxsError) as e:
        interp.GridMap.weights(rg, np.zeros(0), np.zeros(0), np.zeros((0, 4)), np.zeros((0, 4)))
    assert e.value.code == -1
    with pytest.raises(NxsError) as e:
        gm.mesh_to_grid(np.zeros((c["tri"].shape[0], 0)))
    assert e.value.code == -1
    bad = gm.export(); bad["tris"] = bad["tris"].copy(); bad["tris"][0] = bad["nels"]
    with pytest.raises(NxsError) as e:
        interp.GridMap.import_(bad)
    assert e.value.code == -1
    with pytest.raises(NxsError) as e:
        gm.restrict(np.full(c["tri"].shape[0], 5, np.int32), 5)
    assert e.value.code == -1
    gm.close(); rg.close()


# ---- the handle: updateGridMean's elemental leg on a loaded grid -----------------------------------------------------------------------------------------

ELEMENTAL = ("conc", "thick", ("damage", True), "ice_mask", ("sigma_11", True))


def _toy_grid(lm):
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_grid_remap_golden as MG
    x, y = lm.coord_x, lm.coord_y
    return MG.grid(7, 7, 17000., 0.2, 0.5 * (x.min() + x.max()), 0.5 * (y.min() + y.max()))


def test_means_to_grid_conservative_on_the_toy_mesh(host_binary, tmp_path):
    from nextsim_amd import dynamics, interp
    gm_, p, g, lms, fields = cases.make_case("toy")
    lm, f = lms[0], fields[0]
    assert lm.num_elements == 2368
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3) - 1, np.int32)
    gx, gy, cx, cy = _toy_grid(lm)
    G = gx.size
    rg, gmap = _make(lm.coord_x, lm.coord_y, tri, gx, gy, cx, cy)
    assert gmap.info()["failed"] == 0 and 0 < gmap.info()["wet"] < G
    # 1. nothing configured
    with pytest.raises(dynamics.NxsError) as e:
        fe.means_to_grid_conservative(gmap)
    assert e.value.code == NXS_ERR_STATE
    fe.means_configure(ELEMENTAL, ("VT_x",))
    for _ in range(3):
        fe.step()
        fe.means_update(1. / 3.)
    el0, nod0, de, dn = fe.means_get()
    grid0 = fe.means_to_grid(lm.coord_x.min(), lm.coord_y.max(), 10000., 10, 10)
    # the host application (pinned to the real bamg by tests/test_grid_remap_host.py) on means_get's rows, missing value 0.
    want = R.run_host(host_binary, tmp_path, lm.coord_x, lm.coord_y, tri, gx, gy, cx.ravel(), cy.ravel(), el0, np.zeros((G, el0.shape[1])), miss=0.)
    _lists_equal(gmap.export(), want)
    m2g = want["m2g_out"]                                    # [G][n_el]
    miss = -1e14
    start = np.zeros((len(ELEMENTAL), G))
    got = fe.means_to_grid_conservative(gmap, miss, start)
    assert got is start

    def masked(grid):
        out = grid.copy()
        ice = out[3]
        for k, v in enumerate(ELEMENTAL):
            if isinstance(v, tuple) and v[1]:
                out[k] = np.where((ice <= 0.) & (out[k] != miss), 0., out[k])
        return out
    assert R.same_bits(got, masked(0. + m2g.T))
    wet = np.zeros(G, bool); wet[want["gridP"]] = True
    assert (got[3][wet] > 0).any() and (got[0][~wet] == 0).all()          # land cells got the missing value 0., not miss_val
    # 2. the += into grids that are not zero, and a masked variable where the ice mask is not positive
    base = np.random.default_rng(3).standard_normal((len(ELEMENTAL), G))
    base[3] = np.where(np.arange(G) % 2 == 0, -5., 0.5)                    # every other cell ends with ice_mask <= 0 on land and on thin rows
    base[2, 5] = miss                                                       # a cell that already holds miss_val keeps it
    grid = base.copy()
    fe.means_to_grid_conservative(gmap, miss, grid)
    plus = base + m2g.T
    assert R.same_bits(grid, masked(plus))
    assert (masked(plus) != plus).any()
    # 3. the regular-grid route and the accumulators are untouched, bit for bit
    el1, nod1, _, _ = fe.means_get()
    assert R.same_bits(el1, el0) and R.same_bits(nod1, nod0)
    grid1 = fe.means_to_grid(lm.coord_x.min(), lm.coord_y.max(), 10000., 10, 10)
    assert R.same_bits(grid1[0], grid0[0]) and R.same_bits(grid1[1], grid0[1])
    # 4. a map on another mesh
    c, rg2, other = _case_map("one_cell")
    with pytest.raises(dynamics.NxsError) as e:
        fe.means_to_grid_conservative(other)
    assert e.value.code == NXS_ERR_STATE
    # 5. a mask flag without ice_mask is refused at nxs_dyn_means_configure already (NXS_ERR_INVALID) and leaves the configuration that was there
    with pytest.raises(dynamics.NxsError) as e:
        fe.means_configure((("conc", True),), ())
    assert e.value.code == -1
    again = fe.means_to_grid_conservative(gmap, miss, np.zeros((len(ELEMENTAL), G)))
    assert R.same_bits(again, got)
    other.close(); rg2.close(); gmap.close(); rg.close(); fe.close()
