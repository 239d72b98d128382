"""Conservative remapping between the mesh and a grid of quadrilateral cells (nxs_gridmap_*, include/nxs_interp.h), without a device: the per-cell
functions the kernels run (nextsim_amd/csrc/nxs_remap_core.inl with NC = 4) and host loops for the rest (tests/native/gridmap_host.cpp) against the
REAL contrib/bamg -- ConservativeRemappingWeights, ConservativeRemappingMeshToGrid, ConservativeRemappingGridToMesh -- as the committed golden file
holds it (tests/golden/bamg_grid_remap.npz).  Bar: equal as uint64; NaNs by position.  No device."""
import os
import sys

import numpy as np
import pytest

import grid_remap_ref as R
from oracle import pyoracle as O

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_golden  # noqa: E402
import make_grid_remap_golden as MG  # noqa: E402


@pytest.fixture(scope="module")
def binaries(tmp_path_factory):
    d = tmp_path_factory.mktemp("gridmap")
    return R.build_host(str(d / "gridmap_host")), R.build_host(str(d / "gridmap_host_san"), sanitize=True)


def _run(binary, tmp, name, nv):
    c = R.case(name)
    return c, R.run_host(binary, tmp, c["x"], c["y"], c["tri"], c["gridX"], c["gridY"], c["cornerX"].ravel(), c["cornerY"].ravel(),
                         c[f"m2g_in{nv}"], c[f"g2m_in{nv}"], local=c["local"])


@pytest.mark.parametrize("sanitized", [False, True])
@pytest.mark.parametrize("nv", [1, 7])
@pytest.mark.parametrize("name", R.CASES)
def test_host_build_of_the_device_code_gives_the_real_bamgs_bits(binaries, tmp_path, name, nv, sanitized):
    """lists, weights, restricted lists and both applications; the second build runs under AddressSanitizer and UBSan and must exit clean"""
    c, got = _run(binaries[int(sanitized)], tmp_path, name, nv)
    assert got["failed"] == 0
    assert (c["gridP"].size, c["tris"].size, got["longest"]) == R.COUNTS[name]     # no cell is left out of the comparison
    for k in ("gridP", "off", "tris", "r_gridP", "r_off", "r_tris"):
        assert np.array_equal(got[k], c[k]), k
    assert np.array_equal(R.bits(got["w"]), R.bits(c["w"])) and np.array_equal(R.bits(got["r_w"]), R.bits(c["r_w"]))
    assert R.same_bits(got["m2g_out"], c[f"m2g_out{nv}"])
    assert R.same_bits(got["g2m_out"], c[f"g2m_out{nv}"])


def test_the_cases_reach_what_they_are_there_for():
    c = R.case("long_rows")
    assert np.diff(c["off"]).max() > 96                      # beyond kMaxVisit, inside kMaxVisitBig
    assert R.case("all_land")["gridP"].size == 0 and R.case("one_cell")["gridP"].size == 1
    c = R.case("coarse")
    wet = np.zeros(c["gridX"].size, bool); wet[c["gridP"]] = True
    assert 0 < wet.sum() < wet.size
    assert np.array_equal(R.bits(c["m2g_out7"][~wet]), np.full((int((~wet).sum()), 7), np.float64(R.MISS)).view(np.uint64))   # land keeps miss_val
    assert np.isnan(c["m2g_out7"][wet]).any() and np.isinf(c["m2g_out7"][wet]).any()
    c = R.case("fine")
    assert np.unique(c["tris"], return_counts=True)[1].min() >= 2      # every triangle touched by several cells
    assert np.diff(c["off"]).max() <= 8
    c = R.case("inside")                                                   # "the whole cell is in the triangle" (counter == num_corners)
    alone = np.flatnonzero(np.diff(c["off"]) == 1)
    assert alone.size >= 10 and np.allclose(c["w"][c["off"][alone]], 250. * 250., rtol=1e-9)
    c = R.case("aligned")                                                  # the reference loses area on collinear edges; parity includes that
    rows_area = np.add.reduceat(c["w"], c["off"][:-1])
    assert (rows_area < 0.75 * 9e6).any()
    r = R.case("coarse")
    assert 0 < r["r_tris"].size < r["tris"].size and r["r_gridP"].size <= r["gridP"].size


def test_capacity_overflow_fails_the_cell_and_is_counted(binaries, tmp_path):
    c = R.case("long_rows")
    got = R.run_host(binaries[1], tmp_path, c["x"], c["y"], c["tri"], c["gridX"], c["gridY"], c["cornerX"].ravel(), c["cornerY"].ravel(),
                     c["m2g_in1"], c["g2m_in1"], cap=300)
    long = np.diff(c["off"]) > 300
    assert got["failed"] == int(long.sum()) > 0
    assert np.array_equal(got["gridP"], c["gridP"][~long])          # failed cells get no row; the others keep theirs
    assert got["longest"] <= 300


def test_a_cell_that_is_not_convex_overflows_its_points_or_stays_within_them(binaries, tmp_path):
    """A star-shaped "cell" over a fine mesh: whatever the walk does with it, it does inside its arrays (the sanitized build)."""
    c = R.case("long_rows")
    cx = np.array([[2000., 30000., 16000., 15000.]]); cy = np.array([[2000., 3000., 14000., 29000.]])   # corner 2 pulled inwards
    px, py = np.array([15000.]), np.array([8000.])
    got = R.run_host(binaries[1], tmp_path, c["x"], c["y"], c["tri"], px, py, cx.ravel(), cy.ravel(), c["m2g_in1"], np.zeros((1, 1)))
    assert got["failed"] + got["gridP"].size == 1


def test_three_corner_forms_still_give_the_regrid_fixture(tmp_path):
    """oracle/remap_host.cpp (frozen) compiles against the generalised core and gives tests/golden/bamg_remap.npz's bits."""
    import test_remap as T
    z = np.load(T.GOLD)
    for name in T.NAMES:
        out, visits, nf = T._host_remap(make_golden.remap_cases()[name], z[name + "_seed"])
        assert nf == 0 and np.array_equal(out.view(np.uint64), z[name].view(np.uint64)), name


@pytest.mark.skipif(O.bamg_shim() is None or not os.path.isdir(MG.REF), reason="the reference and oracle/_ref (real contrib/bamg) are not present here")
def test_real_bamg_regenerates_the_golden_file(tmp_path):
    dst = str(tmp_path / "again.npz")
    MG.make(dst)
    a, b = np.load(dst), np.load(R.GOLD)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
