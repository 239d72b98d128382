"""The device code of the coupler's put compiled for the host (tests/cpl_out_host_kernel.cpp: nxs_remap::grid_values<NV> inside the loops of k_gridmap_send /
nxs_gridmap_send_rows, and nxs_fsd_diag_body.inl) against the fixtures of the real bamg and tests/cpl_out_ref.py: bit for bit, NaN equal to NaN.  The same program
runs once under -fsanitize=address,undefined as a stand-alone binary.  No device."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import cpl_out_ref as CO  # noqa: E402
import grid_remap_ref as G  # noqa: E402
from test_cpl_out_ref import fsd_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EL = (1, 4, 5, 8, 9, 12, 13, 24)          # every build, the tile edge and the cap (NXS_MEANS_MAX_VARS)


def _build(dst, sanitize=False):
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc")]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "cpl_out_host_kernel.cpp"), "-o", dst])
    return dst


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("hostk") / "cpl_out_host_kernel"))


def run_send(binary, tmp, lists, nels, data_mesh, data_grid):
    data_mesh = np.ascontiguousarray(data_mesh, np.float64)
    fin, fout = os.path.join(str(tmp), "send_in.bin"), os.path.join(str(tmp), "send_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("5i", nels, lists["G"], lists["gridP"].size, lists["tris"].size, data_mesh.shape[1]))
        for a in (lists["gridP"], lists["off"], lists["tris"]):
            f.write(np.ascontiguousarray(a, np.int32).tobytes())
        for a in (lists["w"], lists["cornerX"], lists["cornerY"], data_mesh, data_grid):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    subprocess.check_call([binary, "send", fin, fout])
    return np.fromfile(fout).reshape(data_mesh.shape[1], lists["G"])


def run_fsd(binary, tmp, mech, D_conc, up, centres, opts=None):
    o = dict(CO.DEFAULTS, **(opts or {}))
    nb, n = mech.shape
    pad = lambda a: np.concatenate([np.asarray(a, np.float64), np.zeros(16 - len(a))])   # noqa: E731
    fin, fout = os.path.join(str(tmp), "fsd_in.bin"), os.path.join(str(tmp), "fsd_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("2i", nb, n))
        f.write(struct.pack("3d", o["dmax_c_threshold"], o["fsd_unbroken_floe_size"], o["fsd_min_floe_size"]))
        for a in (pad(up), pad(centres), mech, D_conc):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    subprocess.check_call([binary, "fsd", fin, fout])
    return np.fromfile(fout).reshape(2, n)


def awkward_rows(nels, n_el, seed=3):
    """mesh accumulators with negative values, a zero row, a -0. and one NaN triangle"""
    rng = np.random.default_rng(seed + n_el)
    a = rng.normal(0., 3., (nels, n_el))
    a[nels // 3] = 0.
    a[nels // 2, 0] = -0.
    a[(2 * nels) // 3] = np.nan
    return a


def awkward_grid(n_el, Gs, seed=9):
    g = np.random.default_rng(seed).normal(0., 1., (n_el, Gs))
    g[:, ::7] = -0.                                               # the += turns these into +0. on dry cells and zero sums
    return g


@pytest.mark.parametrize("name", G.CASES)
def test_the_send_body_on_the_golden_lists(binary, tmp_path, name):
    c = G.case(name)
    lists, nels = CO.lists_of(c), c["tri"].shape[0]
    wet = np.zeros(lists["G"], bool)
    wet[lists["gridP"]] = True
    for nv in (1, 7):                                             # the real bamg's outputs
        got = run_send(binary, tmp_path, lists, nels, c[f"m2g_in{nv}"], np.zeros((nv, lists["G"])))
        assert G.same_bits(got.T[wet] + 0., c[f"m2g_out{nv}"][wet] + 0.) and not got.T[~wet].any() and not np.signbit(got.T[~wet]).any()
    for n_el in N_EL:
        el, grid = awkward_rows(nels, n_el), awkward_grid(n_el, lists["G"])
        got = run_send(binary, tmp_path, lists, nels, el, grid)
        assert G.same_bits(got, CO.send_rows(lists, el, grid.copy())), (name, n_el)


@pytest.mark.parametrize("nb", [1, 2, 12, 16])
def test_the_fsd_diag_body(binary, tmp_path, nb):
    mech, D_conc, up, centres = fsd_case(nb)
    got = run_fsd(binary, tmp_path, mech, D_conc, up, centres)
    want = CO.fsd_diag(mech, D_conc, up, centres)
    assert G.same_bits(got[0], want[0]) and G.same_bits(got[1], want[1])
    opts = {"dmax_c_threshold": 0.25, "fsd_unbroken_floe_size": 300., "fsd_min_floe_size": 35.}
    got = run_fsd(binary, tmp_path, mech, D_conc, up, centres, opts)
    want = CO.fsd_diag(mech, D_conc, up, centres, **opts)
    assert G.same_bits(got[0], want[0]) and G.same_bits(got[1], want[1])
    none = run_fsd(binary, tmp_path, np.zeros((0, D_conc.size)), D_conc, up, centres)      # M_num_fsd_bins == 0
    assert not none.any()


def test_the_same_program_under_the_sanitizers(tmp_path):
    exe = _build(str(tmp_path / "cpl_out_host_kernel_san"), sanitize=True)
    for name in ("long_rows", "all_land", "one_cell"):
        c = G.case(name)
        lists, nels = CO.lists_of(c), c["tri"].shape[0]
        for n_el in (5, 13, 24):
            el, grid = awkward_rows(nels, n_el), awkward_grid(n_el, lists["G"])
            assert G.same_bits(run_send(exe, tmp_path, lists, nels, el, grid), CO.send_rows(lists, el, grid.copy()))
    for nb in (1, 16):
        mech, D_conc, up, centres = fsd_case(nb)
        got = run_fsd(exe, tmp_path, mech, D_conc, up, centres)
        want = CO.fsd_diag(mech, D_conc, up, centres)
        assert G.same_bits(got[0], want[0]) and G.same_bits(got[1], want[1])
