"""The source of the two element-forcing kernels (nextsim_amd/csrc/nxs_thermo_forcing_kernels.inl, with the shared nxs_grid_to_mesh_body.inl) compiled for the host
(tests/thermo_forcing_host_kernel.cpp).  The blend against the numpy expression of ExternalData::get (tests/thermo_forcing_ref.py), the ingest against the REAL bamg's
InterpFromGridToMeshx as the committed golden file holds it (tests/golden/bamg_grid_to_mesh.npz): bit for bit, without contraction on either side.  So the
transcription -- the 16-byte pairs and the odd tail, the row table, the routing of columns to rows and snapshots -- is checked without a device; what
tests/test_gpu_thermo_forcing.py adds is the device and the handle.  No device."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import thermo_forcing_ref as R

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bamg_grid_to_mesh.npz")
NAMES = ("bilinear", "triangle", "nearest", "contours_nan", "row_major")
SIZES = (1, 2, 3, 255, 256, 257, 1027)      # below, at and above a block of 256 lanes; 1027: odd, above two blocks of 2 x 256 elements


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "thermo_forcing_host_kernel")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "thermo_forcing_host_kernel.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("Ne", SIZES)
def test_the_blend_source_on_the_host_gives_numpys_bits(binary, tmp_path, Ne, shift):
    tab = R.table(shift)
    d0, d1 = R.snapshots(Ne)
    before = np.full((10, Ne), -12345.678)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("2i", 0, Ne))
        for mode, c0, c1, factor, bias in tab:
            f.write(struct.pack("2i4d", mode, 0, c0, c1, factor, bias))
        f.write(d0.tobytes()); f.write(d1.tobytes()); f.write(before.tobytes())
    subprocess.check_call([binary, fin, fout])
    got = np.fromfile(fout).reshape(10, Ne)
    seen = set()
    for k, row in enumerate(tab):
        want = R.blend(row, d0[k], d1[k])
        if want is None:
            assert np.array_equal(got[k], before[k]), (k, "an OFF row was written")
            continue
        same = R.same_bits(got[k], want)
        assert same.all(), (k, row, np.flatnonzero(~same)[:5], got[k][~same][:3], want[~same][:3])
        if row[0] == R.STEP and row[3] != 0.:
            assert np.isfinite(got[k]).all(), (k, "a STEP row saw snapshot 1")      # d1 holds NaN and +-Inf, d0 does not
        seen.add(row[0])
    assert seen == {R.LINEAR, R.STEP}
    if Ne >= 255:      # the table is not vacuous: LINEAR with (1, 0) and STEP differ (the sign of zero, NaN in d1), and the signed zeros are there
        lin10 = next(k for k, r in enumerate(tab) if r[:3] == (R.LINEAR, 1., 0.) and r[3] == 1.)
        assert not R.same_bits(got[lin10], R.blend((R.STEP, 0., 0., 1., -0.), d0[lin10], d1[lin10])).all()
        live = got[np.array([r[0] != R.OFF for r in tab])]
        assert np.signbit(live[live == 0]).any()


@pytest.mark.parametrize("skip", [0, 1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_the_ingest_source_on_the_host_gives_the_real_bamgs_bits(binary, tmp_path, name, skip):
    """every seeded case as it lies; its three columns go to rows and snapshots by a permutation, one column skipped (each in turn)"""
    z = np.load(GOLD)
    xs, ys, data, xm, ym, interp, rm = make_golden.grid_to_mesh_cases()[name]
    want = z[name]                                   # [nods, 3]
    Ne, N_data = xm.size, data.shape[2]
    M, N = (data.shape[1], data.shape[0]) if rm else (data.shape[0], data.shape[1])
    rng = np.random.default_rng(NAMES.index(name) * 3 + skip)
    slots = rng.permutation(20)[:N_data]             # distinct (snapshot, row) pairs
    row, snap = (slots % 10).astype(np.int32), (slots // 10).astype(np.int32)
    row[skip] = -1
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("10i", 1, Ne, M, N, N_data, xs.size, ys.size, interp, int(rm), 0))
        f.write(struct.pack("d", 1e8))
        for a in (xs, ys, data, xm, ym):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(row.tobytes()); f.write(snap.tobytes())
    subprocess.check_call([binary, fin, fout])
    got = np.fromfile(fout).reshape(2, 10, Ne)
    written = np.zeros((2, 10), bool)
    for j in range(N_data):
        if row[j] < 0:
            continue
        assert np.array_equal(got[snap[j], row[j]], want[:, j]), (name, j, int(row[j]), int(snap[j]))
        written[snap[j], row[j]] = True
    assert written.sum() == N_data - 1 and (got[~written] == -777.).all()      # the skipped column went nowhere
    assert Ne % 256 != 0 and Ne > 256                                           # a ragged last block, more than one block
