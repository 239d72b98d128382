"""The source of nxs_mapx_forward_point and of the nodal forcing kernels (nextsim_amd/csrc/nxs_mapx_body.inl, nxs_nodal_forcing_kernels.inl) compiled for the host
(tests/nodal_forcing_host_kernel.cpp, g++ -O2 -ffp-contract=off).  The projection against the REAL forward_mapx and the transform against the restated
transformData whose only projection is the real library's, both as the committed fixture holds them (tests/golden/mapx_forward.npz, made by
tests/golden/make_nodal_forcing_golden.py); the wrap and the blend against their numpy expressions (tests/nodal_forcing_ref.py): bit for bit.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import nodal_forcing_ref as R
from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mapx_forward.npz")
SIZES = (1, 2, 3, 4, 255, 256, 257, 511, 512, 513, 1026, 1027)      # Nn even and odd; below, at and above one and two blocks of 2 x 256 nodes


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "nodal_forcing_host_kernel")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "nodal_forcing_host_kernel.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def polar(name):
    m = dynamics.mapx_polar_north(**R.MPP[name])
    return m, np.array([getattr(m, k) for k in _abi.MAPX_POLAR_FIELDS])


def run(binary, tmp_path, payload):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(payload)
    subprocess.check_call([binary, fin, fout])
    return np.fromfile(fout)


def run_transform(binary, tmp_path, case, cyclic_x=False, cyclic_y=False):
    data = case["data"]
    M, N, nd = data.shape
    pairs = case["pairs"]
    j0, j1, ew = ([p[q] for p in pairs] + [0] * (4 - len(pairs)) for q in range(3))
    import math
    payload = struct.pack("12i", 1, M, N, nd, len(pairs), int(case["per_point"]), int(case["rotation_angle"] != 0.), int(cyclic_x), int(cyclic_y), 0, 0, 0)
    payload += struct.pack("12i", *j0, *j1, *(int(e) for e in ew)) + polar(case["map"])[1].tobytes()
    payload += struct.pack("2d", math.cos(-case["rotation_angle"]), math.sin(-case["rotation_angle"]))
    for a in (case["grid_y"], case["lat"], case["lon"], data):
        payload += np.ascontiguousarray(a, np.float64).tobytes()
    return run(binary, tmp_path, payload).reshape(M + int(cyclic_y), N + int(cyclic_x), nd)


@pytest.mark.parametrize("name", sorted(R.MPP))
def test_polar_north_gives_the_real_librarys_constants(gold, name):
    got = polar(name)[1]
    assert R.same_bits(got, gold["polar_" + name]).all(), dict(zip(_abi.MAPX_POLAR_FIELDS, got - gold["polar_" + name]))


@pytest.mark.parametrize("name", sorted(R.MPP))
def test_the_projection_source_on_the_host_gives_forward_mapxs_bits(binary, gold, tmp_path, name):
    lat, lon = R.forward_points()
    assert np.array_equal(lat, gold["lat"]) and np.array_equal(lon, gold["lon"])
    assert lat.min() == 20. and lat.max() == 90. and (lon < 0.).any() and (lon >= 360.).any() and ((lat == 90.).sum() >= 9) and (lon == 0.).sum() >= 29
    out = run(binary, tmp_path, struct.pack("2i", 0, lat.size) + polar(name)[1].tobytes() + lat.tobytes() + lon.tobytes())
    x, y = out[:lat.size], out[lat.size:]
    bad = ~(R.same_bits(x, gold["x_" + name]) & R.same_bits(y, gold["y_" + name]))
    assert not bad.any(), (int(bad.sum()), lat[bad][:5], lon[bad][:5], (x - gold["x_" + name])[bad][:5], (y - gold["y_" + name])[bad][:5])
    xl, yl = dynamics.mapx_forward(polar(name)[0], lat, lon, device=-1)      # the door's host side runs the same body
    assert np.abs(xl - x).max() <= 4 * R.U * np.abs(x).max() and np.abs(yl - y).max() <= 4 * R.U * np.abs(y).max()


@pytest.mark.parametrize("name", sorted(R.transform_cases()))
def test_the_transform_source_on_the_host_gives_the_fixtures_bits(binary, gold, tmp_path, name):
    case = R.transform_cases()[name]
    got, want = run_transform(binary, tmp_path, case), gold["t_" + name]
    bad = ~R.same_bits(got, want)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    data = case["data"]
    named = {j for p in case["pairs"] for j in p[:2] if p[2] or case["rotation_angle"] != 0.}
    for j in range(data.shape[2]):
        if j not in named:      # a scalar column, or a pair nothing is asked of: back byte for byte
            assert got[:, :, j].tobytes() == data[:, :, j].tobytes(), (name, j)
        else:
            assert not np.array_equal(got[:, :, j], data[:, :, j]), (name, j)
    zero = np.argwhere((data == 0.).all(axis=2))
    for yi, xi in zero:      # a zero vector stays 0., 0. (unless it lies in a pole row, which takes the mean)
        if case["grid_y"][yi] != 90.:
            for j in named:
                assert got[yi, xi, j] == 0., (name, yi, xi, j)


def test_the_fixtures_cases_are_the_ones_asked_for():
    c = R.transform_cases()
    assert sorted(v["data"].shape[:2] for v in c.values()) == [(2, 2), (5, 8), (5, 8), (5, 8), (33, 72), (33, 72)]
    assert any(v["grid_y"][0] == 90. for v in c.values()) and any(v["grid_y"][-1] == 90. for v in c.values()) and any(90. not in v["grid_y"] for v in c.values())
    assert any((v["data"] == 0.).all(axis=2).any() for v in c.values())
    assert any(v["per_point"] and (v["lat"] == 90.).any() and 90. not in v["grid_y"] for v in c.values())      # lat == 90 without a pole row
    assert any(v["rotation_angle"] != 0. for v in c.values()) and any(v["rotation_angle"] == 0. for v in c.values())
    assert any(len(v["pairs"]) == 2 and v["data"].shape[2] == 5 for v in c.values())                            # two pairs and a scalar column


@pytest.mark.parametrize("cyclic_x, cyclic_y", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", ["g5x8_pole_first_rotated", "g33x72_pole_last"])
def test_the_wrap_source_on_the_host_gives_numpys_bits(binary, gold, tmp_path, name, cyclic_x, cyclic_y):
    case = R.transform_cases()[name]
    got = run_transform(binary, tmp_path, case, cyclic_x, cyclic_y)
    want, _, _ = R.wrap(gold["t_" + name], case["lon"], case["lat"], cyclic_x, cyclic_y)
    assert R.same_bits(got, want).all()
    if cyclic_x and cyclic_y:
        assert (got[-1, -1] == 0.).all() and not np.signbit(got[-1, -1]).any()      # the corner neither loop of the reference reaches


def blend_case(Nn, shift):
    rng = np.random.default_rng(1000 * shift + Nn)
    d0, d1 = rng.normal(0., 10., 5 * Nn), rng.normal(0., 10., 5 * Nn)
    d0[::7] = 0.; d0[3::11] = -0.                                     # signed zeros
    d1[::5] = np.nan; d1[1::5] = np.inf; d1[2::9] = -np.inf           # what a STEP group must never see
    modes = [(R.LINEAR, 0.25, 0.75, 1., 0.), (R.STEP, 0.3, 0.7, -2., -0.), (R.OFF, 0., 0., 1., 0.), (R.LINEAR, 1., 0., 0., 0.5), (R.STEP, 0., 0., 0., -0.), (R.LINEAR, 0.5, 0.5, 1.5, -3.)]
    return d0, d1, [modes[(shift + k) % len(modes)] for k in range(3)]


@pytest.mark.parametrize("shift", range(6))
@pytest.mark.parametrize("Nn", SIZES)
def test_the_blend_source_on_the_host_gives_numpys_bits(binary, tmp_path, Nn, shift):
    d0, d1, tab = blend_case(Nn, shift)
    before = np.full(5 * Nn, -12345.678)
    payload = struct.pack("2i", 2, Nn) + b"".join(struct.pack("2i4d", m, 0, c0, c1, fa, bi) for m, c0, c1, fa, bi in tab) + d0.tobytes() + d1.tobytes() + before.tobytes()
    got = run(binary, tmp_path, payload)
    off = (0, 2 * Nn, 4 * Nn, 5 * Nn)
    for k, row in enumerate(tab):
        sl = slice(off[k], off[k + 1])
        want = R.blend(*row, d0[sl], d1[sl])
        if want is None:
            assert np.array_equal(got[sl], before[sl]), (k, "an OFF group was written")
            continue
        same = R.same_bits(got[sl], want)
        assert same.all(), (k, row, np.flatnonzero(~same)[:5], got[sl][~same][:3], want[~same][:3])
        if row[0] == R.STEP:
            assert np.isfinite(got[sl]).all(), (k, "a STEP group saw snapshot 1")
