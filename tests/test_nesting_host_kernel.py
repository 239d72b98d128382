"""The source of the nesting and diffusion kernels (nextsim_amd/csrc/nxs_nesting_kernels.inl) compiled for the host (tests/nesting_host_kernel.cpp) against the numpy
restatement of nestingIce(), nestingDynamics(), diffuse() and ExternalData::get (tests/nesting_ref.py): bit for bit, without contraction on either side, the
exponential too (the host's exp on both sides).  So the transcription -- the 16-byte pairs and the odd tails, the records' two halves, the second half of M_VT at an
odd node count, the gathers through the table -- is checked without a device; what tests/test_gpu_nesting.py adds is the device and the handle.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cases
import nesting_ref as R
from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 255, 256, 257, 1027)      # below, at and above a block of 256 lanes; 1027: odd, above two blocks of 2 x 256 elements
STATE_ROWS = ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young", "sigma0", "sigma1", "sigma2", "damage", "ridge_ratio")
# (young-ice rows, where sigma and the damage live, the datasets' table)
VARIANTS = {"young-arrays": (True, "arrays", R.TIMES), "classic-records-bbm": (False, "records_bbm", R.TIMES_B), "young-records-evp": (True, "records_evp", R.TIMES),
            "classic-arrays-b": (False, "arrays", R.TIMES_B)}


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "nesting_host_kernel")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "nesting_host_kernel.cpp"), "-o", exe])
    return exe


def _nodes(Ne):
    return Ne // 2 + 3      # never Ne; above it (1, 2, 3), below it, odd (3, 131) and even (4, 130, 516): the second half of M_VT is 16-byte aligned or not


def _run_nudge(binary, tmp_path, which, Ne, Nn, cfg, young, home, times, s0, s1, st):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec, dmg_rec = int(home != "arrays"), int(home == "records_bbm")
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", 0, Ne, Nn, _abi.NUDGE_FUNCTIONS[cfg["nudge_function"]], int(young), rec, dmg_rec, which))
        f.write(struct.pack("3d", cfg["nudge_scale"], np.float64(cfg["time_step"]) / np.float64(cfg["nudge_timescale"]),
                            np.float64(cfg["dtime_step"]) / np.float64(cfg["nudge_timescale"])))
        for ds in _abi.NEST_DATASETS:
            m, c0, c1, fac, bias = times[ds]
            f.write(struct.pack("2i4d", m, 0, c0, c1, fac, bias))
        for s in (s0, s1):
            for k in _abi.NEST_ELEMENT_ROWS + _abi.NEST_NODE_ROWS:
                f.write(np.ascontiguousarray(s[k], np.float64).tobytes())
        for k in STATE_ROWS:
            f.write(st[k].tobytes())
        f.write(st["VT"].tobytes())
    subprocess.check_call([binary, fin, fout])
    raw = np.fromfile(fout)
    assert raw.size == 12 * Ne + 2 * Nn
    got = {k: raw[j * Ne:(j + 1) * Ne] for j, k in enumerate(STATE_ROWS)}
    got["VT"] = raw[11 * Ne:11 * Ne + 2 * Nn]
    return got, raw[11 * Ne + 2 * Nn:]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("function", ["linear", "exponential"])
@pytest.mark.parametrize("Ne", SIZES)
def test_the_nudge_source_on_the_host_gives_numpys_bits(binary, tmp_path, Ne, function, variant):
    young, home, times = VARIANTS[variant]
    Nn = _nodes(Ne)
    cfg = dict(R.CFG, nudge_function=function)
    s0, s1 = R.snapshots(Ne, Nn, times, cfg["nudge_scale"])
    st0 = R.state(Ne, Nn)
    # nestingIce
    want = R.nesting_ice({k: v.copy() for k, v in st0.items()}, (s0, s1), times, cfg, young)
    got, _ = _run_nudge(binary, tmp_path, 0, Ne, Nn, cfg, young, home, times, s0, s1, st0)
    for k in want:
        same = R.same_bits(got[k], want[k])
        assert same.all(), ("ice", k, np.flatnonzero(~same)[:5], got[k][~same][:3], want[k][~same][:3])
    touched = ("conc", "thick", "snow_thick") + (("conc_young", "h_young", "hs_young") if young else ())
    for k in st0:                                                            # no row the loop does not name moved
        assert k in touched or got[k].tobytes() == st0[k].tobytes(), k
        assert np.isfinite(got[k]).all(), (k, "a STEP dataset saw snapshot 1")
    # nestingDynamics
    want = R.nesting_dynamics({k: v.copy() for k, v in st0.items()}, (s0, s1), times, cfg)
    got, slot3 = _run_nudge(binary, tmp_path, 1, Ne, Nn, cfg, young, home, times, s0, s1, st0)
    for k in want:
        same = R.same_bits(got[k], want[k])
        assert same.all(), ("dynamics", home, k, np.flatnonzero(~same)[:5], got[k][~same][:3], want[k][~same][:3])
        assert np.isfinite(got[k]).all(), (k, "a STEP dataset saw snapshot 1")
    if home == "records_evp":
        assert (slot3 == -777.).all()                                        # the slot that is not the damage went back with its bits
    if function == "linear":
        fN = R.f_nudge("linear", R.get(times["distance_elements"], s0["dist"], s1["dist"]), cfg["nudge_scale"])
        assert fN[-1] == 0. and (Ne < 3 or (fN[0] == 1. and fN[Ne // 2] == 0. and ((fN > 0) & (fN < 1)).any() == (Ne > 3)))
        # fNudge = 0: the row is rewritten as x + 0*(...), so the last entry (a signed zero in every row) is a zero again -- with the sign numpy gives it (above)
        zeros = np.array([got[k][-1] for k in ("sigma0", "sigma1", "sigma2", "damage", "ridge_ratio")])
        assert (zeros == 0.).all() and not np.signbit(zeros[[0, 2, 4]]).any()      # (+0.0 went in there: +0.0 + (+-0.0) is +0.0)
    else:
        fN = R.f_nudge("exponential", R.get(times["distance_elements"], s0["dist"], s1["dist"]), cfg["nudge_scale"])
        assert ((fN > 0) & (fN <= 1)).all() and (Ne < 3 or fN[0] == 1.)


# ---- diffuse ----------------------------------------------------------------------------------------------------------------------------------
def _mesh(n, Ne, shuffle):
    """the first Ne triangles of cases.rect_mesh(n, 1); shuffle: in a random numbering, so that neighbours are far apart and the table is not banded"""
    x, y, tri, _ = cases.rect_mesh(n, 1)
    if Ne == 2:                                                              # a triangle and the one across its first edge: each the other's only neighbour
        full = dynamics.mesh_element_connectivity(np.ascontiguousarray(tri + 1, np.int32).ravel(), x.size)
        e = int(np.flatnonzero(~np.isnan(full[:, 0]))[0])
        tri = tri[[e, int(full[e, 0]) - 1]]
    tri = tri[:Ne] if Ne else tri
    if shuffle:
        tri = tri[np.random.default_rng(5).permutation(tri.shape[0])]
    ec = dynamics.mesh_element_connectivity(np.ascontiguousarray(tri + 1, np.int32).ravel(), x.size)
    return np.ascontiguousarray(tri, np.int32), ec


def _table(ec):
    return np.ascontiguousarray(np.where(np.isnan(ec), 0, ec).astype(np.int32) - 1)


def _run_diffuse(binary, tmp_path, ec, sst, sss, k_sst, k_sss, dx, dt):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    Ne = sst.size
    factor = [np.float64(k) * np.float64(dt) / np.float64(np.power(np.float64(dx), 2.)) for k in (k_sst, k_sss)]
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", 1, Ne, int(k_sst > 0), int(k_sss > 0), 0, 0, 0, 0))
        f.write(struct.pack("2d", *factor))
        f.write(_table(ec).tobytes()); f.write(sst.tobytes()); f.write(sss.tobytes())
    subprocess.check_call([binary, fin, fout])
    raw = np.fromfile(fout)
    return raw[:Ne], raw[Ne:]


def _fields(Ne, seed=0):
    rng = np.random.default_rng(seed + Ne)
    sst, sss = rng.normal(size=Ne) - 1., 33. + rng.normal(size=Ne)
    sst[Ne // 2] = -0.
    sss[0] = -0.
    return sst, sss


DIFF_MESHES = [(1, 1), (1, 2), (10, 255), (10, 256), (10, 257), (20, 0)]      # (n of rect_mesh, the first Ne triangles; 0: all 894 = 3 blocks and a ragged fourth)
DIFF_ON = {"sst": (1200., 0.), "sss": (0., 350.), "both": (1200., 350.), "sst-negative-sss": (800., -5.), "none": (0., -1.)}


@pytest.mark.parametrize("on", DIFF_ON)
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("n,Ne", DIFF_MESHES)
def test_the_diffusion_source_on_the_host_gives_numpys_bits(binary, tmp_path, n, Ne, shuffle, on):
    tri, ec = _mesh(n, Ne, shuffle)
    Ne = tri.shape[0]
    k_sst, k_sss = DIFF_ON[on]
    dx, dt = 1500.5, 900.
    sst, sss = _fields(Ne)
    got = _run_diffuse(binary, tmp_path, ec, sst, sss, k_sst, k_sss, dx, dt)
    for g, v, k, name in zip(got, (sst, sss), (k_sst, k_sss), ("sst", "sss")):
        want = R.diffuse(v, k, dx, dt, ec)
        assert R.same_bits(g, want).all(), (name, np.flatnonzero(~R.same_bits(g, want))[:5])
        if k <= 0.:
            assert g.tobytes() == v.tobytes(), (name, "a field that is off was written")      # byte for byte, -0.0 included
        else:
            assert Ne == 1 or not np.array_equal(g, v)
    if Ne == 1 and k_sss > 0:
        assert np.isnan(ec).all() and np.signbit(sss[0]) and got[1][0] == 0. and not np.signbit(got[1][0])      # v += 0. + 0. + 0.: -0.0 becomes +0.0
    if Ne > 256:
        t = _table(ec)
        assert (t >= 0).all(1).any() and (t < 0).any()
        if shuffle:
            assert np.abs(t - np.arange(Ne)[:, None])[t >= 0].mean() > Ne / 8      # not banded


def test_a_nan_reaches_exactly_its_element_and_its_edge_neighbours(binary, tmp_path):
    tri, ec = _mesh(20, 0, True)
    Ne = tri.shape[0]
    t = _table(ec)
    e = int(np.flatnonzero((t >= 0).all(1))[7])
    sst, sss = _fields(Ne)
    sst[e] = np.nan
    got_sst, got_sss = _run_diffuse(binary, tmp_path, ec, sst, sss, 1200., 350., 1500.5, 900.)
    hit = np.zeros(Ne, bool)
    hit[e] = True
    hit[t[e]] = True                                                         # the table is symmetric: e's neighbours are the elements that name e
    assert hit.sum() == 4 and np.array_equal(np.isnan(got_sst), hit) and np.isfinite(got_sss).all()
    assert np.array_equal(np.flatnonzero((t == e).any(1)), np.sort(t[e]))


@pytest.mark.parametrize("value", [0., -0., 1.7, -271.35, 1e-310])
def test_a_constant_field_comes_back_with_its_bits(binary, tmp_path, value):
    """the discrete identity the scheme has on a bounded mesh (no element-wise conservation is claimed: not every element has three neighbours): with a constant field
    every flux is factor*(c - c) = +0. exactly and v + (0. + 0. + 0.) is v, apart from the sign of zero"""
    tri, ec = _mesh(20, 0, True)
    Ne = tri.shape[0]
    c = np.full(Ne, value)
    got_sst, got_sss = _run_diffuse(binary, tmp_path, ec, c, c.copy(), 1200., 350., 1500.5, 900.)
    for g in (got_sst, got_sss):
        if value == 0.:
            assert (g == 0.).all() and not np.signbit(g).any()               # -0.0 + (+0.) is +0.0
        else:
            assert g.tobytes() == c.tobytes()
