"""The source of the three node-map kernels (nextsim_amd/csrc/nxs_nodemap_kernels.inl) compiled for the host (tests/nodal_receive_host_kernel.cpp, g++ -O2
-ffp-contract=off) against tests/golden/nodal_receive.npz, which the REAL bamg made: the weights kernel's six rows -- on the library's own integer plane and convex
completion, behind a brute-force locator the program supplies in place of the device's bucket grid -- give the real library's interpolation of the identity matrix exactly, the source and gather kernels the restated chain (tests/nodal_receive_ref.py) bit for bit.  The same program once more under
-fsanitize=address,undefined, run directly: every array is an allocation of exactly its size.  No device, no Python in the sanitised run."""
import os
import struct
import subprocess

import numpy as np
import pytest

import nodal_forcing_ref as NF
import nodal_receive_ref as R
from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "nodal_receive_host_kernel.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"), SRC]
SIZES = (1, 255, 256, 257)


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "nodal_receive_host_kernel")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def sanitised(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk_san") / "nodal_receive_host_kernel_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] + FLAGS + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLD)


def run(binary, tmp_path, payload):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(payload)
    subprocess.check_call([binary, fin, fout])
    return np.fromfile(fout)


def weights_payload(src, px, py):
    return (struct.pack("4i", 0, src["x"].size, src["tri"].shape[0], px.size) + np.ascontiguousarray(src["tri"], np.int32).tobytes() + src["x"].tobytes() + src["y"].tobytes()
            + px.tobytes() + py.tobytes())


def run_weights(binary, tmp_path, src, px, py):
    out = run(binary, tmp_path, weights_payload(src, px, py))
    N = px.size
    v = out[:3 * N].reshape(3, N).T.astype(np.int32)
    a = out[3 * N:6 * N].reshape(3, N).T.copy()
    return v, a, out[6 * N:].astype(np.int64)


def receive_payload(G, reduced, fields, v, w, a, b, factor, bias, pairs=(), rotate=None, east_west=None, get=False):
    R_, N, n = reduced.size, v.shape[0], fields.shape[0]
    j0 = [p[0] for p in pairs] + [0] * (2 - len(pairs))
    j1 = [p[1] for p in pairs] + [0] * (2 - len(pairs))
    mode, c, s, cs, sn = 0, 1., 0., np.zeros(R_), np.zeros(R_)
    if rotate is not None:
        if np.ndim(rotate[0]):
            mode, cs, sn = 2, np.ascontiguousarray(rotate[0]), np.ascontiguousarray(rotate[1])
        else:
            mode, c, s = 1, rotate[0], rotate[1]
    mp = np.zeros(15)
    lat, lon = np.zeros(R_), np.zeros(R_)
    if east_west is not None:
        mp, lat, lon = east_west["map_array"], east_west["lat"], east_west["lon"]
    pad = lambda x: np.concatenate([np.broadcast_to(np.asarray(x, np.float64), (n,)), np.zeros(4 - n)])  # noqa: E731
    identity = R_ == G and np.array_equal(reduced, np.arange(G))
    p = struct.pack("16i", 1, G, R_, N, n, len(pairs), *j0, *j1, int(east_west is not None), mode, int(get), int(not identity), 0, 0)
    p += pad(a).tobytes() + pad(b).tobytes() + pad(factor).tobytes() + pad(bias).tobytes() + struct.pack("2d", c, s) + np.ascontiguousarray(mp, np.float64).tobytes()
    p += np.ascontiguousarray(reduced, np.int32).tobytes() + cs.tobytes() + sn.tobytes() + np.ascontiguousarray(lat).tobytes() + np.ascontiguousarray(lon).tobytes()
    p += np.ascontiguousarray(fields, np.float64).tobytes()
    for k in range(3):
        p += np.ascontiguousarray(v[:, k], np.int32).tobytes()
    for k in range(3):
        p += np.ascontiguousarray(w[:, k], np.float64).tobytes()
    return p


def run_receive(binary, tmp_path, G, reduced, fields, v, w, *args, **kw):
    out = run(binary, tmp_path, receive_payload(G, reduced, fields, v, w, *args, **kw))
    n, R_, N = fields.shape[0], reduced.size, v.shape[0]
    return out[:n * R_].reshape(n, R_), out[n * R_:].reshape(n, N)


def polar():
    m = dynamics.mapx_polar_north(**NF.MPP["NpsNextsim"])
    return m, np.array([getattr(m, k) for k in _abi.MAPX_POLAR_FIELDS])


def forward(lat, lon):
    x, y = dynamics.mapx_forward(polar()[0], np.array([lat]), np.array([lon]), device=-1)
    return float(x[0]), float(y[0])


@pytest.mark.parametrize("name", ["full", "strip"])
def test_the_weights_source_on_the_host_gives_the_real_librarys_weights(binary, gold, tmp_path, name):
    src = R.source(name)
    px, py = gold["px_" + name], gold["py_" + name]
    assert np.array_equal(px, R.targets(src)[0]) and np.array_equal(py, R.targets(src)[1])
    v, a, counts = run_weights(binary, tmp_path, src, px, py)
    W = gold["W_" + name]
    assert counts[0] == 0 and counts[3] == 0 and counts[2] == int((R.D.locate(src["x"], src["y"], src["tri"], px, py)[0] < 0).sum()) > 0
    assert (v >= 0).all() and (v < src["x"].size).all()
    assert np.array_equal(R.dense(v, a, src["x"].size).view(np.uint64), W.view(np.uint64))
    # the three vertices are a triangle of the source in its own vertex order (up to the walk-dependent choice at a hull vertex, where two weights are 0)
    vr, _ = R.weights_from_dense(W, src["tri"])
    more = (W != 0).sum(1) > 1
    assert np.array_equal(v[more], vr[more]) and more.sum() > 0.9 * px.size
    d = R.awkward_data(src)
    for k in range(2):      # ... so the restated apply on them gives the real library's bits, the NaN node included
        assert R.equal(R.apply(v, a, d[:, k]), gold["Y_" + name][:, k])


def test_the_weights_source_counts_the_targets_in_the_notch(binary, gold, tmp_path):
    src = R.source("notch")
    px, py = gold["px_notch"], gold["py_notch"]
    _, _, counts = run_weights(binary, tmp_path, src, px, py)
    fill = gold["fill_notch"]
    assert fill.size > 0 and counts[0] == fill.size and counts[1] == fill.min()


@pytest.mark.parametrize("N", SIZES)
def test_the_weights_source_at_the_launch_edges(binary, gold, tmp_path, N):
    src = R.source("strip")
    sel = np.linspace(0, gold["px_strip"].size - 1, N).astype(int)
    v, a, _ = run_weights(binary, tmp_path, src, gold["px_strip"][sel].copy(), gold["py_strip"][sel].copy())
    assert np.array_equal(R.dense(v, a, src["x"].size).view(np.uint64), gold["W_strip"][sel].view(np.uint64))


def case(name, gold, n_var, N=None, R_cut=None):
    """Fixture weights cut to N targets; the source cut to its first R_cut reduced points (vertices folded into range: any vertex is as good as another to a gather)."""
    src = R.source(name)
    v, w = R.weights_from_dense(gold["W_" + name], src["tri"])
    if N is not None:
        sel = np.linspace(0, v.shape[0] - 1, N).astype(int)
        v, w = v[sel].copy(), w[sel].copy()
    reduced, theta, lat, lon = src["reduced"], src["theta"], src["lat"], src["lon"]
    if R_cut is not None:
        reduced, theta, lat, lon = reduced[:R_cut].copy(), theta[:R_cut].copy(), lat[:R_cut].copy(), lon[:R_cut].copy()
        v = (v % R_cut).astype(np.int32)
    return dict(G=src["G"], reduced=reduced, theta=theta, lat=lat, lon=lon, v=v, w=w, fields=R.fields_case(src["G"], n_var))


COEF = dict(a=[2., 1., -0.5, 1.], b=[0., 0.25, 0., -3.], factor=[1.5, -2., 1., 0.], bias=[0., 0.5, -0., 7.])


def coef(n):
    return {k: np.array(v[:n]) for k, v in COEF.items()}


@pytest.mark.parametrize("get", [False, True])
@pytest.mark.parametrize("n_var", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["full", "strip"])
def test_source_and_gather_on_the_host_give_the_restatements_bits(binary, gold, tmp_path, name, n_var, get):
    c, k = case(name, gold, n_var), coef(n_var)
    pairs = [(0, 1)] if n_var >= 2 else []
    if n_var == 4:
        pairs = [(0, 1), (3, 2)]
    rot = R.uniform_rotation()
    stage, rows = run_receive(binary, tmp_path, c["G"], c["reduced"], c["fields"], c["v"], c["w"], k["a"], k["b"], k["factor"], k["bias"], pairs, rot, None, get)
    assert R.equal(stage, R.loaded_data(c["fields"], c["reduced"], k["a"], k["b"], pairs, rot))
    want = R.receive(c["fields"], c["reduced"], k["a"], k["b"], c["v"], c["w"], pairs, rot, None, k["factor"] if get else None, k["bias"] if get else None)
    assert R.equal(rows, want)
    if name == "strip":
        assert not (np.abs(stage) > 1e19).any()      # the land column never reaches loaded_data


@pytest.mark.parametrize("name", ["full", "strip"])
def test_the_per_point_rotation_on_the_host(binary, gold, tmp_path, name):
    c, k = case(name, gold, 3), coef(3)
    rot = R.cos_sin_theta(R.MAP_ROTATION, c["theta"])
    stage, rows = run_receive(binary, tmp_path, c["G"], c["reduced"], c["fields"], c["v"], c["w"], k["a"], k["b"], k["factor"], k["bias"], [(0, 1)], rot, None, False)
    assert R.equal(stage, R.loaded_data(c["fields"], c["reduced"], k["a"], k["b"], [(0, 1)], rot))
    assert R.equal(rows, R.receive(c["fields"], c["reduced"], k["a"], k["b"], c["v"], c["w"], [(0, 1)], rot))
    assert not R.equal(stage[:2], R.loaded_data(c["fields"], c["reduced"], k["a"], k["b"])[:2]) and R.equal(stage[2], R.loaded_data(c["fields"], c["reduced"], k["a"], k["b"])[2])


def test_the_east_north_pair_on_the_host_within_the_derived_bound(binary, gold, tmp_path):
    c, k = case("strip", gold, 2), coef(2)
    c["fields"] = np.where(np.abs(c["fields"]) > 1e19, c["fields"], 0.3 * c["fields"])      # wave stresses: well under a degree per second
    ew = dict(lat=c["lat"], lon=c["lon"], forward=forward, map_array=polar()[1])
    rot = R.cos_sin_theta(R.MAP_ROTATION, c["theta"])
    stage, rows = run_receive(binary, tmp_path, c["G"], c["reduced"], c["fields"], c["v"], c["w"], k["a"], k["b"], k["factor"], k["bias"], [(0, 1)], None, ew, True)
    det = {}
    want = R.loaded_data(c["fields"], c["reduced"], k["a"], k["b"], [(0, 1)], None, ew, details=det)
    bound = NF.bound_east_north(det[0])      # section 6l's derived bound, unchanged
    assert (np.abs(stage - want) <= bound[None, :]).all() and (bound > 0).any()
    assert not np.array_equal(stage, R.loaded_data(c["fields"], c["reduced"], k["a"], k["b"]))
    # the gather after it: bit for bit on the program's own source rows
    with np.errstate(invalid="ignore"):
        assert R.equal(rows, np.stack([k["factor"][j] * R.apply(c["v"], c["w"], stage[j]) + k["bias"][j] for j in range(2)]))
    # east/north THEN the rotation, the reference's order
    stage2, _ = run_receive(binary, tmp_path, c["G"], c["reduced"], c["fields"], c["v"], c["w"], k["a"], k["b"], k["factor"], k["bias"], [(0, 1)], rot, ew, True)
    assert R.equal(np.stack(R.rotated(stage[0], stage[1], *rot)), stage2)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("R_", SIZES)
def test_the_launch_edges_on_the_host(binary, tmp_path, N, R_):
    """1, 255, 256, 257 reduced points and targets: below, at and above one block of 256 threads (on the host the guard `i >= n` and the exact allocations)"""
    c, k = R.synthetic_case(R_, N, 3), coef(3)
    rot = R.cos_sin_theta(R.MAP_ROTATION, c["theta"])
    stage, rows = run_receive(binary, tmp_path, c["G"], c["reduced"], c["fields"], c["v"], c["w"], k["a"], k["b"], k["factor"], k["bias"], [(0, 1)], rot, None, True)
    assert stage.shape == (3, R_) and rows.shape == (3, N) and not (stage == -777.).any() and not (rows == -777.).any()
    assert R.equal(rows, R.receive(c["fields"], c["reduced"], k["a"], k["b"], c["v"], c["w"], [(0, 1)], rot, None, k["factor"], k["bias"]))


def test_the_stand_alone_program_under_address_and_undefined_sanitizers(sanitised, gold, tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    jobs = []
    for name in R.CASES:
        jobs.append(weights_payload(R.source(name), gold["px_" + name], gold["py_" + name]))
    jobs.append(weights_payload(R.source("strip"), gold["px_strip"][:1].copy(), gold["py_strip"][:1].copy()))
    for n_var, N, R_ in ((1, 1, 1), (2, 255, 257), (3, 256, 255), (4, 257, 256)):
        c, k = R.synthetic_case(R_, N, n_var), coef(n_var)
        pairs = [(0, 1)] if n_var >= 2 else []
        ew = dict(lat=c["lat"], lon=c["lon"], map_array=polar()[1]) if n_var == 2 else None
        rot = R.cos_sin_theta(R.MAP_ROTATION, c["theta"]) if n_var >= 3 else R.uniform_rotation()
        jobs.append(receive_payload(c["G"], c["reduced"], c["fields"], c["v"], c["w"], k["a"], k["b"], k["factor"], k["bias"], pairs, rot, ew, True))
    for i, p in enumerate(jobs):
        fin, fout = str(tmp_path / f"in{i}.bin"), str(tmp_path / f"out{i}.bin")
        with open(fin, "wb") as f:
            f.write(p)
        r = subprocess.run([sanitised, fin, fout], env=env, capture_output=True, text=True)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (i, r.returncode, r.stderr[-2000:])
