"""The source of the two load kernels (nextsim_amd/csrc/nxs_nodemap_load_kernels.inl) compiled for the host (tests/mesh_forcing_host_kernel.cpp, g++ -O2
-ffp-contract=off), run on the fixture's weights and compared bit for bit with tests/golden/mesh_forcing.npz, which the REAL bamg made; every shape of the call
against the restatement (tests/mesh_forcing_ref.py).  The same program once more under -fsanitize=address,undefined, run directly: every array is an allocation of
exactly its size.  No device, no Python in the sanitised run."""
import os
import struct
import subprocess

import numpy as np
import pytest

import mesh_forcing_ref as MF
import nodal_forcing_ref as NF
import nodal_receive_ref as R
from test_nodal_receive_host_kernel import forward, polar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "mesh_forcing_host_kernel.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"), SRC]
SIZES = (1, 255, 256, 257)


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mfk") / "mesh_forcing_host_kernel")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def sanitised(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mfk_san") / "mesh_forcing_host_kernel_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] + FLAGS + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(MF.GOLD))


def payload(G, reduced, fields, n_var, n_step, v, w, co, pairs=(), rotate=None, east_west=None, skip=()):
    R_, N, n_cols = reduced.size, v.shape[0], n_var * n_step
    assert fields.shape == (n_cols, G)
    j0 = [p[0] for p in pairs] + [0] * (2 - len(pairs))
    j1 = [p[1] for p in pairs] + [0] * (2 - len(pairs))
    mode, c, s, cs, sn = 0, 1., 0., np.zeros(R_), np.zeros(R_)
    if rotate is not None:
        if np.ndim(rotate[0]):
            mode, cs, sn = 2, np.ascontiguousarray(rotate[0]), np.ascontiguousarray(rotate[1])
        else:
            mode, c, s = 1, rotate[0], rotate[1]
    mp, lat, lon = np.zeros(15), np.zeros(R_), np.zeros(R_)
    if east_west is not None:
        mp, lat, lon = east_west["map_array"], east_west["lat"], east_west["lon"]
    pad = lambda x: np.concatenate([np.broadcast_to(np.asarray(x, np.float64), (n_cols,)), np.zeros(8 - n_cols)])  # noqa: E731
    identity = R_ == G and np.array_equal(reduced, np.arange(G))
    keep = sum(1 << k for k in range(n_cols) if k not in skip)
    p = struct.pack("16i", G, R_, N, n_var, n_step, len(pairs), *j0, *j1, int(east_west is not None), mode, int(not identity), keep, 0, 0)
    p += b"".join(pad(co[k]).tobytes() for k in ("scale_factor", "add_offset", "a", "b")) + struct.pack("2d", c, s) + np.ascontiguousarray(mp, np.float64).tobytes()
    p += np.ascontiguousarray(reduced, np.int32).tobytes() + cs.tobytes() + sn.tobytes() + np.ascontiguousarray(lat).tobytes() + np.ascontiguousarray(lon).tobytes()
    p += np.ascontiguousarray(fields, np.float64).tobytes()
    for k in range(3):
        p += np.ascontiguousarray(v[:, k], np.int32).tobytes()
    for k in range(3):
        p += np.ascontiguousarray(w[:, k], np.float64).tobytes()
    return p


def run(binary, tmp_path, G, reduced, fields, n_var, n_step, v, w, co, pairs=(), rotate=None, east_west=None, skip=()):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(payload(G, reduced, fields, n_var, n_step, v, w, co, pairs, rotate, east_west, skip))
    subprocess.check_call([binary, fin, fout])
    out = np.fromfile(fout)
    n_cols, R_, N = n_var * n_step, reduced.size, v.shape[0]
    return out[:n_cols * R_].reshape(n_cols, R_), out[n_cols * R_:].reshape(n_cols - len(skip), N)


@pytest.mark.parametrize("kind", MF.KINDS)
@pytest.mark.parametrize("name", MF.SOURCES)
def test_both_kernels_on_the_host_give_the_fixtures_bits(binary, gold, tmp_path, name, kind):
    src = R.source(name)
    v, w = MF.weights(name, kind)
    f = MF.raw_fields(src["G"], src["reduced"])
    stage, rows = run(binary, tmp_path, src["G"], src["reduced"], f, 3, 2, v, w, MF.coef(), MF.PAIRS, R.uniform_rotation())
    assert R.equal(stage, MF.fixture_load(name)) and np.isfinite(stage).all()
    assert R.equal(rows, gold[f"Y_{kind}_{name}"].T)


@pytest.mark.parametrize("n_step", [1, 2])
@pytest.mark.parametrize("n_var", [1, 2, 3, 4])
def test_every_shape_of_the_load_on_the_host(binary, tmp_path, n_var, n_step):
    src = R.source("strip")
    v, w = MF.weights("strip", "nodes")
    c8 = MF.coef8()
    cols = [s * 4 + j for s in range(n_step) for j in range(n_var)]
    co = {k: c8[k][cols] for k in c8}
    f = MF.raw_fields(src["G"], src["reduced"], 8)[cols]
    pairs = [] if n_var < 2 else [(0, 1)] if n_var < 4 else [(0, 1), (3, 2)]
    rot = R.cos_sin_theta(R.MAP_ROTATION, src["theta"])
    skip = (n_var * n_step - 1,) if n_var * n_step > 1 else ()      # the last column is loaded (a pair may need it) but not gathered
    stage, rows = run(binary, tmp_path, src["G"], src["reduced"], f, n_var, n_step, v, w, co, pairs, rot, None, skip)
    assert R.equal(stage, MF.loaded_data(f, src["reduced"], n_var, n_step, pairs=pairs, rotate=rot, **co))
    want = MF.ingest(f, src["reduced"], n_var, n_step, v, w, pairs=pairs, rotate=rot, **co)
    assert R.equal(rows, want[[c for c in range(n_var * n_step) if c not in skip]])


def test_the_east_north_pair_on_the_host_within_the_derived_bound(binary, tmp_path):
    src = R.source("strip")
    v, w = MF.weights("strip", "elements")
    f = MF.raw_fields(src["G"], src["reduced"])
    f = np.where(np.abs(f) > 1e19, f, 0.3 * f)
    co = MF.coef()
    ew = dict(lat=src["lat"], lon=src["lon"], forward=forward, map_array=polar()[1])
    stage, rows = run(binary, tmp_path, src["G"], src["reduced"], f, 3, 2, v, w, co, MF.PAIRS, None, ew)
    det = {}
    want = MF.loaded_data(f, src["reduced"], 3, 2, pairs=MF.PAIRS, east_west=ew, details=det, **co)
    for fstep in range(2):      # section 6l's derived bound, unchanged, in EVERY forcing step
        bound = NF.bound_east_north(det[(fstep, 0)])
        assert (np.abs(stage[3 * fstep:3 * fstep + 2] - want[3 * fstep:3 * fstep + 2]) <= bound[None, :]).all() and (bound > 0).any()
        assert R.equal(stage[3 * fstep + 2], want[3 * fstep + 2])
    assert not np.array_equal(stage, MF.loaded_data(f, src["reduced"], 3, 2, **co))
    assert R.equal(rows, np.stack([R.apply(v, w, stage[c]) for c in range(6)]))      # the gather after it: bit for bit on the program's own rows
    rot = R.uniform_rotation()
    stage2, _ = run(binary, tmp_path, src["G"], src["reduced"], f, 3, 2, v, w, co, MF.PAIRS, rot, ew)      # east/north THEN the rotation, the reference's order
    for fstep in range(2):
        assert R.equal(np.stack(R.rotated(stage[3 * fstep], stage[3 * fstep + 1], *rot)), stage2[3 * fstep:3 * fstep + 2])


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("R_", SIZES)
def test_the_launch_edges_on_the_host(binary, tmp_path, N, R_):
    """1, 255, 256, 257 reduced points and targets: below, at and above one block of 256 threads (on the host the guard `i >= n` and the exact allocations)"""
    c, co = MF.synthetic_case(R_, N, 8), MF.coef8()
    rot = R.cos_sin_theta(R.MAP_ROTATION, c["theta"])
    pairs = [(0, 1), (3, 2)]
    stage, rows = run(binary, tmp_path, c["G"], c["reduced"], c["fields"], 4, 2, c["v"], c["w"], co, pairs, rot)
    assert stage.shape == (8, R_) and rows.shape == (8, N) and not (stage == -777.).any() and not (rows == -777.).any()
    assert R.equal(stage, MF.loaded_data(c["fields"], c["reduced"], 4, 2, pairs=pairs, rotate=rot, **co))
    assert R.equal(rows, MF.ingest(c["fields"], c["reduced"], 4, 2, c["v"], c["w"], pairs=pairs, rotate=rot, **co))


def test_the_stand_alone_program_under_address_and_undefined_sanitizers(sanitised, tmp_path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    jobs = []
    for name in MF.SOURCES:
        for kind in MF.KINDS:
            src = R.source(name)
            v, w = MF.weights(name, kind)
            jobs.append(payload(src["G"], src["reduced"], MF.raw_fields(src["G"], src["reduced"]), 3, 2, v, w, MF.coef(), MF.PAIRS, R.uniform_rotation()))
    c8 = MF.coef8()
    for n_var, n_step, N, R_ in ((1, 1, 1, 1), (2, 2, 255, 257), (3, 1, 256, 255), (4, 2, 257, 256)):
        n_cols = n_var * n_step
        c = MF.synthetic_case(R_, N, n_cols)
        co = {k: c8[k][:n_cols] for k in c8}
        pairs = [] if n_var < 2 else [(0, 1)] if n_var < 4 else [(0, 1), (3, 2)]
        ew = dict(lat=c["lat"], lon=c["lon"], map_array=polar()[1]) if n_var == 2 else None
        rot = R.cos_sin_theta(R.MAP_ROTATION, c["theta"]) if n_var >= 3 else R.uniform_rotation()
        jobs.append(payload(c["G"], c["reduced"], c["fields"], n_var, n_step, c["v"], c["w"], co, pairs, rot, ew, (0,) if n_cols > 1 else ()))
    for i, p in enumerate(jobs):
        fin, fout = str(tmp_path / f"in{i}.bin"), str(tmp_path / f"out{i}.bin")
        with open(fin, "wb") as f:
            f.write(p)
        r = subprocess.run([sanitised, fin, fout], env=env, capture_output=True, text=True)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (i, r.returncode, r.stderr[-2000:])
