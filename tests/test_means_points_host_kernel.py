"""The per-point body of nxs_dyn_means_points_update (nextsim_amd/csrc/nxs_means_points_body.inl) compiled for the host (tests/means_points_host_kernel.cpp,
g++ -O2 -ffp-contract=off) and fed the located triangles and integer area coordinates: the bits of the fixture the REAL contrib/bamg wrote
(tests/golden/means_points.npz, made by tests/golden/make_means_points_golden.py) and of the restatement tests/means_points_ref.py -- which is itself held to the
fixture here.  No device, no tolerance."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import drifters_ref as R  # noqa: E402
import make_means_points_golden as G  # noqa: E402
import means_points_ref as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "means_points.npz")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "means_points_host_kernel")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "means_points_host_kernel.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def case():
    c = G.means_points_case()
    c["z"] = dict(np.load(GOLD))
    return c


def run(binary, tmp_path, it, tri, dd, n_owned, el, nod, ge, gn, pairs=(), cs=None, sn=None, miss_val=G.MISS, ice_col=-1, el_mask=(), nod_mask=(), Nn=None):
    """One updateGridMean by the host build of the body: returns (ge, gn) after it."""
    Gn = it.size
    n_el, n_nod = ge.shape[0], gn.shape[0]
    Ne, Nn = tri.shape[0], (int(tri.max()) + 1 if Nn is None else Nn)
    bits = lambda m: sum(1 << k for k, v in enumerate(m) if v)  # noqa: E731
    first = [p[0] for p in pairs] + [0] * (12 - len(pairs))
    second = [p[1] for p in pairs] + [0] * (12 - len(pairs))
    v3 = np.where((it >= 0)[:, None], tri[np.maximum(it, 0)], 0).astype(np.int32)
    payload = struct.pack("10i", Gn, n_el, n_nod, len(pairs), ice_col, n_owned, int(cs is not None), Ne, Nn, 0) + struct.pack("2I", bits(el_mask), bits(nod_mask))
    payload += struct.pack("24i", *first, *second) + struct.pack("d", miss_val)
    payload += it.astype(np.int32).tobytes() + v3.tobytes() + np.ascontiguousarray(dd, np.int64).tobytes()
    if cs is not None:
        payload += np.ascontiguousarray(cs, np.float64).tobytes() + np.ascontiguousarray(sn, np.float64).tobytes()
    for a in (el, nod, ge, gn):
        payload += np.ascontiguousarray(a, np.float64).tobytes()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(payload)
    subprocess.check_call([binary, fin, fout])
    out = np.fromfile(fout)
    return out[:n_el * Gn].reshape(n_el, Gn), out[n_el * Gn:].reshape(n_nod, Gn)


def test_the_fixture_has_no_ties_and_the_cases_asked_for(case):
    c, z = case, case["z"]
    assert G.ties(c) == (0, 0, 0)
    assert np.array_equal(z["gx"], c["gx"]) and np.array_equal(z["gy"], c["gy"]) and c["gx"].size == 41 * 53
    loc = G.located(c)
    for k in ("it1", "dd1", "it2", "dd2"):
        assert np.array_equal(loc[k], z[k]), k
    nn = c["x"].size
    box = R.mesh_bbox(c["x"] + c["UM1"][:nn], c["y"] + c["UM1"][nn:])
    outside = (c["gx"] < box[0]) | (c["gx"] > box[1]) | (c["gy"] < box[2]) | (c["gy"] > box[3])
    it = z["it1"]
    assert outside.sum() > 10 and ((it < 0) & ~outside).sum() > 50 and (it >= c["n_owned"]).sum() > 100 and ((it >= 0) & (it < c["n_owned"])).sum() > 100
    assert not np.array_equal(z["it1"], z["it2"])                                   # the second mesh puts points into other triangles
    assert c["n_owned"] == c["tri"].shape[0] - c["tri"].shape[0] // 3
    assert (c["el"] < 0).any() and (~c["el"][:c["n_owned"]].any(1)).any() and np.isnan(c["nod"]).all(1).sum() == 1
    # the NaN node is seen from an owned element (NaN * 1.) and from a ghost element (NaN * 0.: still a NaN)
    sees = (c["tri"][np.maximum(it, 0)] == c["nan_node"]).any(1) & (it >= 0)
    assert (sees & (it < c["n_owned"])).any() and (sees & (it >= c["n_owned"])).any() and np.isnan(z["gn1"][[0, 2, 3]][:, sees]).all()
    assert not z["gn1"][1][sees & (z["ge1"][2] <= 0.)].any()                         # (VT_y is masked: a NaN is not miss_val, the rule makes it 0.)
    assert (z["lsm"] == 0).sum() > 50 and (z["ge2_lsm"][:, z["lsm"] == 0] == G.MISS).all() and (z["gn2_lsm"][:, z["lsm"] == 0] == G.MISS).all()
    assert not np.array_equal(z["gn2_theta"][0], z["gn2"][0])


@pytest.mark.parametrize("rotation", ["north_east", "grid_theta"])
def test_the_restatement_gives_the_real_bamgs_bits(case, rotation):
    c, z = case, case["z"]
    g = G.chain(c, P.interp, rotation)
    if rotation == "grid_theta":
        assert P.equal(g["gn2"], z["gn2_theta"]) and P.equal(g["ge2"], z["ge2"])
        return
    for k in ("ge1", "gn1", "ge2", "gn2", "ge2_lsm", "gn2_lsm"):
        assert P.equal(g[k], z[k]), k
    assert np.array_equal(g["lsm"], z["lsm"])


@pytest.mark.parametrize("rotation", ["north_east", "grid_theta"])
def test_the_body_on_the_host_gives_the_fixtures_bits(binary, case, tmp_path, rotation):
    c, z = case, case["z"]
    cs, sn = P.cos_sin(rotation, G.ROTATION_ANGLE, c["lon"], c["theta"])
    ge, gn = np.zeros((3, c["gx"].size)), np.zeros((4, c["gx"].size))
    for k in (1, 2):
        ge, gn = run(binary, tmp_path, z[f"it{k}"], c["tri"], z[f"dd{k}"], c["n_owned"], c["el"], c["nod"], ge, gn, G.PAIRS, cs, sn, G.MISS, G.ICE_COL, G.EL_MASK, G.NOD_MASK,
                     Nn=c["x"].size)
        if rotation == "north_east":
            assert P.equal(ge, z[f"ge{k}"]) and P.equal(gn, z[f"gn{k}"]), k
    assert P.equal(ge, z["ge2"]) and P.equal(gn, z["gn2" if rotation == "north_east" else "gn2_theta"])


def small_case(seed, n_el, n_nod, Gn=300):
    """A handful of triangles and points with made-up (it, dd): the body is told where each point lies."""
    rng = np.random.default_rng(seed)
    Nn, Ne = 40, 60
    tri = np.stack([rng.permutation(Nn)[:3] for _ in range(Ne)]).astype(np.int32)
    it = rng.integers(-1, Ne, Gn)
    dd = rng.integers(1, 2 ** 40, (Gn, 3))
    dd[it < 0] = 0
    el, nod = rng.normal(0., 3., (Ne, n_el)), rng.normal(0., 3., (Nn, n_nod))
    ge, gn = rng.normal(0., 1., (n_el, Gn)), rng.normal(0., 1., (n_nod, Gn))
    cs, sn = np.cos(rng.uniform(-4., 4., Gn)), np.sin(rng.uniform(-4., 4., Gn))      # (any two numbers per point: the body only multiplies by them)
    return dict(tri=tri, it=it, dd=dd, el=el, nod=nod, ge=ge, gn=gn, cs=cs, sn=sn, Nn=Nn, Ne=Ne, n_owned=35)


def located_interp(s):
    """means_points_ref's interpolation with the location GIVEN (s["it"], s["dd"]) instead of looked for."""
    def f(x, y, tri, data, px, py, nodal):
        data = np.asarray(data, np.float64)
        data = data[:, None] if data.ndim == 1 else data
        out = np.zeros((s["it"].size, data.shape[1]))
        m = np.flatnonzero(s["it"] >= 0)
        it, dd = s["it"][m], s["dd"][m]
        if nodal:
            det = (dd[:, 0] + dd[:, 1] + dd[:, 2]).astype(np.float64)
            a = [dd[:, k].astype(np.float64) / det for k in range(3)]
            with np.errstate(invalid="ignore"):
                out[m] = a[0][:, None] * data[tri[it, 0]] + a[1][:, None] * data[tri[it, 1]] + a[2][:, None] * data[tri[it, 2]]
        else:
            out[m] = data[it]
        return out
    return f


def both(binary, tmp_path, s, pairs=(), rotate=True, miss_val=G.MISS, ice_col=-1, el_mask=(), nod_mask=()):
    cs, sn = (s["cs"], s["sn"]) if rotate else (None, None)
    got = run(binary, tmp_path, s["it"], s["tri"], s["dd"], s["n_owned"], s["el"], s["nod"], s["ge"], s["gn"], pairs, cs, sn, miss_val, ice_col, el_mask, nod_mask, Nn=s["Nn"])
    ge, gn = s["ge"].copy(), s["gn"].copy()
    z = np.zeros(s["it"].size)
    P.update_grid_mean(ge if ge.shape[0] else None, gn if gn.shape[0] else None, None, None, s["tri"], s["n_owned"], s["el"], s["nod"], z, z, pairs, cs, sn, miss_val, ice_col,
                       el_mask, nod_mask, located_interp(s))
    return got, (ge, gn)


@pytest.mark.parametrize("n_el, n_nod, pairs", [(1, 2, ((0, 1),)), (3, 4, ((0, 1), (2, 3))), (24, 24, tuple((2 * k, 2 * k + 1) for k in range(12))), (0, 5, ((4, 0),)), (6, 0, ()),
                                                (2, 3, ((0, 1), (0, 1))), (2, 3, ((0, 1), (1, 2))), (2, 4, ())])
@pytest.mark.parametrize("rotate", [True, False])
def test_shapes_pairs_and_modes(binary, tmp_path, n_el, n_nod, pairs, rotate):
    """1 and NXS_MEANS_MAX_VARS variables, no nodal list (no proc-mask leg), no elemental list, 0 / 1 / 12 pairs, a pair listed twice, two pairs sharing a column, NONE"""
    s = small_case(100 * n_el + n_nod, n_el, n_nod)
    (ge, gn), (we, wn) = both(binary, tmp_path, s, pairs, rotate)
    assert P.equal(ge, we) and P.equal(gn, wn)
    if n_nod and pairs and rotate:
        (_, gn0), _ = both(binary, tmp_path, s, pairs, False)
        assert not np.array_equal(gn0[pairs[0][0]], gn[pairs[0][0]])               # the rotation did something
    if len(pairs) == 2 and pairs[0] == pairs[1] and rotate:
        (_, once), _ = both(binary, tmp_path, s, pairs[:1])
        assert not np.array_equal(once[0], gn[0])                                   # listed twice: rotated twice


def test_a_first_component_equal_to_miss_val_is_not_rotated(binary, tmp_path):
    s = small_case(5, 1, 2)
    miss = 2.5
    inside = np.flatnonzero(s["it"] >= 0)
    s["nod"][:, 0] = miss                                      # a0 * m + a1 * m + a2 * m: equal to m exactly only where the three quotients sum to 1 in that order
    (ge, gn), (we, wn) = both(binary, tmp_path, s, ((0, 1),), miss_val=miss)
    assert P.equal(ge, we) and P.equal(gn, wn)
    outside = np.flatnonzero(s["it"] < 0)
    hit = np.zeros(s["it"].size, bool)
    out = located_interp(s)(None, None, s["tri"], s["nod"], None, None, True)
    hit[inside] = out[inside, 0] == miss
    assert hit.sum() > 10 and (~hit[inside]).sum() >= 0 and outside.size > 0
    # where it was skipped the second component came through unrotated: value * proc_mask added to what was there
    pm = ((s["it"] >= 0) & (s["it"] < s["n_owned"])).astype(np.float64)
    assert np.array_equal(gn[1][hit], (s["gn"][1] + out[:, 1] * pm)[hit])
    # and a miss_val of 0. skips every point that was not found (interp_out = 0. there)
    s2 = small_case(6, 1, 2)
    (_, gn2), (_, wn2) = both(binary, tmp_path, s2, ((0, 1),), miss_val=0.)
    assert P.equal(gn2, wn2)


def test_nan_times_proc_mask_zero_stays_nan(binary, tmp_path):
    s = small_case(7, 1, 2)
    s["nod"][:] = np.nan
    (ge, gn), (we, wn) = both(binary, tmp_path, s, ((0, 1),))
    assert P.equal(gn, wn)
    ghost, notfound = s["it"] >= s["n_owned"], s["it"] < 0
    assert ghost.sum() > 20 and np.isnan(gn[:, ghost]).all() and np.array_equal(gn[:, notfound], s["gn"][:, notfound] + 0. * 0.)


@pytest.mark.parametrize("ice_is_masked_itself", [False, True])
def test_the_ice_mask_rule(binary, tmp_path, ice_is_masked_itself):
    """ice_mask 0, negative and positive after the accumulation; a value equal to miss_val is left alone"""
    miss = -7.
    s = small_case(8, 3, 2)
    Gn = s["it"].size
    s["el"][:, 2] = np.repeat([0., -1., 2.], s["Ne"] // 3)
    s["ge"][2] = 0.
    s["ge"][2, ::7] = -3.; s["ge"][2, 1::7] = 5.
    s["el"][:, 1] = 0.; s["ge"][1, ::2] = miss                 # a masked elemental value that IS miss_val after the accumulation (miss + 0.)
    s["nod"][:, 0] = 0.; s["gn"][0, ::3] = miss
    el_mask = (0, 1, 1 if ice_is_masked_itself else 0)
    (ge, gn), (we, wn) = both(binary, tmp_path, s, (), False, miss, 2, el_mask, (1, 0))
    assert P.equal(ge, we) and P.equal(gn, wn)
    ice = s["ge"][2] + np.where(s["it"] >= 0, s["el"][np.maximum(s["it"], 0), 2], 0.)
    assert (ice == 0).sum() > 10 and (ice < 0).sum() > 10 and (ice > 0).sum() > 10
    low = ice <= 0.
    assert (ge[1][low & (np.arange(Gn) % 2 == 0)] == miss).all() and not ge[1][low & (np.arange(Gn) % 2 == 1)].any()
    assert (gn[0][low & (np.arange(Gn) % 3 == 0)] == miss).all() and not gn[0][low & (np.arange(Gn) % 3 != 0)].any()
    assert np.array_equal(ge[0], s["ge"][0] + np.where(s["it"] >= 0, s["el"][np.maximum(s["it"], 0), 0], 0.))      # an unmasked variable is never touched
    assert np.array_equal(ge[2], np.where(low, 0., ice) if ice_is_masked_itself else ice)
