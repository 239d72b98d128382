"""tests/slab_fsd_ref.py, the restatement of thermo()'s slab loop as an OASIS build compiles it (FE.cpp:5413-6133 with melt_type 3, the FSD branches of the limit
block, redistributeThermoFSD, the in-loop weldingRoach and the mechanical healing): pinned against slab_ref.slab where both cover the same lines, against
hand-computed elements, on designed strata, away from every edge, and sensitive to planted mistakes.  Then the source of the two kernels of nxs_dyn_slab_coupled
compiled for the host (tests/slab_fsd_host_kernel.cpp) against the restatement, bit for bit.  Parity with a binary of the reference is NOT pinned (model/ cannot
be compiled here).  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import fsd_ref as FS
import slab_fsd_ref as S
import slab_ref as R
from nextsim_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALB = FR.default_config()["ocean_albedo"]
F = np.float64


@pytest.fixture(scope="module")
def mesh():
    gm = cases.global_mesh("toy")
    return gm, np.ascontiguousarray(gm.tri, np.int64)


def run(mesh, nb, young, melt_type, thermo="winton", dist=0, welding=FS.WELD_ROACH, debug=0, opts=None, drop=(), inputs=None, **kw):
    gm, tri = mesh
    inp, fsd, s, broken, sets = inputs if inputs is not None else S.make_inputs(gm.x, gm.y, tri, nb, young)
    cfg = R.category_config(young, **(opts or {}))
    ccfg = CR.default_config(thermo_type=thermo)
    fcfg = S.fsd_config(nb, young, distinguish_mech_fsd=dist, welding_type=welding, debug_fsd=debug)
    work, bins = R.copy(inp), S.copy_fsd(fsd)
    rows, w1, w2, info = S.slab_coupled(work, bins, cfg, ccfg, fcfg, ALB, tri, young, R.DT, R.clock(), melt_type=melt_type, drop=drop, **kw)
    return dict(rows=rows, work=work, bins=bins, w1=w1, w2=w2, info=info, inp=inp, fsd=fsd, sets=sets, broken=broken, cfg=cfg, ccfg=ccfg, fcfg=fcfg, strata=s)


# ---- 1: the two restatements
@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("melt_type", [1, 2])
def test_melt_type_1_and_2_are_slab_refs_bits(mesh, melt_type, young):
    """on slab_ref.make_inputs, all 29 rows, every row in place and the NXS_SLAB_BR_* word; the new word has no bit of melt_type 3 or of redistributeThermoFSD"""
    gm, tri = mesh
    inp, _, _ = R.make_inputs(gm.x, gm.y, tri)
    Ne = tri.shape[0]
    for thermo in ("winton", "zero_layer"):
        cfg, ccfg = R.category_config(young, melt_type=melt_type, temp_dep_healing=1, use_meltponds=1), CR.default_config(thermo_type=thermo)
        a = R.copy(inp)
        rows, words = R.slab(a, cfg, ccfg, ALB, tri, young, R.DT, R.clock(last_step_of_day=1))
        b = R.copy(inp)
        bins = {"conc_fsd": np.tile(inp["conc"] + (inp["conc_young"] if young else 0.), (1, 1)), "conc_mech_fsd": None}
        rows2, w1, w2, info = S.slab_coupled(b, bins, cfg, ccfg, S.fsd_config(1, young), ALB, tri, young, R.DT, R.clock(last_step_of_day=1))
        for k in R.ROWS:
            assert R.same_bits(rows[k], rows2[k]).all(), k
        for k in R.IN_PLACE:
            assert R.same_bits(a[k], b[k]).all(), k
        assert np.array_equal(words, w1)
        others = sum(S.BIT2[k] for k in ("melt3", "unbroken", "ctot_break", "lateral", "lat_melting", "fills_lead", "del_c_fsd_ge0", "young_shrinks"))
        assert not (w2 & np.uint32(others)).any() and w2.shape == (Ne,)


# ---- 2: hand-computed elements.  One element, the default constants: qi = Lf * rhoi = 333.55e3 * 917, qs = Lf * rhos = 333.55e3 * 330, PhiM = 0.5, ddt = 900,
# mld = constant_mld, bins of 10 m from 10 m (bin_widths 10, bin_centres 15, 25, 35)
def _one(young, nb, bins, mech=None, melt_type=3, dist=0, welding=FS.WELD_NONE, opts=None, **rows):
    tri = np.array([[0, 1, 2]], np.int64)
    inp = R.blank_inputs(1, 3, **rows)
    cfg, ccfg = R.category_config(young, **(opts or {})), CR.default_config(thermo_type="zero_layer")
    fcfg = S.fsd_config(nb, young, distinguish_mech_fsd=dist, welding_type=welding)
    fsd = {"conc_fsd": np.array(bins, F).reshape(nb, 1), "conc_mech_fsd": None if mech is None else np.array(mech, F).reshape(nb, 1)}
    out = S.slab_coupled(inp, fsd, cfg, ccfg, fcfg, ALB, tri, young, R.DT, R.clock(), melt_type=melt_type)
    return inp, fsd, out, ccfg, cfg


MELTING = {"K:hi": 1.99, "K:hi_old": 2., "K:del_hi": -0.01, "K:hs": 0.1, "K:tfrw": -1.8, "sst": -1.7, "sss": 33., "F:Qow": -60., "tice0": -5.}


def test_by_hand_an_unbroken_element_follows_melt_type_2_on_ctot():
    """classic category, conc = 0.8 all in the last of 3 bins: |0.8 - ctot| = 0 < 1e-7.  del_c_melt = PhiM * (1 - 0.8) * min(0, -60) * 900 / (1.99 qi + 0.1 qs),
    del_c = (conc / ctot) * del_c_melt = del_c_melt, Qow becomes -30; lat_melt_rate stays 0, so redistributeThermoFSD refreezes: the last bin takes del_c_fsd =
    M_conc - old_conc"""
    inp, fsd, (rows, w1, w2, info), ccfg, cfg = _one(False, 3, [0., 0., 0.8], conc=0.8, thick=1.6, snow_thick=0.08, **MELTING)
    qi, qs = F(333.55e3) * F(917.), F(333.55e3) * F(330.)
    del_c_melt = F(0.5) * (F(1.) - F(0.8)) * F(-60.) * F(900.) / (F(1.99) * qi + F(0.1) * qs)
    conc = F(0.8) + del_c_melt
    assert inp["conc"][0] == conc and -1e-5 < del_c_melt < 0
    assert w2[0] == S.BIT2["melt3"] | S.BIT2["unbroken"]
    assert fsd["conc_fsd"][2][0] == F(0.8) + (conc - F(0.8)) and fsd["conc_fsd"][0][0] == 0. and fsd["conc_fsd"][1][0] == 0.
    # Qow = -60 * (1 - PhiM) = -30, then Qow -= del_c * hs * qs / ddt; Qa = Qow * old_ow_fraction (no Qia)
    Qow = F(-60.) * (F(1.) - F(0.5))
    Qow = Qow - del_c_melt * F(0.1) * qs / F(900.)
    assert rows["Qa"][0] == Qow * (F(1.) - F(0.8))


def test_by_hand_a_broken_element_melts_laterally():
    """classic category, conc = 0.8 as bins 0.2, 0.3, 0.3 of widths 10 and centres 15, 25, 35; tw_new - tfrw = dT.  lat_melt_rate = -3e-6 * pow(dT, 1.36) * 2;
    cat0_del_c = lat * 0.2 / 10 * 900; del_c_melt = cat0 + lat * (0.2 * 2 / 15) * 900 + lat * (0.3 * 2 / 25) * 900.  redistributeThermoFSD: fsd_dr = (0, 0.3 / 10, 0,
    0), dfsd_dr = (0.03, -0.03, 0); bin 0 += 900 lat (-0.03 + 0.2 * 2 / 15) + cat0, bin 1 += 900 lat (0.03 + 0.3 * 2 / 25), bin 2 stays"""
    inp, fsd, (rows, w1, w2, info), ccfg, cfg = _one(False, 3, [0.2, 0.3, 0.3], conc=0.8, thick=1.6, snow_thick=0.08, **MELTING)
    mld = F(ccfg["constant_mld"])
    tw_new = F(-1.7) - F(900.) * (F(-60.) + F(0.)) / (mld * R.rhow * R.cpw)
    dT = tw_new - F(-1.8)
    lat = -F(3.e-6) * F(R._pow(float(dT), 1.36))
    lat = lat * F(2.)
    cat0 = lat * F(0.2) / F(10.) * F(900.)
    d = F(0.) + cat0
    d = d + lat * (F(0.2) * F(2.) / F(15.)) * F(900.)
    d = d + lat * (F(0.3) * F(2.) / F(25.)) * F(900.)
    assert w2[0] == S.BIT2["melt3"] | S.BIT2["lateral"] | S.BIT2["lat_melting"]
    assert inp["conc"][0] == F(0.8) + (F(0.8) / F(0.8)) * d and -0.01 < d < 0
    dr1 = F(0.3) / F(10.)
    b0 = F(0.2) + F(900.) * lat * (-(dr1 - F(0.)) + F(0.2) * F(2.) / F(15.))
    b0 = b0 + cat0
    b1 = F(0.3) + F(900.) * lat * (-(F(0.) - dr1) + F(0.3) * F(2.) / F(25.))
    assert (fsd["conc_fsd"][0][0], fsd["conc_fsd"][1][0], fsd["conc_fsd"][2][0]) == (b0, b1, F(0.3))
    assert abs((b0 + b1 + 0.3) - inp["conc"][0]) < 1e-4       # (the reference's budget closes only to first order: its own debug check allows 1e-7 of drift a step)


THIN = {"K:hi": 0.005, "K:hi_old": 0.02, "K:del_hi": -0.015, "K:hs": 0., "K:tfrw": -1.8, "sst": -1.7, "sss": 33., "F:Qow": -60., "tice0": -5.}


def test_by_hand_melt_out_with_young_ice_rescales_the_bins():
    """young category, conc 0.5 + young 0.25 as bins 0.25, 0.5 (sum 0.75 > old_conc 0.5, M_conc_young > 0), hi = 0.005 < hmin: every bin times (1 - 0.5 / 0.75);
    without the mechanical bins the else of FE.cpp:5754 then zeroes them all the same; with them the mechanical bins (0.375, 0.375) are rescaled too and nothing is
    zeroed"""
    st = dict(conc=0.5, thick=0.01, conc_young=0.25, h_young=0.025, **THIN)
    inp, fsd, (rows, w1, w2, info), *_ = _one(True, 2, [0.25, 0.5], melt_type=2, **st)
    assert w1[0] & R.BIT["limit"] and w2[0] == S.BIT2["limit_rescaled"] | S.BIT2["limit_zeroed"] and not fsd["conc_fsd"].any() and inp["conc"][0] == 0.
    inp, fsd, (rows, w1, w2, info), *_ = _one(True, 2, [0.25, 0.5], mech=[0.375, 0.375], melt_type=2, dist=1, **st)
    assert w2[0] == S.BIT2["limit_rescaled"] | S.BIT2["limit_mech_rescaled"]
    assert fsd["conc_fsd"][0][0] == F(0.25) + (-F(0.5)) * F(0.25) / F(0.75) and fsd["conc_fsd"][1][0] == F(0.5) + (-F(0.5)) * F(0.5) / F(0.75)
    assert fsd["conc_mech_fsd"][0][0] == F(0.375) + (-F(0.5)) * F(0.375) / F(0.75) == fsd["conc_mech_fsd"][1][0]
    assert abs(fsd["conc_fsd"].sum() - 0.25) < 1e-15           # what is left is the young ice's share


def test_by_hand_melt_out_without_young_ice():
    """classic category: nothing is rescaled; the bins are zeroed, and with the mechanical bins kept apart NOTHING is touched (the else is the inner if's)"""
    st = dict(conc=0.5, thick=0.01, **THIN)
    inp, fsd, (rows, w1, w2, info), *_ = _one(False, 2, [0.25, 0.25], melt_type=2, **st)
    assert w1[0] & R.BIT["limit"] and w2[0] == S.BIT2["limit_zeroed"] and not fsd["conc_fsd"].any()
    inp, fsd, (rows, w1, w2, info), *_ = _one(False, 2, [0.25, 0.25], mech=[0.125, 0.375], melt_type=2, dist=1, **st)
    assert w2[0] == 0 and fsd["conc_fsd"].tolist() == [[0.25], [0.25]] and fsd["conc_mech_fsd"].tolist() == [[0.125], [0.375]]


def test_by_hand_refreezing_that_fills_the_lead():
    """young category, conc 0.75 + young 0.125, a heat loss of 5e4 W/m2 over the lead of 0.125: newice / h_young_min is far above it, M_conc_young = 1 - 0.75 =
    0.25 and 0.75 + 0.25 == 1.: the last bin is 1., the others 0."""
    inp, fsd, (rows, w1, w2, info), *_ = _one(True, 3, [0.25, 0.25, 0.375], conc=0.75, thick=1.5, conc_young=0.125, h_young=0.0125,
                                              **dict(MELTING, **{"K:hi": 2.001, "K:del_hi": 0.001, "F:Qow": 5e4}))
    assert inp["conc_young"][0] == 0.25 and inp["conc"][0] == 0.75 and w1[0] & R.BIT["supercooled"]
    assert w2[0] == S.BIT2["fills_lead"] and fsd["conc_fsd"].ravel().tolist() == [0., 0., 1.]


def test_by_hand_mechanical_healing_reads_the_new_relaxation_time():
    """classic category, freezing (del_hi > 0), temp_dep_healing: section 9 writes M_time_relaxation_damage = max(25 days * 20 / deltaT, ddt) and 9.b reads THAT:
    w = min(1, 900 / it), mech = mech * (1 - w) + w * bins; the bins are unbroken (no welding below the gate) and take del_c_fsd = 0"""
    inp, fsd, (rows, w1, w2, info), *_ = _one(False, 2, [0., 0.5], mech=[0.25, 0.25], melt_type=3, dist=1, welding=FS.WELD_ROACH, opts=dict(temp_dep_healing=1), conc=0.5,
                                              thick=1., time_relaxation_damage=900., **dict(MELTING, **{"K:hi": 2.001, "K:del_hi": 0.001, "F:Qow": 10.}))
    theal = inp["time_relaxation_damage"][0]
    assert theal > 1e4 and w1[0] & R.BIT["heal_ice"] and w2[0] == S.BIT2["healed"] and info["ndt_mrg"][0] == 0
    w = min(F(1.), F(900.) / F(theal))
    assert fsd["conc_mech_fsd"][0][0] == F(0.25) * (F(1.) - w) + w * F(0.) and fsd["conc_mech_fsd"][1][0] == F(0.25) * (F(1.) - w) + w * F(0.5)
    assert fsd["conc_fsd"].ravel().tolist() == [0., 0.5]


# ---- 3: designed strata
@pytest.mark.parametrize("young", [True, False])
def test_every_new_bit_is_taken_and_not_taken_on_designed_strata(mesh, young):
    Ne = mesh[1].shape[0]
    seen = {}
    for dist in (0, 1):
        r = run(mesh, 3, young, 3, dist=dist, opts=dict(temp_dep_healing=1))
        for k in S.BRANCHES2:
            seen[k] = max(seen.get(k, 0), int(S.took2(r["w2"], k).sum()))
            assert not S.took2(r["w2"], k).all(), k
        for k, m in r["sets"].items():
            assert m.sum() >= 0.02 * Ne, k
        assert S.took2(r["w2"], "ctot_break")[r["sets"]["ctot_break"]].all()
        assert (S.took2(r["w2"], "fills_lead")[r["sets"]["fills_lead"]]).all() == young
        if young:
            assert S.took2(r["w2"], "young_shrinks")[r["sets"]["young_shrinks"] & (r["broken"] == 1)].all()
        assert np.isfinite(r["bins"]["conc_fsd"]).all() and not r["info"]["weld_crash"]
    only_young = ("limit_rescaled", "limit_mech_rescaled", "fills_lead", "del_c_fsd_ge0", "young_shrinks")
    for k in S.BRANCHES2:
        assert (seen[k] >= 0.02 * Ne) == (young or k not in only_young), (k, seen[k])


# ---- 4: no decision on an edge
@pytest.mark.parametrize("young", [True, False])
def test_no_decision_sits_on_an_edge(mesh, young):
    """every input and every bin one unit in the last place away from and towards zero (zeros and ones stay, as in tests/test_slab_ref.py), and the argument of
    melt_type 3's pow moved by +-4 units: both branch words stay"""
    gm, tri = mesh
    base = S.make_inputs(gm.x, gm.y, tri, 3, young)
    r0 = run(mesh, 3, young, 3, dist=1, opts=dict(temp_dep_healing=1), inputs=base)
    w1 = R.edge_of_the_reference(base[0], r0["cfg"], r0["w1"])
    # The one FSD decision that sits on an edge by the reference's own arithmetic: where young ice thicker than h_young_max_sharp is handed to the old ice
    # (FE.cpp:5523-5530) del_c = M_conc_young - tmp and M_conc_young = tmp, so del_c_fsd = ((M_conc + del_c) - old_conc) + (tmp - old_conc_young) is zero but for
    # its roundings, and del_c_fsd >= 0 (FE.cpp:4585) is decided by them.  Both sides give the same bins to some 1e-17: the bit is not compared there.
    sharp = R.took(r0["w1"], "n4_sharp")
    own = lambda w2: np.where(sharp, w2 & np.uint32(~S.BIT2["del_c_fsd_ge0"] & 0xFFFFFFFF), w2)
    for direction in (1, -1):
        inp = R.moved_one_ulp(base[0], direction)
        fsd = R.moved_one_ulp(base[1], direction)
        r = run(mesh, 3, young, 3, dist=1, opts=dict(temp_dep_healing=1), inputs=(inp, fsd) + base[2:])
        assert np.array_equal(R.edge_of_the_reference(base[0], r0["cfg"], r["w1"]), w1), np.flatnonzero(r["w1"] != r0["w1"])[:5]
        assert np.array_equal(own(r["w2"]), own(r0["w2"])), (np.flatnonzero(r["w2"] != r0["w2"])[:5], (r["w2"] ^ r0["w2"])[r["w2"] != r0["w2"]][:5])
    for shift in (4, -4):
        r = run(mesh, 3, young, 3, dist=1, opts=dict(temp_dep_healing=1), inputs=base, dtw_shift=shift)
        assert np.array_equal(r["w1"], r0["w1"]) and np.array_equal(r["w2"], r0["w2"])


# ---- 5: the welding's loop stays short
@pytest.mark.parametrize("nb", [2, 7, 16])
def test_the_welding_takes_at_most_8_sub_steps(mesh, nb):
    r = run(mesh, nb, True, 3)
    ndt = r["info"]["ndt_mrg"]
    assert ndt.max() <= 8 and (ndt >= 2).sum() > 50 and (ndt == 0).sum() > 50 and (ndt == -1).sum() > 50, np.bincount(ndt + 1)


# ---- 6: planted mistakes
def _differs(a, b):
    worst = 0.
    for k in R.ROWS:
        worst = max(worst, float(np.nanmax(np.abs(a["rows"][k] - b["rows"][k]) / np.maximum(1., np.abs(b["rows"][k])))))
    for k in R.IN_PLACE:
        worst = max(worst, float(np.nanmax(np.abs(a["work"][k] - b["work"][k]) / np.maximum(1., np.abs(b["work"][k])))))
    for k in ("conc_fsd", "conc_mech_fsd"):
        if a["bins"][k] is not None:
            worst = max(worst, float(np.nanmax(np.abs(a["bins"][k] - b["bins"][k]) / np.maximum(1., np.abs(b["bins"][k])))))
    return worst, not (np.array_equal(a["w1"], b["w1"]) and np.array_equal(a["w2"], b["w2"]))


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_a_planted_mistake_is_noticed(mesh, mistake):
    """each by some row at more than 1e-6 in |a - b| / max(1, |b|), or by a branch word.  `<=` for `<` at the unbroken test needs an element ON the edge, which
    the designed inputs avoid: twenty are made, their last bin exactly 1e-7 below ctot"""
    kw = dict(dist=1, opts=dict(temp_dep_healing=1))
    if mistake == "else_outer":
        kw["dist"] = 0
    inputs = None
    if mistake == "unbroken_le":
        gm, tri = mesh
        inputs = S.make_inputs(gm.x, gm.y, tri, 3, True)
        inp, fsd = inputs[0], inputs[1]
        e = np.flatnonzero((inputs[2] == R.STRATA.index("melt_myi")) & ~inputs[4]["young_shrinks"])[:20]
        assert e.size == 20
        # ctot = 2^-23 without young ice and the last bin 2^-23 - 1e-7: the difference is exact (Sterbenz), so |M_conc_fsd[nb-1] - ctot| IS the double 1e-7
        tot = F(2.) ** -23
        inp["conc"][e] = tot
        for k in ("conc_young", "h_young", "hs_young", "conc_myi", "thick_myi", "fyi_fraction"):
            inp[k][e] = 0.
        inp["thick"][e], inp["snow_thick"][e] = tot * inp["K:hi_old"][e], tot * inp["K:hs"][e]
        fsd["conc_fsd"][:, e] = np.array([1e-7, 0., tot - F(1e-7)])[:, None]
        assert (np.abs(fsd["conc_fsd"][2][e] - (inp["conc"][e] + inp["conc_young"][e])) == 1e-7).all()
    good = run(mesh, 3, True, 3, inputs=inputs, **kw)
    bad = run(mesh, 3, True, 3, inputs=inputs, drop=(mistake,), **kw)
    worst, words = _differs(bad, good)
    print(mistake, worst, words)
    assert worst > 1e-6 or words, (mistake, worst)


# ---- 7: the kernels' source on the host
@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "slab_fsd_host_kernel")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-builtin", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "slab_fsd_host_kernel.cpp"), "-o", exe])
    return exe


def _write_slab_input(path, Ne, Nn, tri, inp, cfg, ccfg, young, dt, clock):
    """the input of tests/slab_host_kernel.cpp (tests/test_slab_host_kernel.py writes the same)"""
    E = _abi.COL_ENUMS
    with open(path, "wb") as f:
        f.write(struct.pack("20i", Ne, Nn, int(young), int(ccfg["thermo_type"] == "winton"), E["freezingpoint_type"][ccfg["freezingpoint_type"]],
                            E["mld_source"][ccfg["mld_source"]], dt, *[int(cfg[k]) for k in _abi.SLAB_CONFIG_INTS], *[int(clock[k]) for k in _abi.SLAB_CLOCK]))
        f.write(struct.pack("15d", *[cfg[k] for k in _abi.SLAB_CONFIG_REALS], ccfg["freezingpoint_mu"], ccfg["snow_cond"], ccfg["constant_mld"], ALB))
        f.write(tri.astype(np.int32).tobytes())
        f.write(inp["wind"].tobytes())
        for k in R.FLUX + R.COL + ("precip", "mld", "conc_upd") + R.IN_PLACE:
            f.write(inp[k].tobytes())


@pytest.mark.parametrize("welding", [FS.WELD_NONE, FS.WELD_ROACH], ids=["noweld", "roach"])
@pytest.mark.parametrize("dist", [0, 1], ids=["bins", "mech"])
@pytest.mark.parametrize("melt_type", [1, 2, 3])
@pytest.mark.parametrize("young", [True, False], ids=["young", "classic"])
@pytest.mark.parametrize("nb", [1, 2, 3, 7, 16])
def test_the_kernel_source_on_the_host_gives_the_restatements_bits(binary, mesh, tmp_path, nb, young, melt_type, dist, welding):
    gm, tri = mesh
    Ne = tri.shape[0]
    r = run(mesh, nb, young, melt_type, thermo="winton" if nb % 2 else "zero_layer", dist=dist, welding=welding, debug=1, opts=dict(temp_dep_healing=1))
    cfg, ccfg, fcfg, inp, fsd = r["cfg"], r["ccfg"], r["fcfg"], r["inp"], r["fsd"]
    fin, ffsd, fout = (str(tmp_path / k) for k in ("in.bin", "fsd.bin", "out.bin"))
    _write_slab_input(fin, Ne, gm.x.size, tri, inp, cfg, ccfg, young, R.DT, R.clock())
    t = fcfg["tables"]
    with open(ffsd, "wb") as f:
        f.write(struct.pack("8i", melt_type, nb, dist, welding, 1, 1, 0, 0))
        f.write(struct.pack("d", fcfg["welding_kappa"]))
        for k in ("bin_widths", "bin_centres", "area_scaled_up", "area_scaled_centered", "area_scaled_binwidth"):
            f.write(np.ascontiguousarray(t[k], np.float64).tobytes())
        f.write(np.ascontiguousarray(t["alpha_merge"], np.int32).tobytes())
        f.write(fsd["conc_fsd"].tobytes())
        f.write(fsd["conc_mech_fsd"].tobytes())
    subprocess.check_call([binary, fin, ffsd, fout])
    raw = np.fromfile(fout)
    n0 = len(R.ROWS) + len(R.IN_PLACE) + 1
    got = raw[:(n0 + 2 * nb + 1) * Ne].reshape(n0 + 2 * nb + 1, Ne)
    flags = raw[(n0 + 2 * nb + 1) * Ne:]
    for i, k in enumerate(R.ROWS + R.IN_PLACE):
        want = r["rows"][k] if i < len(R.ROWS) else r["work"][k]
        same = R.same_bits(got[i], want)
        assert same.all(), (k, int((~same).sum()), np.flatnonzero(~same)[:5], got[i][~same][:3], want[~same][:3])
    assert np.array_equal(got[n0 - 1].astype(np.uint32), r["w1"])
    bad = got[n0 + 2 * nb].astype(np.uint32) != r["w2"]
    assert not bad.any(), (np.flatnonzero(bad)[:5], got[n0 + 2 * nb][bad][:5], r["w2"][bad][:5])
    for j, k in enumerate(("conc_fsd", "conc_mech_fsd")):
        same = R.same_bits(got[n0 + j * nb:n0 + (j + 1) * nb], r["bins"][k])
        assert same.all(), (k, np.argwhere(~same)[:5])
    if not dist:
        assert np.array_equal(r["bins"]["conc_mech_fsd"], fsd["conc_mech_fsd"])                 # attached but not kept apart: left alone
    assert flags.tolist() == [float(r["info"]["thermo_fsd_crash"]), float(r["info"]["weld_crash"])]
    if melt_type == 3 and nb > 1:
        assert S.took2(r["w2"], "lateral").sum() > 50 and S.took2(r["w2"], "unbroken").sum() > 50
