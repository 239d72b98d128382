"""thermo()'s slab loop with floe-size bins attached on the device (nxs_dyn_slab_coupled: k_coupled_thermo, k_coupled_bins) against tests/slab_fsd_ref.py, the
line-by-line restatement of FE.cpp:5413-6133 as an OASIS build compiles it (whose parity with a binary of the reference is NOT pinned: model/ cannot be compiled
here).  Each round writes the designed flux rows AND column rows through the device_rows doors of nxs_dyn_fluxes_get / nxs_dyn_column_get, so that neither
earlier slice's tolerance enters, then runs slab_coupled(dt, clock) and fsd_update().  Under melt_type 1 and 2 nothing calls more than sqrt and round and
everything is required BIT FOR BIT: the 29 rows, every row written in place, the bins, the mechanical bins, time_relaxation_damage and both branch words, over
three consecutive rounds whose state feeds the next.  Under melt_type 3 the device's pow enters: both branch words are the restatement's on every element
(tests/test_slab_fsd_ref.py shows that no element sits on an edge), every element that does not take the pow is bit for bit, and the rest is measured as |device
- restatement| / max(1, |restatement|) per row, printed, and bounded by four times the figure recorded on the MI355X, capped at 1e-9; a recorded 0 means bits.
ONE BIT IS DECIDED BY ROUNDINGS ALONE: where young ice thicker than h_young_max_sharp is handed to the old ice (FE.cpp:5523-5530, NXS_SLAB_BR_N4_SHARP) del_c_fsd
is zero but for its roundings, so NXS_SLAB_FSD_BR_DEL_C_FSD_GE0 (FE.cpp:4585) has no margin there (tests/test_slab_fsd_ref.py exempts it from its no-edge check
for that reason).  It is still required to be the restatement's here: that branch is only reached with lat_melt_rate == 0, so no library call enters del_c_fsd,
and the device does the restatement's IEEE operations one by one (the build is uncontracted).  A device build that contracted or reordered them would show up
first in this bit, and at once in the bins, which are compared bit for bit on the same elements."""
import functools

import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import fsd_ref as FS
import slab_fsd_ref as S
import slab_ref as R
from nextsim_amd import _abi

pytestmark = pytest.mark.gpu

DT = R.DT
CAP = 1e-9
ALB = FR.default_config()["ocean_albedo"]
BINS = ("bins", "mech_bins", "bins_updated", "mech_bins_updated")
# Largest |device - restatement| / max(1, |restatement|) recorded on the MI355X per row under melt_type 3 (the device's pow against glibc's), over the prints of
# test_melt_type_3: both meshes, 2 / 7 / 16 bins, both categories, both thermo types, three rounds.  The bound is 4 * the figure, capped at 1e-9, and 0 means
# bits.  Key: the row, "state:<name>" for a row written in place, or one of BINS.  A row that is not listed was recorded as 0.
RECORDED = {
    "Qa": 8.88e-15,       # (one unit in the last place of Qow, which the melt rate enters times hi * qi; it is below the last place of every other row)
}


def _key(i, k):
    return k if i < len(R.ROWS) else "state:" + k


def _bound(key):
    return min(CAP, 4. * RECORDED.get(key, 0.))


@functools.lru_cache(maxsize=None)
def _case(kind, young, nb):
    gm, p, g, lms, fields = cases.make_case(kind, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE if young else _abi.NXS_ICECAT_CLASSIC)
    lm, f = lms[0], fields[0]
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp, fsd, strata, broken, sets = S.make_inputs(lm.coord_x, lm.coord_y, tri, nb, young)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    return p, lm, f, tri, inp, fsd, finp


def _handle(kind, young, nb, thermo="winton", melt_type=None, opts=None, fopts=None, sane=False, mech=True, attach=True):
    p, lm, f, tri, inp, fsd, finp = _case(kind, young, nb)
    inp = R.sane_inputs(inp, f) if sane else R.copy(inp)
    ccfg = CR.default_config(thermo_type=thermo)
    cfg = R.category_config(young, **(opts or {}))
    fcfg = S.fsd_config(nb, young, **(fopts or {}))
    fe, f = R.gpu_handle(p, lm, f, inp, finp, ccfg, cfg)
    if attach:
        S.attach(fe, fsd, fcfg, mech)
    if melt_type is not None:
        fe.slab_coupled_configure(melt_type)
    return fe, f, tri, inp, S.copy_fsd(fsd, mech), cfg, ccfg, fcfg


def _round(fe, f, tri, ref, bins, cfg, ccfg, fcfg, young, melt_type, flags, what, measure=None):
    """one round on the device and in the restatement (ref and bins are updated in place and then take the device's rows: both start the next round from the same
    bits); measure: a dict that collects the worst figures of the elements that take the pow (every other element must still be bit for bit); None: everything
    bit for bit"""
    clock = R.clock(**flags)
    mech = bins["conc_mech_fsd"] is not None
    got, st, words, words2, b1, b2, before, after = S.gpu_round(fe, f, ref, bins, DT, clock, mech)
    rows, ref_words, ref_words2, info = S.slab_coupled(ref, bins, cfg, ccfg, fcfg, ALB, tri, young, DT, clock, melt_type=melt_type)
    assert np.array_equal(words, ref_words), (what, "branches", np.flatnonzero(words != ref_words)[:5], [hex(int(v)) for v in (words ^ ref_words)[words != ref_words][:5]])
    assert np.array_equal(words2, ref_words2), (what, "fsd branches", np.flatnonzero(words2 != ref_words2)[:5], [hex(int(v)) for v in (words2 ^ ref_words2)[words2 != ref_words2][:5]])
    for k in before:                                            # the flux rows and the column rows are read-only: the same bits before and after
        assert R.same_bits(before[k], after[k]).all(), (what, "read-only row", k)
    exact = ~S.pow_taken(ref, ref_words2)
    assert measure is not None or exact.all()
    pairs = [(_key(i, k), (got[k], rows[k]) if i < len(R.ROWS) else (st[k], ref[k])) for i, k in enumerate(R.ROWS + R.IN_PLACE)]
    pairs += [("bins", (b1["conc_fsd"], bins["conc_fsd"].copy()))] + ([("mech_bins", (b1["conc_mech_fsd"], bins["conc_mech_fsd"].copy()))] if mech else [])
    S.update_fsd(ref, bins, fcfg, young)
    pairs += [("bins_updated", (b2["conc_fsd"], bins["conc_fsd"]))] + ([("mech_bins_updated", (b2["conc_mech_fsd"], bins["conc_mech_fsd"]))] if mech else [])
    for key, (dev, want) in pairs:
        same = R.same_bits(dev, want)
        bad = np.argwhere(~(same | ~exact))                     # (exact broadcasts over the bins)
        assert bad.size == 0, (what, key, "not bit for bit without the pow", bad[:5])
        if measure is not None:
            assert np.array_equal(np.isfinite(dev), np.isfinite(want)), (what, key)
            ok = np.isfinite(want)
            worst = float(np.max(np.abs(dev[ok] - want[ok]) / np.maximum(1., np.abs(want[ok])))) if ok.any() else 0.
            measure[key] = max(measure.get(key, 0.), worst)
    for k in R.IN_PLACE:
        ref[k] = st[k].copy()
    bins["conc_fsd"] = b2["conc_fsd"].copy()
    if mech:
        bins["conc_mech_fsd"] = b2["conc_mech_fsd"].copy()
    return got, st, words, words2, info


CASES = [(kind, nb, young, thermo) for kind in ("small", "toy") for nb in (2, 7, 16) for young in (True, False) for thermo in ("winton", "zero_layer")]
ROUNDS = ({}, dict(last_step_of_day=1), dict(first_step_of_day=1))


@pytest.mark.parametrize("melt_type", [1, 2])
@pytest.mark.parametrize("kind,nb,young,thermo", CASES)
def test_three_rounds_bit_for_bit(kind, nb, young, thermo, melt_type):
    """the mechanical bins kept apart (so that they are rescaled and healed) under melt_type 1, attached but not kept apart under melt_type 2"""
    fe, f, tri, inp, bins, cfg, ccfg, fcfg = _handle(kind, young, nb, thermo, melt_type, opts=dict(temp_dep_healing=1), fopts=dict(distinguish_mech_fsd=int(melt_type == 1)))
    ref = R.copy(inp)
    seen = np.uint32(0)
    for call, flags in enumerate(ROUNDS):
        got, st, words, words2, info = _round(fe, f, tri, ref, bins, cfg, ccfg, fcfg, young, melt_type, flags, f"{kind} {nb} {thermo} young={young} round {call}")
        seen |= np.bitwise_or.reduce(words2)
        assert info["ndt_mrg"].max() <= 8
    for k in ("limit_zeroed" if melt_type == 2 else "healed", "welded") + (("limit_rescaled",) if young else ()):
        assert seen & np.uint32(S.BIT2[k]), k
    assert not fe.fsd_get()["weld_crash"]
    fe.close()


@pytest.mark.parametrize("kind,nb,young,thermo", CASES)
def test_melt_type_3(kind, nb, young, thermo):
    """the device's pow: every element that does not take it is bit for bit, over three rounds with the mechanical bins kept apart"""
    fe, f, tri, inp, bins, cfg, ccfg, fcfg = _handle(kind, young, nb, thermo, 3, opts=dict(temp_dep_healing=1), fopts=dict(distinguish_mech_fsd=1))
    ref = R.copy(inp)
    measure = {}
    seen = np.uint32(0)
    for call, flags in enumerate(ROUNDS):
        got, st, words, words2, info = _round(fe, f, tri, ref, bins, cfg, ccfg, fcfg, young, 3, flags, f"melt 3 {kind} {nb} {thermo} young={young} round {call}", measure=measure)
        seen |= np.bitwise_or.reduce(words2)
    print(f"RECORD {kind} {nb} {thermo} young={young}: " + ", ".join(f'"{k}": {v:.2e}' for k, v in measure.items() if v > 0))
    for k in ("melt3", "unbroken", "ctot_break", "lateral", "lat_melting", "welded", "healed") + (("fills_lead", "young_shrinks", "del_c_fsd_ge0", "limit_mech_rescaled") if young else ()):
        assert seen & np.uint32(S.BIT2[k]) or (nb == 1 and k in ("lateral", "lat_melting")), k
    fe.close()
    for k, v in measure.items():
        assert v <= _bound(k), (kind, nb, thermo, young, k, v, _bound(k))


@pytest.mark.parametrize("young,thermo", [(True, "winton"), (False, "zero_layer")])
def test_with_melt_type_1_every_non_bin_row_is_slabs(young, thermo):
    """slab_coupled on a handle with bins against slab() on a second handle without, both from the device's own fluxes and column"""
    a, fa, tri, inp, bins, cfg, ccfg, fcfg = _handle("small", young, 7, thermo, 1, opts=dict(melt_type=2))      # (the slab's own melt_type is overridden)
    b, fb, *_ = _handle("small", young, 7, thermo, opts=dict(melt_type=1), attach=False)
    for fe in (a, b):
        fe.fluxes(); fe.column(DT)
    a.slab_coupled(DT, R.clock()); b.slab(DT, R.clock())
    ra, rb = a.slab_rows(), b.slab_rows()
    for k in R.ROWS:
        assert R.same_bits(ra[k], rb[k]).all(), k
    sa, sb = R.device_state(a), R.device_state(b)
    for k in sa:
        assert R.same_bits(sa[k], sb[k]).all(), k
    assert np.array_equal(a.debug_array("slab_branches"), b.debug_array("slab_branches")) and np.abs(ra["vice_melt"]).max() > 0
    a.close(); b.close()


def test_the_next_step_reads_what_slab_coupled_wrote():
    """after slab_coupled() and fsd_update(), the next step is bit for bit that of a second handle given the restated state and bins through put_state / put_coupled"""
    from nextsim_amd import dynamics
    fe, f, tri, inp, bins, cfg, ccfg, fcfg = _handle("small", True, 7, "winton", 2, opts=dict(temp_dep_healing=1), fopts=dict(distinguish_mech_fsd=1), sane=True)
    ref = R.copy(inp)
    _round(fe, f, tri, ref, bins, cfg, ccfg, fcfg, True, 2, {}, "before the step")
    assert not np.array_equal(ref["time_relaxation_damage"], inp["time_relaxation_damage"]) and not np.array_equal(ref["conc"], inp["conc"])
    fe.step(); fe.synchronize()
    p, lm = _case("small", True, 7)[:2]
    fe2 = dynamics.FiniteElementDynamics(p)
    f2 = dict(f, **{k: ref[k] for k in R.STATE})
    fe2.set_mesh(lm); fe2.put_state(f2); fe2.set_forcing(f2)
    fe2.put_coupled(conc_fsd=bins["conc_fsd"]); fe2.fsd_put(conc_mech_fsd=bins["conc_mech_fsd"])
    fe2.step(); fe2.synchronize()
    sa, sb = fe.get_state(), fe2.get_state()
    for k in sa:
        assert R.same_bits(sa[k], sb[k]).all(), k
    assert R.same_bits(fe.get_coupled(False, 7)["conc_fsd"], fe2.get_coupled(False, 7)["conc_fsd"]).all()
    assert np.abs(sa["VT"]).max() > 0 and np.isfinite(sa["VT"]).all()
    fe.close(); fe2.close()


def test_call_order_and_what_is_missing():
    from nextsim_amd import dynamics
    fe, f, tri, inp, bins, cfg, ccfg, fcfg = _handle("small", True, 2, attach=False)
    Ne = tri.shape[0]
    clock = R.clock()

    def refused(call, text, code=-4):
        with pytest.raises(dynamics.NxsError) as e:
            call()
        assert e.value.code == code and text in str(e.value), (e.value.code, str(e.value))
        return True

    coupled = lambda: fe.slab_coupled(DT, clock)
    fe.fluxes(); fe.column(DT)
    fe.slab_coupled_configure(3)                                                                 # accepted without bins: the call asks for them
    assert refused(coupled, "no floe-size bins are attached")
    fe.put_coupled(conc_fsd=bins["conc_fsd"])
    assert refused(coupled, "before nxs_dyn_fsd_configure")
    assert refused(lambda: fe.slab(DT, clock), "floe-size bins are attached")                    # slab() is as it was
    with pytest.raises(dynamics.NxsError) as e:
        fe.slab_configure(melt_type=3)
    assert e.value.code == -1 and "OASIS" in str(e.value)
    fe.fsd_configure(fcfg["tables"], **FS.library_options(fcfg))
    fe.put_coupled(conc_fsd=np.zeros((3, Ne)))
    assert refused(coupled, "configured for 2 bins, 3 attached")
    fe.put_coupled(conc_fsd=bins["conc_fsd"])
    fe.fsd_configure(fcfg["tables"], **FS.library_options(dict(fcfg, distinguish_mech_fsd=1)))
    assert refused(coupled, "distinguish_mech_fsd without M_conc_mech_fsd")
    fe.fsd_put(conc_mech_fsd=bins["conc_mech_fsd"])
    assert refused(lambda: fe.slab_coupled(0, clock), "dt = 0", -1) and fe.L.nxs_dyn_slab_coupled(fe.h, DT, None) == -1 and b"no clock" in fe.L.nxs_dyn_last_error(fe.h)
    assert refused(lambda: fe.debug_array("slab_fsd_branches"), "no nxs_dyn_slab_coupled")
    assert refused(lambda: fe.slab_coupled_configure(4), "melt_type = 4 (1 .. 3", -1)
    fe.slab_coupled_configure(3)
    coupled()
    assert refused(coupled, "second nxs_dyn_slab without a new nxs_dyn_column")                   # the column's rows are spent, as by slab()
    assert len(fe.slab_rows()) == len(R.ROWS) and fe.slab_get(("age",))["age"].shape == (Ne,) and fe.debug_array("slab_branches").shape == (Ne,)
    # what slab() refuses, slab_coupled() refuses
    fe.slab_configure(**dict(cfg, newice_type=1))
    fe.fluxes(); fe.column(DT)
    assert refused(coupled, "newice_type = 1 on a handle of the young-ice category")
    fe.slab_configure(**cfg)
    # after set_mesh on a live handle: both configurations survived, the rows and the bins went with the mesh
    lm = fe.lm
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    assert refused(coupled, "before nxs_dyn_column on this mesh")
    R.feed_flux_state(fe, inp, _case("small", True, 2)[6])
    fe.column_set_forcing(precip=inp["precip"], snow=np.ones(Ne))
    fe.column_put(tice1=inp["tice1"], tice2=inp["tice2"])
    fe.slab_put(**{k: inp[k] for k in R.SLAB_STATE})
    fe.fluxes(); fe.column(DT)
    assert refused(coupled, "no floe-size bins are attached")
    S.attach(fe, bins, dict(fcfg, distinguish_mech_fsd=1))
    coupled()
    assert (fe.debug_array("slab_fsd_branches").astype(np.uint32) & np.uint32(S.BIT2["melt3"])).any()    # melt_type 3 survived set_mesh
    fe.close()
    fe2 = dynamics.FiniteElementDynamics(_case("small", True, 2)[0])
    with pytest.raises(dynamics.NxsError) as e:
        fe2.slab_coupled_configure(2)
    assert e.value.code == -4 and "before nxs_dyn_slab_configure" in str(e.value)
    fe2.close()


def test_thermo_fsd_crash_is_raised_by_one_element_and_cleared():
    """under debug_fsd, with every bin unbroken, the mechanical bins equal to the bins and no welding.  The first round starts from the designed state, whose
    "no_room" stratum holds more ice than a cell (conc = 1 plus young ice): its sums do not close and the flag is raised, as the restatement says.  fsd_update
    then makes the bins the state's, and in the second round the sums of FE.cpp:4635-4646 close on every element; in the third one element's last bin is 1e-3
    too large"""
    fe, f, tri, inp, bins, cfg, ccfg, fcfg = _handle("small", True, 2, "winton", 3, fopts=dict(debug_fsd=1, distinguish_mech_fsd=1, welding_type=FS.WELD_NONE))
    tot = inp["conc"] + inp["conc_young"]
    ref, b = R.copy(inp), {"conc_fsd": np.stack([np.zeros_like(tot), tot]), "conc_mech_fsd": np.stack([np.zeros_like(tot), tot])}
    *_, info = _round(fe, f, tri, ref, b, cfg, ccfg, fcfg, True, 3, {}, "the designed state", measure={})
    assert info["thermo_fsd_crash"] and fe.slab_coupled_info()["thermo_fsd_crash"] == 1
    *_, info = _round(fe, f, tri, ref, b, cfg, ccfg, fcfg, True, 3, {}, "closed sums", measure={})
    assert not info["thermo_fsd_crash"] and fe.slab_coupled_info()["thermo_fsd_crash"] == 0
    e = int(np.flatnonzero((ref["conc"] > 0.3) & (ref["conc"] + ref["conc_young"] < 0.9) & (inp["K:del_hi"] > 0) & (inp["K:hi"] > 0.5))[0])
    b["conc_fsd"][1][e] += 1e-3
    *_, info = _round(fe, f, tri, ref, b, cfg, ccfg, fcfg, True, 3, {}, "one open sum", measure={})
    assert info["thermo_fsd_crash"]
    assert fe.slab_coupled_info()["thermo_fsd_crash"] == 1 and fe.slab_coupled_info()["thermo_fsd_crash"] == 0      # reported once
    assert not fe.fsd_get()["weld_crash"]
    fe.close()
