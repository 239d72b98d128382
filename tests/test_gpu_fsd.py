"""The floe-size distribution on the device (include/nxs_dyn.h, nxs_dyn_fsd_*) against the line-faithful restatement tests/fsd_ref.py.

fsd_init, fsd_update and fsd_weld (welding and healing) have no libm call: the device must give the restatement's bits.  The inputs (fsd_ref.update_inputs,
weld_inputs) put at least 5 % of the elements on every branch, and the tests check that on the restatement's own branch record.

fsd_breakup calls tanh / pow / log, the device's on one side and the host libm's on the other.  Everything they do not touch -- cleared bins, untouched
elements, breakup_in_dt, break-up type NONE, the mechanical-bin copy -- is compared bitwise.  The bins, damage, cum_damage and cum_wave_damage of broken elements
are compared within four times the largest absolute difference recorded on the MI355X for the break-up type and the number of bins (BREAKUP_RECORDED; the
test prints the figure per array, DESIGN 6d records them), and in no case more than num_bins * 1e-13 -- a wrong bin index or a missing k <= j term moves a bin
by 1e-3 and more.  UNIFORM_SIZE and ZHANG stay within four units of the last place of 1.  DUMONT is two orders above: its redistributor is a quotient of
DIFFERENCES of powers, pow(up, e) - pow(low, e), whose exponent e = max(-log2(fragility), 1e-6) goes down to 1e-6 where the tanh saturate -- the powers are
then 1 + O(1e-6) and a last-bit difference between two pow implementations is a 1e-10 relative difference of beta.

Meshes: `small` (2.9 k triangles) with and without the young-ice category, and `toy`, whose element count is no multiple of the kernels' block of 256.
"""
import functools

import numpy as np
import pytest

import cases
import fsd_ref as R
from nextsim_amd import _abi

pytestmark = pytest.mark.gpu

BINS = (1, 2, 12, _abi.NXS_FSD_MAX_BINS)
# largest |device - restatement| recorded on the MI355X (ROCm 7.2 device libm against glibc) over the arrays and the three damage types of
# test_breakup_against_the_restatement, per (break-up type, number of bins)
BREAKUP_RECORDED = {(R.UNIFORM_SIZE, 1): 7.22e-16, (R.UNIFORM_SIZE, 2): 9.03e-16, (R.UNIFORM_SIZE, 12): 2.23e-16, (R.UNIFORM_SIZE, 16): 2.23e-16,
                    (R.ZHANG, 1): 7.22e-16, (R.ZHANG, 2): 8.89e-16, (R.ZHANG, 12): 2.23e-16, (R.ZHANG, 16): 2.23e-16,
                    (R.DUMONT, 1): 1.12e-16, (R.DUMONT, 2): 8.50e-15, (R.DUMONT, 12): 1.45e-14, (R.DUMONT, 16): 2.71e-14}


def _bound(breakup_type, n):
    b = 4. * BREAKUP_RECORDED[(breakup_type, n)]
    assert b <= n * 1e-13
    return b


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@functools.lru_cache(maxsize=None)
def _case(kind, young):
    return cases.make_case(kind, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE if young else _abi.NXS_ICECAT_CLASSIC)


def _handle(kind, young, st, cfg, lm_f=None):
    """A handle on mesh `kind` whose state is the case's with the members of `st` in their place, the bins attached and the FSD configured."""
    from nextsim_amd import dynamics
    if lm_f is None:
        gm, p, g, lms, fields = _case(kind, young)
        lm, f = lms[0], fields[0]
    else:
        p, lm, f = lm_f
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    f = dict(f)
    for k in ("conc", "conc_young", "thick", "h_young", "damage", "time_relaxation_damage"):
        if k in st:
            f[k] = np.ascontiguousarray(st[k])
    fe.put_state(f); fe.set_forcing(f)
    fe.put_coupled(cum_damage=st.get("cum_damage"), conc_fsd=st["conc_fsd"])
    fe.fsd_put(conc_mech_fsd=st.get("conc_mech_fsd"), cum_wave_damage=st.get("cum_wave_damage"))
    fe.fsd_configure(cfg["tables"], **R.library_options(cfg))
    return fe


def _num_elements(kind):
    return _case(kind, True)[3][0].num_elements


def test_the_second_mesh_is_no_multiple_of_the_block():
    assert _num_elements("toy") % 256 != 0 and _num_elements("toy") > 256 and _num_elements("small") > 2 * 256


MESHES = [("small", True), ("small", False), ("toy", True)]


@pytest.mark.parametrize("n", BINS)
@pytest.mark.parametrize("kind,young", MESHES)
def test_init_and_update_are_the_restatements_bits(kind, young, n):
    Ne = _num_elements(kind)
    cfg = R.default_config(n, R.standard_tables(n), young, distinguish_mech_fsd=1)
    st = R.update_inputs(n, Ne, young)
    ref = R.copy_state(st)
    branch = R.update_fsd(ref, cfg)
    for b in R.UPDATE_BRANCHES:
        assert (branch == b).mean() >= 0.05, (b, (branch == b).mean())
    ctot = st["conc"] + st["conc_young"] if young else st["conc"]
    assert ((ctot >= 1.) & (st["conc_fsd"].sum(0) == 0.)).sum() >= 1          # the division by a zero ctot2 is among the inputs
    fe = _handle(kind, young, st, cfg)
    fe.fsd_update(); fe.synchronize()
    got = dict(conc_fsd=fe.get_coupled(False, n)["conc_fsd"], **fe.fsd_get(n))
    for k in ("conc_fsd", "conc_mech_fsd"):
        assert _bits(got[k], ref[k]), k
    assert not _bits(got["conc_fsd"], st["conc_fsd"])
    # the same without the mechanical bins: they are left alone
    cfg0 = dict(cfg, distinguish_mech_fsd=0)
    fe.put_coupled(conc_fsd=st["conc_fsd"]); fe.fsd_put(conc_mech_fsd=st["conc_mech_fsd"]); fe.fsd_configure(cfg0["tables"], **R.library_options(cfg0))
    fe.fsd_update(); fe.synchronize()
    assert _bits(fe.get_coupled(False, n)["conc_fsd"], ref["conc_fsd"]) and _bits(fe.fsd_get(n)["conc_mech_fsd"], st["conc_mech_fsd"])
    # initFsd's distribution
    fe.fsd_configure(cfg["tables"], **R.library_options(cfg))
    ini = R.copy_state(st); R.init_fsd(ini, cfg)
    fe.fsd_init(); fe.synchronize()
    assert _bits(fe.get_coupled(False, n)["conc_fsd"], ini["conc_fsd"]) and _bits(fe.fsd_get(n)["conc_mech_fsd"], ini["conc_mech_fsd"])
    assert np.array_equal(ini["conc_fsd"][n - 1], ctot) and (n == 1 or not ini["conc_fsd"][:n - 1].any())
    fe.close()


@functools.lru_cache(maxsize=None)
def _weld_reference(n, Ne, distinguish, ddt=900.):
    cfg = R.default_config(n, R.standard_tables(n), False, distinguish_mech_fsd=distinguish, debug_fsd=1)
    cfg["welding_kappa"] = R.WELD_K / (ddt * cfg["tables"]["area_scaled_up"][n - 1])
    st, freezing, g = R.weld_inputs(n, Ne)
    ref = R.copy_state(st)
    ndt, crash, zeroed = R.weld(ref, cfg, ddt, freezing)
    return cfg, st, freezing, ref, ndt, crash, zeroed


@pytest.mark.parametrize("n", BINS)
@pytest.mark.parametrize("kind,young", [("small", False), ("toy", True)])
def test_weld_is_the_restatements_bits(kind, young, n):
    Ne = _num_elements(kind)
    ddt = 900.
    cfg, st, freezing, ref, ndt, crash, zeroed = _weld_reference(n, Ne, 1)
    cfg = dict(cfg, young=young)                                       # (welding and healing do not read the ice categories)
    for name, mask in (("not freezing", ndt == -1), ("below the gate", ndt == 0), ("ndt_mrg 1", ndt == 1), ("ndt_mrg 2", ndt == 2), ("ndt_mrg >= 5", ndt >= 5)):
        assert mask.mean() >= 0.05, (name, mask.mean())
    assert not crash
    print(f"weld n={n} {kind}: ndt_mrg up to {ndt.max()}; elements with a bin in (-1e-12, 0) zeroed by the reference for these inputs: {zeroed}")
    w = np.minimum(1., ddt / st["time_relaxation_damage"])
    assert (w == 1.).mean() > 0.05 and (w < 1.).mean() > 0.05           # healing on both sides of its cap
    fe = _handle(kind, young, st, cfg)
    fe.fsd_weld(ddt, freezing); fe.synchronize()
    got = dict(conc_fsd=fe.get_coupled(False, n)["conc_fsd"], **fe.fsd_get(n))
    assert _bits(got["conc_fsd"], ref["conc_fsd"]) and _bits(got["conc_mech_fsd"], ref["conc_mech_fsd"])
    assert got["weld_crash"] == 0
    off = freezing == 0
    assert _bits(got["conc_fsd"][:, off], st["conc_fsd"][:, off]) and _bits(got["conc_mech_fsd"][:, off], st["conc_mech_fsd"][:, off])
    if n > 1:
        assert (got["conc_fsd"][:, ndt >= 1] != st["conc_fsd"][:, ndt >= 1]).any(0).all()      # every welded element moved
    assert not _bits(got["conc_mech_fsd"], st["conc_mech_fsd"])
    fe.close()


def test_weld_crash_flag_and_welding_none():
    n, kind = 12, "toy"
    Ne = _num_elements(kind)
    cfg, st, freezing, ref, ndt, crash, zeroed = _weld_reference(n, Ne, 1)
    # a bin above 1 is a crash condition of the sanity check (FE.cpp:4802) under debug_fsd: the flag rises, and the next fsd_get reports it once
    bad = R.copy_state(st)
    i = int(np.flatnonzero(ndt >= 1)[0])
    bad["conc_fsd"][n - 1, i] = 1.5
    rb = R.copy_state(bad)
    _, c_ref, _ = R.weld(rb, cfg, 900., freezing)
    assert c_ref
    fe = _handle(kind, True, bad, cfg)
    fe.fsd_weld(900., freezing); fe.synchronize()
    assert fe.fsd_get()["weld_crash"] == 1 and fe.fsd_get()["weld_crash"] == 0
    assert _bits(fe.get_coupled(False, n)["conc_fsd"], rb["conc_fsd"])
    # welding NONE: the healing alone
    cfg0 = dict(cfg, welding_type=R.WELD_NONE)
    r0 = R.copy_state(st); R.weld(r0, cfg0, 900., freezing)
    fe.put_coupled(conc_fsd=st["conc_fsd"]); fe.fsd_put(conc_mech_fsd=st["conc_mech_fsd"]); fe.fsd_configure(cfg0["tables"], **R.library_options(cfg0))
    fe.fsd_weld(900., freezing); fe.synchronize()
    assert _bits(fe.get_coupled(False, n)["conc_fsd"], st["conc_fsd"]) and _bits(fe.fsd_get(n)["conc_mech_fsd"], r0["conc_mech_fsd"])
    fe.close()


# ---- break-up ---------------------------------------------------------------------------------------------------------------------------------------------

def _breakup(kind, young, n, mutate=None, **over):
    Ne = _num_elements(kind)
    cfg = R.default_config(n, R.standard_tables(n), young, **over)
    st, wlbk, g = R.breakup_inputs(n, Ne, young, cfg["tables"])
    if mutate:
        mutate(st, wlbk)
    ref = R.copy_state(st)
    flags = R.redistribute_fsd(ref, cfg, wlbk)
    fe = _handle(kind, young, st, cfg)
    got_flags = fe.fsd_breakup(wlbk)
    got = dict(conc_fsd=fe.get_coupled(True, n)["conc_fsd"], cum_damage=fe.get_coupled(True, 0)["cum_damage"], damage=fe.get_state()["damage"],
               **fe.fsd_get(n if "conc_mech_fsd" in st else 0, True))
    fe.close()
    return cfg, st, wlbk, ref, flags, got, got_flags


KEYS = ("conc_fsd", "conc_mech_fsd", "damage", "cum_damage", "cum_wave_damage")


@pytest.mark.parametrize("n", BINS)
@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("damage_type", [0, 1, 2])
@pytest.mark.parametrize("breakup_type", [R.UNIFORM_SIZE, R.ZHANG, R.DUMONT])
def test_breakup_against_the_restatement(breakup_type, damage_type, young, n):
    kind = "small" if n != 2 else "toy"
    cfg, st, wlbk, ref, (in_dt, crash, what), got, got_flags = _breakup(kind, young, n, breakup_type=breakup_type, fsd_damage_type=damage_type,
                                                                        distinguish_mech_fsd=1, debug_fsd=1)
    assert got_flags == (in_dt, crash) == (True, False)
    for w in (0, 1, 2):
        assert (what == w).mean() >= 0.05
    # the inputs: both sides of each tanh's zero, its saturated range, M_thick at exactly 0 and above
    c, lam = cfg["tables"]["bin_centres"], wlbk[what == 2]
    arg = (c[:, None] - cfg["breakup_coef1"] * lam) / (cfg["breakup_coef2"] * lam)
    assert (arg < 0).any() and (arg > 0).any() and (np.abs(arg) > 19.).any() and (np.abs(arg) < 1.).any()
    assert ((st["thick"] == 0.) & (what == 2)).any() and ((st["thick"] > 0.) & (what == 2)).any()
    assert (wlbk[what == 1] >= 499.).all() and (lam < 499.).all()
    # untouched by the libm: bitwise
    for k in KEYS:
        assert _bits(got[k][..., what == 1], st[k][..., what == 1]), k                      # ice, no waves: nothing is written
        assert _bits(got[k][..., what == 0], ref[k][..., what == 0]), k                      # no ice: the bins cleared, the rest left
    assert not got["conc_fsd"][:, what == 0].any() and not got["conc_mech_fsd"][:, what == 0].any()
    assert _bits(got["conc_mech_fsd"][:, what == 2], got["conc_fsd"][:, what == 2])              # "mech FSD and real FSD are the same after break-up"
    nothick = (what == 2) & (st["thick"] == 0.)
    for k in ("damage", "cum_damage", "cum_wave_damage"):
        assert _bits(got[k][nothick], st[k][nothick]), k                                  # damage is written only where M_thick > 0
    # the broken elements
    worst = {k: float(np.abs(got[k] - ref[k]).max()) for k in KEYS}
    print(f"breakup type {breakup_type} damage {damage_type} young {young} n={n}: max |device - restatement| " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    BREAKUP_BOUND = _bound(breakup_type, n)
    for k in KEYS:
        assert worst[k] <= BREAKUP_BOUND, (k, worst[k])
    # ... and a kernel that does nothing is 1e3 bounds away (the bins from two bins on; at one bin the only bin gets back what it lost: the damage shows it)
    if n > 1:
        assert np.abs(st["conc_fsd"] - ref["conc_fsd"]).max() > 1e3 * BREAKUP_BOUND
    if damage_type:
        assert np.abs(st["damage"] - ref["damage"]).max() > 1e3 * BREAKUP_BOUND and np.abs(st["cum_wave_damage"] - ref["cum_wave_damage"]).max() > 1e3 * BREAKUP_BOUND
    else:
        assert _bits(got["damage"], st["damage"])
    if not young and n > 1:
        # neither breakup_cell_average_thickness nor the young-ice category: the thickness is 0 before the max, so d_flex comes from breakup_thick_min alone
        # (FE.cpp:4304-4310).  A kernel that took M_thick there lands where the restatement with breakup_cell_average_thickness lands: far from this result
        alt = R.copy_state(st)
        R.redistribute_fsd(alt, dict(cfg, breakup_cell_average_thickness=1), wlbk)
        assert np.abs(alt["conc_fsd"] - ref["conc_fsd"]).max() > 1e3 * BREAKUP_BOUND and np.abs(alt["conc_fsd"] - got["conc_fsd"]).max() > 1e3 * BREAKUP_BOUND


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("breakup_type", [R.UNIFORM_SIZE, R.ZHANG, R.DUMONT])
def test_breakup_with_the_cell_average_thickness(breakup_type, young):
    """breakup_cell_average_thickness: sea_ice_thickness = M_thick, with and without the young-ice category (FE.cpp:4305-4306)."""
    n = 12
    cfg, st, wlbk, ref, (in_dt, crash, what), got, got_flags = _breakup("small", young, n, breakup_type=breakup_type, fsd_damage_type=2, distinguish_mech_fsd=1,
                                                                        debug_fsd=1, breakup_cell_average_thickness=1)
    assert got_flags == (in_dt, crash) == (True, False)
    worst = {k: float(np.abs(got[k] - ref[k]).max()) for k in KEYS}
    print(f"breakup type {breakup_type} cell average young {young} n={n}: max |device - restatement| " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    bound = _bound(breakup_type, n)
    for k in KEYS:
        assert worst[k] <= bound, (k, worst[k])
    # ... and it is the cell average that was used: the restatement without the option (thick + h_young over ctot, or 0) ends elsewhere
    alt = R.copy_state(st)
    R.redistribute_fsd(alt, dict(cfg, breakup_cell_average_thickness=0), wlbk)
    assert np.abs(alt["conc_fsd"] - got["conc_fsd"]).max() > 1e3 * bound


@pytest.mark.parametrize("damage_type", [1, 2])
@pytest.mark.parametrize("breakup_type", [R.UNIFORM_SIZE, R.ZHANG])
def test_breakup_damage_reads_the_mechanical_bins_where_they_are_not_distinguished(breakup_type, damage_type):
    """distinguish_mech_fsd = 0 with fsd_damage_type 1 / 2: tot_broken_area is summed over the rows of M_conc_mech_fsd as they are attached -- not the
    real bins, which nothing copies from them here (FE.cpp:4458-4461)."""
    n = 12
    cfg, st, wlbk, ref, (in_dt, crash, what), got, got_flags = _breakup("small", True, n, breakup_type=breakup_type, fsd_damage_type=damage_type,
                                                                        distinguish_mech_fsd=0, debug_fsd=1)
    assert got_flags == (in_dt, crash) == (True, False)
    assert _bits(got["conc_mech_fsd"][:, what != 0], st["conc_mech_fsd"][:, what != 0])            # read, not written (cleared where there is no ice)
    worst = {k: float(np.abs(got[k] - ref[k]).max()) for k in KEYS}
    print(f"breakup type {breakup_type} damage {damage_type} not distinguished n={n}: max |device - restatement| " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    bound = _bound(breakup_type, n)
    for k in KEYS:
        assert worst[k] <= bound, (k, worst[k])
    # the damage from the real bins instead (the state with the mechanical rows replaced by them) is 1e3 bounds away
    alt = R.copy_state(st); alt["conc_mech_fsd"] = alt["conc_fsd"].copy()
    R.redistribute_fsd(alt, cfg, wlbk)
    assert np.abs(alt["damage"] - got["damage"]).max() > 1e3 * bound


def test_breakup_crash_flag_rises():
    """The mini check of FE.cpp:4426-4436: under debug_fsd a sum of the bins more than 2e-7 away from the total concentration raises `crash` -- here the
    mechanical bins of three broken elements sum to ctot (1 +- 1e-3), and break-up resets the real bins to them."""
    n = 12

    def spoil(st, wlbk):
        ctot = st["conc"] + st["conc_young"]
        i = np.flatnonzero((ctot > 0.) & (wlbk < 499.))[:3]              # broken elements
        assert i.size == 3
        st["conc_mech_fsd"][:, i] *= np.array([1.001, 0.999, 1.001])
    for debug, want in ((1, True), (0, False)):
        cfg, st, wlbk, ref, (in_dt, crash, what), got, got_flags = _breakup("toy", True, n, mutate=spoil, breakup_type=R.ZHANG, distinguish_mech_fsd=1, debug_fsd=debug)
        assert crash == want and got_flags == (True, want)


@pytest.mark.parametrize("kind,young", MESHES)
def test_breakup_type_none_and_the_mechanical_copy_are_bitwise(kind, young):
    n = 12
    cfg, st, wlbk, ref, (in_dt, crash, what), got, got_flags = _breakup(kind, young, n, breakup_type=R.NONE, fsd_damage_type=2, distinguish_mech_fsd=1, debug_fsd=1)
    assert got_flags == (in_dt, crash)
    for k in KEYS:
        assert _bits(got[k], ref[k]), k          # (type NONE: P = 1 - exp(-cpl / tau) from the host, no device libm call reaches a result)
    b = what == 2
    assert _bits(got["conc_fsd"][:, b], st["conc_mech_fsd"][:, b]) and not _bits(st["conc_fsd"][:, b], st["conc_mech_fsd"][:, b])   # the real bins reset to the mechanical ones
    assert crash == bool((np.abs((st["conc"] + st["conc_young"] * young)[b] - st["conc_mech_fsd"][:, b].sum(0)) > 2e-7).any())


def test_breakup_without_waves_anywhere_and_device_wlbk():
    n, kind = 2, "toy"
    Ne = _num_elements(kind)
    cfg = R.default_config(n, R.standard_tables(n), True, breakup_type=R.ZHANG)
    st, wlbk, g = R.breakup_inputs(n, Ne, True, cfg["tables"])
    st.pop("conc_mech_fsd")                                                    # (not distinguished, damage type 0: the mechanical bins are not needed)
    fe = _handle(kind, True, st, cfg)
    assert fe.fsd_breakup(np.full(Ne, 1000.)) == (False, False)               # M_breakup_in_dt stays false
    ref = R.copy_state(st)
    R.redistribute_fsd(ref, cfg, np.full(Ne, 1000.))
    assert _bits(fe.get_coupled(False, n)["conc_fsd"], ref["conc_fsd"])
    # M_wlbk as a device pointer, no flags wanted: the call returns without waiting
    from nextsim_amd import dynamics
    d = dynamics.device_put(wlbk)
    assert fe.fsd_breakup(d, want_flags=False) is None
    fe.synchronize()
    dynamics.device_free(d)
    ref2 = R.copy_state(ref); R.redistribute_fsd(ref2, cfg, wlbk)
    assert np.abs(fe.get_coupled(False, n)["conc_fsd"] - ref2["conc_fsd"]).max() <= _bound(R.ZHANG, n)
    # damage types 1 / 2 read the mechanical bins: refused without them
    from nextsim_amd.dynamics import NxsError
    cfg2 = dict(cfg, fsd_damage_type=2)
    fe.fsd_configure(cfg2["tables"], **R.library_options(cfg2))
    with pytest.raises(NxsError) as e:
        fe.fsd_breakup(wlbk)
    assert e.value.code == -4
    fe.close()


def test_configure_refusals_on_a_handle():
    from nextsim_amd.dynamics import NxsError
    n, kind = 12, "toy"
    Ne = _num_elements(kind)
    cfg = R.default_config(n, R.standard_tables(n), True)
    st = R.update_inputs(n, Ne, True)
    fe = _handle(kind, True, st, cfg)
    for bad in (dict(tables=R.standard_tables(2)), dict(breakup_type=7), dict(welding_type=2), dict(fsd_damage_type=3), dict(breakup_prob_type=1)):
        c = dict(cfg, **bad)
        with pytest.raises(NxsError) as e:
            fe.fsd_configure(c["tables"], **R.library_options(c))
        assert e.value.code == -1, bad
    t = {k: v.copy() for k, v in cfg["tables"].items()}
    t["alpha_merge"][5, 2] = -999
    with pytest.raises(NxsError) as e:
        fe.fsd_configure(t, **R.library_options(cfg))
    assert e.value.code == -1 and "alpha_merge[5][2]" in str(e.value)
    fe.fsd_update(); fe.synchronize()                                          # a refused configuration leaves the previous one
    fe.put_coupled(conc_fsd=st["conc_fsd"][:3])                                # another number of bins attached: the kernels refuse
    with pytest.raises(NxsError) as e:
        fe.fsd_update()
    assert e.value.code == -4
    fe.close()


# ---- residency --------------------------------------------------------------------------------------------------------------------------------------------

def _sequence(through_host, breakup=True, options=None, cum=True):
    n, kind = 12, "small"
    gm, p, g, lms, fields = _case(kind, True)
    lm, f = lms[0], fields[0]
    Ne = lm.num_elements
    cfg = R.default_config(n, R.standard_tables(n), True, breakup_type=R.ZHANG, fsd_damage_type=2, distinguish_mech_fsd=1)
    rng = np.random.default_rng(5)
    ctot = f["conc"] + f["conc_young"]
    st = dict(conc_fsd=np.ascontiguousarray(R._weights(rng, n, Ne, 4.) * ctot), conc_mech_fsd=np.ascontiguousarray(R._weights(rng, n, Ne, 4.) * ctot),
              cum_wave_damage=np.zeros(Ne))
    if cum:
        st["cum_damage"] = np.zeros(Ne)
    wlbk = np.where(rng.random(Ne) < 0.5, rng.uniform(20., 300., Ne), 1000.)
    fe = _handle(kind, True, st, cfg)
    for k, v in (options or {}).items():
        fe.set_option(k, v)
    keep = {k: f[k] for k in _abi.STATE_INPUT}

    def host():
        if through_host:
            fe.synchronize()
            s, c, m = fe.get_state(), fe.get_coupled(cum, n), fe.fsd_get(n, True)
            fe.put_state(dict(s, **keep)); fe.put_coupled(cum_damage=c.get("cum_damage"), conc_fsd=c["conc_fsd"])
            fe.fsd_put(conc_mech_fsd=m["conc_mech_fsd"], cum_wave_damage=m["cum_wave_damage"])
    fe.step(); host()
    fe.fsd_update(); host()
    if breakup:
        fe.fsd_breakup(wlbk, want_flags=False); host()
    fe.step(); fe.synchronize()
    out = dict(fe.get_state(), **fe.get_coupled(cum, n)); out.update(fe.fsd_get(n, True))
    out["kernel"] = fe.traffic_model()["substep_kernel_name"]
    fe.close()
    return out


# every family of the sub-step loop leaves M_damage either in its array or in the records of k_pack_state, and the handle says which (sig_loc): the one-kernel-
# per-loop family, the patch kernels, and -- with no cum_damage attached, which they do not carry -- the resident loop and the data-flow launch
SEQUENCES = [(None, True, "k_substep_fused"), ({"fused": 0}, True, "k_sigma + k_solve_move"), ({"fused": 2, "substeps_per_launch": 2, "pair_regs": 1}, True, "k_substep_pair"),
             ({"fused": 4}, False, "k_substep_resident"), ({"fused": 2, "substeps_per_launch": 2, "pair_regs": 1, "pair_flow": 1}, False, "k_substep_flow"),
             ({"fused": 3}, False, "k_substep_multi")]


@pytest.mark.parametrize("options,cum,kernel", SEQUENCES)
def test_resident_sequence_equals_the_sequence_through_the_host(options, cum, kernel):
    a, b = _sequence(False, True, options, cum), _sequence(True, True, options, cum)
    assert a["kernel"] == b["kernel"] == kernel
    for k in a:
        if k not in ("weld_crash", "kernel"):
            assert _bits(a[k], b[k]), k
    # the damage fsd_breakup wrote is what the next step's sub-step loop read: without the break-up the second step ends elsewhere
    c = _sequence(False, False, options, cum)
    assert not _bits(a["damage"], c["damage"]) and not _bits(a["sigma0"], c["sigma0"]) and not _bits(a["VT"], c["VT"])
    assert (a["cum_wave_damage"] > 0).any() and not c["cum_wave_damage"].any()


# ---- regrid -----------------------------------------------------------------------------------------------------------------------------------------------

def test_regrid_carries_the_mechanical_bins_and_cum_wave_damage():
    import test_gpu_regrid_handle as T
    from nextsim_amd import dynamics
    xo, yo, to, xn, yn, tn, prev, ng = T._pair("rect")
    gm, gm2 = T._global_mesh(xo, yo, to, ng), T._global_mesh(xn, yn, tn, ng)
    p, lm, f = T._fields(gm, True)
    _, lm2, f2 = T._fields(gm2, True)
    Ne, Nn, n = lm.num_elements, lm.num_nodes, 3
    rng = np.random.default_rng(12)
    ctot = f["conc"] + f["conc_young"]
    fsd, mech = np.ascontiguousarray(R._weights(rng, n, Ne) * ctot), np.ascontiguousarray(R._weights(rng, n, Ne) * ctot)
    cum, cumw = rng.uniform(0., 0.2, Ne), rng.uniform(0., 0.1, Ne)
    inputs = {k: f2[k] for k in dynamics.REGRID_INPUTS}
    res = []
    for attached in (True, False):
        fe = dynamics.FiniteElementDynamics(p)
        fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
        fe.put_coupled(cum_damage=cum, conc_fsd=fsd)
        extras = []
        if attached:
            fe.fsd_put(conc_mech_fsd=mech, cum_wave_damage=cumw)
        else:      # the same arrays as the caller's own variables of kind `none` with the same bounds
            extras = [dict(old=mech[b].copy(), transformation="none", min=0., max=1.) for b in range(n)] + [dict(old=cumw.copy(), transformation="none", min=0.)]
        fe.step(); fe.synchronize()
        st = fe.get_state()
        info = fe.regrid(lm2, prev, ng, inputs, extras, moved=(lm.coord_x + st["UM"][:Nn], lm.coord_y + st["UM"][Nn:]))
        out = dict(fe.get_coupled(True, n), info=info)
        if attached:
            out.update(fe.fsd_get(n, True))
        else:
            out.update(conc_mech_fsd=np.stack([x["new"] for x in extras[:n]]), cum_wave_damage=extras[n]["new"])
        res.append(out)
        fe.close()
    a, b = res
    assert a["info"]["nb_var_element"] == b["info"]["nb_var_element"] == 13 + 1 + n + n + 1
    for k in ("conc_fsd", "cum_damage", "conc_mech_fsd", "cum_wave_damage"):
        assert a[k].shape[-1] == lm2.num_elements and _bits(a[k], b[k]), k
    assert a["conc_mech_fsd"].min() >= 0. and a["conc_mech_fsd"].max() <= 1. and a["cum_wave_damage"].min() >= 0. and a["cum_wave_damage"].max() > 0.


# ---- a partitioned handle ---------------------------------------------------------------------------------------------------------------------------------

def test_two_ranks_sharing_the_device_give_the_single_rank_bits():
    n, kind, ddt = 12, "small", 900.
    gm, p, g, lms1, fields1 = _case(kind, True)
    _, p2, _, lms, fields = cases.make_case(kind, nparts=2)
    Ne = gm.num_elements
    assert np.array_equal(lms1[0].elem_gid, np.arange(Ne)) and any(lm.num_elements > lm.local_nelements for lm in lms)      # ghost elements among them
    cfg = R.default_config(n, R.standard_tables(n), True, breakup_type=R.DUMONT, fsd_damage_type=2, distinguish_mech_fsd=1)
    cfg["welding_kappa"] = R.WELD_K / (ddt * cfg["tables"]["area_scaled_up"][n - 1])
    st, wlbk, _ = R.breakup_inputs(n, Ne, True, cfg["tables"])
    w, freezing, _ = R.weld_inputs(n, Ne)
    st["time_relaxation_damage"] = w["time_relaxation_damage"]

    def run(lm_f, idx):
        loc = {k: np.ascontiguousarray(v[..., idx]) for k, v in st.items()}
        fe = _handle(kind, True, loc, cfg, lm_f)
        fe.fsd_update(); fe.fsd_breakup(wlbk[idx]); fe.fsd_weld(ddt, freezing[idx]); fe.synchronize()
        out = dict(fe.get_coupled(True, n), damage=fe.get_state()["damage"]); out.update(fe.fsd_get(n, True))
        fe.fsd_init(); fe.synchronize()
        out["init"] = fe.get_coupled(False, n)["conc_fsd"]
        fe.close()
        return out
    one = run((p, lms1[0], fields1[0]), np.arange(Ne))
    assert one["weld_crash"] == 0
    for lm, f in zip(lms, fields):
        got = run((p2, lm, f), lm.elem_gid)
        for k in ("conc_fsd", "conc_mech_fsd", "cum_damage", "cum_wave_damage", "damage", "init"):
            assert _bits(got[k], one[k][..., lm.elem_gid]), (lm.rank, k)         # owned and ghost elements alike
