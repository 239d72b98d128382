"""The coupled build's terms on the device (include/nxs_dyn.h: nxs_dyn_set_wave_stress, nxs_dyn_put_coupled, nxs_dyn_get_coupled), single rank.

References: the wave stress against the oracle's phase functions composed as in tests/test_coupled_abi.py (the reference's left-associated sum, so the
tolerances are those of tests/test_gpu_parity.py for the same comparison: 1e-13 after a sub-step, 1e-10 after a step); the cumulated damage and the
floe-size bins against exact floating-point identities.  The bound of the damage identity over S sub-steps is derived, not measured: each of the S additions
rounds once in damage (<= 2^-53, damage <= 1) and once in cum_damage (<= 2^-53 max(1, cum)), hence S 2^-52 max(1, cum_end).

Several ranks: tests/test_gpu_coupled_multirank.py.
"""
import numpy as np
import pytest

import cases
from test_coupled_abi import composed_explicit_solve, smooth_wave_stress

pytestmark = pytest.mark.gpu

STATE_KEYS = ("VT", "UM", "UT", "sigma0", "sigma1", "sigma2", "damage", "conc", "thick", "snow_thick",
              "ridge_ratio", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi")
PAIR = {"fused": 2, "substeps_per_launch": 2, "pair_regs": 1}
# every setting of the sub-step family: (options, the kernel that runs with nothing attached, the kernel that runs with cum_damage attached)
FAMILIES = [({"fused": 0}, "k_sigma + k_solve_move", "k_sigma + k_solve_move"),
            ({"fused": 1}, "k_substep_fused", "k_substep_fused"),
            ({"fused": 3}, "k_substep_multi", "k_substep_fused"),
            (PAIR, "k_substep_pair", "k_substep_pair"),
            (dict(PAIR, pair_move=0), "k_substep_pair", "k_substep_pair"),
            (dict(PAIR, pair_flow=1), "k_substep_flow", "k_substep_pair"),
            ({"fused": 2, "substeps_per_launch": 4}, "k_substep_multi", "k_substep_fused"),
            ({"fused": 2, "substeps_per_launch": 3}, "k_substep_multi", "k_substep_fused"),
            ({"fused": 4}, "k_substep_resident", "k_substep_fused")]


def _handle(kind="small", options=None, **over):
    from nextsim_amd import dynamics
    gm, p, g, lms, fields = cases.make_case(kind, **over)
    lm, f = lms[0], fields[0]
    fe = dynamics.FiniteElementDynamics(p)
    for k, v in (options or {}).items():
        fe.set_option(k, v)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    return fe, lm, p, f


def _bits_equal(a, b, keys, what):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), f"{what}: {k} differs"


# ---- 1. wave stress against the oracle -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dyn", ["bbm", "evp", "mevp"])
@pytest.mark.parametrize("substeps,tol", [(1, 1e-13), (120, 1e-10)])
def test_wave_stress_against_the_composed_oracle(dyn, substeps, tol):
    from oracle import pyoracle as O
    over = dict(dynamics_type=dyn) if substeps == 120 else dict(dynamics_type=dyn, substeps=1, dtime_step=200. / 120.)
    fe, lm, p, f = _handle("small", **over)
    tau = smooth_wave_stress(lm)
    assert 0.05 <= np.abs(tau).max() <= 0.2
    fe.set_wave_stress(tau)
    fe.step(); fe.synchronize()
    got = fe.get_state()
    ref = O.OracleRank(lm, p, f)
    composed_explicit_solve([ref], [tau]); ref.update()
    plain = O.OracleRank(lm, p, f)
    plain.step()
    # one sub-step: every key relative to its maximum, except the damage -- tiny after one sub-step, so its round-off is judged as an absolute 1e-15, exactly as
    # tests/test_gpu_parity.py::test_one_substep judges it
    keys = STATE_KEYS if substeps == 120 else tuple(k for k in STATE_KEYS if k != "damage")
    if substeps == 1:
        print(f"wave stress {dyn} S=1: damage abs err {np.abs(got['damage'] - ref.arr['damage']).max():.3e}")
        assert np.abs(got["damage"] - ref.arr["damage"]).max() <= 1e-15
    for k in keys:
        err = cases.rel_err(got[k], ref.arr[k])
        print(f"wave stress {dyn} S={substeps}: {k} rel err {err:.3e}")
    for k in keys:
        assert cases.rel_err(got[k], ref.arr[k]) <= tol, k
    # the run with the term differs from the run without by far more than the tolerance: the test cannot pass with the term missing
    assert cases.rel_err(ref.arr["VT"], plain.arr["VT"]) > 1e3 * tol
    assert cases.rel_err(got["VT"], plain.arr["VT"]) > 1e3 * tol
    # the diagnostic stays drag * wind
    np.testing.assert_allclose(fe.get_diag()["D_tau_a"], plain.work_array("D_tau_a", 2 * lm.num_nodes), rtol=1e-15, atol=1e-18)
    fe.close()


# ---- 2. wave stress, device only, bitwise ------------------------------------------------------------------------------------------------------------------

def test_wave_stress_gives_the_same_bits_on_every_kernel_family():
    base = None
    for options, _, _ in FAMILIES + [({"fused": 1, "work_arrays": 1}, "", ""), ({"fused": 1, "prep_fused": 1}, "", ""), (dict(PAIR, prep_fused=1), "", "")]:
        fe, lm, p, f = _handle("small", options)
        fe.set_wave_stress(smooth_wave_stress(lm))
        fe.step(); fe.step(); fe.synchronize()
        got = fe.get_state()
        if base is None:
            base = got
        _bits_equal(got, base, STATE_KEYS, str(options))
        fe.close()


@pytest.mark.parametrize("options", [{"fused": 0}, {"fused": 1}, PAIR])
def test_detached_and_zero_wave_stress_equal_a_handle_that_never_had_it(options):
    never, lm, p, f = _handle("small", options)
    never.step(); never.synchronize()
    want = never.get_state()
    a, _, _, _ = _handle("small", options)
    a.set_wave_stress(smooth_wave_stress(lm)); a.step(); a.synchronize()
    assert cases.rel_err(a.get_state()["VT"], want["VT"]) > 1e-7
    a.put_state(f); a.set_wave_stress(None); a.step(); a.synchronize()
    _bits_equal(a.get_state(), want, STATE_KEYS, "attach, detach, step")
    z, _, _, _ = _handle("small", options)
    z.set_wave_stress(np.zeros(2 * lm.num_nodes)); z.step(); z.synchronize()
    tau_a = z.get_diag()["D_tau_a"]
    assert not np.any((tau_a == 0.) & np.signbit(tau_a))      # (x + 0. == x bit for bit unless x is -0.)
    _bits_equal(z.get_state(), want, STATE_KEYS, "zeros attached")
    for h in (never, a, z):
        h.close()


# ---- 3. - 5. cumulated damage ---------------------------------------------------------------------------------------------------------------------------------

def _no_healing(f):
    f = dict(f)
    f["time_relaxation_damage"] = np.full_like(f["time_relaxation_damage"], 1e300)
    return f


@pytest.mark.parametrize("options", [{"fused": 0}, {"fused": 1}])
def test_cumulated_damage_of_one_sub_step_is_the_damage_itself(options):
    # (the stresses of an evolved state -- one default step -- so that the first sub-step from zero damage does reach the damage criterion)
    ev, lm, p, f = _handle("small")
    ev.step(); ev.synchronize()
    f = _no_healing(dict(f, **ev.get_state())); f["damage"] = np.zeros(lm.num_elements)
    ev.close()
    fe, lm, p, _ = _handle("small", options, substeps=1, dtime_step=200. / 120.)
    fe.put_state(f)
    fe.put_coupled(cum_damage=np.zeros(lm.num_elements))
    fe.explicitSolve(); fe.synchronize()
    dam, cum = fe.get_state()["damage"], fe.get_coupled()["cum_damage"]
    print(f"one sub-step {options}: {(dam > 0).sum()} of {dam.size} elements damaged")
    assert np.array_equal(dam.view(np.uint64), cum.view(np.uint64))
    assert (dam > 0).sum() > 10
    fe.close()


@pytest.mark.parametrize("options", [{"fused": 0}, {"fused": 1}, PAIR, dict(PAIR, pair_move=0)])
def test_cumulated_damage_over_a_step_follows_the_damage(options):
    fe, lm, p, f = _handle("small", options)
    S = p.substeps
    assert S == 120
    rng = np.random.default_rng(5)
    cum0 = rng.uniform(0.5, 3., lm.num_elements)
    f = _no_healing(f)
    fe.put_state(f); fe.put_coupled(cum_damage=cum0)
    fe.explicitSolve(); fe.synchronize()
    st, cum1 = fe.get_state(), fe.get_coupled()["cum_damage"]
    keep = (f["conc"] > 0.1) & (st["conc"] > 0.1)
    lhs = np.abs((cum1 - cum0) - (st["damage"] - f["damage"]))[keep]
    bound = (S * 2.**-52 * np.maximum(1., cum1))[keep]
    print(f"cum_damage {options}: worst |d cum - d damage| / bound = {(lhs / bound).max():.3f}; elements damaged {(cum1 != cum0).sum()} of {lm.num_elements}")
    assert (cum1 != cum0).sum() > 10
    assert np.all(lhs <= bound)
    fe.close()


@pytest.mark.parametrize("options", [{"fused": 1}, PAIR, dict(PAIR, pair_move=0)])
def test_cumulated_damage_with_healing_against_the_oracles_branch_trace(options):
    from oracle import pyoracle as O
    fe, lm, p, f = _handle("small", options)
    cum0 = np.random.default_rng(6).uniform(0.5, 3., lm.num_elements)
    fe.put_coupled(cum_damage=cum0)
    fe.step(); fe.synchronize()
    cum1, got = fe.get_coupled()["cum_damage"], fe.get_state()
    ref = O.OracleRank(lm, p, f)
    ref.enable_branch_trace()
    ref.step()
    tr = ref.branch_trace()
    never = tr["damage_substeps"] == 0
    sure = (tr["damage_substeps"] > 0) & ((tr["flags"] & 1) == 0)
    print(f"branch trace: {never.sum()} elements never damaged, {sure.sum()} surely damaged, of {lm.num_elements}")
    assert sure.sum() > 10
    assert np.array_equal(cum1[never].view(np.uint64), cum0[never].view(np.uint64))
    assert np.all(cum1[sure] > cum0[sure])
    assert cases.rel_err(got["damage"], ref.arr["damage"]) <= 1e-10
    fe.close()


def test_cumulated_damage_gives_the_same_bits_on_every_kernel_family():
    base, fused_model = None, None
    for options, plain_kernel, cum_kernel in FAMILIES:
        fe, lm, p, f = _handle("small", options)
        fe.step(); fe.synchronize()
        assert fe.traffic_model()["substep_kernel_name"] == plain_kernel, (options, fe.traffic_model()["substep_kernel_name"])
        fe.put_state(f)
        fe.put_coupled(cum_damage=np.random.default_rng(7).uniform(0.5, 3., lm.num_elements))
        fe.step(); fe.step(); fe.synchronize()
        assert fe.traffic_model()["substep_kernel_name"] == cum_kernel, (options, fe.traffic_model()["substep_kernel_name"])
        got = fe.get_state(); got["cum_damage"] = fe.get_coupled()["cum_damage"]
        # the traffic model prices the plan that RAN: every element has one writer on a single rank, whatever the options wanted ...
        t = fe.traffic_model()
        assert t["substep_unique_bytes"] <= t["substep_scheme_bytes"], (options, t)
        fe.put_coupled(); fe.put_state(f); fe.step(); fe.synchronize()
        t_off = fe.traffic_model()
        if t_off["substep_kernel_name"] == cum_kernel:       # (no fall-back: the same plan with and without)
            assert t["substep_scheme_bytes"] - t_off["substep_scheme_bytes"] == 16. * lm.num_elements == t["substep_unique_bytes"] - t_off["substep_unique_bytes"], (options, t, t_off)
        # ... and a plan that fell back to one patch kernel per sub-step on the default cut is priced like that kernel asked for by name
        if options == {"fused": 1}:
            fused_model = t
        if cum_kernel == "k_substep_fused" and options.get("fused") != 4:
            assert (t["substep_scheme_bytes"], t["substep_unique_bytes"]) == (fused_model["substep_scheme_bytes"], fused_model["substep_unique_bytes"]), (options, t, fused_model)
        if base is None:
            base = got
        _bits_equal(got, base, ("cum_damage", "damage", "sigma0", "sigma1", "sigma2", "VT", "UM"), str(options))
        fe.close()


@pytest.mark.parametrize("dyn", ["evp", "mevp"])
def test_evp_leaves_the_cumulated_damage_alone(dyn):
    fe, lm, p, f = _handle("small", dynamics_type=dyn)
    cum0 = np.random.default_rng(8).uniform(0.5, 3., lm.num_elements)
    fe.put_coupled(cum_damage=cum0)
    fe.step(); fe.synchronize()
    assert np.array_equal(fe.get_coupled()["cum_damage"].view(np.uint64), cum0.view(np.uint64))
    fe.close()


# ---- 6. floe-size bins -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nbins", [1, 3, 12])
@pytest.mark.parametrize("options", [{"fused": 0}, {}])
def test_fsd_bins_are_scaled_by_the_surface_ratio_exactly(nbins, options):
    fe, lm, p, f = _handle("toy", options)
    Ne = lm.num_elements
    fsd0 = np.random.default_rng(9).uniform(0.01, 0.9, (nbins, Ne))
    fe.put_coupled(conc_fsd=fsd0)
    fe.explicitSolve(); fe.synchronize()
    s_old = fe.get_diag()["surface"]
    fe.update(); fe.synchronize()
    s_new = fe.get_diag()["surface"]
    fsd1 = fe.get_coupled(cum_damage=False, num_fsd_bins=nbins)["conc_fsd"]
    on_neumann = np.isin(lm.indices.reshape(-1, 3) - 1, lm.neumann_flags).any(1)
    scaled = (f["conc"] > 0.) & ~on_neumann
    kinds = (scaled.sum(), ((f["conc"] > 0.) & on_neumann).sum(), (f["conc"] <= 0.).sum())
    assert all(k > 0 for k in kinds), kinds          # scaled, on a Neumann node, ice-free
    want = np.where(scaled, fsd0 * (s_old / s_new), fsd0)
    assert np.array_equal(fsd1.view(np.uint64), want.view(np.uint64))
    assert np.any(fsd1[:, scaled] != fsd0[:, scaled])
    fe.close()


def test_free_drift_leaves_the_bins_alone():
    from nextsim_amd import _abi
    fe, lm, p, f = _handle("toy", dynamics_type=_abi.NXS_DYN_FREE_DRIFT)
    fsd0 = np.random.default_rng(10).uniform(0.01, 0.9, (3, lm.num_elements))
    cum0 = np.full(lm.num_elements, 1.5)
    fe.put_coupled(cum_damage=cum0, conc_fsd=fsd0)
    fe.step(); fe.synchronize()
    out = fe.get_coupled(num_fsd_bins=3)
    assert np.array_equal(out["conc_fsd"], fsd0) and np.array_equal(out["cum_damage"], cum0)
    fe.close()


# ---- 8. round trip and life cycle --------------------------------------------------------------------------------------------------------------------------------

def test_round_trip_life_cycle_and_error_codes():
    import ctypes as C
    from nextsim_amd import _abi, dynamics
    gm, p, g, lms, fields = cases.make_case("small")
    lm, f = lms[0], fields[0]
    Ne, Nn = lm.num_elements, lm.num_nodes
    fe = dynamics.FiniteElementDynamics(p)
    c = _abi.Coupled()
    tau = smooth_wave_stress(lm)
    assert fe.L.nxs_dyn_set_wave_stress(fe.h, _abi.dptr(tau)) == -4           # NXS_ERR_STATE before set_mesh
    assert fe.L.nxs_dyn_put_coupled(fe.h, C.byref(c)) == -4
    assert fe.L.nxs_dyn_get_coupled(fe.h, C.byref(c)) == -4
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    rng = np.random.default_rng(11)
    cum, fsd = rng.normal(size=Ne), rng.normal(size=(5, Ne))
    fe.put_coupled(cum_damage=cum, conc_fsd=fsd)
    out = fe.get_coupled(num_fsd_bins=5)
    assert np.array_equal(out["cum_damage"].view(np.uint64), cum.view(np.uint64)) and np.array_equal(out["conc_fsd"].view(np.uint64), fsd.view(np.uint64))
    fsd7 = rng.normal(size=(7, Ne))
    fe.put_coupled(cum_damage=cum, conc_fsd=fsd7)                              # another number of bins
    assert np.array_equal(fe.get_coupled(num_fsd_bins=7)["conc_fsd"], fsd7)
    for bad in (dict(num_fsd_bins=5), dict(cum_damage=False, num_fsd_bins=5)):   # not the attached number
        with pytest.raises(dynamics.NxsError) as e:
            fe.get_coupled(**bad)
        assert e.value.code == -1
    c = _abi.Coupled(); c.num_fsd_bins = -1
    assert fe.L.nxs_dyn_put_coupled(fe.h, C.byref(c)) == -1
    c = _abi.Coupled(); c.num_fsd_bins = 3
    assert fe.L.nxs_dyn_put_coupled(fe.h, C.byref(c)) == -1                    # bins without an array
    c = _abi.Coupled(); c.conc_fsd = _abi.dptr(fsd)
    assert fe.L.nxs_dyn_put_coupled(fe.h, C.byref(c)) == -1                    # an array without bins
    assert np.array_equal(fe.get_coupled(num_fsd_bins=7)["conc_fsd"], fsd7)    # (a refused put changes nothing)
    fe.put_coupled(cum_damage=cum)                                             # the bins are detached, cum_damage stays
    assert np.array_equal(fe.get_coupled()["cum_damage"], cum)
    with pytest.raises(dynamics.NxsError) as e:
        fe.get_coupled(cum_damage=False, num_fsd_bins=7)
    assert e.value.code == -1
    fe.put_coupled()                                                           # both NULL: detached
    with pytest.raises(dynamics.NxsError) as e:
        fe.get_coupled()
    assert e.value.code == -1
    # check_fields_fast: a NaN in tau_wi, and only then
    assert fe.checkFieldsFast() == 0
    fe.set_wave_stress(tau)
    assert fe.checkFieldsFast() == 0
    bad = tau.copy(); bad[Nn + 17] = np.nan
    fe.set_wave_stress(bad)
    assert fe.checkFieldsFast() == 1
    fe.set_wave_stress(None)
    assert fe.checkFieldsFast() == 0
    # set_mesh detaches
    fe.put_coupled(cum_damage=cum, conc_fsd=fsd); fe.set_wave_stress(bad)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    with pytest.raises(dynamics.NxsError) as e:
        fe.get_coupled()
    assert e.value.code == -1
    assert fe.checkFieldsFast() == 0
    fe.close()


# ---- 9. the default path is untouched -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options,kernel", [({"fused": 1}, "k_substep_fused"), (PAIR, "k_substep_pair")])
def test_default_path_and_traffic_model_are_untouched(options, kernel):
    never, lm, p, f = _handle("small", options)
    Ne, Nn = lm.num_elements, lm.num_nodes
    never.step(); never.synchronize()
    t0, want = never.traffic_model(), never.get_state()
    assert t0["substep_kernel_name"] == kernel
    fe, _, _, _ = _handle("small", options)
    fe.put_coupled(cum_damage=np.ones(Ne), conc_fsd=np.ones((12, Ne))); fe.set_wave_stress(smooth_wave_stress(lm))
    fe.step(); fe.synchronize()
    fe.put_coupled(); fe.set_wave_stress(None); fe.put_state(f)
    fe.step(); fe.synchronize()
    assert fe.traffic_model() == t0
    _bits_equal(fe.get_state(), want, STATE_KEYS, "attached, detached, step")
    figures = [k for k, v in t0.items() if isinstance(v, float)]

    def delta(attach):
        attach(); fe.put_state(f); fe.step(); fe.synchronize()
        t = fe.traffic_model()
        assert t["substep_kernel_name"] == kernel
        fe.put_coupled(); fe.set_wave_stress(None)
        return {k: t[k] - t0[k] for k in figures if t[k] != t0[k]}
    d = delta(lambda: fe.put_coupled(cum_damage=np.ones(Ne)))
    assert d.pop("substep_unique_bytes") == 16. * Ne and d.pop("substep_scheme_bytes") == 16. * Ne and not d, d    # (every element has one writer)
    d = delta(lambda: fe.set_wave_stress(smooth_wave_stress(lm)))
    assert d.pop("prep_unique_bytes") == 16. * Nn and d.pop("prep_scheme_bytes") == 16. * Nn and not d, d
    d = delta(lambda: fe.put_coupled(conc_fsd=np.ones((12, Ne))))
    assert d == {"update_bytes": 16. * 12 * Ne}, d
    never.close(); fe.close()
