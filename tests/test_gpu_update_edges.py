"""k_update<REC, FSD> (update(), FE.cpp:3946-4131) against oracle.pyoracle.OracleRank.update() on the branch table of tests/update_ref.py, BIT FOR BIT -- NaN
payloads and the sign of zero included -- and k_free_drift against ref_free_drift at its edges.  update() has no libm call and both sides are built with
-ffp-contract=off, so there is nothing to tolerate; tests/test_update_ref.py has shown (without a device) that the table takes every decision of update() in
block 0, in the ragged last block and in every displacement zone, and that a bitwise comparison on it notices a wrong operator, clamp or bound.

The procedure of one parameter combination (run_update):
  1. the toy case with M_UM = UM_A, one sub-step (or four) of dtime_step / substeps = 200 / 120 s; explicitSolve() on the device, explicit_solve() on the oracle;
  2. the device's M_surface (get_diag) has the oracle's bits -- the precondition: update() divides it by the new surface;
  3. REC = 0: get_state() with the stresses brings M_sigma home from the sub-step loop's records, k_update<false> will run; the oracle takes the device's
     stresses, so that both start from the same bits (they come out of the sub-step loop, which is held to 1e-10, not to the bit);
  4. partial put_state of the table's nine element vectors and of UM_B (sigma and damage stay where they are); the same values into the oracle's arrays;
  5. update() on both; every output compared as uint64;
  6. REC = 1: four sub-steps in two launches of k_substep_pair leave the stresses in the records, no get_state of the stresses before update():
     k_update<true> runs and must give the bits of the REC = 0 run of the same four sub-steps;
  7. which instantiation ran is read back from the library (debug array "update_launch"), not assumed.

Device against device -- k_update<true> against k_update<false>, the bins build against the plain one -- every bit of every entry counts.  Against the oracle one
bit of one kind of entry is open: the SIGN of the NaN in ridge_ratio on the elements of the row "NaN h_young" that take the young-ice ridging branch
(sign_open()).  There ridge_ratio = 1. - (1. - ridge) * thick / (thick + newice) with newice = NaN; IEEE 754 (6.3) does not specify the sign of a NaN result and
the two processors differ: gfx950 has no f64 subtraction, a - b is v_add_f64 with a negated source, so 1. - NaN comes out with the sign flipped
(0xfff80000005a5a05), while x86's subsd returns the NaN as it is (0x7ff80000005a5a05).  The row "NaN ridge_ratio" subtracts twice and agrees again.  The tests
assert that the entries that differ in that sign alone are EXACTLY that set after one update() -- 29 elements under every young-ice combination, none under
the classic ones, none in any other vector --, payload and quiet bit included in the comparison; anything else fails.  After a second update() the sign has been
through further subtractions and a division of two NaNs, whose choice IEEE leaves open as well: there the set may be any part of the row's ridge_ratio."""
import ctypes as C
import time

import numpy as np
import pytest

import update_ref as U

pytestmark = pytest.mark.gpu

STATE_OUT = U.ELEMENT + U.SIGMA
# k_free_drift: the largest per-node relative difference |device - oracle| / |oracle| seen on the MI355X where hypot reaches the result (VT and UT, the rows with
# one norm under and one over the 0.01 floor and every ordinary node); the assertion allows four times that, the project's convention for rows with a libm call
FREE_DRIFT_MEASURED = 1.85e-15    # (VT 1.844e-15, UT 1.847e-15; the planted rows themselves 0)
# the sub-step loop that leaves M_sigma in its element records: k_substep_pair, two launches of two sub-steps (an even number of record swaps)
REC_OPTIONS = {"fused": 2, "substeps_per_launch": 2, "pair_regs": 1}
REC_SUBSTEPS = 4
FREE_DRIFT_CAP = 1e-14            # of the field's maximum: tests/test_gpu_parity.py, test_free_drift_and_no_motion


def put(fe, arrays):
    """nxs_dyn_put_state with only `arrays` set: every other member NULL = the device copy is current."""
    from nextsim_amd import _abi
    s = _abi.State()
    keep = []
    for k, v in arrays.items():
        a = np.ascontiguousarray(v, np.float64)
        keep.append(a)
        if k.startswith("sigma"):
            s.sigma[int(k[-1])] = _abi.dptr(a)
        else:
            setattr(s, k, _abi.dptr(a))
    fe._chk(fe.L.nxs_dyn_put_state(fe.h, C.byref(s)))


def get(fe, keys):
    """nxs_dyn_get_state of `keys` alone (asking for a stress or the damage brings the records home: only where the test means to)."""
    from nextsim_amd import _abi
    out = {k: np.empty(2 * fe.lm.num_nodes if k in _abi.STATE_NODAL else fe.lm.num_elements) for k in keys}
    s = _abi.State()
    for k, a in out.items():
        if k.startswith("sigma"):
            s.sigma[int(k[-1])] = _abi.dptr(a)
        else:
            setattr(s, k, _abi.dptr(a))
    fe._chk(fe.L.nxs_dyn_get_state(fe.h, C.byref(s)))
    return out


def same_bits(got, want, what, su=None, sign_open=None):
    """Asserts that `got` has the bits of `want`.  sign_open: a bool mask of the entries at which, where both hold a NaN, its sign may differ (payload and quiet bit
    still count); None: nowhere.  Returns the indices at which that sign alone differs."""
    idx = U.bits_differ(got, want)
    sign_only = np.empty(0, np.int64)
    if sign_open is not None and idx.size:
        loose = U.bits_differ(got, want, nan_sign=False)
        sign_only = np.setdiff1d(idx, loose)
        sign_only = sign_only[sign_open[sign_only]]
        idx = np.setdiff1d(idx, sign_only)
    if idx.size:
        gb, wb = np.ascontiguousarray(got).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)
        rows = [(int(e), su.row_name(e) if su is not None and got.size == su.Ne else "", f"{got[e]!r} {int(gb[e]):#018x}", f"{want[e]!r} {int(wb[e]):#018x}") for e in idx[:6]]
        raise AssertionError(f"{what}: {idx.size} entries differ in their bits; (element, row, device, expected): {rows}")
    return sign_only


def sign_open(su):
    """The elements whose ridge_ratio is a NaN of unspecified sign after one update() (the module docstring): the row "NaN h_young" where the host restatement takes
    the young-ice ridging branch.  Empty under the classic category."""
    arr = dict(su.tab, **{k: np.zeros(su.Ne) for k in U.SIGMA})                # (no decision of update() reads a stress)
    branch = U.update(arr, su.s_a, su.s_b, su.corners, su.prm)[2]
    name = np.array([x[0] for x in su.rows])[su.row]
    return (name == "NaN h_young") & ((branch & U.BIT["RIDGING"]) != 0)


def run_update(name, pair_loop=False, fetch_stresses=True, bins=0, updates=1, with_oracle=True):
    """The procedure of the module docstring.  pair_loop: the sub-step loop is k_substep_pair (REC_SUBSTEPS sub-steps, the stresses end in the records) and not
    one plain sub-step; fetch_stresses: get_state() of the stresses before update() (step 3), which brings them home -- k_update<false> -- and hands them to the
    oracle.  Returns a dict: the device's outputs, the oracle's (None without), the launches and the inputs."""
    from nextsim_amd import dynamics
    from oracle import pyoracle as O
    substeps, options = (REC_SUBSTEPS, REC_OPTIONS) if pair_loop else (1, {})
    su = U.Setup(U.COMBINATIONS[name], substeps)
    fe = dynamics.FiniteElementDynamics(su.p)
    try:
        for k, v in options.items():
            fe.set_option(k, v)
        fe.set_mesh(su.lm); fe.put_state(su.f); fe.set_forcing(su.f)
        fsd0 = None
        if bins:
            fsd0 = np.random.default_rng(9).uniform(0.01, 0.9, (bins, su.Ne))
            fe.put_coupled(conc_fsd=fsd0)
        fe.explicitSolve(); fe.synchronize()
        same_bits(fe.get_diag()["surface"], su.s_a, "M_surface after explicitSolve against measure() with UM_A", su)   # 2.
        ref = None
        if with_oracle:
            ref = O.OracleRank(su.lm, su.p, su.f)
            ref.explicit_solve()
            same_bits(ref.work_array("surface", su.Ne), su.s_a, "the oracle's M_surface", su)
        damage0 = None
        if fetch_stresses:                                                                                              # 3.
            home = get(fe, U.SIGMA + ("damage",))
            damage0 = home["damage"]
            if ref is not None:
                for k in U.SIGMA:
                    ref.arr[k][:] = home[k]
        put(fe, dict(su.tab, UM=su.um_b))                                                                               # 4.
        if ref is not None:
            for k in U.ELEMENT:
                ref.arr[k][:] = su.tab[k]
            ref.arr["UM"][:] = su.um_b
            ref_damage0 = ref.arr["damage"].copy()
        launches = []
        for _ in range(updates):                                                                                        # 5.
            fe.update(); fe.synchronize()
            launches.append(tuple(int(v) for v in fe.debug_array("update_launch")))
            if ref is not None:
                ref.update()
        out = get(fe, U.ELEMENT)                                # (no stress asked for yet: a second update() of the caller's would still find the records)
        diag = fe.get_diag()
        out.update(surface=diag["surface"], D_del_ci_ridge_myi=diag["D_del_ci_ridge_myi"])
        if bins:
            out["conc_fsd"] = fe.get_coupled(cum_damage=False, num_fsd_bins=bins)["conc_fsd"]
        out.update(get(fe, U.SIGMA + ("damage",)))
    finally:
        fe.close()
    want = None
    if ref is not None:
        want = {k: ref.arr[k].copy() for k in STATE_OUT}
        want.update(surface=ref.work_array("surface", su.Ne), D_del_ci_ridge_myi=ref.work_array("D_del_ci_ridge_myi", su.Ne))
        assert np.array_equal(ref.arr["damage"], ref_damage0)
    return dict(su=su, out=out, want=want, launches=launches, damage0=damage0, fsd0=fsd0)


COMPARED = STATE_OUT + ("surface", "D_del_ci_ridge_myi")


def assert_equals_oracle(r, what, keys=COMPARED, updates=1):
    """Every vector of `keys` has the oracle's bits, but for the sign of the NaN of ridge_ratio on sign_open(): after one update() that sign differs on exactly
    that set (so on none under the classic category), after two on any part of the row "NaN h_young".  Returns the number of such entries."""
    su = r["su"]
    first = sign_open(su)
    name = np.array([x[0] for x in su.rows])[su.row]
    is_open = first if updates == 1 else (name == "NaN h_young")
    n = 0
    for k in keys:
        idx = same_bits(r["out"][k], r["want"][k], f"{what}: {k}", su, sign_open=is_open if k == "ridge_ratio" else None)
        if k == "ridge_ratio":
            if updates == 1:
                assert np.array_equal(idx, np.flatnonzero(first)), (f"{what}: the NaN of ridge_ratio differs in its sign alone on {idx.size} elements, on "
                                                                    f"{int(first.sum())} of the row 'NaN h_young' it should", idx[:6], np.flatnonzero(first)[:6])
            n = int(idx.size)
        else:
            assert idx.size == 0
    if not su.prm["young"]:
        assert n == 0 and not first.any()
    if "surface" in keys:
        same_bits(r["out"]["surface"], su.s_b, f"{what}: M_surface against measure() with UM_B", su)
    return n


def assert_equals_device(got, want, what, keys=COMPARED + ("damage",)):
    """Two runs on the device: every bit of every entry, the sign of a NaN included."""
    for k in keys:
        idx = same_bits(got["out"][k], want["out"][k], f"{what}: {k}", got["su"])
        assert idx.size == 0


@pytest.mark.parametrize("name", list(U.COMBINATIONS))
def test_update_has_the_oracles_bits(name):
    """k_update<false> after one sub-step and after four, k_update<true> after four: all against the oracle's update() on the same inputs, and the records' run
    against the arrays' run.  For "classic newice 4" this settles what the bound of conc_myi reads: M_conc_young as it stands, like FE.cpp:4126-4128."""
    t0 = time.perf_counter()
    a = run_update(name)
    assert a["launches"] == [(0, 0, U.BLOCK)], a["launches"]
    n_sign = assert_equals_oracle(a, f"{name}, k_update<false>, 1 sub-step")
    assert same_bits(a["out"]["damage"], a["damage0"], "M_damage is not update()'s to change", a["su"]).size == 0
    a2 = run_update(name, pair_loop=True)
    assert a2["launches"] == [(0, 0, U.BLOCK)], a2["launches"]
    assert assert_equals_oracle(a2, f"{name}, k_update<false>, {REC_SUBSTEPS} sub-steps") == n_sign
    b = run_update(name, pair_loop=True, fetch_stresses=False, with_oracle=False)
    assert b["launches"] == [(1, 0, U.BLOCK)], b["launches"]                  # the stresses were in the records
    assert_equals_device(b, a2, f"{name}: k_update<true> against k_update<false>")
    # (what does not depend on the sub-step loop also equals the one-sub-step run)
    assert_equals_device(b, a, f"{name}: k_update<true> against the one-sub-step run", U.ELEMENT + ("surface", "D_del_ci_ridge_myi"))
    scaled = (a["su"].tab["conc"] > 0.) & ~a["su"].on_neumann
    moved = [int((U.bits_differ(a["out"][k], a["su"].tab[k]).size)) for k in U.ELEMENT]
    assert any(np.any(a2["out"][k][scaled] != 0.) for k in U.SIGMA), "the sub-step loop left no stress to scale"
    print(f"{name}: Ne={a['su'].Ne}, {len(a['su'].rows)} rows, {int(scaled.sum())} elements scaled; entries changed per vector {moved}; "
          f"three handles and two oracle runs in {time.perf_counter() - t0:.2f} s; NaN entries of ridge_ratio equal to the oracle's but for their sign: {n_sign}")


@pytest.mark.parametrize("rec", [False, True])
def test_update_with_bins_attached(rec):
    """k_update<REC, true>: every bin times surf_ratio exactly where (conc > 0) && !on_neumann holds for the INPUT conc -- the -0, negative and NaN rows leave their
    bins alone, bit for bit --, nothing else touched, and the other outputs those of the build without bins."""
    bins = 3
    r = run_update("young", pair_loop=rec, fetch_stresses=not rec, bins=bins, with_oracle=not rec)
    assert r["launches"] == [(1 if rec else 0, 1, U.BLOCK)], r["launches"]
    su = r["su"]
    plain = run_update("young", pair_loop=rec, fetch_stresses=not rec, with_oracle=False)
    assert plain["launches"] == [(1 if rec else 0, 0, U.BLOCK)], plain["launches"]
    assert_equals_device(r, plain, f"bins attached, k_update<{str(rec).lower()}, true> against k_update<{str(rec).lower()}, false>")
    if not rec:
        assert_equals_oracle(r, "bins attached, k_update<false, true>")
    conc_in = su.tab["conc"]
    scaled = (conc_in > 0.) & ~su.on_neumann
    ratio = su.s_a / su.s_b
    want = np.where(scaled, r["fsd0"] * ratio, r["fsd0"])
    for k in range(bins):
        assert same_bits(r["out"]["conc_fsd"][k], want[k], f"bin {k}", su).size == 0
    name = np.array([x[0] for x in su.rows])[su.row]
    for row in ("gate conc -0", "gate conc 0", "gate conc -1e-18", "conc negative", "NaN conc"):
        m = name == row
        assert m.sum() >= 4 and not scaled[m].any()
        assert np.array_equal(r["out"]["conc_fsd"][:, m].view(np.uint64), r["fsd0"][:, m].view(np.uint64)), row
    m = (name == "gate conc 1e-300") & ~su.on_neumann & (su.zone != U.STILL)
    assert m.any() and np.all(r["out"]["conc_fsd"][:, m] != r["fsd0"][:, m])        # the smallest positive conc of the table opens the gate
    m = su.on_neumann & (conc_in > 0.) & (ratio != 1.)
    assert m.any() and np.array_equal(r["out"]["conc_fsd"][:, m], r["fsd0"][:, m])  # only the flag stops these


@pytest.mark.parametrize("rec", [False, True])
def test_a_second_update_without_a_solve(rec):
    """update() twice: the second one finds surface_old == surface, hence surf_ratio == 1.0, and works on the first one's output (clamped, but for the NaN rows)."""
    r = run_update("young", pair_loop=True, fetch_stresses=not rec, updates=2)
    assert r["launches"] == [(1 if rec else 0, 0, U.BLOCK)] * 2, r["launches"]
    if rec:                                                     # (the oracle's stresses are not the records': the stresses against the arrays' run instead)
        twin = run_update("young", pair_loop=True, updates=2, with_oracle=False)
        assert_equals_device(r, twin, "second update, k_update<true> against k_update<false>")
        keys = U.ELEMENT + ("surface", "D_del_ci_ridge_myi")
    else:
        keys = COMPARED
    n_sign = assert_equals_oracle(r, "second update", keys, updates=2)
    once = run_update("young", pair_loop=True, with_oracle=False)
    assert U.bits_differ(once["out"]["D_del_ci_ridge_myi"], r["out"]["D_del_ci_ridge_myi"]).size, "the second update() left D_del_ci_ridge_myi as the first one wrote it"
    print(f"second update, REC = {int(rec)}: NaN entries of ridge_ratio equal to the oracle's but for their sign: {n_sign}")


def test_update_launch_before_any_update():
    from nextsim_amd import dynamics
    su = U.Setup({})
    fe = dynamics.FiniteElementDynamics(su.p)
    try:
        fe.set_mesh(su.lm); fe.put_state(su.f); fe.set_forcing(su.f)
        with pytest.raises(dynamics.NxsError, match="update_launch"):
            fe.debug_array("update_launch")
    finally:
        fe.close()


# ---- k_free_drift (updateFreeDriftVelocity, FE.cpp:10140-10176) at its edges ------------------------------------------------------------------------------------

FLOOR = 0.01
#            name                         VT              VT - ocean        VT - wind        bitwise
FD_ROWS = (("all three equal",           (0.3, -0.2),    (0., 0.),         (0., 0.),        True),
           ("both norms 0.005 or less",  (0.125, 0.0625), (0.003, 0.004),  (0.001, -0.002), True),     # (the result does not depend on hypot's last bit)
           ("on the floor: (0.01, 0) / (0, -0.01)", (FLOOR, -FLOOR), (FLOOR, 0.), (0., -FLOOR), True),   # hypot(x, 0) == |x|, and 0.01 > 0.01 is false
           ("on the floor: (0, -0.01) / (0.01, 0)", (FLOOR, -FLOOR), (0., -FLOOR), (FLOOR, 0.), True),
           ("ocean under, wind over",    (0.25, 0.5),    (0.002, 0.001),   (5., -3.),       False),
           ("ocean over, wind under",    (0.25, 0.5),    (0.3, 0.4),       (0.003, -0.002), False))


def test_free_drift_at_its_edges():
    from nextsim_amd import _abi, dynamics
    from oracle import pyoracle as O
    import cases
    gm, p, g, lms, fields = cases.make_case(U.MESH, dynamics_type=_abi.NXS_DYN_FREE_DRIFT)
    lm, f = lms[0], {k: v.copy() for k, v in fields[0].items()}
    Nn = lm.num_nodes
    rng = np.random.default_rng(21)
    f["VT"] = rng.uniform(-0.3, 0.3, 2 * Nn); f["ocean"] = rng.uniform(-0.2, 0.2, 2 * Nn); f["wind"] = rng.uniform(-10., 10., 2 * Nn)
    f["UT"] = np.zeros(2 * Nn)
    dirichlet = np.asarray(lm.mask_dirichlet, bool)[:Nn]
    f["UT"][np.concatenate([dirichlet, dirichlet])] = rng.uniform(-50., 50., 2 * int(dirichlet.sum()))      # a Dirichlet node keeps whatever it holds
    free = np.flatnonzero(~dirichlet)
    last = (Nn // U.BLOCK) * U.BLOCK
    assert last < Nn and dirichlet[:U.BLOCK].any() and dirichlet[last:].any()
    planted = {}
    for block in (free[free < U.BLOCK], free[free >= last]):                   # node block 0 and the ragged last one
        assert block.size >= 2 * len(FD_ROWS)
        for j, row in enumerate(FD_ROWS + FD_ROWS):                            # twice each: first and last free nodes of the block
            nd = int(block[j] if j < len(FD_ROWS) else block[-1 - (j - len(FD_ROWS))])
            name, vt, d_oce, d_air, bitwise = row
            for c in range(2):
                f["VT"][nd + c * Nn] = vt[c]
                f["ocean"][nd + c * Nn] = vt[c] - d_oce[c]
                f["wind"][nd + c * Nn] = vt[c] - d_air[c]
            planted[nd] = row
    for nd, (name, vt, d_oce, d_air, bitwise) in planted.items():             # the differences the kernel will form are the ones meant, exactly
        du, dv = f["VT"][nd] - f["ocean"][nd], f["VT"][nd + Nn] - f["ocean"][nd + Nn]
        au, av = f["VT"][nd] - f["wind"][nd], f["VT"][nd + Nn] - f["wind"][nd + Nn]
        if name.startswith("on the floor"):
            assert (du, dv) == d_oce and (au, av) == d_air
        if bitwise:
            assert np.hypot(du, dv) <= FLOOR and np.hypot(au, av) <= FLOOR
        else:
            assert (np.hypot(du, dv) > 2 * FLOOR) != (np.hypot(au, av) > 2 * FLOOR) and min(np.hypot(du, dv), np.hypot(au, av)) <= FLOOR / 2
    fe = dynamics.FiniteElementDynamics(p)
    try:
        fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
        fe.step(); fe.synchronize()
        got = fe.get_state()
    finally:
        fe.close()
    ref = O.OracleRank(lm, p, f)
    ref.step()
    both = np.concatenate([dirichlet, dirichlet])
    for k in ("VT", "UT"):
        assert same_bits(got[k][both], f[k][both], f"free drift: {k} of the Dirichlet nodes").size == 0
        assert np.array_equal(ref.arr[k][both], f[k][both])
    assert same_bits(got["UM"], f["UM"], "free drift: M_UM").size == 0
    bound = min(4. * FREE_DRIFT_MEASURED, FREE_DRIFT_CAP)
    worst = {}
    for nd, (name, vt, d_oce, d_air, bitwise) in planted.items():
        for k in ("VT", "UT"):
            d = np.array([got[k][nd], got[k][nd + Nn]]); r = np.array([ref.arr[k][nd], ref.arr[k][nd + Nn]])
            if bitwise:
                assert same_bits(d, r, f"free drift, node {nd}, {name}: {k}").size == 0
            else:
                assert np.hypot(*r) > 0.                            # (a drag-weighted mean of wind and ocean that is not at rest: the figure is defined)
                worst[name] = max(worst.get(name, 0.), float(np.hypot(*(d - r)) / np.hypot(*r)))
    rel = {}
    for k in ("VT", "UT"):
        d = np.hypot(got[k][:Nn] - ref.arr[k][:Nn], got[k][Nn:] - ref.arr[k][Nn:])
        r = np.hypot(ref.arr[k][:Nn], ref.arr[k][Nn:])
        # a free node at rest in the oracle would make its relative difference meaningless: there is none (a tiny norm only makes the figure larger, never smaller)
        assert r[~dirichlet].min() > 0., k
        rel[k] = float((d[~dirichlet] / r[~dirichlet]).max())
        assert cases.rel_err(got[k], ref.arr[k]) <= FREE_DRIFT_CAP, k
    print(f"free drift, {U.MESH}: Nn={Nn}, {len(planted)} planted nodes ({sum(1 for r in planted.values() if r[4])} bitwise); largest per-node relative difference "
          f"where hypot reaches the result: VT {rel['VT']:.3e}, UT {rel['UT']:.3e}; planted rows {worst}")
    assert set(worst) == {row[0] for row in FD_ROWS if not row[4]}
    for name, w in worst.items():                                  # one norm under and one over the floor: the rows themselves
        assert w <= bound, (name, w, bound)
    assert max(rel.values()) <= bound, (rel, bound)
