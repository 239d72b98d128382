"""tests/update_ref.py -- the numpy restatement of update() (FE.cpp:3946-4131) -- against oracle.pyoracle.OracleRank.update() on the branch table, bit for bit;
that the table takes every decision of update() where a kernel could get it wrong (block 0, the ragged last block, every displacement zone); and that the
comparison notices each of eight planted mistakes.  No device: tests/test_gpu_update_edges.py runs k_update on the same inputs."""
import numpy as np
import pytest

import update_ref as U

_runs = {}


def oracle_run(name):
    """The oracle's update() on the table of combination `name`: (setup, inputs, the oracle's outputs, its D_del, its surface).  Computed once."""
    if name in _runs:
        return _runs[name]
    from oracle import pyoracle as O
    su = U.Setup(U.COMBINATIONS[name])
    ref = O.OracleRank(su.lm, su.p, su.f)
    ref.explicit_solve()                                                # prep records M_surface with UM_A
    s_old = ref.work_array("surface", su.Ne)
    rng = np.random.default_rng(5)
    for k in U.SIGMA:
        ref.arr[k][:] = rng.normal(size=su.Ne) * 1e3                    # (after one sub-step from rest most of them are 0)
    for k in U.ELEMENT:
        ref.arr[k][:] = su.tab[k]
    ref.arr["UM"][:] = su.um_b
    before = {k: ref.arr[k].copy() for k in U.ELEMENT + U.SIGMA}
    ref.update()
    after = {k: ref.arr[k].copy() for k in U.ELEMENT + U.SIGMA}
    _runs[name] = su, before, s_old, after, ref.work_array("D_del_ci_ridge_myi", su.Ne), ref.work_array("surface", su.Ne)
    return _runs[name]


def mismatches(name, mutate=None):
    su, before, s_old, after, D_ref, s_new = oracle_run(name)
    out, D, branch = U.update(before, s_old, s_new, su.corners, su.prm, mutate)
    bad = {}
    for k in U.ELEMENT + U.SIGMA:
        idx = U.bits_differ(out[k], after[k])
        if idx.size:
            bad[k] = idx
    idx = U.bits_differ(D, D_ref)
    if idx.size:
        bad["D_del_ci_ridge_myi"] = idx
    return su, bad, branch


def test_the_mesh_and_the_zones():
    su = U.Setup({})
    assert su.Ne >= 3 * U.BLOCK and su.Ne % U.BLOCK != 0 and su.on_neumann.any()
    ratio = su.s_a / su.s_b
    still, conv, div = (su.zone == z for z in (U.STILL, U.CONVERGING, U.DIVERGING))
    assert np.all(ratio[still] == 1.0)                                                       # exactly: the same sum of the same bits, divided by itself
    assert 1.05 <= ratio[conv].min() and ratio[conv].max() <= 1.25
    assert 0.80 <= ratio[div].min() and ratio[div].max() <= 0.95
    assert np.all(su.jac_a > 0.) and np.all(su.jac_b > 0.)                                   # no triangle flips
    n = len(su.rows)
    for z in (still, conv, div):
        assert (z & ~su.on_neumann).sum() >= 10 * n                                          # every row many times in every zone
    assert (su.on_neumann & ~still).sum() >= n                                               # on-Neumann elements whose surface changes: only the flag stops the scaling
    assert n <= su.Ne - (su.Ne // U.BLOCK) * U.BLOCK                                         # the ragged last block holds every row
    print(f"{U.MESH}: Ne={su.Ne}, {n} rows; still {still.sum()}, converging {conv.sum()} (surf_ratio {ratio[conv].min():.4f} .. {ratio[conv].max():.4f}), "
          f"diverging {div.sum()} ({ratio[div].min():.4f} .. {ratio[div].max():.4f}), between {(su.zone == U.BETWEEN).sum()}, on Neumann {su.on_neumann.sum()}")


def test_the_threshold_rows_sit_on_their_thresholds():
    """Where nothing scales them -- the still zone -- the rows hold exactly min_c, min_h, new_conc_young == conc_young, a true thickness of 50 and a sum of 1."""
    su, bad, branch = mismatches("young")
    still = su.zone == U.STILL
    name = np.array([r[0] for r in su.rows])[su.row]
    took = lambda bit: (branch & U.BIT[bit]) != 0     # noqa: E731

    def where(row):
        m = still & (name == row)
        assert m.sum() >= 3, row
        return m
    m = where("conc at min_c")
    assert np.all(su.tab["conc"][m] == su.p.min_c) and np.all(took("FAIL_MIN_C")[m])
    assert np.all(took("RIDGING")[where("conc one ulp above min_c")])
    m = where("thick at min_h")
    assert np.all(su.tab["thick"][m] == su.p.min_h) and np.all(took("FAIL_MIN_H")[m])
    assert np.all(took("RIDGING")[where("thick one ulp above min_h")])
    assert np.all(took("FAIL_NCY")[where("new young equals young")])
    m = where("true thickness exactly 50")
    assert np.all(su.tab["thick"][m] / su.tab["conc"][m] == 50.) and not np.any(took("CAP_50")[m & ~su.on_neumann])
    m = where("conc + young exactly 1")
    assert not np.any(took("OW_BELOW_0")[m]) and not np.any(took("OW_ABOVE_1")[m])
    for row in ("gate conc -0", "gate conc -1e-18", "gate conc 0", "NaN conc"):               # the gate is closed by the value alone
        assert np.all(took("GATE_CONC")[(name == row)])
    assert np.all(took("ICE_FREE_LEFTOVER")[name == "gate conc 0"])
    assert np.all(took("YOUNG_ZEROED")[name == "young 0 with thickness"])


@pytest.mark.parametrize("name", list(U.COMBINATIONS))
def test_restatement_gives_the_oracles_bits(name):
    su, bad, branch = mismatches(name)
    assert not bad, {k: [(int(e), su.row_name(e)) for e in v[:5]] for k, v in bad.items()}


@pytest.mark.parametrize("name", list(U.COMBINATIONS))
def test_the_table_takes_every_decision_everywhere(name):
    su, bad, branch = mismatches(name)
    want = U.expected_bits(su.prm)
    e = np.arange(su.Ne)
    last = (su.Ne // U.BLOCK) * U.BLOCK

    def taken(mask):
        word = np.bitwise_or.reduce(branch[mask])
        return {k for k in U.BITS if word & U.BIT[k]}
    assert taken(e >= 0) == want, (want - taken(e >= 0), taken(e >= 0) - want)               # nothing that should be impossible either
    assert taken(e < U.BLOCK) == want, ("block 0", want - taken(e < U.BLOCK))
    assert taken(e >= last) == want, ("the last block", want - taken(e >= last))
    for z in (U.STILL, U.CONVERGING, U.DIVERGING):
        got = taken(su.zone == z)
        assert set(U.RATIO_BITS) & want <= got, (U.ZONE_NAMES[z], (set(U.RATIO_BITS) & want) - got)
        assert got == want, (U.ZONE_NAMES[z], want - got)                                    # (the table does more than asked: every decision in every zone)


YOUNG_ONLY = ("min_c_ge", "min_h_ge", "ncy_le")


@pytest.mark.parametrize("mutation", U.MUTATIONS)
def test_a_planted_mistake_is_noticed(mutation):
    su, bad, branch = mismatches("young", mutation)
    assert bad, mutation
    rows_hit = sorted({su.row_name(e) for v in bad.values() for e in v})
    print(f"{mutation}: {sum(v.size for v in bad.values())} entries differ in {sorted(bad)}; rows: {rows_hit[:6]}")
    must = {"min_c_ge": "conc at min_c", "min_h_ge": "thick at min_h", "ncy_le": "new young equals young", "no_cap_50": "true thickness 120",
            "fmin_fmax": "NaN conc_myi", "myi_bound_without_young": "myi above conc", "d_del_of_the_first_block": "myi 1.3 above 1"}
    if mutation in must:
        assert must[mutation] in rows_hit
    else:
        assert all(su.on_neumann[e] for v in bad.values() for e in v)                         # neumann_one_corner: only on-Neumann elements can differ
    if mutation not in YOUNG_ONLY:                                                            # ... and under the classic category, where the mistake can show there
        assert mismatches("classic newice 4", mutation)[1], mutation


def test_a_nan_that_comes_out_is_the_one_that_went_in():
    """Each NaN row carries a payload of its own; where update() hands a NaN on (the ridge ratio, the young ice's thickness, conc_myi and D_del) the oracle's
    output holds that payload, and so does the restatement's (test_restatement_gives_the_oracles_bits)."""
    su, before, s_old, after, D_ref, s_new = oracle_run("young")
    name = np.array([r[0] for r in su.rows])[su.row]
    payload = lambda a: a.view(np.uint64) & U.NAN_PAYLOAD     # noqa: E731
    seen = 0
    for row, member, outputs in (("NaN ridge_ratio", "ridge_ratio", ("ridge_ratio",)), ("NaN h_young", "h_young", ("h_young", "ridge_ratio")),
                                 ("NaN conc_myi", "conc_myi", ("conc_myi",)), ("NaN thick", "thick", ("ridge_ratio",))):
        m = name == row
        want = payload(before[member][m])
        assert np.all(want >= 0x5a5a00) and np.unique(want).size == 1
        for k in outputs:
            out = after[k][m]
            nan = np.isnan(out)
            assert np.all(payload(out[nan]) == want[nan]), (row, k)
            seen += int(nan.sum())
    m = name == "NaN conc_myi"
    assert np.all(np.isnan(D_ref[m])) and np.all(payload(D_ref[m]) == payload(before["conc_myi"][m]))
    assert seen >= 40, seen
    for row in ("NaN conc", "NaN conc_young"):                    # these are clamped away: no NaN leaves update()
        m = name == row
        assert not any(np.isnan(after[k][m]).any() for k in U.ELEMENT) and not np.isnan(D_ref[m]).any()


def test_min_and_max_are_selections():
    nan = float("nan")
    assert U.std_min(nan, 1.) != U.std_min(nan, 1.) and U.std_min(1., nan) == 1.              # the first argument unless the second is smaller
    assert U.std_max(nan, 1.) != U.std_max(nan, 1.) and U.std_max(1., nan) == 1.
    assert np.signbit(U.std_max(-0., 0.)) and not np.signbit(U.std_max(0., -0.))              # equal arguments: the first one
    assert not np.signbit(U.std_min(0., -0.)) and np.signbit(U.std_min(-0., 0.))
