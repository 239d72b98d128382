"""tests/ocean_coupled_ref.py, the restatement of a coupled ocean's receive and of thermo()'s three OceanType::COUPLED sites, checked without a device: the
receive with a = 1, b = 0, factor = 1, bias = 0 gives the real bamg's grid-to-mesh outputs (tests/golden/bamg_grid_remap.npz) on every golden case up to the
sign of zero; each planted mistake changes at least one bit on the designed inputs; the guarded loops differ from the slab-ocean loops exactly where the
reference's guards say."""
import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import grid_remap_ref as G
import ocean_coupled_ref as OC
import slab_fsd_ref as SFR
import slab_ref as SR

ALB = FR.default_config()["ocean_albedo"]


def _same(a, b):
    return G.same_bits(a, b)


@pytest.mark.parametrize("name", G.CASES)
def test_the_receive_with_unit_coefficients_is_the_real_bamgs_grid_to_mesh(name):
    c = G.case(name)
    fields = [c["g2m_in7"][:, v] for v in range(5)]
    got = OC.receive(OC.lists_of(c), fields, 1., 0., 1., 0.)
    want = c["g2m_out7"][:, :5].T
    assert _same(got + 0., want + 0.)                           # up to the sign of zero: factor * x + bias turns a -0. into +0.
    assert not np.signbit(got[got == 0.]).any()
    one = OC.receive(OC.lists_of(c), [c["g2m_in1"][:, 0]], 1., 0., 1., 0.)
    assert _same(one + 0., c["g2m_out1"].T + 0.)
    touched = np.zeros(c["tri"].shape[0], bool); touched[c["tris"]] = True
    assert np.isnan(got[:, ~touched]).all()                    # 0 * (1 / 0.)
    if name == "all_land":
        assert np.isnan(got).all()


@pytest.mark.parametrize("name", ["coarse", "fine", "one_cell"])
def test_the_receive_is_the_interleaved_application_then_get(name):
    """the property the kernel is held to: grid_to_mesh on the interleaved, transformed input, then factor * x + bias -- here with the golden lists"""
    c = G.case(name)
    for n_var in (1, 3, 5):
        fields, a, b, factor, bias = OC.awkward_fields(c["gridX"].size, n_var)
        got = OC.receive(OC.lists_of(c), fields, a, b, factor, bias)
        x = OC.receive(OC.lists_of(c), list(OC.interleaved(fields, a, b).T), 1., 0., 1., 0., drop=("no_get",))
        with np.errstate(all="ignore"):
            assert _same(got, factor[:, None] * x + bias[:, None])
        for m in ("transform_after", "no_get") if n_var >= 3 else ():        # (the first variable's coefficients are 1, 0, 1, 0)
            assert not _same(got, OC.receive(OC.lists_of(c), fields, a, b, factor, bias, drop=(m,))), m


@pytest.fixture(scope="module")
def col_case():
    gm = cases.global_mesh("small")
    tri = np.ascontiguousarray(gm.tri, np.int64)
    inp, strata, calm = CR.make_inputs(gm.x, gm.y, tri)
    inp.update({k: v for k, v in OC.received_rows(inp).items() if k in ("ocean_temp", "ocean_salt")})
    return tri, inp


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
def test_the_column_resets_before_the_heat_flux(col_case, thermo, young):
    tri, inp = col_case
    cfg = CR.default_config(thermo_type=thermo, freezingpoint_type="unesco")
    work = CR.copy(inp)
    rows, _ = OC.column(work, cfg, tri, young, CR.DT)
    assert _same(work["sst"], inp["ocean_temp"]) and _same(work["sss"], inp["ocean_salt"])
    assert not rows["Qdw"].any() and not rows["Fdw"].any()
    assert _same(rows["tfrw"], CR.freezing_point(cfg, inp["ocean_salt"]))
    late = CR.copy(inp)
    bad, _ = OC.column(late, cfg, tri, young, CR.DT, drop=("reset_after_qio",))
    assert not _same(bad["Qio"], rows["Qio"]) and not _same(bad["tfrw"], rows["tfrw"]) and _same(late["sst"], work["sst"])
    with pytest.raises(AssertionError):
        OC.column(CR.copy(inp), CR.default_config(thermo_type=thermo), tri, young, CR.DT)       # LINEAR: FE.cpp:1246


def test_qow_takes_the_absorbed_share_of_the_short_wave():
    gm = cases.global_mesh("small")
    tri = np.ascontiguousarray(gm.tri, np.int64)
    finp, _ = FR.make_inputs(gm.x, gm.y, tri)
    rows, _ = FR.ow_bulk_fluxes(finp, FR.default_config(), tri)
    qsrml = OC.received_rows({"sst": finp["sst"], "sss": finp["sss"]})["qsrml"]
    got = OC.qow(rows, qsrml)
    assert _same(OC.qow(rows, qsrml, drop=("qsw_kept",)), rows["Qow"])                           # the slab ocean's statement
    assert not _same(got, rows["Qow"]) and (rows["Qsw_ow"] != 0).any()
    assert _same(OC.qow(rows, np.ones_like(qsrml)), rows["Qow"])


@pytest.fixture(scope="module")
def slab_case():
    gm = cases.global_mesh("small")
    tri = np.ascontiguousarray(gm.tri, np.int64)
    inp, strata, calm = SR.make_inputs(gm.x, gm.y, tri)
    rec = OC.received_rows(inp)
    inp["sst"], inp["sss"] = rec["ocean_temp"], rec["ocean_salt"]                                  # (what the column left)
    return gm, tri, inp


@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
def test_the_slab_keeps_sst_and_sss_and_heals_from_the_received_salinity(slab_case, thermo):
    gm, tri, inp = slab_case
    ccfg = CR.default_config(thermo_type=thermo, freezingpoint_type="unesco")
    cfg = SR.category_config(True, temp_dep_healing=1)
    clock = SR.clock()
    a, b, c = SR.copy(inp), SR.copy(inp), SR.copy(inp)
    rows, words = OC.slab(a, cfg, ccfg, ALB, tri, True, SR.DT, clock)
    slab_rows, slab_words = SR.slab(b, cfg, ccfg, ALB, tri, True, SR.DT, clock)
    assert _same(a["sst"], inp["sst"]) and _same(a["sss"], inp["sss"])
    assert not _same(b["sst"], inp["sst"]) and not _same(b["sss"], inp["sss"])
    for k in SR.ROWS:                                                                              # delsss still feeds D_delS, and every other row is the slab ocean's
        assert _same(rows[k], slab_rows[k]), k
    assert np.array_equal(words, slab_words) and np.abs(rows["delS"]).max() > 0
    for k in SR.IN_PLACE:
        assert k in ("sst", "sss", "time_relaxation_damage") or _same(a[k], b[k]), k
    differs = a["time_relaxation_damage"] != b["time_relaxation_damage"]
    assert differs.any() and not differs[a["thick"] <= 0].any()                                   # the Tbot path is live, and only where there is ice
    OC.slab(c, cfg, ccfg, ALB, tri, True, SR.DT, clock, drop=("tbot_advanced",))
    assert _same(c["time_relaxation_damage"], b["time_relaxation_damage"]) and _same(c["sst"], inp["sst"])


def test_the_coupled_loop_with_bins_takes_the_same_three_guards(slab_case):
    gm, tri, _ = slab_case
    nb = 6
    inp, fsd, strata, groups, sets = SFR.make_inputs(gm.x, gm.y, tri, nb, True)
    rec = OC.received_rows(inp)
    inp["sst"], inp["sss"] = rec["ocean_temp"], rec["ocean_salt"]
    ccfg = CR.default_config(freezingpoint_type="unesco")
    cfg = SR.category_config(True, temp_dep_healing=1)
    fcfg = SFR.fsd_config(nb, True)
    a, b, fa, fb = SR.copy(inp), SR.copy(inp), SFR.copy_fsd(fsd), SFR.copy_fsd(fsd)
    ra = OC.slab_coupled(a, fa, cfg, ccfg, fcfg, ALB, tri, True, SR.DT, SR.clock())
    rb = SFR.slab_coupled(b, fb, cfg, ccfg, fcfg, ALB, tri, True, SR.DT, SR.clock())
    assert _same(a["sst"], inp["sst"]) and _same(a["sss"], inp["sss"]) and not _same(b["sss"], inp["sss"])
    assert (a["time_relaxation_damage"] != b["time_relaxation_damage"]).any()
    for k in SR.ROWS:
        assert _same(ra[0][k], rb[0][k]), k
    assert _same(fa["conc_fsd"], fb["conc_fsd"])                                                 # the bins themselves do not read the salinity
