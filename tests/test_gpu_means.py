"""The Moorings time means on the device (include/nxs_dyn.h: nxs_dyn_means_*) against tests/means_ref.py, the numpy restatement of updateMeans
(FE.cpp:8518-9024) fed with the host copies of the very fields the device accumulates.

Tolerances: every variable without a math-library call is compared BIT FOR BIT (acc += x * tf is a rounded product and a rounded sum on both sides;
sigma_n, sigma_s and divergence against the vectors nxs_dyn_ice_diagnostics returned: the two kernels share one statement of that arithmetic).
taux, tauy and taumod contain hypot (FE.cpp:8980, 8996), the device's own compensated one (means_hypot) against the C library's in numpy.
  taumod: rtol 4e-16, the bound tests/test_gpu_parity.py applies to D_sigma1 = hypot(...).  Its two terms are non-negative, so nothing cancels.
  taux, tauy: tau_i * conc and tau_a * |wind| * wind_x * (1 - conc) have either sign and cancel (the water drags the ice against the wind), so an error of the
  second term is not small relative to the SUM.  Their bound is therefore absolute, derived, and relative to the terms: with u = 2^-53, two hypot results that are
  each within one unit in the last place differ by <= 4 u relative; each of the six roundings behind it (wind2 * wind, tau_a * wind2, * (1 - conc), the sum,
  * time_factor, the accumulation) may fall differently on the two sides, <= 2 u each: |device - numpy| <= 16 u * sum over the calls of
  (|tau_i conc| + |tau_a wind2 (1 - conc)|) * time_factor, which means_ref.MeansRef keeps in nod_terms.
A NaN (drag_ui of an element without ice is 0 / 0 in the reference too) must be a NaN on both sides.
"""
import numpy as np
import pytest

import cases
import means_ref as R
from test_coupled_abi import smooth_wave_stress

pytestmark = pytest.mark.gpu

HYPOT_RTOL = 4e-16     # tests/test_gpu_parity.py::test_ice_diagnostics_kernel_and_a_moorings_record_from_device_arrays, D_sigma1


def _handle(kind="small", nparts=1, rank=0, options=None, **over):
    from nextsim_amd import dynamics
    gm, p, g, lms, fields = cases.make_case(kind, nparts=nparts, **over)
    lm, f = lms[rank], fields[rank]
    fe = dynamics.FiniteElementDynamics(p)
    for k, v in (options or {}).items():
        fe.set_option(k, v)
    fe.set_mesh(lm); fe.put_state(f); fe.set_forcing(f)
    return fe, lm, p, f


def _tau_ow(lm):
    """a synthetic D_tau_ow (the open-water drag coefficient the thermodynamics writes), one value per element"""
    tri = lm.indices.reshape(-1, 3) - 1
    L = max(np.ptp(lm.coord_x), np.ptp(lm.coord_y))
    return np.ascontiguousarray(1.3e-3 * (1. + 0.2 * np.sin(5. * lm.coord_x[tri].mean(1) / L) * np.cos(3. * lm.coord_y[tri].mean(1) / L)))


def _same(a, b):
    """bit-identical, a NaN matching any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _reference(fe, lm, p, elemental, nodal):
    from nextsim_amd import dynamics
    nec, _ = dynamics.mesh_connectivity(lm.indices, lm.num_nodes)
    return R.MeansRef(lm.num_nodes, lm.num_elements, lm.local_nelements, p.ice_cat_type == 1, elemental, nodal, nec)


def _ref_update(ref, fe, f, tf, tau_wi=None, tau_ow=None):
    fe.synchronize()
    st = fe.get_state()
    host, _ = fe.updateIceDiagnostics()
    ref.update(tf, st, diag=fe.get_diag(), ice_diag=host, wind=f["wind"], tau_wi=tau_wi, tau_ow=tau_ow, drag_ui=f["drag_ui"], drag_ui_young=f["drag_ui_young"])
    return st, host


def _compare(ref, el, nod, what):
    for k, name in enumerate(ref.elemental):
        assert _same(el[:, k], ref.el[:, k]), f"{what}: elemental {name} differs"
    for k, name in enumerate(ref.nodal):
        if name in R.LIBM:
            ok = np.isfinite(ref.nod[:, k])
            err = np.abs(nod[ok, k] - ref.nod[ok, k]) / np.abs(ref.nod[ok, k]).clip(1e-300)
            print(f"{what}: {name} max rel err {err.max():.3e}, {np.count_nonzero(nod[ok, k] != ref.nod[ok, k])} of {ok.sum()} values differ")
    for k, name in enumerate(ref.nodal):
        if name in R.LIBM:
            assert np.array_equal(np.isnan(nod[:, k]), np.isnan(ref.nod[:, k])), name
            if name == "taumod":
                np.testing.assert_allclose(nod[:, k], ref.nod[:, k], rtol=HYPOT_RTOL, atol=0, err_msg=f"{what}: {name}")
            else:
                ok = np.isfinite(ref.nod[:, k])
                assert np.all(np.abs(nod[ok, k] - ref.nod[ok, k]) <= 16 * 2.0 ** -53 * ref.nod_terms[ok, k]), f"{what}: {name}"
        else:
            assert _same(nod[:, k], ref.nod[:, k]), f"{what}: nodal {name} differs"


# ---- 1. accumulation parity, 2. snapshot mode ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage", [1, 0])
def test_accumulation_parity_every_variable_then_snapshot(stage):
    steps = 3
    fe, lm, p, f = _handle("small", options={"means_stage": stage}, dynamics_type="bbm", ice_cat_type=1)
    assert p.ice_cat_type == 1 and p.dynamics_type == 0
    tau_wi, tau_ow = smooth_wave_stress(lm), _tau_ow(lm)
    fe.set_wave_stress(tau_wi)
    fe.means_set_tau_ow(tau_ow)
    fe.means_configure(R.ELEMENTAL, R.NODAL)
    ref = _reference(fe, lm, p, R.ELEMENTAL, R.NODAL)
    tf = 1. / steps
    for _ in range(steps):
        fe.step()
        fe.means_update(tf)
        st, host = _ref_update(ref, fe, f, tf, tau_wi, tau_ow)
    el, nod, de, dn = fe.means_get()
    assert de and dn and el.shape == (lm.num_elements, len(R.ELEMENTAL)) and nod.shape == (lm.num_nodes, len(R.NODAL))
    _compare(ref, el, nod, f"{steps} steps, stage {stage}")
    # the comparison is not of zeros: the fields moved and every column holds something
    assert np.abs(el[:, R.ELEMENTAL.index("divergence")]).max() > 0 and np.abs(el[:, R.ELEMENTAL.index("sigma_s")]).max() > 0
    assert np.abs(el[:, R.ELEMENTAL.index("damage")]).max() > 0 and el[:, R.ELEMENTAL.index("ice_mask")].max() == steps
    for k, name in enumerate(R.NODAL):
        assert np.nanmax(np.abs(nod[:, k])) > 0, name
    # 2. snapshot mode: reset, one update(1.0) = the fields themselves
    fe.means_reset()
    e0, n0, _, _ = fe.means_get()
    assert not e0.any() and not n0.any()
    fe.means_update(1.0)
    el, nod, _, _ = fe.means_get()
    Nn = lm.num_nodes
    dg = fe.get_diag()
    for name, want in (("conc", host["D_conc"]), ("thick", host["D_thick"]), ("snow", host["D_snow_thick"]), ("conc_cons", st["conc"]), ("damage", st["damage"]),
                       ("ridge_ratio", st["ridge_ratio"]), ("conc_young", st["conc_young"]), ("conc_myi", st["conc_myi"]), ("thick_myi", st["thick_myi"]),
                       ("dci_ridge_myi", dg["D_del_ci_ridge_myi"]), ("sigma_11", st["sigma0"]), ("sigma_22", st["sigma1"]), ("sigma_12", st["sigma2"]),
                       ("sigma_n", host["D_sigma0"]), ("sigma_s", host["D_sigma1"]), ("divergence", host["D_divergence"])):
        assert np.array_equal(el[:, R.ELEMENTAL.index(name)], want), name      # (0.0 + x * 1.0 == x; value equality: a -0.0 comes back as +0.0)
    for name, want in (("VT_x", st["VT"][:Nn]), ("VT_y", st["VT"][Nn:]), ("wind_x", f["wind"][:Nn]), ("wind_y", f["wind"][Nn:]),
                       ("tau_ax", dg["D_tau_a"][:Nn]), ("tau_ay", dg["D_tau_a"][Nn:]), ("tauwix", tau_wi[:Nn]), ("tauwiy", tau_wi[Nn:])):
        assert np.array_equal(nod[:, R.NODAL.index(name)], want), name
    fe.close()


def test_classic_category_and_an_odd_row_length():
    """ice_cat_type classic (no young-ice terms in conc / thick / drag_ui / ice_mask), EVP, and rows of 3 and 1 variables (the 8-byte tail of the row stream)"""
    el_ids, nod_ids = ("thick", "drag_ui", "ice_mask"), ("VT_y",)
    for stage in (1, 0):
        fe, lm, p, f = _handle("small", options={"means_stage": stage}, dynamics_type="evp", ice_cat_type=0, newice_type=1)
        fe.means_configure(el_ids, nod_ids)
        ref = _reference(fe, lm, p, el_ids, nod_ids)
        for _ in range(2):
            fe.step(); fe.means_update(0.5)
            _ref_update(ref, fe, f, 0.5)
        el, nod, _, _ = fe.means_get()
        _compare(ref, el, nod, f"classic, stage {stage}")
        assert np.array_equal(el[:, 1], np.full(lm.num_elements, p.quad_drag_coef_air * 0.5 + p.quad_drag_coef_air * 0.5))
        fe.close()


# ---- 3. ghosts -------------------------------------------------------------------------------------------------------------------------------------------

def test_ghost_element_rows_stay_zero_and_ghost_node_rows_are_filled():
    fe, lm, p, f = _handle("small", nparts=2, rank=0)
    assert 0 < lm.local_nelements < lm.num_elements and lm.local_ndof < lm.num_nodes
    el_ids, nod_ids = ("conc", "thick", "ice_mask", "conc_cons", "drag_ui"), ("wind_x", "wind_y", "VT_x")
    for stage in (1, 0):
        fe.set_option("means_stage", stage)
        fe.means_configure(el_ids, nod_ids)
        ref = _reference(fe, lm, p, el_ids, nod_ids)
        for _ in range(2):
            fe.means_update(0.5)        # (no step: a rank of two needs its neighbour for that; the state is what put_state brought)
            _ref_update(ref, fe, f, 0.5)
        el, nod, _, _ = fe.means_get()
        _compare(ref, el, nod, f"partition, stage {stage}")
        assert not el[lm.local_nelements:].view(np.uint64).any()                     # +0.0 exactly, every ghost row
        assert np.abs(el[:lm.local_nelements, 0]).max() > 0
        assert np.array_equal(nod[lm.local_ndof:, 0], f["wind"][lm.local_ndof:lm.num_nodes]) and np.abs(nod[lm.local_ndof:, 0]).max() > 0
    fe.close()


# ---- 4. no side effects ----------------------------------------------------------------------------------------------------------------------------------

def test_means_do_not_touch_the_state_nor_the_default_path():
    a, lm, p, f = _handle("small")
    b, _, _, _ = _handle("small")
    b.means_configure(R.ELEMENTAL, [n for n in R.NODAL if n != "tauwix" and n != "tauwiy"])
    b.means_set_tau_ow(_tau_ow(lm))
    for _ in range(3):
        a.step()
        b.step(); b.means_update(1. / 3.)
    a.synchronize(); b.synchronize()
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint64), sb[k].view(np.uint64)), k
    ta, tb = a.traffic_model(), b.traffic_model()
    assert ta == tb
    # a handle with nothing configured: the same model and kernel before and after means calls were made on it
    for call in (lambda: a.means_update(1.0), lambda: a.means_get()):
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == -4
    a.means_reset()
    a.means_configure((), ())
    a.step(); a.synchronize()
    b.means_configure((), ())
    b.step(); b.synchronize()
    assert a.traffic_model() == ta == b.traffic_model()
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint64), sb[k].view(np.uint64)), k
    a.close(); b.close()


# ---- 5. grid ---------------------------------------------------------------------------------------------------------------------------------------------

def _oracle_grid(lm, um, local_nelements, el, nod, ncols, nrows, xmin, ymax, spacing, miss_val, ice_col, el_mask, nod_mask, ge=None, gn=None):
    from oracle import pyoracle as O
    Nn = lm.num_nodes
    x, y = lm.coord_x + um[:Nn], lm.coord_y + um[Nn:]

    def sample(rows):
        return O.bamg_interp_mesh_to_grid(lm.indices, x, y, rows, xmin, ymax, spacing, spacing, ncols, nrows, 0.)
    pm = (np.arange(lm.num_elements) < local_nelements).astype(np.float64)
    return R.grid_mean(sample, el.shape[1], nod.shape[1], pm, el, nod, ncols, nrows, miss_val, ice_col, el_mask, nod_mask, ge, gn)


def _bamg_built():
    from oracle import pyoracle as O
    return O.bamg_shim() is not None


@pytest.mark.skipif(not _bamg_built(), reason="oracle/_ref (real contrib/bamg) not present on this box")
@pytest.mark.parametrize("nparts,rank", [(1, 0), (2, 0)])
def test_means_to_grid_against_the_real_bamg(nparts, rank):
    fe, lm, p, f = _handle("small", nparts=nparts, rank=rank)
    el_ids = [("conc", True), "thick", ("ice_mask", False), ("sigma_n", True), "divergence"]
    nod_ids = [("VT_x", True), "wind_x", ("wind_y", True)]
    fe.means_configure(el_ids, nod_ids)
    steps = 2
    for _ in range(steps):
        if nparts == 1:
            fe.step()
        fe.means_update(1. / steps)
    if nparts == 1:     # an ice-free patch, so that the mask has something to mask: zero the ice-mask column's source there and accumulate once more
        st = fe.get_state()
        full = dict(f); full.update(st)
        tri = lm.indices.reshape(-1, 3) - 1
        hole = lm.coord_x[tri].mean(1) > 0.3 * lm.coord_x.max()
        for k in ("thick", "h_young"):
            full[k] = np.where(hole, 0., full[k])
        fe.put_state(full)
        fe.means_reset()
        fe.means_update(1.0)
    el, nod, _, _ = fe.means_get()
    um = fe.get_state()["UM"]
    ncols, nrows = 70, 50
    x0, x1, y0, y1 = lm.coord_x.min(), lm.coord_x.max(), lm.coord_y.min(), lm.coord_y.max()
    spacing = max((x1 - x0) / (ncols - 3), (y1 - y0) / (nrows - 3))
    args = (x0 - spacing, y1 + spacing, spacing)
    el_mask, nod_mask = [1, 0, 0, 1, 0], [1, 0, 1]
    ge, gn = fe.means_to_grid(*args, ncols, nrows, -1e14)
    we, wn = _oracle_grid(lm, um, lm.local_nelements, el, nod, ncols, nrows, *args, -1e14, 2, el_mask, nod_mask)
    assert _same(ge, we) and _same(gn, wn)
    ice = ge[2]
    assert (ice > 0).any() and (ice <= 0).any()
    if nparts == 1:
        # the mask bites: a masked variable is zero on ice-free cells where the unmasked companion is not
        assert np.any((ice <= 0) & (gn[1] != 0)) and not np.any((ice <= 0) & (gn[2] != 0)) and not np.any((ice <= 0) & (gn[0] != 0))
    else:
        # the proc-mask factor: grid points in ghost elements carry nodal data in the sampling but 0 in the record
        from oracle import pyoracle as O
        Nn = lm.num_nodes
        raw = O.bamg_interp_mesh_to_grid(lm.indices, lm.coord_x + um[:Nn], lm.coord_y + um[Nn:], nod, *args, spacing, ncols, nrows, 0.)
        raw_wind = np.ascontiguousarray(raw[..., 1].T).ravel()
        assert np.any((raw_wind != 0) & (gn[1] == 0))
    # a second call accumulates onto the non-zero grid
    ge2, gn2 = fe.means_to_grid(*args, ncols, nrows, -1e14, ge.copy(), gn.copy())
    we2, wn2 = _oracle_grid(lm, um, lm.local_nelements, el, nod, ncols, nrows, *args, -1e14, 2, el_mask, nod_mask, we.copy(), wn.copy())
    assert _same(ge2, we2) and _same(gn2, wn2)
    assert not _same(ge2, ge)
    fe.close()


def test_a_time_mean_moorings_record_end_to_end(tmp_path):
    from nextsim_amd import io
    fe, lm, p, f = _handle("small")
    fe.means_configure(["conc", "ice_mask"], ["VT_x"])
    for _ in range(2):
        fe.step(); fe.means_update(0.5)
    ncols, nrows = 40, 30
    spacing = np.ptp(lm.coord_x) / (ncols - 1)
    lon = np.zeros((nrows, ncols), np.float32); lat = np.zeros((nrows, ncols), np.float32)
    path = str(tmp_path / "Moorings.nc")
    var = [dict(name=n, standard_name=n, long_name=n, units="1", cell_methods="area: mean") for n in ("sic", "ice_mask", "siu")]
    io.moorings_create(path, lon, lat, var, format=io.NC_CLASSIC)
    ge, gn = io.moorings_append_means(path, 1.0, fe, lm.coord_x.min(), lm.coord_y.max(), spacing, ncols, nrows)
    assert ge.shape == (2, ncols * nrows) and gn.shape == (1, ncols * nrows) and ge[0].max() > 0
    el, nod, _, _ = fe.means_get()
    assert not el.any() and not nod.any()           # resetMeshMean followed the record
    assert io.moorings_file_format(path) == io.NC_CLASSIC
    fe.close()


# ---- 6. remesh and errors --------------------------------------------------------------------------------------------------------------------------------

def test_configuration_survives_set_mesh_with_zeroed_accumulators_of_the_new_size():
    fe, lm, p, f = _handle("small")
    fe.means_configure(["conc", "damage", "ice_mask"], ["VT_x", "wind_y"])
    fe.step(); fe.means_update(1.0)
    el, nod, _, _ = fe.means_get()
    assert el.any() and nod.any()
    gm, p2, g, lms, fields = cases.make_case("tiny")
    lm2, f2 = lms[0], fields[0]
    assert lm2.num_elements != lm.num_elements
    fe.set_mesh(lm2)
    el, nod, de, dn = fe.means_get()
    assert el.shape == (lm2.num_elements, 3) and nod.shape == (lm2.num_nodes, 2) and de and dn
    assert not el.view(np.uint64).any() and not nod.view(np.uint64).any()
    with pytest.raises(Exception) as e:         # update before put_state on the new mesh
        fe.means_update(1.0)
    assert e.value.code == -4
    fe.put_state(f2); fe.set_forcing(f2)
    fe.means_update(0.5)
    ref = _reference(fe, lm2, p, ["conc", "damage", "ice_mask"], ["VT_x", "wind_y"])
    _ref_update(ref, fe, f2, 0.5)
    el, nod, _, _ = fe.means_get()
    _compare(ref, el, nod, "after set_mesh")
    fe.close()


def test_error_codes_and_the_handle_stays_usable():
    from nextsim_amd import dynamics
    gm, p, g, lms, fields = cases.make_case("small")
    lm, f = lms[0], fields[0]
    fe = dynamics.FiniteElementDynamics(p)

    def code(call):
        with pytest.raises(dynamics.NxsError) as e:
            call()
        assert str(e.value).split(": ", 1)[1], "no message"
        return e.value.code
    fe.means_configure(["conc"], ["VT_x"])                       # before set_mesh: allowed, the configuration is the handle's
    assert code(lambda: fe.means_update(1.0)) == -4              # update before set_mesh
    fe.set_mesh(lm)
    assert code(lambda: fe.means_update(1.0)) == -4              # ... before put_state
    fe.put_state(f); fe.set_forcing(f)
    fe.means_update(1.0)
    assert code(lambda: fe.means_configure([999], [])) == -1     # unknown id
    assert code(lambda: fe.means_configure(["VT_x"], [])) == -1  # a nodal id in the elemental list
    assert code(lambda: fe.means_configure([], ["conc"])) == -1
    assert code(lambda: fe.means_configure([("conc", True)], [])) == -1         # mask without ice_mask
    assert code(lambda: fe.means_configure(["conc"], [("VT_x", True)])) == -1
    assert code(lambda: fe.means_configure(["conc"] * 25, [])) == -1            # more than NXS_MEANS_MAX_VARS
    el, nod, _, _ = fe.means_get()                               # the refused configurations left the previous one, accumulators intact
    assert el.shape[1] == 1 and nod.shape[1] == 1 and np.array_equal(nod[:, 0], f["VT"][:lm.num_nodes] * 1.0) and el.any()
    fe.means_configure(["conc"], ["tauwix"])
    assert code(lambda: fe.means_update(1.0)) == -4              # no wave stress attached
    fe.set_wave_stress(smooth_wave_stress(lm))
    fe.means_update(1.0)
    fe.set_wave_stress(None)
    assert code(lambda: fe.means_update(1.0)) == -4
    for name in ("taux", "tauy", "taumod"):
        fe.means_configure([], [name])
        assert code(lambda: fe.means_update(1.0)) == -4          # no tau_ow attached
    fe.means_set_tau_ow(_tau_ow(lm))
    fe.step(); fe.means_update(1.0)
    fe.means_set_tau_ow(None)
    assert code(lambda: fe.means_update(1.0)) == -4
    assert code(lambda: fe.means_to_grid(0., 0., -1., 4, 4)) == -1
    # still a working handle
    fe.means_configure(["conc", ("thick", True), "ice_mask"], [])
    fe.step(); fe.means_update(1.0); fe.synchronize()
    el, nod, de, dn = fe.means_get()
    assert nod is None and dn is None and el.any()
    fe.close()
