"""thermo()'s element forcing on the device (nxs_dyn_thermo_forcing_*): 1. the blend is the host's evaluation of ExternalData::get, bit for bit; 2. the chain
fluxes -> column -> slab -> step -> means_update does not notice whether its ten forcing rows were uploaded or blended on the device; 3. the ingest is
nxs_interp_grid_to_mesh at the same targets, column by column; 4. call order, what goes with the mesh, device memory.  Nothing here has a tolerance: the same
kernels on the same input bits, and two expressions numpy and the device both round operation by operation (the library is built without contraction)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import slab_ref as SR
import thermo_forcing_ref as R
from nextsim_amd import _abi, forcing as F, mesh as M

pytestmark = pytest.mark.gpu

DT = SR.DT
MESHES = ("tiny", "toy", "small", "odd")
BLOCK = 256


def _rect(odd):
    """cases.rect_mesh(24, 1) as a local mesh; odd: without its last triangle.  (A triangulated rectangle with 96 boundary vertices has 2 Nn - 98 triangles, an
    even number whatever n is, and so have tiny, toy and small: the odd Ne, the blend's scalar tail, is made by leaving one triangle out.)"""
    x, y, tri, ng = cases.rect_mesh(24, 1)
    if odd:
        tri = tri[:-1]
        assert np.array_equal(np.unique(tri), np.arange(x.size))          # every node still has an element
    on_b = np.zeros(x.size, bool); on_b[:ng] = True
    gm = M.GlobalMesh(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), tri=np.ascontiguousarray(tri, np.int32), dirichlet=on_b,
                      neumann=np.zeros(x.size, bool), lat=M.polar_stereographic_lat(x, y), name="rect")
    p = F.default_params(ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE)
    p, C_fix, C_alea = F.scale_params_to_mesh(p, gm, alea_factor=0.33)
    lm = M.localize(gm, 1)[0]
    return p, lm, F.localize_fields(F.global_fields(gm, p, "arctic", C_fix, C_alea), lm, gm.num_nodes), ng


@functools.lru_cache(maxsize=None)
def _mesh(kind):
    """(params, local mesh, its fields)"""
    if kind in ("odd", "rect"):
        return _rect(kind == "odd")[:3]
    gm, p, g, lms, fields = cases.make_case(kind, ice_cat_type=_abi.NXS_ICECAT_YOUNG_ICE)
    return p, lms[0], fields[0]


def _fe(kind):
    from nextsim_amd import dynamics
    p, lm, f = _mesh(kind)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    return fe, lm


def _refused(call, *texts, code=-4):
    from nextsim_amd import dynamics
    with pytest.raises(dynamics.NxsError) as e:
        call()
    assert e.value.code == code and all(t in str(e.value) for t in texts), (e.value.code, str(e.value))
    return True


def _named(a):
    return dict(zip(_abi.TF_ROWS, a))


def test_the_meshes_cover_the_kernels_edges():
    sizes = {k: _mesh(k)[1].num_elements for k in MESHES}
    assert any(n % 2 for n in sizes.values()), sizes                      # the scalar tail of the 16-byte pairs
    assert any(n < BLOCK for n in sizes.values()), sizes                  # less than one block
    assert any(n > 2 * 2 * BLOCK and n % (2 * BLOCK) for n in sizes.values()), sizes      # more than two blocks of the blend (2 elements per lane), a ragged last one


# ---- 1. the blend equals the host evaluation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", MESHES)
def test_the_blend_is_the_host_evaluation_bit_for_bit(kind):
    fe, lm = _fe(kind)
    Ne = lm.num_elements
    d0, d1 = R.snapshots(Ne)
    fe.thermo_forcing_pair(_named(d0), _named(d1))
    for which, d in ((0, d0), (1, d1)):                                    # the snapshots went up as they are, NaN and signed zeros included
        got = fe.thermo_forcing_get(which)
        assert all(R.same_bits(got[k], d[i]).all() for i, k in enumerate(_abi.TF_ROWS)), which
    off = [k for k, r in zip(_abi.TF_ROWS, R.TABLE) if r[0] == R.OFF]
    sentinel = np.full(Ne, -12345.678)
    fe.flux_set_atmosphere(**{k: sentinel for k in off if k in _abi.FLUX_ATMOSPHERE})       # an OFF row is the host's, through the old calls
    fe.column_set_forcing(**{k: sentinel for k in off if k in _abi.COL_FORCING})
    assert len(off) == 2
    # three times inside the interval and its two end points: fcoeff = |t - t1| / fdt, |t - t0| / fdt (every LINEAR row on its own interval: scaled per row)
    for t in (0., 0.125, 0.5, 0.8125, 1.):
        tab = []
        for k, (mode, c0, c1, factor, bias) in enumerate(R.TABLE):
            if mode == R.LINEAR and (c0, c1) not in ((1., 0.), (0., 1.)):
                tk = (t + 0.1 * k) % 1. if 0. < t < 1. else t
                c0, c1 = abs(tk - 1.) / 1., abs(tk - 0.) / 1.
            tab.append((mode, c0, c1, factor, bias))
        fe.thermo_forcing_time(R.time_rows(tab))
        got = fe.thermo_forcing_get(2)
        for k, name in enumerate(_abi.TF_ROWS):
            want = R.blend(tab[k], d0[k], d1[k])
            if want is None:
                assert np.array_equal(got[name], sentinel), (name, "an OFF row was written")
                continue
            same = R.same_bits(got[name], want)
            assert same.all(), (kind, t, name, tab[k], np.flatnonzero(~same)[:5], got[name][~same][:3], want[~same][:3])
            if tab[k][0] == R.STEP and tab[k][3] != 0.:
                assert np.isfinite(got[name]).all(), (name, "a STEP row saw snapshot 1")
    live = np.concatenate([got[k] for k, r in zip(_abi.TF_ROWS, R.TABLE) if r[0] != R.OFF])
    assert np.signbit(live[live == 0]).any() and np.isnan(live).any()      # the special values were there
    fe.close()


# ---- 2. the chain does not notice ------------------------------------------------------------------------------------------------------------
def _chain_rows(inp, finp, Ne):
    """both snapshots of the ten rows (sane values: the designed atmosphere and a second one some hours later) and each row's mode, factor and bias"""
    s0 = dict(tair=finp["tair"], mslp=finp["mslp"], Qsw_in=finp["Qsw_in"], humidity=finp["dair"], longwave=finp["Qlw_in"],
              precip=inp["precip"], snow=np.linspace(0.1, 0.9, Ne), ocean_temp=inp["sst"], ocean_salt=inp["sss"], mld=inp["mld"])
    s1 = dict(tair=finp["tair"] + 1.5, mslp=finp["mslp"] * 1.002, Qsw_in=finp["Qsw_in"] * 0.8, humidity=finp["dair"] + 0.7, longwave=finp["Qlw_in"] + 12.,
              precip=inp["precip"] * 1.3, snow=None, ocean_temp=inp["sst"] + 0.05, ocean_salt=inp["sss"] - 0.02, mld=None)
    mode = {k: R.STEP if s1[k] is None else R.LINEAR for k in s0}          # snowfr and mld: datasets with one snapshot
    factor = dict.fromkeys(s0, 1.); bias = dict.fromkeys(s0, 0.)
    factor["Qsw_in"], bias["tair"], factor["precip"] = 0.9, -0.3, 0.5
    s0 = {k: np.ascontiguousarray(v, np.float64) for k, v in s0.items()}
    s1 = {k: np.ascontiguousarray(v, np.float64) for k, v in s1.items() if v is not None}
    return s0, s1, mode, factor, bias


def _chain_tab(step, mode, factor, bias):
    """the atmosphere and the ocean come from different products: two intervals, two pairs of coefficients"""
    ta, to = (step + 1) / 6., (step + 2) / 24.
    return [(mode[k], *((abs(ta - 1.), ta) if k in _abi.FLUX_ATMOSPHERE + ("precip",) else (abs(to - 1.), to)), factor[k], bias[k]) for k in _abi.TF_ROWS]


@pytest.mark.parametrize("kind", ["small", "toy"])
def test_the_chain_does_not_notice(kind):
    """handle A uploads the host-evaluated rows through the old calls each step, handle B blends them on the device: the young-ice category, Winton, a nudged
    ocean with the mixed layer depth from its row, so that all ten rows are read"""
    p, lm, f = _mesh(kind)
    Ne = lm.num_elements
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp = SR.sane_inputs(SR.make_inputs(lm.coord_x, lm.coord_y, tri)[0], f)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    ccfg = CR.default_config(thermo_type="winton", ocean_type="nudged", mld_source="row")
    s0, s1, mode, factor, bias = _chain_rows(inp, finp, Ne)
    A, fA = SR.gpu_handle(p, lm, f, inp, finp, ccfg, SR.category_config(True))
    B, fB = SR.gpu_handle(p, lm, f, inp, finp, ccfg, SR.category_config(True))
    B.thermo_forcing_pair(s0, s1)
    el_names = ("tair", "mslp", "Qsw_in", "d2m", "Qlw_in", "precip", "snowfr", "ocean_temp", "ocean_salt", "mld", "sst", "Qa", "tsurf", "wspeed", "conc", "thick")
    for fe in (A, B):
        fe.means_configure(el_names, ("VT_x", "taux"))
    for step in range(3):
        tab = _chain_tab(step, mode, factor, bias)
        rows = {k: R.blend(tab[i], s0[k], s1.get(k)) for i, k in enumerate(_abi.TF_ROWS)}
        A.flux_set_atmosphere(**{k: rows[k] for k in _abi.FLUX_ATMOSPHERE})
        A.column_set_forcing(**{k: rows[k] for k in _abi.COL_FORCING})
        B.thermo_forcing_time(R.time_rows(tab))
        got = B.thermo_forcing_get(2)
        for k in _abi.TF_ROWS:
            assert np.array_equal(got[k], rows[k]), (step, k)
        out = []
        for fe in (A, B):
            fe.fluxes(); fe.column(DT); fe.slab(DT, SR.clock(first_step_of_day=int(step == 1))); fe.step(); fe.means_update(0.25 + 0.25 * (step == 1))
            fe.synchronize()
            o = {"flux:" + k: v for k, v in fe.fluxes_get().items()}
            o.update({"col:" + k: v for k, v in fe.column_rows().items()})
            o.update({"slab:" + k: v for k, v in fe.slab_rows().items()})
            o.update({"state:" + k: v for k, v in fe.get_state().items()})
            o.update({"flux_get:" + k: v for k, v in fe.flux_get().items()})
            o.update({"column_get:" + k: v for k, v in fe.column_get().items()})
            o.update({"slab_get:" + k: v for k, v in fe.slab_get().items()})
            el, nod = fe.means_get()[:2]
            o["means:el"], o["means:nod"] = el, nod
            out.append(o)
        assert out[0].keys() == out[1].keys()
        for k in out[0]:
            assert np.array_equal(out[0][k], out[1][k]), (kind, step, k)
        assert np.abs(out[1]["state:VT"]).max() > 0 and out[1]["means:el"].any() and np.abs(out[1]["col:Qdw"]).max() > 0      # the nudging ran: ocean_temp was read
    A.close(); B.close()


# ---- 3. the ingest equals nxs_interp_grid_to_mesh -------------------------------------------------------------------------------------------
def _grid(lm, N=37, M_=29, descending_x=False, descending_y=True, seed=0, N_data=7):
    """a grid around the mesh's barycentres (an uneven number of cells per axis: the barycentres are on no grid line), its data with NaN in it"""
    rng = np.random.default_rng(seed)
    tri = lm.indices.reshape(-1, 3).astype(np.int64) - 1
    bx, by = lm.coord_x[tri].mean(1), lm.coord_y[tri].mean(1)
    xs = np.linspace(bx.min() - 0.02 * np.ptp(bx), bx.max() + 0.02 * np.ptp(bx), N)
    ys = np.linspace(by.min() - 0.02 * np.ptp(by), by.max() + 0.02 * np.ptp(by), M_)
    if descending_x:
        xs = xs[::-1].copy()
    if descending_y:
        ys = ys[::-1].copy()
    data = rng.normal(size=(M_, N, N_data))
    data[M_ // 3:M_ // 3 + 4, N // 2 - 2:N // 2 + 2, 0] = np.nan
    rx, ry = bx.copy(), by.copy()
    far = 10. * (np.ptp(bx) + np.ptp(by))
    rx[0] -= far; ry[1] += far                                             # targets outside the grid, in x and in y
    rx[2], ry[2] = xs[-1], ys[-1]                                           # exactly on the last coordinate of both axes
    rx[3] = xs[-1]; ry[4] = ys[0]; rx[5] = xs[N // 2]
    return xs, ys, data, rx, ry


INGEST = [dict(interp=1), dict(interp=0), dict(interp=2), dict(interp=1, descending_x=True, descending_y=False), dict(interp=0, descending_x=True),
          dict(interp=1, contours=True), dict(interp=2, contours=True, descending_y=False), dict(interp=1, row_major=True), dict(interp=0, row_major=True, contours=True),
          dict(interp=1, N_data=1)]


@pytest.mark.parametrize("case", INGEST, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
@pytest.mark.parametrize("kind", ["tiny", "odd"])
def test_the_ingest_is_nxs_interp_grid_to_mesh_bit_for_bit(kind, case):
    from nextsim_amd.interp import InterpFromGridToMeshx
    case = dict(case)
    interp, contours, row_major, N_data = case.pop("interp"), case.pop("contours", False), case.pop("row_major", False), case.pop("N_data", 7)
    fe, lm = _fe(kind)
    Ne = lm.num_elements
    xs, ys, data, rx, ry = _grid(lm, seed=interp, N_data=N_data, **case)
    rx2, ry2 = rx + 0.37 * (xs[1] - xs[0]), ry - 0.21 * (ys[1] - ys[0])    # a second dataset's targets: other coordinates
    if contours:                                                           # one more coordinate than cells: the centres are taken
        data = data[:-1, :-1]
    if row_major:
        data = np.ascontiguousarray(np.transpose(data, (1, 0, 2)))
    rng = np.random.default_rng(N_data)
    slots = rng.permutation(20)[:N_data]
    row, snap = (slots % 10).astype(int), (slots // 10).astype(int)
    if N_data > 1:
        row[2] = -1                                                        # a skipped column
    _refused(lambda: fe.thermo_forcing_ingest(1, xs, ys, data, row, snap, 1e8, interp, row_major), "no targets")
    fe.thermo_forcing_targets(0, rx, ry)
    fe.thermo_forcing_targets(1, rx2, ry2)
    for set_, (tx, ty) in enumerate(((rx, ry), (rx2, ry2))):
        want = InterpFromGridToMeshx(xs, ys, data, tx, ty, 1e8, interp, row_major)
        fe.thermo_forcing_ingest(set_, xs, ys, data, row, snap, 1e8, interp, row_major)
        got = [fe.thermo_forcing_get(w, [_abi.TF_ROWS[r] for r, s in zip(row, snap) if r >= 0 and s == w]) for w in (0, 1)]
        for j in range(N_data):
            if row[j] < 0:
                continue
            assert np.array_equal(got[snap[j]][_abi.TF_ROWS[row[j]]], want[:, j]), (kind, set_, j, int(row[j]), int(snap[j]))
        assert want.shape == (Ne, N_data) and (want[:2] == 1e8).all() and np.isfinite(want).all()      # outside the grid -> default; NaN -> default
        if set_ == 0 and not contours:
            assert (want[2] != 1e8).all()                                  # exactly on the last coordinate of both axes: found
        if kind == "odd" and interp != 2 and N_data > 1:
            assert (want[:, 0] == 1e8).sum() > (want[:, 1] == 1e8).sum() >= 2                                 # elements around the NaN cells, in their column alone
    given = {w: {int(r) for r, s in zip(row, snap) if r >= 0 and s == w} for w in (0, 1)}
    for w in (0, 1):                                                       # nothing else became present
        missing = [k for i, k in enumerate(_abi.TF_ROWS) if i not in given[w]]
        if missing:
            _refused(lambda: fe.thermo_forcing_get(w, missing[:1]), "is missing")
    fe.close()


# ---- 4. states and lifetime --------------------------------------------------------------------------------------------------------------------
def _lin(names):
    return {k: dict(mode="linear", fcoeff0=0.25, fcoeff1=0.75) for k in names}


def test_call_order_and_what_is_missing():
    from nextsim_amd import dynamics
    p, lm, f = _mesh("tiny")
    Ne = lm.num_elements
    d0, d1 = R.snapshots(Ne)
    fe = dynamics.FiniteElementDynamics(p)
    assert _refused(lambda: fe.thermo_forcing_time(_lin(["tair"])), "before set_mesh")
    fe.set_mesh(lm)
    assert _refused(lambda: fe.thermo_forcing_time(_lin(["tair"])), "tair is LINEAR", "missing")
    fe.thermo_forcing_pair(dict(tair=d0[0], mld=d0[9]))                     # snapshot 0 only
    assert _refused(lambda: fe.thermo_forcing_time(_lin(["tair"])), "tair is LINEAR")
    assert _refused(lambda: fe.thermo_forcing_time({"mslp": dict(mode="step")}), "mslp is STEP")
    assert _refused(lambda: fe.thermo_forcing_time({"tair": dict(mode=7)}), "unknown mode 7", code=-1)
    assert _refused(lambda: fe.thermo_forcing_get(2, ["tair"]), "is missing") and _refused(lambda: fe.thermo_forcing_get(1, ["tair"]), "is missing")
    assert _refused(lambda: fe.thermo_forcing_get(3, ["tair"]), code=-1)
    fe.thermo_forcing_time({"tair": dict(mode="step"), "mld": dict(mode="step", factor=2.)})      # a row with snapshot 0 only: constant / nearest_daily
    got = fe.thermo_forcing_get(2, ["tair", "mld"])
    assert R.same_bits(got["tair"], d0[0] + 0.).all() and R.same_bits(got["mld"], 2. * d0[9] + 0.).all()
    fe.thermo_forcing_pair({}, dict(tair=d1[0]))                            # a NULL row of s0: that snapshot's device copy is current
    fe.thermo_forcing_time(_lin(["tair"]))
    assert R.same_bits(fe.thermo_forcing_get(2, ["tair"])["tair"], 0.25 * d0[0] + 0.75 * d1[0] + 0.).all()
    xs, ys, data, rx, ry = _grid(lm)
    assert _refused(lambda: fe.thermo_forcing_ingest(0, xs, ys, data, [0] * 7, [0] * 7), "two columns", code=-1)
    assert _refused(lambda: fe.thermo_forcing_ingest(0, xs, ys, data, [0, 1, 2, 3, 4, 5, 10], [0] * 7), "row 10", code=-1)
    assert _refused(lambda: fe.thermo_forcing_ingest(0, xs, ys, data, [0, 1, 2, 3, 4, 5, 6], [0, 0, 0, 2, 0, 0, 0]), "snapshot 2", code=-1)
    assert _refused(lambda: fe.thermo_forcing_ingest(4, xs, ys, data, [0, 1, 2, 3, 4, 5, 6], [0] * 7), "set = 4", code=-1)
    assert _refused(lambda: fe.thermo_forcing_targets(-1, rx, ry), "set = -1", code=-1)
    assert _refused(lambda: fe.thermo_forcing_ingest(0, xs[:-3], ys, data, [0, 1, 2, 3, 4, 5, 6], [0] * 7), "1 or 0 more", code=-1)
    assert _refused(lambda: fe.thermo_forcing_ingest(0, xs, ys, data, [0, 1, 2, 3, 4, 5, 6], [0] * 7), "no targets")
    fe.close()


def _give_and_blend(fe, lm, seed=3):
    Ne = lm.num_elements
    d0, d1 = R.snapshots(Ne, seed)
    fe.thermo_forcing_pair(_named(d0), _named(d1))
    fe.thermo_forcing_time(R.time_rows(R.table(1)))
    names = [k for k, r in zip(_abi.TF_ROWS, R.table(1)) if r[0] != R.OFF]
    return fe.thermo_forcing_get(2, names)


def test_the_rows_go_with_the_mesh():
    """after set_mesh on another mesh and after nxs_dyn_regrid every row is missing again: time and get say so, and giving them again on the new mesh is a fresh
    handle's result"""
    from nextsim_amd import dynamics
    p, lm, f = _mesh("tiny")
    p2, lm2, f2 = _mesh("toy")
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    _give_and_blend(fe, lm)
    fe.thermo_forcing_targets(0, *_grid(lm)[3:])
    fe.set_params(p2); fe.set_mesh(lm2)
    tab = R.time_rows(R.table(1))
    xs, ys, data, rx, ry = _grid(lm2)
    assert _refused(lambda: fe.thermo_forcing_time(tab), "missing")
    for w in (0, 1, 2):
        assert _refused(lambda: fe.thermo_forcing_get(w, ["tair"]), "is missing"), w
    assert _refused(lambda: fe.thermo_forcing_ingest(0, xs, ys, data, [0, 1, 2, 3, 4, 5, 6], [0] * 7), "no targets")
    again = _give_and_blend(fe, lm2)
    fresh = dynamics.FiniteElementDynamics(p2)
    fresh.set_mesh(lm2)
    want = _give_and_blend(fresh, lm2)
    assert again.keys() == want.keys() and all(R.same_bits(again[k], want[k]).all() for k in want)
    fe.close(); fresh.close()
    # nxs_dyn_regrid: an identity regrid of the rectangle (the reference sets interpolated = false there too)
    p, lm, f, ng = _rect(False)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    _give_and_blend(fe, lm)
    fe.thermo_forcing_targets(2, *_grid(lm)[3:])
    prev = np.arange(1, lm.num_nodes + 1, dtype=np.float64)
    fe.regrid(lm, prev, ng, {k: f[k] for k in dynamics.REGRID_INPUTS}, (), moved=(lm.coord_x, lm.coord_y))
    assert _refused(lambda: fe.thermo_forcing_time(tab), "missing")
    for w in (0, 1, 2):
        assert _refused(lambda: fe.thermo_forcing_get(w, ["mslp"]), "is missing"), w
    xs, ys, data, rx, ry = _grid(lm)
    assert _refused(lambda: fe.thermo_forcing_ingest(2, xs, ys, data, [0, 1, 2, 3, 4, 5, 6], [0] * 7), "no targets")
    again = _give_and_blend(fe, lm)
    fresh = dynamics.FiniteElementDynamics(p)
    fresh.set_mesh(lm)
    want = _give_and_blend(fresh, lm)
    assert all(R.same_bits(again[k], want[k]).all() for k in want)
    fe.close(); fresh.close()


def test_fluxes_run_on_blended_rows_and_an_upload_overrides_them():
    """nxs_dyn_fluxes with no flux_set_atmosphere call at all once time has written the five rows; a later flux_set_atmosphere row overrides the blended one until
    the next time"""
    from nextsim_amd import dynamics
    p, lm, f = _mesh("small")
    Ne = lm.num_elements
    tri = np.ascontiguousarray(lm.indices.reshape(-1, 3).astype(np.int64) - 1)
    inp = SR.sane_inputs(SR.make_inputs(lm.coord_x, lm.coord_y, tri)[0], f)
    finp, _ = FR.make_inputs(lm.coord_x, lm.coord_y, tri, drag_ui0=p.quad_drag_coef_air)
    s0, s1, mode, factor, bias = _chain_rows(inp, finp, Ne)
    tab = _chain_tab(0, mode, factor, bias)
    rows = {k: R.blend(tab[i], s0[k], s1.get(k)) for i, k in enumerate(_abi.TF_ROWS)}

    def handle():
        fe = dynamics.FiniteElementDynamics(p)
        fs = dict(f, **{k: inp[k].copy() for k in SR.STATE[:-1]}, wind=inp["wind"].copy(), time_relaxation_damage=inp["time_relaxation_damage"].copy())
        fe.set_mesh(lm); fe.put_state(fs); fe.set_forcing(fs)
        fe.flux_configure(**FR.default_config(force_neutral_atmosphere=1))
        fe.flux_put(**dict({k: finp[k] for k in _abi.FLUX_STATE}, tice0=inp["tice0"], sst=inp["sst"], sss=inp["sss"], pond_fraction=inp["pond_fraction"],
                           lid_volume=inp["lid_volume"]))
        return fe

    B = handle()
    assert _refused(B.fluxes, "an atmosphere row is missing")
    B.thermo_forcing_pair(s0, s1)
    B.thermo_forcing_time({k: v for k, v in R.time_rows(tab).items() if k in _abi.FLUX_ATMOSPHERE})
    B.fluxes()                                                             # no flux_set_atmosphere call at all
    A = handle()
    A.flux_set_atmosphere(**{k: rows[k] for k in _abi.FLUX_ATMOSPHERE})
    A.fluxes()
    a, b = A.fluxes_get(), B.fluxes_get()
    assert all(np.array_equal(a[k], b[k]) for k in a) and np.abs(b["Qia"]).max() > 0
    warm = rows["tair"] + 4.
    for fe in (A, B):
        fe.flux_set_atmosphere(tair=warm)                                  # overrides the blended row ...
        fe.fluxes()
    assert np.array_equal(B.thermo_forcing_get(2, ["tair"])["tair"], warm)
    a2, b2 = A.fluxes_get(), B.fluxes_get()
    assert all(np.array_equal(a2[k], b2[k]) for k in a2) and not np.array_equal(b2["Qia"], b["Qia"])
    B.thermo_forcing_time({k: v for k, v in R.time_rows(tab).items() if k in _abi.FLUX_ATMOSPHERE})      # ... until the next time
    B.fluxes()
    b3 = B.fluxes_get()
    assert np.array_equal(B.thermo_forcing_get(2, ["tair"])["tair"], rows["tair"]) and all(np.array_equal(b3[k], b[k]) for k in b if k != "tau_ow")
    A.close(); B.close()


def test_handles_give_the_forcing_pool_back():
    """four cycles of create / pair / time / ingest / destroy leave the free device memory where it settled (twenty rows of the 10 km mesh are 9 MB: a pool
    that was not released would cost 37 MB over the four cycles)"""
    from nextsim_amd import dynamics
    L = dynamics.load_library()
    L.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        a, b = C.c_size_t(), C.c_size_t()
        assert L.hipMemGetInfo(C.byref(a), C.byref(b)) == 0
        return a.value
    gm, p, g, lms, fields = cases.make_case("10km")
    lm = lms[0]
    Ne = lm.num_elements
    rng = np.random.default_rng(0)
    d = rng.normal(size=(10, Ne))
    xs, ys, data, rx, ry = _grid(lm, N_data=2)

    def cycle():
        fe = dynamics.FiniteElementDynamics(p)
        fe.set_mesh(lm)
        fe.thermo_forcing_pair(_named(d), _named(d))
        fe.thermo_forcing_time(_lin(_abi.TF_ROWS))
        fe.thermo_forcing_targets(0, rx, ry)
        fe.thermo_forcing_ingest(0, xs, ys, data, ["tair", "mld"], [0, 1])
        fe.thermo_forcing_ingest(0, xs, ys, np.concatenate([data, data], 2), ["tair", "mld", None, "snow"], [0, 1, 0, 0])      # the data buffer grows
        fe.synchronize()
        fe.close()
    for _ in range(3):
        cycle()
    mid = free_bytes()
    for _ in range(4):
        cycle()
    end = free_bytes()
    assert 4 * Ne * 8 * 20 > 32 << 20 and mid - end < 3 << 20, (mid, end, (mid - end) / 4)
