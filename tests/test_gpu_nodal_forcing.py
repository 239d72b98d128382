"""The dynamics' nodal forcing on the device (nxs_mapx_forward, nxs_dyn_forcing_*, nxs_dyn_set_forcing_time_rows, nxs_dyn_set_element_depth): 1. the projection on
the device against the host body; 2. the ingest without vectors is nxs_interp_grid_to_mesh at the nodes, column by column, bit for bit; 3. the rotation and the
wrap are the host's bits; 4. the east/north transform is held to the ONE tolerance derived in tests/nodal_forcing_ref.py, against the host body; 5. the blend per
group is nxs_dyn_set_forcing_time's and numpy's expression, and the step does not notice; 6. call order, what goes with the mesh, device memory; 7. a handle that
never calls the new entry points.  The targets are synthetic numbers inside and outside the grid box."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import nodal_forcing_ref as R
from nextsim_amd import _abi, forcing as F, mesh as M

pytestmark = pytest.mark.gpu

MESHES = ("tiny", "toy", "odd", "shuffled")
BLOCK = 256
STATE_KEYS = ("VT", "UM", "UT", "conc", "thick", "snow_thick", "damage", "ridge_ratio", "sigma0", "sigma1", "sigma2")


@functools.lru_cache(maxsize=None)
def _mesh(kind):
    """(params, local mesh, its fields, geometric vertices)"""
    if kind == "odd":          # a rectangle with an odd number of nodes: 96 on the boundary + 25 * 25
        x, y, tri, ng = cases.rect_mesh(25, 1)
        on_b = np.zeros(x.size, bool); on_b[:ng] = True
        gm = M.GlobalMesh(x=np.ascontiguousarray(x, np.float64), y=np.ascontiguousarray(y, np.float64), tri=np.ascontiguousarray(tri, np.int32), dirichlet=on_b,
                          neumann=np.zeros(x.size, bool), lat=M.polar_stereographic_lat(x, y), name="rect")
    elif kind == "shuffled":   # the small mesh with node and element numbers permuted at random
        g0 = cases.global_mesh("small")
        rng = np.random.default_rng(7)
        pn, pe = rng.permutation(g0.num_nodes), rng.permutation(g0.num_elements)
        inv = np.empty_like(pn); inv[pn] = np.arange(pn.size)
        gm = M.GlobalMesh(x=g0.x[pn].copy(), y=g0.y[pn].copy(), tri=np.ascontiguousarray(inv[g0.tri][pe].astype(np.int32)), dirichlet=g0.dirichlet[pn].copy(),
                          neumann=g0.neumann[pn].copy(), lat=g0.lat[pn].copy(), name="shuffled")
        ng = 0
    else:
        gm, p, g, lms, fields = cases.make_case(kind)
        return p, lms[0], fields[0], 0
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    lm = M.localize(gm, 1)[0]
    return p, lm, F.localize_fields(F.global_fields(gm, p, "arctic", C_fix, C_alea), lm, gm.num_nodes), ng


def _fe(kind, state=False):
    from nextsim_amd import dynamics
    p, lm, f, _ = _mesh(kind)
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    if state:
        fe.put_state(f)
    return fe, lm, f


def _refused(call, *texts, code=-4):
    from nextsim_amd import dynamics
    with pytest.raises(dynamics.NxsError) as e:
        call()
    assert e.value.code == code and all(t in str(e.value) for t in texts), (e.value.code, str(e.value))
    return True


def test_the_meshes_cover_the_kernels_edges():
    sizes = {k: _mesh(k)[1].num_nodes for k in MESHES}
    assert any(n % 2 for n in sizes.values()) and any(n % 2 == 0 for n in sizes.values()), sizes      # the v half by scalars, and by 16-byte pairs
    assert any(n < 2 * BLOCK for n in sizes.values()), sizes                                           # less than one block of the blend
    assert any(n > 2 * 2 * BLOCK and n % (2 * BLOCK) for n in sizes.values()), sizes                   # more than two blocks, a ragged last one


# ---- 1. the projection --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.MPP))
def test_the_projection_on_the_device_is_within_the_bound_of_the_host_body(name):
    from nextsim_amd import dynamics
    lat, lon = R.forward_points()
    m = dynamics.mapx_polar_north(**R.MPP[name])
    xh, yh = dynamics.mapx_forward(m, lat, lon, device=-1)
    xd, yd = dynamics.mapx_forward(m, lat, lon, device=0)
    bound = R.bound_forward(xh, yh, lat)
    ex, ey = np.abs(xd - xh), np.abs(yd - yh)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(bound > 0., np.maximum(ex, ey) / bound, 0.))
    print(f"mapx_forward {name}: largest |got - want| / bound = {worst:.3f}; largest |got - want| = {max(ex.max(), ey.max()):.3e} m")
    pole = lat == 90.
    assert pole.sum() >= 9 and R.same_bits(xd[pole], xh[pole]).all() and R.same_bits(yd[pole], yh[pole]).all()      # t = 0 on both sides
    assert (ex <= bound).all() and (ey <= bound).all(), (worst, lat[np.argmax(np.maximum(ex, ey) - bound)])
    low = lat <= 89.
    assert (bound[low] < 1e-9 * np.hypot(xh, yh)[low]).all()                                          # not vacuous: a relative 1e-9 at most up to 89 N


# ---- 2. without vectors the ingest is nxs_interp_grid_to_mesh ----------------------------------------------------------------------------------------
def _grid(lm, N=37, M_=29, descending_x=False, descending_y=True, seed=0, N_data=5):
    """a grid around the mesh's nodes, its data with NaN in it, and targets inside and outside its box"""
    rng = np.random.default_rng(seed)
    bx, by = lm.coord_x, lm.coord_y
    xs = np.linspace(bx.min() - 0.02 * np.ptp(bx), bx.max() + 0.02 * np.ptp(bx), N)
    ys = np.linspace(by.min() - 0.02 * np.ptp(by), by.max() + 0.02 * np.ptp(by), M_)
    if descending_x:
        xs = xs[::-1].copy()
    if descending_y:
        ys = ys[::-1].copy()
    data = rng.normal(size=(M_, N, N_data))
    data[M_ // 3:M_ // 3 + 4, N // 2 - 2:N // 2 + 2, 0] = np.nan
    rx, ry = bx + 0.013 * (xs[1] - xs[0]), by - 0.017 * (ys[1] - ys[0])
    far = 10. * (np.ptp(bx) + np.ptp(by))
    rx[0] -= far; ry[1] += far                                             # targets outside the grid, in x and in y
    rx[2], ry[2] = xs[-1], ys[-1]                                           # exactly on the last coordinate of both axes
    rx[3] = xs[-1]; ry[4] = ys[0]; rx[5] = xs[N // 2]
    return xs, ys, data, rx, ry


def _deinterleave(want, row, snap, Nn):
    """[Nn, N_data] of nxs_interp_grid_to_mesh -> {(snapshot, row name): [Nn]}"""
    return {(int(s), _abi.NF_ROWS[r]): want[:, j] for j, (r, s) in enumerate(zip(row, snap)) if r >= 0}


def _check_rows(fe, want, ctx):
    for w in (0, 1):
        names = [k for (s, k) in want if s == w]
        got = fe.forcing_get(w, names) if names else {}
        for k in names:
            assert np.array_equal(got[k], want[(w, k)]), (ctx, w, k)


INGEST = [dict(interp=1), dict(interp=0), dict(interp=2), dict(interp=1, descending_x=True, descending_y=False), dict(interp=0, descending_x=True),
          dict(interp=1, contours=True), dict(interp=1, row_major=True), dict(interp=1, N_data=1)]


@pytest.mark.parametrize("case", INGEST, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
@pytest.mark.parametrize("kind", ["tiny", "odd"])
def test_the_ingest_without_vectors_is_nxs_interp_grid_to_mesh_bit_for_bit(kind, case):
    from nextsim_amd.interp import InterpFromGridToMeshx
    case = dict(case)
    interp, contours, row_major, N_data = case.pop("interp"), case.pop("contours", False), case.pop("row_major", False), case.pop("N_data", 5)
    fe, lm, _ = _fe(kind)
    Nn = lm.num_nodes
    xs, ys, data, rx, ry = _grid(lm, seed=interp, N_data=N_data, **case)
    if contours:
        data = data[:-1, :-1]
    if row_major:
        data = np.ascontiguousarray(np.transpose(data, (1, 0, 2)))
    row = np.array([1, 4, -1, 2, 0][:N_data]) if N_data > 1 else np.array([3])          # V before U, a skipped column
    snap = np.array([1, 0, 0, 0, 1][:N_data])
    _refused(lambda: fe.forcing_ingest(1, xs, ys, data, row, snap, 1e8, interp, row_major), "no targets")
    fe.forcing_targets(1, rx, ry)
    want = InterpFromGridToMeshx(xs, ys, data, rx, ry, 1e8, interp, row_major)
    fe.forcing_ingest(1, xs, ys, data, row, snap, 1e8, interp, row_major)
    _check_rows(fe, _deinterleave(want, row, snap, Nn), (kind, case))
    assert want.shape == (Nn, N_data) and (want[:2] == 1e8).all() and np.isfinite(want).all()
    if not row_major:
        assert np.array_equal(fe.forcing_grid(), data, equal_nan=True)                   # nothing was asked of the grid data
    given = {(int(s), _abi.NF_ROWS[r]) for r, s in zip(row, snap) if r >= 0}
    for w in (0, 1):                                                                     # nothing else became present
        for k in _abi.NF_ROWS:
            if (w, k) not in given:
                _refused(lambda: fe.forcing_get(w, [k]), "is missing")
    fe.close()


# ---- 3. the rotation and the wrap are the host's bits -------------------------------------------------------------------------------------------------
def _host_forward(m):
    from nextsim_amd import dynamics

    def f(lat, lon):
        x, y = dynamics.mapx_forward(m, [lat], [lon], device=-1)
        return float(x[0]), float(y[0])
    return f


def _latlon_targets(lm, lat, lon, seed, cyclic_x):
    """node positions in (lon, lat): inside the grid box (the wrap column's interval among them) and outside it"""
    rng = np.random.default_rng(seed)
    Nn = lm.num_nodes
    lo, hi = min(lon[0], lon[-1]), max(lon[0], lon[-1]) + (abs(lon[-1] - lon[-2]) if cyclic_x else 0.)
    rx = rng.uniform(lo, hi, Nn)
    ry = rng.uniform(min(lat[0], lat[-1]), max(lat[0], lat[-1]), Nn)
    rx[0] = lo - 1.; ry[1] = max(lat[0], lat[-1]) + 3. * abs(lat[-1] - lat[-2])          # (beyond a wrap row too)
    if cyclic_x:
        rx[2:6] = hi - abs(lon[-1] - lon[-2]) * np.array([0.9, 0.5, 0.1, 0.])            # inside the wrap interval, and on its last coordinate
    return rx, ry


@pytest.mark.parametrize("cyclic", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("kind", ["tiny", "odd"])
def test_the_rotation_and_the_wrap_are_the_hosts_bits(kind, cyclic):
    from nextsim_amd.interp import InterpFromGridToMeshx
    case = R.transform_cases()["g33x72_rotation_only"]
    fe, lm, _ = _fe(kind)
    cx, cy = cyclic
    lat, lon, data = case["lat"], case["lon"], case["data"]
    rx, ry = _latlon_targets(lm, lat, lon, 5, cx)
    fe.forcing_targets(0, rx, ry)
    row, snap = ["wind_u", "wind_v", "ocean_v", "ssh", "ocean_u"], [0, 0, 1, 1, 1]
    vec = dict(pairs=case["pairs"], rotation_angle=case["rotation_angle"])
    assert all(not p[2] for p in case["pairs"])
    for rotate in (False, True):
        fe.forcing_ingest(0, lon, lat, data, row, snap, 1e8, 1, False, cx, cy, vec if rotate else None)
        grid = R.transform(data, lat, lon, lat, case["pairs"], None, case["rotation_angle"]) if rotate else data
        wgrid, wx, wy = R.wrap(grid, lon, lat, cx, cy)
        got = fe.forcing_grid()
        assert got.shape == wgrid.shape and R.same_bits(got, wgrid).all(), (kind, cyclic, rotate)
        want = InterpFromGridToMeshx(wx, wy, wgrid, rx, ry, 1e8, 1, False)
        rows = np.array([_abi.NF_ROWS.index(r) for r in row])
        _check_rows(fe, _deinterleave(want, rows, snap, lm.num_nodes), (kind, cyclic, rotate))
        assert (want[0] == 1e8).all() and (want[1] == 1e8).all()
        if cx:
            assert (want[2:6] != 1e8).all()                                              # the wrap interval is part of the grid
    assert _refused(lambda: fe.forcing_ingest(0, np.append(lon, 180.), np.append(lat, 92.5), data, row, snap, 1e8, 1, False, True, False), "only pixel centres", code=-1)
    fe.close()


# ---- 4. the east/north transform: the one tolerance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, cyclic_x", [("g33x72_pole_last", True), ("g5x8_pole_first_rotated", False), ("g5x8_per_point_pole_point", False), ("g5x8_no_pole", True),
                                            ("g2x2_pole_last", False)])
def test_the_east_north_transform_is_within_the_bound_of_the_host_body(name, cyclic_x):
    import math
    from nextsim_amd import dynamics
    from nextsim_amd.interp import InterpFromGridToMeshx
    case = R.transform_cases()[name]
    data, lat, lon, gy, pairs, ang = case["data"], case["lat"], case["lon"], case["grid_y"], case["pairs"], case["rotation_angle"]
    Mg, Ng, nd = data.shape
    m = dynamics.mapx_polar_north(**R.MPP[case["map"]])
    det = {}
    want = R.transform(data, lat, lon, gy, pairs, _host_forward(m), ang, case["per_point"], details=det)      # the host body
    # the bound per grid point and column
    B = np.zeros_like(data)
    biggest = 0.
    for k, (j0, j1, ew) in enumerate(pairs):
        if not ew:
            continue
        d = det[k]
        b = R.bound_east_north(d).reshape(Mg, Ng)
        held = d["d"] > 0.
        assert (d["rho"][held] >= 4. * d["d"][held]).all()                               # where the derivation holds
        capped = held & (d["lat_point"] <= 89.) & (d["speed"] >= 1.)
        assert capped.sum() >= 2 and (b.ravel()[capped] < 1e-6 * d["speed"][capped]).all(), (name, (b.ravel()[capped] / d["speed"][capped]).max())      # not vacuous
        biggest = max(biggest, (b.ravel()[capped] / d["speed"][capped]).max())
        pole = 0 if gy[0] == 90. else None
        pole = Mg - 1 if gy[Mg - 1] == 90. else pole
        if pole is not None:
            nxt = 1 if pole == 0 else Mg - 2
            vals = np.abs(data[nxt][:, [j0, j1]]).max() * math.sqrt(2.)
            b[pole, :] = b[nxt, :].max() + Ng * 2. * R.U * vals
        B[:, :, j0], B[:, :, j1] = b, b
        if ang != 0.:
            mix = (abs(math.cos(ang)) + abs(math.sin(ang))) * b + 6. * R.U * np.hypot(want[:, :, j0], want[:, :, j1])
            B[:, :, j0], B[:, :, j1] = mix, mix
    if case["per_point"]:      # an x-y grid: its own axes, positions in metres
        xs, ys = 1e5 * np.arange(-4., 4.), gy
    else:
        xs, ys = lon, lat
    kind = "odd" if Mg > 5 else "tiny"
    fe, lm, _ = _fe(kind)
    rx, ry = _latlon_targets(lm, ys, xs, 11, cyclic_x)
    fe.forcing_targets(2, rx, ry)
    row = (["wind_u", "wind_v", "ocean_u", "ocean_v", "ssh"] if nd == 5 else ["ocean_u", "ocean_v", "ssh"] if nd == 3 else ["wind_u", "wind_v"])
    snap = [1] * nd
    vec = dict(pairs=pairs, lat=lat, lon=lon, map=m, rotation_angle=ang, per_point=case["per_point"])
    fe.forcing_ingest(2, xs, ys, data, row, snap, 1e8, 1, False, cyclic_x, False, vec)
    got = fe.forcing_grid()
    wgrid, wx, wy = R.wrap(want, xs, ys, cyclic_x, False)
    bgrid = R.wrap(B, xs, ys, cyclic_x, False)[0]
    err = np.abs(got - wgrid)
    exact = bgrid == 0.                                                                  # scalar columns, pairs nothing is asked of, zero vectors, lat == 90 without a pole row
    assert R.same_bits(got[exact], wgrid[exact]).all(), (name, int((~R.same_bits(got, wgrid) & exact).sum()))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(exact, 0., err / bgrid)
    print(f"east/north {name}: largest |got - want| / bound = {ratio.max():.3f} on the grid; largest bound / speed on the capped points = {biggest:.3e}")
    assert (err <= bgrid).all(), (name, ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
    assert (err[~exact] > 0.).any() or Mg == 2                                           # (the device's functions are not glibc's: the bound is needed)
    # the node rows: the same bound carried through the bilinear weights, + the roundings of the four-term sum
    node_want = InterpFromGridToMeshx(wx, wy, wgrid, rx, ry, 1e8, 1, False)
    node_b = InterpFromGridToMeshx(wx, wy, bgrid, rx, ry, 0., 1, False) + 16. * R.U * InterpFromGridToMeshx(wx, wy, np.abs(wgrid), rx, ry, 0., 1, False)
    node_got = fe.forcing_get(1, row)
    worst = 0.
    for j, k in enumerate(row):
        e = np.abs(node_got[k] - node_want[:, j])
        assert (e <= node_b[:, j]).all(), (name, k, (e - node_b[:, j]).max())
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, np.nanmax(np.where(node_b[:, j] > 0., e / node_b[:, j], 0.)))
    print(f"east/north {name}: largest |got - want| / bound = {worst:.3f} at the nodes")
    fe.close()


def test_branches_that_are_not_built_are_refused():
    from nextsim_amd import dynamics
    case = R.transform_cases()["g5x8_no_pole"]
    fe, lm, _ = _fe("tiny")
    lat, lon, data = case["lat"], case["lon"], case["data"]
    rx, ry = _latlon_targets(lm, lat, lon, 1, False)
    fe.forcing_targets(0, rx, ry)
    row, snap = ["wind_u", "wind_v", "ocean_u", "ocean_v", "ssh"], [0] * 5
    m = dynamics.mapx_polar_north(**R.MPP["NpsNextsim"])
    base = dict(lat=lat, lon=lon, map=m)
    ing = lambda vec, row=row, **kw: fe.forcing_ingest(0, lon, lat, kw.pop("data", data), row, snap, 1e8, 1, kw.pop("row_major", False), False, False, vec)  # noqa: E731
    assert _refused(lambda: ing(dict(base, pairs=[(0, 1, True)], is_wav_dir=[0])), "wave direction", code=-1)
    assert _refused(lambda: ing(dict(base, pairs=[(0, 1, True)], gridded_rotation_angle=True)), "gridded_rotation_angle", code=-1)
    assert _refused(lambda: ing(dict(base, pairs=[(0, 1, True), (1, 2, True)])), "named twice", code=-1)
    assert _refused(lambda: ing(dict(base, pairs=[(0, 5, True)])), "names column 5", code=-1)
    assert _refused(lambda: ing(dict(base, pairs=[(0, 1, True)]), row=[None, "wind_v", "ocean_u", "ocean_v", "ssh"]), "is skipped", code=-1)
    assert _refused(lambda: ing(dict(pairs=[(0, 1, True)], map=m)), "latitudes and longitudes", code=-1)
    assert _refused(lambda: ing(dict(base, pairs=[(0, 1, True)]), data=np.ascontiguousarray(np.transpose(data, (1, 0, 2))), row_major=True), "row_major", code=-1)
    assert _refused(lambda: ing(dict(base, pairs=[(0, 1, True)] * 5)), "vector pairs", code=-1)
    ing(dict(base, pairs=[(0, 1, True)], gridded_rotation_angle=True, rotation_angle=0.2))      # with a rotation angle the reference never reaches that branch
    fe.close()


# ---- 5. the blend per group --------------------------------------------------------------------------------------------------------------------------
def _snapshots(f, Nn, Ne, seed=0):
    rng = np.random.default_rng(seed)
    f0 = {k: np.ascontiguousarray(f[k], np.float64) for k in ("wind", "ocean", "ssh", "element_depth")}
    f1 = dict(wind=f0["wind"] * 1.1 + rng.normal(0., 0.5, 2 * Nn), ocean=f0["ocean"] * 0.9 + rng.normal(0., 0.01, 2 * Nn), ssh=f0["ssh"] + rng.normal(0., 0.01, Nn),
              element_depth=f0["element_depth"])
    return f0, f1


@pytest.mark.parametrize("kind", MESHES)
def test_equal_coefficients_are_set_forcing_time_bit_for_bit_and_the_step_does_not_notice(kind):
    from nextsim_amd import dynamics
    p, lm, f, _ = _mesh(kind)
    Nn, Ne = lm.num_nodes, lm.num_elements
    f0, f1 = _snapshots(f, Nn, Ne)
    c0, c1 = 0.3125, 0.6875
    factor, bias = (0.9, 1.0, 1.0), (0., 0., 0.02)

    def stepped(route):
        fe = dynamics.FiniteElementDynamics(p)
        fe.set_mesh(lm); fe.put_state(f)
        route(fe)
        fe.step(); fe.synchronize()
        out = fe.get_state()
        launches = fe.timing()["substep_launches"]
        fe.close()
        return out, launches

    def old(fe):
        fe.set_forcing_pair(f0, f1)
        fe.set_forcing_time(c0, c1, factor, bias)

    def new_equal(fe):
        fe.set_forcing_pair(f0, f1)
        fe.set_forcing_time_rows({g: dict(mode="linear", fcoeff0=c0, fcoeff1=c1, factor=factor[k], bias=bias[k]) for k, g in enumerate(_abi.NF_GROUPS)})

    tab = {"wind": (R.LINEAR, 0.25, 0.75, 0.9, 0.), "ocean": (R.STEP, 0.1, 0.9, 1.0, 0.), "ssh": (R.LINEAR, 0.5, 0.5, 1.0, 0.02)}      # an hourly atmosphere beside a daily ocean
    blended = {g: R.blend(*tab[g], f0[g], f1[g]) for g in tab}

    def new_different(fe):
        fe.set_forcing_pair(f0, dict(f1, ocean=np.full(2 * Nn, np.nan)))                    # a STEP group never reads snapshot 1
        fe.set_forcing_time_rows({g: dict(mode=tab[g][0], fcoeff0=tab[g][1], fcoeff1=tab[g][2], factor=tab[g][3], bias=tab[g][4]) for g in tab})

    def numpy_different(fe):
        fe.set_forcing(dict(blended, element_depth=f0["element_depth"]))

    a, la = stepped(old)
    b, lb = stepped(new_equal)
    for k in STATE_KEYS:
        assert np.array_equal(a[k], b[k]), (kind, k)
    c, lc = stepped(new_different)
    d, ld = stepped(numpy_different)
    for k in STATE_KEYS:
        assert np.array_equal(c[k], d[k]), (kind, k)
    assert la == lb == lc == ld and np.isfinite(c["VT"]).all() and np.abs(c["VT"]).max() > 0 and not np.array_equal(a["VT"], c["VT"])


# ---- 6. call order, what goes with the mesh, device memory ---------------------------------------------------------------------------------------------
def _lin(groups=_abi.NF_GROUPS):
    return {g: dict(mode="linear", fcoeff0=0.25, fcoeff1=0.75) for g in groups}


def test_call_order_and_mixing_the_two_routes():
    from nextsim_amd import dynamics
    p, lm, f, _ = _mesh("tiny")
    Nn, Ne = lm.num_nodes, lm.num_elements
    f0, f1 = _snapshots(f, Nn, Ne)
    xs, ys, data, rx, ry = _grid(lm, N_data=5)
    fe = dynamics.FiniteElementDynamics(p)
    assert _refused(lambda: fe.set_forcing_time_rows(_lin()), "before set_mesh")
    fe.set_mesh(lm); fe.put_state(f)
    assert _refused(lambda: fe.forcing_ingest(0, xs, ys, data, [0, 1, 2, 3, 4], [0] * 5), "no targets")
    assert _refused(lambda: fe.set_forcing_time_rows(_lin()), "wind is LINEAR", "missing")
    assert _refused(lambda: fe.set_forcing_time_rows({"ssh": dict(mode="step")}), "ssh is STEP")
    assert _refused(lambda: fe.set_forcing_time_rows({"ssh": dict(mode=7)}), "unknown mode 7", code=-1)
    assert _refused(lambda: fe.forcing_get(0, ["ssh"]), "is missing") and _refused(lambda: fe.forcing_get(2, ["ssh"]), code=-1)
    assert _refused(lambda: fe.forcing_targets(4, rx, ry), "set = 4", code=-1)
    fe.forcing_targets(3, rx, ry)
    assert _refused(lambda: fe.forcing_ingest(3, xs, ys, data, [0] * 5, [0] * 5), "two columns", code=-1)
    assert _refused(lambda: fe.forcing_ingest(3, xs, ys, data, [0, 1, 2, 3, 5], [0] * 5), "row 5", code=-1)
    assert _refused(lambda: fe.forcing_ingest(3, xs, ys, data, [0, 1, 2, 3, 4], [0, 0, 2, 0, 0]), "snapshot 2", code=-1)
    assert _refused(lambda: fe.forcing_ingest(3, xs[:-3], ys, data, [0, 1, 2, 3, 4], [0] * 5), "1 or 0 more", code=-1)
    assert _refused(lambda: fe.forcing_ingest(3, xs, ys, data[:-1, :-1], [0, 1, 2, 3, 4], [0] * 5, cyclic_x=True), "only pixel centres", code=-1)
    # the ingest alone: snapshot 0 of everything, then STEP groups, the depth alone -- no set_forcing_pair at all
    fe.forcing_ingest(3, xs, ys, data, [0, 1, 2, 3, 4], [0] * 5)
    assert _refused(lambda: fe.set_forcing_time(0.5, 0.5), "before set_forcing_pair")      # the pair is not complete
    fe.set_forcing_time_rows({g: dict(mode="step") for g in _abi.NF_GROUPS})
    assert _refused(fe.step, code=-4)                                                       # the element depth is still missing
    fe.set_element_depth(f0["element_depth"])
    fe.step(); fe.synchronize()
    fe.forcing_ingest(3, xs, ys, data, [0, 1, 2, 3, 4], [1] * 5)
    fe.set_forcing_time(0.5, 0.5)                                                           # all ten half-rows by the ingest: the pair is there
    # mixing: the pair's rows with ingested ones
    fe2 = dynamics.FiniteElementDynamics(p)
    fe2.set_mesh(lm); fe2.put_state(f)
    fe2.set_forcing_pair(f0, f1)
    fe2.forcing_targets(0, rx, ry)
    fe2.forcing_ingest(0, xs, ys, data[:, :, 1:3], ["wind_v", "ssh"], [1, 0])
    from nextsim_amd.interp import InterpFromGridToMeshx
    want = InterpFromGridToMeshx(xs, ys, np.ascontiguousarray(data[:, :, 1:3]), rx, ry, 1e8, 1, False)
    g0, g1 = fe2.forcing_get(0), fe2.forcing_get(1)
    assert np.array_equal(g1["wind_v"], want[:, 0]) and np.array_equal(g0["ssh"], want[:, 1])
    assert np.array_equal(g0["wind_u"], f0["wind"][:Nn]) and np.array_equal(g0["wind_v"], f0["wind"][Nn:]) and np.array_equal(g1["wind_u"], f1["wind"][:Nn])
    assert np.array_equal(g1["ocean_v"], f1["ocean"][Nn:]) and np.array_equal(g1["ssh"], f1["ssh"])
    fe.close(); fe2.close()


def test_the_rows_go_with_the_mesh():
    from nextsim_amd import dynamics
    p, lm, f, _ = _mesh("tiny")
    p2, lm2, f2, _ = _mesh("toy")
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm)
    xs, ys, data, rx, ry = _grid(lm)
    fe.forcing_targets(0, rx, ry)
    fe.forcing_ingest(0, xs, ys, data, [0, 1, 2, 3, 4], [0] * 5)
    fe.set_params(p2); fe.set_mesh(lm2)
    xs, ys, data, rx, ry = _grid(lm2)
    assert _refused(lambda: fe.forcing_ingest(0, xs, ys, data, [0, 1, 2, 3, 4], [0] * 5), "no targets")
    assert _refused(lambda: fe.set_forcing_time_rows({"ssh": dict(mode="step")}), "missing")
    assert _refused(lambda: fe.forcing_get(0, ["ssh"]), "is missing")
    assert _refused(fe.forcing_grid, "no nxs_dyn_forcing_ingest")
    fe.close()
    # nxs_dyn_regrid: an identity regrid of the rectangle
    p, lm, f, ng = _mesh("odd")
    fe = dynamics.FiniteElementDynamics(p)
    fe.set_mesh(lm); fe.put_state(f)
    xs, ys, data, rx, ry = _grid(lm)
    fe.forcing_targets(1, rx, ry)
    fe.forcing_ingest(1, xs, ys, data, [0, 1, 2, 3, 4], [0] * 5)
    before = fe.forcing_get(0)
    prev = np.arange(1, lm.num_nodes + 1, dtype=np.float64)
    fe.regrid(lm, prev, ng, {k: f[k] for k in dynamics.REGRID_INPUTS}, (), moved=(lm.coord_x, lm.coord_y))
    assert _refused(lambda: fe.forcing_ingest(1, xs, ys, data, [0, 1, 2, 3, 4], [0] * 5), "no targets")
    assert _refused(lambda: fe.forcing_get(0, ["wind_u"]), "is missing")
    fe.forcing_targets(1, rx, ry)
    fe.forcing_ingest(1, xs, ys, data, [0, 1, 2, 3, 4], [0] * 5)
    again = fe.forcing_get(0)
    assert all(np.array_equal(before[k], again[k]) for k in before)
    fe.close()


def _free_bytes():
    from nextsim_amd import dynamics
    L = dynamics.load_library()
    L.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    a, b = C.c_size_t(), C.c_size_t()
    assert L.hipMemGetInfo(C.byref(a), C.byref(b)) == 0
    return a.value


def test_handles_give_the_pool_back():
    """four cycles of create / targets / ingest (the grid buffers grow) / blend / destroy leave the free device memory where it settled"""
    from nextsim_amd import dynamics
    gm, p, g, lms, fields = cases.make_case("10km")
    lm, f = lms[0], fields[0]
    case = R.transform_cases()["g33x72_pole_last"]
    m = dynamics.mapx_polar_north(**R.MPP["NpsNextsim"])
    rx, ry = _latlon_targets(lm, case["lat"], case["lon"], 3, True)
    vec = dict(pairs=case["pairs"], lat=case["lat"], lon=case["lon"], map=m)

    def cycle():
        fe = dynamics.FiniteElementDynamics(p)
        fe.set_mesh(lm)
        fe.forcing_targets(0, rx, ry)
        fe.forcing_ingest(0, case["lon"], case["lat"], case["data"][:, :, :2], ["wind_u", "wind_v"], [0, 0], vectors=dict(vec, pairs=case["pairs"][:1]))
        fe.forcing_ingest(0, case["lon"], case["lat"], case["data"], ["wind_u", "wind_v", "ocean_u", "ocean_v", "ssh"], [1, 1, 0, 0, 0], cyclic_x=True, vectors=vec)
        fe.set_forcing_time_rows({"wind": dict(mode="linear", fcoeff0=0.5, fcoeff1=0.5), "ssh": dict(mode="step")})
        fe.synchronize()
        fe.close()
    for _ in range(3):
        cycle()
    mid = _free_bytes()
    for _ in range(4):
        cycle()
    end = _free_bytes()
    assert 4 * lm.num_nodes * 8 * 12 > 8 << 20 and mid - end < 3 << 20, (mid, end, (mid - end) / 4)


# ---- 7. a handle that never calls the new entry points ---------------------------------------------------------------------------------------------------
def test_a_handle_that_never_calls_the_new_entry_points_allocates_nothing_new():
    """the old route twice in a row costs the same device memory both times, and no more than the same handle costs with the new calls left out: the NodalForcing
    pool is made by nxs_dyn_forcing_targets / _ingest alone (the step bits and the launch count of the old route are held by the test above)"""
    from nextsim_amd import dynamics
    gm, p, g, lms, fields = cases.make_case("10km")
    lm, f = lms[0], fields[0]
    Nn, Ne = lm.num_nodes, lm.num_elements
    f0, f1 = _snapshots(f, Nn, Ne)
    xs, ys, data, rx, ry = _grid(lm, N=181, M_=141, N_data=5)

    def cost(new):
        start = _free_bytes()
        fe = dynamics.FiniteElementDynamics(p)
        fe.set_mesh(lm); fe.put_state(f)
        fe.set_forcing_pair(f0, f1)
        fe.set_forcing_time(0.5, 0.5)
        if new:
            fe.forcing_targets(0, rx, ry)
            fe.forcing_ingest(0, xs, ys, data, [0, 1, 2, 3, 4], [0] * 5)
        fe.step(); fe.synchronize()
        used = start - _free_bytes()
        fe.close()
        return used
    cost(False)                                  # (the first handle of the process pays for the runtime's own pools)
    a, b, c = cost(False), cost(False), cost(True)
    assert a == b, (a, b)
    assert c >= a + 2 * Nn * 8 - (2 << 20), (a, c)      # the targets and the grid came on top (to the allocator's granularity)
