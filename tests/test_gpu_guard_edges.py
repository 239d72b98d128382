"""The guards of a run -- k_check_fields, k_check_wave_stress (nxs_dyn_check_fields_fast) and k_regrid_partials, k_regrid_final
(nxs_dyn_check_regridding) -- against oracle.pyoracle.OracleRank.check_fields_fast() / .check_regridding() on the same state, at the places
where such a kernel goes wrong without anybody noticing: the first and last lane of a wave, the first and last thread of a block, the ragged
last block, the v half of a nodal vector, both homes of M_damage, values on and one ulp beyond a bound, the second trip of the grid-stride
loop (Ne > n_partials * BLOCK) and NaN geometry.  Single rank; every test prints what it measures.

The extrema of checkRegridding are PLANTED: one node is moved through M_UM so that one chosen element becomes the unique smallest angle / the
unique smallest (negative) Jacobian / the unique largest Jacobian.  Which element that is, and that the runner-up is at least 1 % away, is
computed by the numpy restatement below (_geometry), which is itself held against the oracle's min_angle and flip.  The largest Jacobian
only reaches the result through the sign test of flip (FE.cpp:1838: min <= 0 && max >= 0), so it is planted in the MIRRORED mesh (UM = -2 x:
every Jacobian negative, flip = 0) where the one positive Jacobian decides flip = 1.
min_angle is held to the bound of tests/test_gpu_parity.py: |device - oracle| <= 1e-10 * oracle."""
import ctypes as C
import time

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

ANGLE_RTOL = 1e-10                 # tests/test_gpu_parity.py, test_check_regridding_and_fields_fast
#            name           lo   hi    (checkFieldsFast, FE.cpp:14536-14655)
ELEMENT_FIELDS = (("thick", 0., 50.), ("snow_thick", 0., 10.), ("conc", 0., 1.), ("damage", 0., 1.), ("ridge_ratio", 0., 1.))
YOUNG_FIELDS = (("h_young", 0., 2.), ("hs_young", 0., 2.), ("conc_young", 0., 1.))
BIG = "h13000"                     # the coarsest disc (edge a multiple of 100 m) with more than 1024 * 256 triangles: 262 842 (h13100: 258 635)


# ---- the rig: a handle and an oracle rank on the same state ---------------------------------------------------------------------------

class Rig:
    def __init__(self, kind="small", forcing=False, case=None, **over):
        from nextsim_amd import dynamics
        from oracle import pyoracle as O
        gm, p, g, lms, fields = case if case is not None else cases.make_case(kind, **over)
        self.lm, self.p, self.f = lms[0], p, fields[0]
        self.fe = dynamics.FiniteElementDynamics(p)
        self.fe.set_mesh(self.lm)
        self.fe.put_state(self.f)
        if forcing:
            self.fe.set_forcing(self.f)
        self.ref = O.OracleRank(self.lm, p, self.f)
        self.Ne, self.Nn = self.lm.num_elements, self.lm.num_nodes
        launch = self.fe.debug_array("guard_launch")            # the library's own launch shape, not a number guessed here
        self.BLOCK, self.n_partials = int(launch[0]), int(launch[1])
        assert self.BLOCK % 64 == 0 and self.n_partials == min(-(-self.Ne // self.BLOCK), 1024)

    def upload(self, *keys):
        """The oracle's arrays `keys` to the device, nothing else (put_state with NULL members)."""
        from nextsim_amd import _abi
        s = _abi.State()
        for k in keys:
            setattr(s, k, _abi.dptr(self.ref.arr[k]))
        self.fe._chk(self.fe.L.nxs_dyn_put_state(self.fe.h, C.byref(s)))

    def flags(self):
        return self.fe.checkFieldsFast(), self.ref.check_fields_fast()

    def poisoned(self, key, index, value):
        """(device flag, oracle flag) with ref.arr[key][index] = value on both sides; the entry is restored afterwards, on both sides."""
        a = self.ref.arr[key]
        keep = a[index]
        a[index] = value
        self.upload(key)
        got = self.flags()
        a[index] = keep
        self.upload(key)
        return got

    def regridding(self, um=None):
        """((min_angle, flip, regrid) of the device, of the oracle) with M_UM = um on both sides."""
        if um is not None:
            self.ref.arr["UM"][:] = um
            self.upload("UM")
        return self.fe.checkRegridding(), self.ref.check_regridding()

    def close(self):
        self.fe.close()


def element_positions(Ne, BLOCK):
    last = (Ne // BLOCK) * BLOCK
    return [i for i in (0, 63, 64, BLOCK - 1, BLOCK, last - 1, last, Ne - 1) if 0 <= i < Ne]


def sweep_cases(Ne, Nn, BLOCK, young):
    """A1: (key, index, bad value) -- every checked field at every position, one bad value at a time; M_VT in the u half alone and in the v half alone."""
    for name, lo, hi in ELEMENT_FIELDS + (YOUNG_FIELDS if young else ()):
        for i in element_positions(Ne, BLOCK):
            yield name, i, hi + 0.5
    for nd in (0, 63, 64, Nn - 1):
        yield "VT", nd, np.nan
        yield "VT", nd + Nn, np.nan


def bound_cases(young):
    """A2: (key, value, must flag) for an element field."""
    for name, lo, hi in ELEMENT_FIELDS + (YOUNG_FIELDS if young else ()):
        for v in (lo, -0.0, hi):
            yield name, v, 0
        for v in (np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf), np.inf, -np.inf, np.nan):
            yield name, v, 1


SPEED_CASES = (((5., 0.), 0), ((0., -5.), 0), ((3., 4.), 0), ((np.nextafter(5., np.inf), 0.), 1),
               ((np.nan, 0.), 1), ((0., np.nan), 1), ((np.inf, np.nan), 1))


# ---- A1 .. A6: the crash flag ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["small", "toy"])
def test_crash_flag_position_sweep(kind):
    """One bad entry at lane 0 / 63 / 64, at the last thread of the first block, the first of the second, both sides of the start of the
    ragged last block and the very last entry; toy has 2368 triangles (9 blocks and a quarter)."""
    r = Rig(kind)
    assert r.p.ice_cat_type == 1 and r.flags() == (0, 0)
    if kind == "toy":
        assert r.Ne == 2368 and r.Ne % r.BLOCK != 0
    n = 0
    for key, i, v in sweep_cases(r.Ne, r.Nn, r.BLOCK, True):
        got = r.poisoned(key, i, v)
        assert got == (1, 1), (key, i, v, got)
        assert r.flags() == (0, 0), ("after restoring", key, i)
        n += 1
    print(f"{kind}: Ne={r.Ne} Nn={r.Nn} BLOCK={r.BLOCK}: {n} single bad entries, every one flagged by the device and the oracle, 0 after restoring")
    r.close()


def test_crash_flag_bounds():
    """On a bound is good, one ulp beyond is bad (the lower one is the smallest denormal below zero), so are the infinities and NaN; |v| = 5 is
    good in three shapes -- (3, 4) needs hypot to be exact there --, one ulp more is bad, a NaN in either half is bad."""
    r = Rig("small")
    n = 0
    for key, v, want in bound_cases(True):
        got = r.poisoned(key, r.Ne - 1, v)
        print(f"{key}[Ne-1] = {v!r}: device {got[0]} oracle {got[1]}")
        assert got == (want, want), (key, v, got)
        n += 1
    for nd in (r.Nn - 1, 64):
        for (u, v), want in SPEED_CASES:
            vt = r.ref.arr["VT"]
            keep = vt[nd], vt[nd + r.Nn]
            vt[nd], vt[nd + r.Nn] = u, v
            r.upload("VT")
            got = r.flags()
            vt[nd], vt[nd + r.Nn] = keep
            r.upload("VT")
            print(f"VT[{nd}] = ({u!r}, {v!r}): device {got[0]} oracle {got[1]}")
            assert got == (want, want), (nd, u, v, got)
            n += 1
    assert r.flags() == (0, 0)
    print(f"{n} bound cases agree")
    r.close()


def test_crash_flag_ignores_the_young_ice_fields_without_the_category():
    """ice_cat_type classic: the state still carries the three young-ice arrays, nobody looks at them (FE.cpp:14589); the other fields still count."""
    r = Rig("small", ice_cat_type=0)
    assert r.p.ice_cat_type == 0 and r.flags() == (0, 0)
    for name, lo, hi in YOUNG_FIELDS:
        for i in (0, r.Ne - 1):
            for v in (hi + 0.5, -1.0, np.nan):
                got = r.poisoned(name, i, v)
                assert got[1] == 0, "the oracle decides: classic does not check the young ice"
                assert got == (0, 0), (name, i, v, got)
    assert r.poisoned("conc", r.Ne - 1, 1.5) == (1, 1)
    print("classic: 18 out-of-range young-ice entries raise no flag on either side, conc still does")
    r.close()


@pytest.mark.parametrize("dyn", ["bbm", "evp"])
def test_crash_flag_reads_damage_where_it_lives(dyn):
    """Under BBM the sub-step loop leaves M_damage in its element records and the array goes stale; put_state brings it home to the array
    (the records then go stale).  A guard reading the wrong home sees, in turn:
      before any step and after a put: the array is current -- 1.5 at Ne-1 must flag;
      stepped from damage[Ne-1] = 1.5: still out of range afterwards (it heals by dt / 25 days only) -- must flag;
      stepped from one ulp above 1 and from -0.5: healed into range by the step, the STALE ARRAY still holds the bad value -- the oracle
      decides (0 on this state), a kernel that reads the array under BBM says 1;
      a healthy step, then damage[Ne-1] = 1.5 by put_state: the array is current and bad, the STALE RECORDS hold the good value -- 1."""
    r = Rig("small", forcing=True, dynamics_type=dyn)
    last = r.Ne - 1
    assert r.flags() == (0, 0)
    assert r.poisoned("damage", last, 1.5) == (1, 1)                       # before any step
    start = {k: v.copy() for k, v in r.ref.arr.items()}
    for bad in (1.5, np.nextafter(1., 2.), -0.5):
        for k in r.ref.arr:
            r.ref.arr[k][:] = start[k]
        r.ref.arr["damage"][last] = bad
        r.fe.put_state(r.ref.arr)
        assert r.flags() == (1, 1)
        r.fe.step(); r.ref.step(); r.fe.synchronize()
        got = r.flags()
        print(f"{dyn}: damage[Ne-1] = {bad!r} -> one step -> oracle's damage {r.ref.arr['damage'][last]!r}: device flag {got[0]} oracle {got[1]}")
        assert got[0] == got[1]
        if bad == 1.5:
            assert got == (1, 1)
    for k in r.ref.arr:
        r.ref.arr[k][:] = start[k]
    r.fe.put_state(r.ref.arr)
    r.fe.step(); r.ref.step(); r.fe.synchronize()
    assert r.flags() == (0, 0)
    assert r.poisoned("damage", last, 1.5) == (1, 1)                       # the array is current again, the records are not
    assert r.flags() == (0, 0)
    r.close()


def test_crash_flag_of_the_wave_stress():
    """k_check_wave_stress: a NaN in M_tau_wi, the u half alone and the v half alone, at the wave and block edges of the nodes."""
    r = Rig("small")
    Nn = r.Nn
    tau = 0.01 * np.random.default_rng(5).standard_normal(2 * Nn)
    r.fe.set_wave_stress(tau)
    assert r.fe.checkFieldsFast() == 0
    nodes = sorted({0, 63, 64, r.BLOCK - 1, r.BLOCK, (Nn // r.BLOCK) * r.BLOCK - 1, (Nn // r.BLOCK) * r.BLOCK, Nn - 1})
    assert {0, 63, 64, Nn - 1} <= set(nodes)
    for nd in nodes:
        for half in (0, Nn):
            bad = tau.copy(); bad[nd + half] = np.nan
            r.fe.set_wave_stress(bad)
            assert r.fe.checkFieldsFast() == 1, (nd, half)
            r.fe.set_wave_stress(None)
            assert r.fe.checkFieldsFast() == 0, ("detached", nd, half)
    print(f"Nn={Nn}: NaN at nodes {nodes}, u half and v half: 1 while attached, 0 once detached")
    r.close()


def _strip_case():
    """A strip whose every vertex lies on the boundary (cases.rect_mesh without interior vertices): Ne = Nn - 2 < Nn."""
    from nextsim_amd import forcing as F, mesh as M
    x, y, tri, nb = cases.rect_mesh(0, 0, L=400e3, H=40e3)
    Nn = x.size
    assert tri.shape[0] == Nn - 2
    gm = M.GlobalMesh(x=x, y=y, tri=tri, dirichlet=np.ones(Nn, bool), neumann=np.zeros(Nn, bool), lat=M.polar_stereographic_lat(x, y), name="strip")
    p, C_fix, C_alea = F.scale_params_to_mesh(F.default_params(), gm, alea_factor=0.33)
    g = F.global_fields(gm, p, "arctic", C_fix, C_alea)
    lms = M.localize(gm, 1)
    return gm, p, g, lms, [F.localize_fields(g, lms[0], Nn)]


def test_crash_flag_on_a_mesh_with_more_nodes_than_elements():
    """The launch covers max(Ne, Nn): the nodes behind the last element are still looked at."""
    r = Rig(case=_strip_case())
    assert r.Nn > r.Ne and r.flags() == (0, 0)
    for idx in (r.Nn - 1, 2 * r.Nn - 1, r.Ne, r.Ne + r.Nn):
        assert r.poisoned("VT", idx, np.nan) == (1, 1), idx
    assert r.poisoned("conc", r.Ne - 1, 1.5) == (1, 1)
    assert r.flags() == (0, 0)
    print(f"strip: Ne={r.Ne} Nn={r.Nn}: a NaN at node Nn-1 (u, v) and at node Ne (u, v) flags")
    r.close()


# ---- A7 .. A9: checkRegridding ---------------------------------------------------------------------------------------------------------------

def _geometry(lm, um):
    """numpy restatement of minAngles (FE.cpp:1758-1768) and of flip's Jacobians (FE.cpp:1824-1839): per element."""
    Nn = lm.num_nodes
    t = lm.indices.reshape(-1, 3).astype(np.int64) - 1
    vx = lm.coord_x[t] + 1. * um[t]; vy = lm.coord_y[t] + 1. * um[t + Nn]
    with np.errstate(all="ignore"):
        s = np.sort(np.stack([np.hypot(vx[:, 1] - vx[:, 0], vy[:, 1] - vy[:, 0]), np.hypot(vx[:, 2] - vx[:, 1], vy[:, 2] - vy[:, 1]),
                              np.hypot(vx[:, 2] - vx[:, 0], vy[:, 2] - vy[:, 0])], 1), 1)
        ang = np.arccos((s[:, 1] ** 2 + s[:, 2] ** 2 - s[:, 0] ** 2) / (2 * s[:, 1] * s[:, 2])) * 45.0 / np.arctan(1.0)
        jac = (vx[:, 1] - vx[:, 0]) * (vy[:, 2] - vy[:, 0]) - (vx[:, 2] - vx[:, 0]) * (vy[:, 1] - vy[:, 0])
    return ang, jac


def _unique_extremum(values, sign):
    """(index, margin) of the smallest (sign = +1) / largest (-1) value; margin = distance to the runner-up over |extremum|."""
    v = sign * values
    k = int(np.argmin(v))
    two = np.partition(v, 1)[:2]
    return k, float((two[1] - two[0]) / abs(two[0]))


def _plant(lm, base_um, t, what, accept):
    """M_UM that moves ONE vertex of element t so that an accepted element becomes the unique extremum `what` ("angle": one side shrunk to a
    tenth; "min_jac" / "max_jac": the vertex pushed through the opposite edge), the runner-up at least 1 % away.  The moved vertex's whole fan
    changes, so the candidates (which vertex, how far) are tried until the restatement says the extremum sits in an accepted element --
    element t itself if possible.  Returns um, the extremum's element, its margin."""
    Nn = lm.num_nodes
    tri = lm.indices.reshape(-1, 3).astype(np.int64) - 1
    px = lm.coord_x + base_um[:Nn]; py = lm.coord_y + base_um[Nn:]
    found = None
    for far in ((0.9,) if what == "angle" else (1.5, 1.25, 2.0, 2.5)):
        for i in range(3):
            for j in (((i + 1) % 3, (i + 2) % 3) if what == "angle" else ((i + 1) % 3,)):
                a, b, c = tri[t, i], tri[t, j], tri[t, 3 - i - j]
                um = base_um.copy()
                if what == "angle":                      # a -> a + 0.9 (b - a)
                    dx, dy = far * (px[b] - px[a]), far * (py[b] - py[a])
                else:                                    # a -> through its foot on the line b c, `far` times the distance
                    ex, ey = px[c] - px[b], py[c] - py[b]
                    s = ((px[a] - px[b]) * ex + (py[a] - py[b]) * ey) / (ex * ex + ey * ey)
                    dx, dy = far * (px[b] + s * ex - px[a]), far * (py[b] + s * ey - py[a])
                um[a] += dx; um[a + Nn] += dy
                ang, jac = _geometry(lm, um)
                k, margin = _unique_extremum(ang if what == "angle" else jac, -1 if what == "max_jac" else +1)
                # a Jacobian extremum must DECIDE flip: the only element of its sign
                alone = what == "angle" or ((jac[k] < 0 and (jac < 0).sum() == 1) if what == "min_jac" else (jac[k] > 0 and (jac > 0).sum() == 1))
                if margin >= 0.01 and accept(k) and alone and (found is None or (k == t and found[1] != t)):
                    found = (um, k, margin)
                if found is not None and found[1] == t:
                    return found
    assert found is not None, f"no unique {what} could be planted around element {t}"
    return found


def _same_regridding(got, want, what):
    dev = abs(got[0] - want[0]) / abs(want[0]) if np.isfinite(want[0]) and want[0] != 0 else (0.0 if (got[0] == want[0] or (np.isnan(got[0]) and np.isnan(want[0]))) else np.inf)
    print(f"{what}: device (min_angle, flip, regrid) = {got}, oracle {want}, |d min_angle| / min_angle = {dev:.3e} (bound {ANGLE_RTOL:.0e})")
    assert got[1:] == want[1:], what
    assert dev <= ANGLE_RTOL, what
    return dev


@pytest.mark.parametrize("kind", ["toy", "small"])
def test_planted_extrema_of_check_regridding(kind):
    r = Rig(kind)
    B, Ne, Nn = r.BLOCK, r.Ne, r.Nn
    zero = np.zeros(2 * Nn)
    mirror = np.concatenate([-2. * r.lm.coord_x, np.zeros(Nn)])          # x -> -x: every Jacobian changes its sign
    healthy = _same_regridding(*r.regridding(zero), "healthy")
    ang0, jac0 = _geometry(r.lm, zero)
    assert abs(ang0.min() - r.ref.check_regridding()[0]) <= 1e-12 * ang0.min() and jac0.min() > 0
    got, want = r.regridding(mirror)
    _same_regridding(got, want, "mirrored")
    assert want[1] == 0 and _geometry(r.lm, mirror)[1].max() < 0          # no positive Jacobian: no flip
    worst = healthy
    for t in (0, B - 1, B, Ne - 1):
        block = t // B
        accept = lambda k: k // B == block                                # noqa: E731
        for what, base in (("angle", zero), ("min_jac", zero), ("max_jac", mirror)):
            um, k, margin = _plant(r.lm, base, t, what, accept)
            ang, jac = _geometry(r.lm, um)
            got, want = r.regridding(um)
            print(f"{kind}: {what} planted around element {t}: extremum in element {k} (block {k // B}), runner-up {100 * margin:.1f} % away")
            worst = max(worst, _same_regridding(got, want, f"{kind} {what} @ {t}"))
            assert k // B == block and margin >= 0.01
            if what == "angle":
                assert abs(want[0] - ang[k]) <= 1e-12 * ang[k] and want[0] < 0.5 * ang0.min() and want[2] == 1
            else:
                assert want[1] == 1 and want[2] == 1                      # without this element there is no flip: it decides
                assert (jac < 0).sum() == 1 if what == "min_jac" else (jac > 0).sum() == 1
    # regrid_angle just above and just below the true minimum angle of the healthy mesh
    got, want = r.regridding(zero)
    for factor, expect in ((1.005, 1), (0.995, 0)):
        p = r.p.copy(); p.regrid_angle = factor * want[0]
        r.fe.set_params(p); r.ref.params.regrid_angle = p.regrid_angle
        g2, w2 = r.regridding()
        worst = max(worst, _same_regridding(g2, w2, f"{kind} regrid_angle = {factor} * min_angle"))
        assert w2[2] == expect and w2[1] == 0
    print(f"{kind}: worst |d min_angle| / min_angle = {worst:.3e}")
    r.close()


@pytest.fixture(scope="module")
def big_rig():
    """The large mesh is generated once for the module."""
    t0 = time.time()
    r = Rig(BIG)
    yield r, time.time() - t0
    r.close()


def test_extrema_beyond_one_pass_of_the_grid(big_rig):
    """n_partials = min(blocks, 1024): from Ne > 1024 * BLOCK on the blocks walk the elements a second time.  The extremum is planted in that second
    trip (index >= 1024 * BLOCK: around the first element of the trip and around the very last element)."""
    t0 = time.time()
    r, t_setup = big_rig
    B, Ne, Nn = r.BLOCK, r.Ne, r.Nn
    assert r.n_partials == 1024 and Ne > 1024 * B
    assert Ne < 1.01 * 1024 * B, "the coarsest mesh that takes the second trip"
    zero = np.zeros(2 * Nn)
    got, want = r.regridding(zero)
    worst = _same_regridding(got, want, "healthy")
    assert got[1] == 0 and want[1] == 0
    for t in (1024 * B, Ne - 1):
        for what in ("angle", "min_jac"):
            um, k, margin = _plant(r.lm, zero, t, what, lambda k: k >= 1024 * B)
            got, want = r.regridding(um)
            print(f"{what} planted around element {t}: extremum in element {k} >= {1024 * B}, runner-up {100 * margin:.1f} % away")
            worst = max(worst, _same_regridding(got, want, f"{what} @ {t}"))
            assert k >= 1024 * B and margin >= 0.01 and want[2] == 1 and want[1] == (what == "min_jac")
    r.regridding(zero)
    print(f"{BIG}: Ne={Ne} > 1024 * {B}; worst |d min_angle| / min_angle = {worst:.3e}; setup {t_setup:.1f} s, test {time.time() - t0:.1f} s")


def test_crash_flag_beyond_the_first_thousand_blocks(big_rig):
    """The same mesh, the crash flag: the launch of k_check_fields is not capped, its last blocks are blocks 1024 .. 1026."""
    r, _ = big_rig
    assert r.flags() == (0, 0)
    for key, i in (("conc", r.Ne - 1), ("thick", 1024 * r.BLOCK), ("VT", r.Nn - 1), ("VT", 2 * r.Nn - 1)):
        assert r.poisoned(key, i, np.nan) == (1, 1), (key, i)
    assert r.flags() == (0, 0)


def _coincide(lm, um, v, onto):
    """um that puts vertex v exactly (bit for bit) where vertex `onto` is."""
    Nn = lm.num_nodes
    for coord, off in ((lm.coord_x, 0), (lm.coord_y, Nn)):
        target = coord[onto] + 1. * um[onto + off]
        d = target - coord[v]
        for _ in range(64):
            if coord[v] + 1. * d == target:
                break
            d = np.nextafter(d, np.inf if coord[v] + 1. * d < target else -np.inf)
        assert coord[v] + 1. * d == target
        um[v + off] = d


@pytest.mark.parametrize("kind", ["toy", "small"])
def test_nan_geometry(kind):
    """std::min_element / max_element start from element 0: a NaN angle or Jacobian THERE is the result (min_angle NaN, no flip, no regrid from it),
    a NaN anywhere else loses every comparison and is skipped.  (a) a NaN vertex, (b) three coincident vertices (0 / 0 in the angle, a zero
    Jacobian), at element 0 and at element Ne-1."""
    r = Rig(kind)
    Nn, Ne = r.Nn, r.Ne
    tri = r.lm.indices.reshape(-1, 3).astype(np.int64) - 1
    assert not set(tri[0]) & set(tri[Ne - 1])
    for e in (0, Ne - 1):
        um = np.zeros(2 * Nn); um[tri[e, 1]] = np.nan; um[tri[e, 1] + Nn] = np.nan
        got, want = r.regridding(um)
        ang, jac = _geometry(r.lm, um)
        assert np.isnan(ang[e]) and np.isnan(jac[e])
        assert np.isnan(want[0]) == (e == 0) and want[1] == 0
        _same_regridding(got, want, f"{kind}: NaN vertex in element {e}")
        um = np.zeros(2 * Nn)
        _coincide(r.lm, um, tri[e, 1], tri[e, 0]); _coincide(r.lm, um, tri[e, 2], tri[e, 0])
        got, want = r.regridding(um)
        ang, jac = _geometry(r.lm, um)
        assert np.isnan(ang[e]) and jac[e] == 0.
        assert np.isnan(want[0]) == (e == 0) and want[1] == 1 and want[2] == 1
        if e != 0:
            assert want[0] == 0.                                           # the neighbours have a side of length 0: acos(1)
        _same_regridding(got, want, f"{kind}: coincident vertices in element {e}")
    # a NaN in the x coordinate alone, of another vertex of element 0
    um = np.zeros(2 * Nn); um[tri[0, 0]] = np.nan
    _same_regridding(*r.regridding(um), f"{kind}: NaN x of the first vertex of element 0")
    got, want = r.regridding(np.zeros(2 * Nn))
    _same_regridding(got, want, f"{kind}: healthy again")
    assert np.isfinite(got[0])
    r.close()
