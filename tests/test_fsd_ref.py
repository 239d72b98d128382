"""nxs_fsd_bins against the restated tables of initFsd() (tests/fsd_ref.py), and invariants of the restatement itself -- they catch a wrong restatement
before the GPU tests compare the kernels with it (tests/test_gpu_fsd.py).  No device."""
import math

import numpy as np
import pytest

import fsd_ref as R
from nextsim_amd import dynamics

EPS = 2. ** -52


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n", [1, 2, 12])
@pytest.mark.parametrize("fsd_type", [R.CONSTANT_SIZE, R.CONSTANT_AREA])
@pytest.mark.parametrize("dmin,width", [(10., 10.), (7.3, 12.7)])
def test_bins_are_the_restated_tables(fsd_type, n, scaled, dmin, width):
    got = dynamics.fsd_bins(fsd_type, n, dmin, width, scaled)
    want = R.fsd_tables(fsd_type, n, dmin, width, scaled)                                # std::pow(x, 2) as x * x
    libm = R.fsd_tables(fsd_type, n, dmin, width, scaled, pow2=lambda x: math.pow(x, 2.))  # ... and as the libm's pow
    for k in R.fsd_tables(0, 1, 1., 1., 0):
        if k == "alpha_merge":
            assert np.array_equal(got[k], want[k])
        else:
            assert _bits(got[k], want[k]), k
    # The library writes x * x: a compiler folds std::pow(x, 2) into the multiplication at -O1 and above, so that is what the reference's build computes, and a
    # product is correctly rounded by definition.  Where this libm's pow(x, 2.) is correctly rounded too the two forms agree; the count says whether it is here.
    differ = sum(int(not _bits(want[k], libm[k])) for k in want if k != "alpha_merge")
    print(f"fsd_type {fsd_type} n={n} scaled={scaled}: tables in which pow(x, 2.) of the libm and x * x differ: {differ}")
    a = got["alpha_merge"]
    for kx in range(n):
        for ky in range(kx + 1):
            assert 1 <= a[kx, ky] <= n, (kx, ky, a[kx, ky])            # weldingRoach indexes tmp_conc_fsd[a - 1] with these
    assert ((a == -999) | ((a >= 1) & (a <= n))).all()
    # what the tables are: contiguous bins from the smallest floe size upwards
    assert got["bin_low_limits"][0] == dmin and np.all(got["bin_up_limits"][:-1] == got["bin_low_limits"][1:])
    assert np.all(got["area_scaled_up"][:-1] == got["area_scaled_low"][1:]) and got["area_scaled_low"][0] == 0.


def test_bins_refusals():
    from nextsim_amd import _abi
    L = dynamics.load_library()
    t = _abi.FsdTables()
    assert L.nxs_fsd_bins(0, 0, 10., 10., 1, t) == -1 and L.nxs_fsd_bins(2, 3, 10., 10., 1, t) == -1 and L.nxs_fsd_bins(0, 3, 10., 10., 1, None) == -1
    assert L.nxs_fsd_bins(1, 40, 10., 10., 1, t) == 0                  # every output NULL: nothing is written; the cap is the kernels', not the tables'


@pytest.mark.parametrize("young", [False, True])
@pytest.mark.parametrize("n", [1, 2, 12, 16])
def test_update_leaves_the_sum_of_the_bins_at_ctot(n, young):
    Ne = 700
    cfg = R.default_config(n, R.standard_tables(n), young, distinguish_mech_fsd=1)
    st = R.update_inputs(n, Ne, young)
    before = R.copy_state(st)
    branch = R.update_fsd(st, cfg)
    for b in R.UPDATE_BRANCHES:
        assert (branch == b).mean() >= 0.05, b
    ctot = st["conc"] + st["conc_young"] if young else st["conc"]
    for rows, rows0 in ((st["conc_fsd"], before["conc_fsd"]), (st["conc_mech_fsd"], before["conc_mech_fsd"])):
        s = rows[0].copy()
        for k in range(1, n):
            s += rows[k]
        finite = np.isfinite(s)
        assert (~finite).sum() == ((ctot >= 1.) & (rows0.sum(0) == 0.)).sum()            # the division by a zero ctot2, and only it
        lo = finite & (ctot < 1.)
        assert np.abs(s - ctot)[lo].max() <= 1e-11
        hi = finite & (ctot >= 1.)
        assert np.abs(s[hi] / ctot[hi] - 1.).max() <= EPS * n
    keep = (branch == "within_1e-11") | (branch == "no_ice")
    assert _bits(st["conc_fsd"][:, keep], before["conc_fsd"][:, keep])
    z = branch == "ctot2_zero"
    assert np.array_equal(st["conc_fsd"][n - 1, z], ctot[z]) and (n == 1 or not st["conc_fsd"][:n - 1, z].any())


@pytest.mark.parametrize("n", [1, 2, 12, 16])
def test_welding_conserves_the_sum_of_the_bins(n):
    Ne, ddt = 600, 900.
    cfg = R.default_config(n, R.standard_tables(n), False, debug_fsd=1)
    cfg["welding_kappa"] = R.WELD_K / (ddt * cfg["tables"]["area_scaled_up"][n - 1])
    st, freezing, g = R.weld_inputs(n, Ne)
    before = R.copy_state(st)
    ndt, crash, zeroed = R.weld(st, cfg, ddt, freezing)
    assert not crash
    for name, mask in (("not freezing", ndt == -1), ("below the gate", ndt == 0), ("1", ndt == 1), ("2", ndt == 2), (">= 5", ndt >= 5)):
        assert mask.mean() >= 0.05, name
    old, new = before["conc_fsd"].sum(0), st["conc_fsd"].sum(0)
    # the final rescale M_conc_fsd[m] = tmp[m] * old_conc_tot / sum(tmp) rounds each bin twice (<= 2^-52 relative each), and the two sums round n times each
    assert np.abs(new - old).max() <= (2 * n + 2) * EPS
    idle = ndt <= 0
    assert _bits(st["conc_fsd"][:, idle], before["conc_fsd"][:, idle])
    if n > 1:     # welding moves area from the small bins into the large ones
        w = ndt >= 1
        assert (st["conc_fsd"][n - 1, w] > before["conc_fsd"][n - 1, w]).all() and (st["conc_fsd"][0, w] < before["conc_fsd"][0, w]).all()
    assert st["conc_fsd"].min() >= 0. and st["conc_fsd"].max() <= 1.


@pytest.mark.parametrize("young", [False, True])
@pytest.mark.parametrize("breakup_type", [R.NONE, R.UNIFORM_SIZE, R.ZHANG, R.DUMONT])
@pytest.mark.parametrize("n", [1, 2, 12, 16])
def test_breakup_without_damage_conserves_the_sum_of_the_bins(n, breakup_type, young):
    Ne = 500
    cfg = R.default_config(n, R.standard_tables(n), young, breakup_type=breakup_type, fsd_damage_type=0, debug_fsd=1)
    st, wlbk, g = R.breakup_inputs(n, Ne, young, cfg["tables"])
    before = R.copy_state(st)
    in_dt, crash, what = R.redistribute_fsd(st, cfg, wlbk)
    assert in_dt and not crash
    b = what == 2
    assert np.abs(st["conc_fsd"][:, b].sum(0) - before["conc_fsd"][:, b].sum(0)).max() <= n * n * 2. ** -53
    assert _bits(st["conc_fsd"][:, what == 1], before["conc_fsd"][:, what == 1]) and not st["conc_fsd"][:, what == 0].any()
    for k in ("damage", "cum_damage", "cum_wave_damage"):           # type 0: tmp = M_damage, nothing moves (x + 0. and max(x, min(x, .)) return x)
        assert _bits(st[k], before[k]), k
    if breakup_type != R.NONE and n > 1:
        assert (st["conc_fsd"][n - 1, b] <= before["conc_fsd"][n - 1, b]).all() and (st["conc_fsd"][0, b] > before["conc_fsd"][0, b]).any()
    if breakup_type == R.NONE:
        assert _bits(st["conc_fsd"][:, b], before["conc_fsd"][:, b])


def test_damage_type_1_falls_through_into_2():
    n, Ne = 12, 300
    out = []
    for dt in (1, 2):
        cfg = R.default_config(n, R.standard_tables(n), True, breakup_type=R.ZHANG, fsd_damage_type=dt, distinguish_mech_fsd=1)
        st, wlbk, g = R.breakup_inputs(n, Ne, True, cfg["tables"])
        R.redistribute_fsd(st, cfg, wlbk)
        out.append(st)
    for k in ("damage", "cum_damage", "cum_wave_damage", "conc_fsd"):
        assert _bits(out[0][k], out[1][k]), k
