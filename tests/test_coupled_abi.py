"""The coupled build's terms (wave stress, cumulated damage, floe-size bins) at the C ABI: the three entry points are exported and declared, the
ctypes mirror of nxs_dyn_coupled matches the header, and the composed wave-stress reference that tests/test_gpu_coupled.py compares the device
with reproduces the oracle's own explicitSolve() bit for bit when the perturbation is left out."""
import ctypes as C
import os
import subprocess

import numpy as np

import cases
from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nxs_dyn_set_wave_stress", "nxs_dyn_put_coupled", "nxs_dyn_get_coupled")


def composed_explicit_solve(ranks, tau_wi=None):
    """explicitSolve() of the oracle composed from its phase functions (the loop of pyoracle.multirank_step without its update()), with M_tau_wi added IN
    PLACE to the work array D_tau_a between prep and the sub-steps: the reference's tau_x = D_tau_a + tau_wi + c_prime * (...) associates left
    (FE.cpp:10509-10518), so this is its expression exactly.  tau_wi: one [2*Nn] vector per rank, or None."""
    from oracle import pyoracle as O
    p = ranks[0].params
    steps = p.substeps
    dte = p.dtime_step / float(steps)
    for i, r in enumerate(ranks):
        r.prep()
        if tau_wi is not None:
            n2 = 2 * r.lm.num_nodes
            np.ctypeslib.as_array(r.work.contents.D_tau_a, shape=(n2,))[:] += tau_wi[i]
    for _ in range(steps):
        for r in ranks:
            r.substep_solve()
        O.exchange_ghosts(ranks)
        if p.dynamics_type != _abi.NXS_DYN_MEVP:
            for r in ranks:
                r.move_mesh(dte)
    if p.dynamics_type == _abi.NXS_DYN_MEVP:
        for r in ranks:
            r.move_mesh(p.dtime_step)
    for _ in range(50):
        for r in ranks:
            r.smoother_sweep()
        O.exchange_ghosts(ranks)
    for r in ranks:
        r.ow_tail()


def wave_stress_at(x, y, L, amplitude=0.12):
    """A smooth M_tau_wi of the size of the wind stress (0.05 - 0.2 N m-2) at the points (x, y); L: the extent of the WHOLE mesh, so that the ranks of a
    partitioned mesh see one field."""
    x, y = x / L, y / L
    return np.ascontiguousarray(np.concatenate([amplitude * (0.6 + 0.4 * np.sin(3. * x + 1.)) * np.cos(2. * y), amplitude * 0.7 * np.sin(2. * x - 0.5 * y + 0.3)]))


def smooth_wave_stress(lm, amplitude=0.12):
    return wave_stress_at(lm.coord_x, lm.coord_y, max(np.ptp(lm.coord_x), np.ptp(lm.coord_y)), amplitude)


def test_the_three_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    for name in NEW:
        assert name in dynamics.EXPORTS, name
        assert hasattr(L, name), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert f" T {name}\n" in out, name
    assert L.nxs_dyn_abi_version() == 2


def test_coupled_layout_matches_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){printf("%zu %zu %zu %zu\\n", sizeof(nxs_dyn_coupled), '
                   'offsetof(nxs_dyn_coupled, num_fsd_bins), offsetof(nxs_dyn_coupled, conc_fsd), offsetof(nxs_dyn_coupled, cum_damage));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert vals == [C.sizeof(_abi.Coupled), _abi.Coupled.num_fsd_bins.offset, _abi.Coupled.conc_fsd.offset, _abi.Coupled.cum_damage.offset]
    assert vals[0] == 24 and vals[1] == 16


def test_the_python_wrapper_has_the_three_methods():
    for name in ("set_wave_stress", "put_coupled", "get_coupled"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))


def test_composed_reference_without_the_perturbation_is_the_oracles_explicit_solve():
    from oracle import pyoracle as O
    for dyn in ("bbm", "evp", "mevp"):
        gm, p, g, lms, fields = cases.make_case("small", dynamics_type=dyn, substeps=12, dtime_step=200. * 12 / 120)
        a, b = O.OracleRank(lms[0], p, fields[0]), O.OracleRank(lms[0], p, fields[0])
        a.explicit_solve()
        composed_explicit_solve([b])
        for k in ("VT", "UM", "UT", "sigma0", "sigma1", "sigma2", "damage"):
            assert np.array_equal(a.arr[k], b.arr[k]), (dyn, k)
        # ... and the perturbation does reach the solve: the harness cannot pass with the term dropped
        c = O.OracleRank(lms[0], p, fields[0])
        composed_explicit_solve([c], [smooth_wave_stress(lms[0])])
        assert cases.rel_err(c.arr["VT"], a.arr["VT"]) > 1e-7, dyn
