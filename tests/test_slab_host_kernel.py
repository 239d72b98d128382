"""The source of the slab kernel (nextsim_amd/csrc/nxs_slab_kernels.inl) compiled for the host (tests/slab_host_kernel.cpp) against tests/slab_ref.py: with
the same libm under both and no contraction, all 29 rows, every row written in place and the branch word are the restatement's BITS (NaN equal to NaN), for both
thermo types, both ice categories and every option -- the assimilation flux and newice_type 3 included: pow and hypot are the same library's on both sides, which
is also the check that the restatement's routes to them (ctypes on libm, numpy's hypot) give glibc's bits.  So the kernel's formulas are the restatement's
without a device in the loop.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import slab_ref as R
from nextsim_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict.fromkeys(_abi.SLAB_CLOCK, 1)
# (options of the slab, the clock); newice_type 1 .. 3 are the classic category's, everything else runs in both categories
OPTIONS = [({}, {}), (dict(newice_type=1), {}), (dict(newice_type=2), {}), (dict(newice_type=3), {}), (dict(melt_type=1), {}),
           (dict(use_assim_flux=1), {}), (dict(use_assim_flux=1, assim_flux_exponent=2.), {}), (dict(temp_dep_healing=1), {}), (dict(use_meltponds=1), {}),
           (dict(reset_by_date=1), dict(myi_reset_now=1)), (dict(reset_by_date=1), ALL), (dict(equal_melting=0), {}), (dict(include_young_ice=0, reset_by_date=1), ALL)]
OPTIONS += [({}, {k: 1}) for k in _abi.SLAB_CLOCK]
CCFG = [dict(), dict(freezingpoint_type="unesco", mld_source="row")]


def _id(o):
    return "-".join(f"{k}={v}" for d in o for k, v in d.items()) or "defaults"


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "slab_host_kernel")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-builtin", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "slab_host_kernel.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def case():
    gm = cases.global_mesh("toy")
    tri = np.ascontiguousarray(gm.tri, np.int64)
    inp, strata, calm = R.make_inputs(gm.x, gm.y, tri)
    return gm, tri, inp


def write_input(path, Ne, Nn, tri, inp, cfg, ccfg, ocean_albedo, young, dt, clock):
    E = _abi.COL_ENUMS
    with open(path, "wb") as f:
        f.write(struct.pack("20i", Ne, Nn, int(young), int(ccfg["thermo_type"] == "winton"), E["freezingpoint_type"][ccfg["freezingpoint_type"]],
                            E["mld_source"][ccfg["mld_source"]], dt, *[int(cfg[k]) for k in _abi.SLAB_CONFIG_INTS], *[int(clock[k]) for k in _abi.SLAB_CLOCK]))
        f.write(struct.pack("15d", *[cfg[k] for k in _abi.SLAB_CONFIG_REALS], ccfg["freezingpoint_mu"], ccfg["snow_cond"], ccfg["constant_mld"], ocean_albedo))
        f.write(tri.astype(np.int32).tobytes())
        f.write(inp["wind"].tobytes())
        for k in R.FLUX + R.COL + ("precip", "mld", "conc_upd") + R.IN_PLACE:
            f.write(inp[k].tobytes())


def run_both(binary, tmp_path, gm, tri, inp, cfg, ccfg, young, clock):
    Ne = tri.shape[0]
    alb = FR.default_config()["ocean_albedo"]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(fin, Ne, gm.x.size, tri, inp, cfg, ccfg, alb, young, R.DT, clock)
    subprocess.check_call([binary, fin, fout])
    got = np.fromfile(fout).reshape(len(R.ROWS) + len(R.IN_PLACE) + 1, Ne)
    work = R.copy(inp)
    rows, words = R.slab(work, cfg, ccfg, alb, tri, young, R.DT, clock)
    return got, rows, work, words


# newice_type 4 is the young-ice category's and 1 .. 3 are the classic one's (nxs_dyn_slab refuses the other pairs): the classic category runs every other option
# on newice_type 1 (slab_ref.category_config)
PAIRS = [(o, y) for o in OPTIONS for y in (True, False) if not (y and "newice_type" in o[0])]


@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("over,young", PAIRS, ids=lambda v: _id(v) if isinstance(v, tuple) else ("young" if v else "classic"))
def test_the_kernel_source_on_the_host_gives_the_restatements_bits(binary, case, tmp_path, over, thermo, young):
    gm, tri, inp = case
    opts, flags = over
    cfg = R.category_config(young, **opts)
    for extra in CCFG if not opts and not flags else CCFG[:1]:
        ccfg = CR.default_config(thermo_type=thermo, **extra)
        clock = R.clock(**flags)
        got, rows, work, words = run_both(binary, tmp_path, gm, tri, inp, cfg, ccfg, young, clock)
        for i, k in enumerate(R.ROWS + R.IN_PLACE):
            want = rows[k] if i < len(R.ROWS) else work[k]
            same = R.same_bits(got[i], want)
            assert same.all(), (k, int((~same).sum()), np.flatnonzero(~same)[:5], got[i][~same][:3], want[~same][:3])
        assert np.array_equal(got[-1].astype(np.uint32), words), np.flatnonzero(got[-1].astype(np.uint32) != words)[:5]
        assert np.abs(got[R.ROWS.index("vice_melt")]).max() > 0 and np.abs(got[R.ROWS.index("Qo")]).max() > 0
        n = len(R.ROWS)
        if not young:
            for k in ("conc_young", "h_young", "hs_young"):
                assert np.array_equal(got[n + R.IN_PLACE.index(k)], inp[k])                         # the young rows are left alone
        if thermo == "zero_layer":
            for k in ("tice1", "tice2"):
                assert np.array_equal(got[n + R.IN_PLACE.index(k)], inp[k])
        if not opts.get("temp_dep_healing"):
            assert np.array_equal(got[n + R.IN_PLACE.index("time_relaxation_damage")], inp["time_relaxation_damage"])
        if not opts.get("use_meltponds"):
            for k in ("pond_volume", "pond_fraction", "lid_volume"):
                assert np.array_equal(got[n + R.IN_PLACE.index(k)], inp[k])
        if opts.get("use_assim_flux"):
            assert R.took(words, "assim").sum() > 40 and np.abs(rows["Qassim"]).max() > 0
        if opts.get("newice_type") == 3:
            assert R.took(words, "n3_h0").any() and not R.took(words, "n3_h0").all()
