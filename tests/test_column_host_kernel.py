"""The source of the column kernel (nextsim_amd/csrc/nxs_column_kernels.inl) compiled for the host (tests/column_host_kernel.cpp) against tests/column_ref.py:
with the same libm under both and no contraction, all 22 rows and the six rows written in place are the restatement's BITS (NaN equal to NaN), for both thermo
types, both ice categories and every option -- EXCHANGE included: the hypot is the same library's on both sides.  So the kernel's formulas are the restatement's
without a device in the loop.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cases
import column_ref as R
from nextsim_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ({}, dict(qio_type="exchange"), dict(freezingpoint_type="unesco"), dict(ocean_type="nudged"), dict(snowfall_source="snowfall"),
           dict(snowfall_source="precip_tair"), dict(mld_source="row"), dict(flooding=0), dict(qio_type="exchange", freezingpoint_type="unesco", ocean_type="nudged", mld_source="row"))
ROWS_IN = (R.FLUX_IN + tuple(k + "_young" for k in R.FLUX_IN)
           + ("conc", "thick", "snow_thick", "conc_young", "h_young", "hs_young", "tice0", "tice1", "tice2", "tsurf_young", "sst", "sss"))


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "column_host_kernel")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-builtin", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "column_host_kernel.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def case():
    gm = cases.global_mesh("toy")
    tri = np.ascontiguousarray(gm.tri, np.int64)
    inp, strata, calm = R.make_inputs(gm.x, gm.y, tri)
    return gm, tri, inp


def write_input(path, Ne, Nn, tri, inp, cfg, young, dt):
    E = _abi.COL_ENUMS
    snow = "snowfall" if cfg["snowfall_source"] == "snowfall" else "snowfr"
    with open(path, "wb") as f:
        f.write(struct.pack("12i", Ne, Nn, int(young), *[E[k][cfg[k]] for k in ("thermo_type", "qio_type", "freezingpoint_type", "ocean_type", "snowfall_source", "mld_source")],
                            int(cfg["flooding"]), dt, 0))
        f.write(struct.pack("8d", *[cfg[k] for k in _abi.COL_CONFIG_REALS]))
        f.write(tri.astype(np.int32).tobytes())
        f.write(inp["VT"].tobytes())
        f.write(inp["ocean"].tobytes())
        for k in ("tair", "precip", snow, "ocean_temp", "ocean_salt", "mld") + ROWS_IN:
            f.write(inp[k].tobytes())


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
@pytest.mark.parametrize("over", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_the_kernel_source_on_the_host_gives_the_restatements_bits(binary, case, tmp_path, over, thermo, young):
    gm, tri, inp = case
    cfg = R.default_config(thermo_type=thermo, **over)
    Ne = tri.shape[0]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    write_input(fin, Ne, gm.x.size, tri, inp, cfg, young, R.DT)
    subprocess.check_call([binary, fin, fout])
    got = np.fromfile(fout).reshape(len(R.ROWS) + len(R.IN_PLACE), Ne)
    work = R.copy(inp)
    rows, rec = R.column(work, cfg, tri, young, R.DT)
    for i, k in enumerate(R.ROWS + R.IN_PLACE):
        want = rows[k] if i < len(R.ROWS) else work[k]      # (hs_young names a row, the slab's snow thickness, and a state member, M_hs_young)
        same = (got[i].view(np.uint64) == np.ascontiguousarray(want).view(np.uint64)) | (np.isnan(got[i]) & np.isnan(want))
        assert same.all(), (k, int((~same).sum()), np.flatnonzero(~same)[:5], got[i][~same][:3], want[~same][:3])
    assert np.abs(got[R.ROWS.index("del_hi")]).max() > 0 and np.abs(got[R.ROWS.index("Qio")]).max() > 0
    if not young:
        assert not got[len(R.HEAD_ROWS) + len(R.ICE_ROWS):len(R.ROWS)].any()                      # the nine young rows are zero
        for k in ("tsurf_young", "h_young", "hs_young"):
            assert np.array_equal(got[len(R.ROWS) + R.IN_PLACE.index(k)], inp[k])                    # and the young rows are left alone
    if thermo == "zero_layer":
        for k in ("tice1", "tice2"):
            assert np.array_equal(got[len(R.ROWS) + R.IN_PLACE.index(k)], inp[k])
