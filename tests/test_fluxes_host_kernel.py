"""The source of the flux kernel (nextsim_amd/csrc/nxs_flux_kernels.inl) compiled for the host (tests/fluxes_host_kernel.cpp) against tests/fluxes_ref.py: with
the same libm under both and no contraction, all 25 rows and the four drags are the restatement's BITS, in both ice categories and under every option.  So the
kernel's formulas are the restatement's without a device in the loop; tests/test_gpu_fluxes.py then measures the device's libm.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cases
import fluxes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QDA = 0.0049
ROWS_IN = ("conc", "snow_thick", "conc_young", "hs_young", "tice0", "tsurf_young", "sst", "pond_fraction", "lid_volume", "drag_ui", "drag_ti", "drag_ui_young", "drag_ti_young")
OPTIONS = ({}, dict(alb_scheme=1), dict(alb_scheme=2), dict(alb_scheme=4), dict(humidity_source="sphuma"), dict(humidity_source="mixrat"), dict(longwave_source="tcc"),
           dict(force_neutral_atmosphere=1), dict(zref_wind=8., zref_temp=3., limiting_lengthscale=2.5))


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostk") / "fluxes_host_kernel")
    # -fno-builtin: a libm call on constants (the Grachev constants of flux_derive) is not folded by the compiler's own arithmetic; -ffp-contract=off as the library
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-builtin", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fluxes_host_kernel.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def case():
    gm = cases.global_mesh("toy")
    tri = np.ascontiguousarray(gm.tri, np.int64)
    inp, calm = R.make_inputs(gm.x, gm.y, tri)
    return gm, tri, inp


@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("over", OPTIONS, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()) or "defaults")
def test_the_kernel_source_on_the_host_gives_the_restatements_bits(binary, case, tmp_path, over, young):
    gm, tri, inp = case
    cfg = R.default_config(**over)
    Ne = tri.shape[0]
    hum = {"dewpoint": "dair", "sphuma": "sphuma", "mixrat": "mixrat"}[cfg["humidity_source"]]
    lw = "Qlw_in" if cfg["longwave_source"] == "Qlw_in" else "tcc"
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", Ne, gm.x.size, int(young), cfg["alb_scheme"], R.HUM[cfg["humidity_source"]], R.LW[cfg["longwave_source"]], cfg["force_neutral_atmosphere"], 0))
        f.write(struct.pack("11d", *[cfg[k] for k in ("alb_ice", "alb_sn", "alb_ponds", "I_0", "ocean_albedo", "drag_ocean_t", "drag_ocean_q", "zref_wind", "zref_temp",
                                                      "limiting_lengthscale")], QDA))
        f.write(tri.astype(np.int32).tobytes())
        f.write(inp["wind"].tobytes())
        for k in ("tair", "mslp", "Qsw_in", hum, lw) + ROWS_IN:
            f.write(inp[k].tobytes())
    subprocess.check_call([binary, fin, fout])
    got = np.fromfile(fout).reshape(len(R.ROWS) + len(R.DRAGS), Ne)
    work = R.copy(inp)
    rows, _ = R.fluxes(work, cfg, tri, young, QDA)
    for i, k in enumerate(R.ROWS + R.DRAGS):
        want = rows[k] if k in rows else work[k]
        same = (got[i].view(np.uint64) == np.ascontiguousarray(want).view(np.uint64)) | (np.isnan(got[i]) & np.isnan(want))
        assert same.all(), (k, int((~same).sum()), float(np.nanmax(np.abs(got[i] - want))))
    assert np.abs(got[R.ROWS.index("Qia")]).max() > 0 and np.isfinite(got).all()
