"""The device code of a coupled ocean compiled for the host (tests/ocean_coupled_host_kernel.cpp: the receive kernel's body and the sources of k_fluxes, k_column
and k_slab with their OceanType::COUPLED statements switched on) against tests/ocean_coupled_ref.py: bit for bit (NaN equal to NaN) on the golden lists of
tests/golden/bamg_grid_remap.npz and on the designed inputs, both thermo types, both ice categories, the mld row on and off.  The same program runs once under
-fsanitize=address,undefined as a stand-alone binary.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cases
import column_ref as CR
import fluxes_ref as FR
import grid_remap_ref as G
import ocean_coupled_ref as OC
import slab_ref as SR
import test_column_host_kernel as TCH
import test_fluxes_host_kernel as TFH
import test_slab_host_kernel as TSH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALB = FR.default_config()["ocean_albedo"]


def _build(dst, sanitize=False):
    cmd = ["g++", "-O2", "-std=c++17", "-fno-builtin", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "nextsim_amd", "csrc")]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "ocean_coupled_host_kernel.cpp"), "-o", dst])
    return dst


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("hostk") / "ocean_coupled_host_kernel"))


def _same(a, b):
    return G.same_bits(a, b)


def transposed(lists):
    """the transposed lists as gridmap_finish makes them: per triangle the indices of its entries in the forward lists, ascending; the cell of every entry"""
    tris, off, gridP, nels = lists["tris"], lists["off"], lists["gridP"], lists["nels"]
    t_pos = np.argsort(tris, kind="stable").astype(np.int32)
    t_off = np.concatenate([[0], np.cumsum(np.bincount(tris, minlength=nels))]).astype(np.int32)
    cell = np.repeat(gridP, np.diff(off)).astype(np.int32)
    return t_off, t_pos, cell


def run_receive(binary, tmp, lists, fields, a, b, factor, bias):
    t_off, t_pos, cell = transposed(lists)
    nv, Gs = len(fields), np.asarray(fields[0]).size
    fin, fout = os.path.join(str(tmp), "rc_in.bin"), os.path.join(str(tmp), "rc_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("4i", lists["nels"], Gs, t_pos.size, nv))
        for arr in (t_off, t_pos, cell):
            f.write(arr.tobytes())
        f.write(np.ascontiguousarray(lists["w"], np.float64).tobytes())
        f.write(np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(v, np.float64), (nv,)) for v in (a, b, factor, bias)], axis=1)).tobytes())
        for fld in fields:
            f.write(np.ascontiguousarray(fld, np.float64).tobytes())
    subprocess.check_call([binary, "receive", fin, fout])
    return np.fromfile(fout).reshape(2, nv, lists["nels"])


@pytest.mark.parametrize("name", G.CASES)
def test_the_receive_body_on_the_golden_lists(binary, tmp_path, name):
    c = G.case(name)
    lists = OC.lists_of(c)
    for n_var in (1, 3, 5):
        fields, a, b, factor, bias = OC.awkward_fields(c["gridX"].size, n_var)
        got = run_receive(binary, tmp_path, lists, fields, a, b, factor, bias)
        want = OC.receive(lists, fields, a, b, factor, bias)
        assert _same(got[0], want) and _same(got[1], want), (name, n_var)
    got = run_receive(binary, tmp_path, lists, [c["g2m_in7"][:, v] for v in range(5)], 1., 0., 1., 0.)
    assert _same(got[0] + 0., c["g2m_out7"][:, :5].T + 0.)                     # the real bamg's outputs, up to the sign of zero


@pytest.fixture(scope="module")
def toy():
    gm = cases.global_mesh("toy")
    return gm, np.ascontiguousarray(gm.tri, np.int64)


@pytest.mark.parametrize("young", [True, False])
def test_the_fluxes_kernel_with_qsrml(binary, tmp_path, toy, young):
    gm, tri = toy
    inp, calm = FR.make_inputs(gm.x, gm.y, tri)
    cfg = FR.default_config()
    Ne = tri.shape[0]
    qsrml = OC.received_rows({"sst": inp["sst"], "sss": inp["sss"]})["qsrml"]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", Ne, gm.x.size, int(young), cfg["alb_scheme"], FR.HUM[cfg["humidity_source"]], FR.LW[cfg["longwave_source"]], cfg["force_neutral_atmosphere"], 0))
        f.write(struct.pack("11d", *[cfg[k] for k in ("alb_ice", "alb_sn", "alb_ponds", "I_0", "ocean_albedo", "drag_ocean_t", "drag_ocean_q", "zref_wind", "zref_temp",
                                                      "limiting_lengthscale")], TFH.QDA))
        f.write(tri.astype(np.int32).tobytes())
        f.write(inp["wind"].tobytes())
        for k in ("tair", "mslp", "Qsw_in", "dair", "Qlw_in") + TFH.ROWS_IN:
            f.write(inp[k].tobytes())
        f.write(qsrml.tobytes())
    subprocess.check_call([binary, "fluxes", fin, fout])
    got = np.fromfile(fout).reshape(len(FR.ROWS) + len(FR.DRAGS), Ne)
    work = FR.copy(inp)
    rows, _ = FR.fluxes(work, cfg, tri, young, TFH.QDA)
    rows = dict(rows, Qow=OC.qow(rows, qsrml))
    for i, k in enumerate(FR.ROWS + FR.DRAGS):
        want = rows[k] if k in rows else work[k]
        assert _same(got[i], want), k
    assert not _same(rows["Qow"], OC.qow(rows, qsrml, drop=("qsw_kept",)))


@pytest.mark.parametrize("mld", ["constant", "row"])
@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
def test_the_column_kernel_under_the_coupled_ocean(binary, tmp_path, toy, thermo, young, mld):
    gm, tri = toy
    inp, strata, calm = CR.make_inputs(gm.x, gm.y, tri)
    inp.update({k: v for k, v in OC.received_rows(inp).items() if k in ("ocean_temp", "ocean_salt")})
    cfg = CR.default_config(thermo_type=thermo, freezingpoint_type="unesco", mld_source=mld)
    Ne = tri.shape[0]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    TCH.write_input(fin, Ne, gm.x.size, tri, inp, cfg, young, CR.DT)
    subprocess.check_call([binary, "column", fin, fout])
    names = CR.ROWS + CR.IN_PLACE + ("sst", "sss")
    got = np.fromfile(fout).reshape(len(names), Ne)
    work = CR.copy(inp)
    rows, _ = OC.column(work, cfg, tri, young, CR.DT)
    for i, k in enumerate(names):
        want = rows[k] if i < len(CR.ROWS) else work[k]
        assert _same(got[i], want), k
    assert _same(got[-2], inp["ocean_temp"]) and _same(got[-1], inp["ocean_salt"]) and not got[CR.ROWS.index("Qdw")].any()
    late, _ = OC.column(CR.copy(inp), cfg, tri, young, CR.DT, drop=("reset_after_qio",))
    assert not _same(late["Qio"], got[CR.ROWS.index("Qio")])


@pytest.mark.parametrize("mld", ["constant", "row"])
@pytest.mark.parametrize("young", [True, False])
@pytest.mark.parametrize("thermo", ["winton", "zero_layer"])
def test_the_slab_kernel_under_the_coupled_ocean(binary, tmp_path, toy, thermo, young, mld):
    gm, tri = toy
    inp, strata, calm = SR.make_inputs(gm.x, gm.y, tri)
    rec = OC.received_rows(inp)
    inp["sst"], inp["sss"] = rec["ocean_temp"], rec["ocean_salt"]              # (what the column left)
    ccfg = CR.default_config(thermo_type=thermo, freezingpoint_type="unesco", mld_source=mld)
    cfg = SR.category_config(young, temp_dep_healing=1)
    clock = SR.clock(last_step_of_day=1)
    Ne = tri.shape[0]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    TSH.write_input(fin, Ne, gm.x.size, tri, inp, cfg, ccfg, ALB, young, SR.DT, clock)
    subprocess.check_call([binary, "slab", fin, fout])
    got = np.fromfile(fout).reshape(len(SR.ROWS) + len(SR.IN_PLACE) + 1, Ne)
    work = SR.copy(inp)
    rows, words = OC.slab(work, cfg, ccfg, ALB, tri, young, SR.DT, clock)
    for i, k in enumerate(SR.ROWS + SR.IN_PLACE):
        want = rows[k] if i < len(SR.ROWS) else work[k]
        same = SR.same_bits(got[i], want)
        assert same.all(), (k, int((~same).sum()), np.flatnonzero(~same)[:5])
    assert np.array_equal(got[-1].astype(np.uint32), words)
    n = len(SR.ROWS)
    assert _same(got[n + SR.IN_PLACE.index("sst")], inp["sst"]) and _same(got[n + SR.IN_PLACE.index("sss")], inp["sss"])
    wrong = SR.copy(inp)
    OC.slab(wrong, cfg, ccfg, ALB, tri, young, SR.DT, clock, drop=("tbot_advanced",))
    assert not _same(wrong["time_relaxation_damage"], got[n + SR.IN_PLACE.index("time_relaxation_damage")])


def test_the_same_program_under_the_sanitizers(tmp_path, toy):
    """address and undefined-behaviour sanitizers on the stand-alone program: the receive on the longest golden lists with five variables, and the three kernels"""
    exe = _build(str(tmp_path / "ocean_coupled_host_kernel_san"), sanitize=True)
    gm, tri = toy
    c = G.case("long_rows")
    fields, a, b, factor, bias = OC.awkward_fields(c["gridX"].size, 5)
    got = run_receive(exe, tmp_path, OC.lists_of(c), fields, a, b, factor, bias)
    assert _same(got[1], OC.receive(OC.lists_of(c), fields, a, b, factor, bias))
    all_land = G.case("all_land")
    assert np.isnan(run_receive(exe, tmp_path, OC.lists_of(all_land), [np.ones(all_land["gridX"].size)], 1., 0., 1., 0.)).all()
    test_the_fluxes_kernel_with_qsrml(exe, tmp_path, toy, True)
    test_the_column_kernel_under_the_coupled_ocean(exe, tmp_path, toy, "winton", True, "row")
    test_the_slab_kernel_under_the_coupled_ocean(exe, tmp_path, toy, "winton", True, "row")
