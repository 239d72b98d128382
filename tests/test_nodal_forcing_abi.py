"""The dynamics' nodal forcing at the C ABI (include/nxs_dyn.h: nxs_mapx_*, nxs_dyn_forcing_*, nxs_dyn_set_forcing_time_rows, nxs_dyn_set_element_depth): exported and
declared, the ctypes mirrors match the header (a compiled offsetof program), the enum values, the ABI version stays 2, the literal constants against the reference's
header as the fixture recorded them, what the entry points refuse without a handle (so without a device) -- plus the resources of the new kernels read from the built
library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
NEW = ("nxs_mapx_constants", "nxs_mapx_polar_north", "nxs_mapx_forward", "nxs_dyn_forcing_targets", "nxs_dyn_forcing_ingest", "nxs_dyn_set_forcing_time_rows",
       "nxs_dyn_set_element_depth", "nxs_dyn_forcing_get")
KERNELS = ("k_mapx_forward", "k_nf_east_north", "k_nf_pole", "k_nf_rotate", "k_nf_wrap", "k_nf_ingest", "k_nf_blend")


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("forcing_targets", "forcing_ingest", "set_forcing_time_rows", "set_element_depth", "forcing_get", "forcing_grid"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))
    for name in ("mapx_constants", "mapx_polar_north", "mapx_forward", "forcing_vectors"):
        assert callable(getattr(dynamics, name))


def test_layouts_and_enums_match_the_header(tmp_path):
    types = {"nxs_mapx_polar": _abi.MapxPolar, "nxs_dyn_forcing_vectors": _abi.ForcingVectors, "nxs_dyn_forcing_rows": _abi.ForcingRows,
             "struct nxs_dyn_forcing_time_rows": _abi.ForcingTimeRows}
    members = {s: [k for k, _ in T._fields_] for s, T in types.items()}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms) + 'printf("\\n");' for s, ms in members.items())
    enums = ["NXS_NF_WIND_U", "NXS_NF_WIND_V", "NXS_NF_OCEAN_U", "NXS_NF_OCEAN_V", "NXS_NF_SSH", "NXS_NF_ROWS", "NXS_NF_SETS", "NXS_NF_MAX_COLUMNS", "NXS_NF_MAX_VECTORS",
             "NXS_NF_GROUP_WIND", "NXS_NF_GROUP_OCEAN", "NXS_NF_GROUP_SSH", "NXS_NF_GROUPS", "NXS_MAPX_CONST_RE_KM", "NXS_MAPX_CONST_PI", "NXS_MAPX_CONST_COUNT"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){' + body + "".join(f'printf("%d ", {e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    for row, (s, ms) in zip(rows, members.items()):
        assert [int(v) for v in row.split()] == [C.sizeof(types[s])] + [getattr(types[s], m).offset for m in ms], s
    assert [int(v) for v in rows[len(types)].split()] == [0, 1, 2, 3, 4, 5, 4, 32, 4, 0, 1, 2, 3, 0, 1, 2]
    assert (_abi.NXS_NF_ROWS, _abi.NXS_NF_SETS, _abi.NXS_NF_MAX_COLUMNS, _abi.NXS_NF_MAX_VECTORS, _abi.NXS_NF_GROUPS) == (5, 4, 32, 4, 3)
    assert _abi.NF_ROWS == ("wind_u", "wind_v", "ocean_u", "ocean_v", "ssh") and _abi.NF_GROUPS == ("wind", "ocean", "ssh")
    assert C.sizeof(_abi.MapxPolar) == 15 * 8


def test_the_header_compiles_as_cxx_too(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "nxs_dyn.h"\nint main(){ struct nxs_dyn_forcing_time_rows t = {}; nxs_dyn_forcing_vectors v = {}; nxs_mapx_polar m = {}; '
                   'return t.mode[0] + v.n_pairs + (int)m.Rg + (&nxs_dyn_set_forcing_time_rows == 0); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_literal_constants_are_the_reference_headers():
    """mapx_Re_km and PI as a translation unit that includes contrib/mapx/include/mapx.h printed them into the fixture"""
    want = np.load(os.path.join(ROOT, "tests", "golden", "mapx_forward.npz"))["constants"]
    got = dynamics.mapx_constants()
    assert got["Re_km"] == want[0] == 6371.228 and got["PI"] == want[1] == 3.141592653589793
    L = dynamics.load_library()
    assert L.nxs_mapx_constants(None, 2) == -1 and L.nxs_mapx_constants((C.c_double * 2)(), -1) == -1


def test_polar_north_refuses_another_aspect():
    L = dynamics.load_library()
    m = _abi.MapxPolar()
    args = (0., 60., -45., 0.001, 90., 135., 6378.273, 0.081816153)
    assert L.nxs_mapx_polar_north(90., *args, None) == -1
    for lat0 in (-90., 0., 89.999):
        assert L.nxs_mapx_polar_north(lat0, *args, C.byref(m)) == -1, lat0
    assert L.nxs_mapx_polar_north(90., *args, C.byref(m)) == 0 and m.Rg == 6378.273 / 0.001 and m.lat1 == 60.
    assert L.nxs_mapx_polar_north(90., 0., 999., *args[2:], C.byref(m)) == 0 and m.lat1 == 90.      # lat1 == 999 means lat0: the other branch of the projection


def test_null_and_range_errors():
    L = dynamics.load_library()
    m, g, v, rows, t = _abi.MapxPolar(), _abi.ForcingGrid(), _abi.ForcingVectors(), _abi.ForcingRows(), _abi.ForcingTimeRows()
    one = (C.c_double * 1)(0.)
    izero = (C.c_int32 * 1)(0)
    for args in ((None, 1, one, one, one, one), (C.byref(m), 1, None, one, one, one), (C.byref(m), 1, one, None, one, one), (C.byref(m), 1, one, one, None, one),
                 (C.byref(m), 1, one, one, one, None), (C.byref(m), -1, one, one, one, one)):
        assert L.nxs_mapx_forward(*args, -1) == -1, args
    assert L.nxs_mapx_forward(C.byref(m), 0, one, one, one, one, -1) == 0
    assert L.nxs_dyn_forcing_targets(None, 0, one, one) == -1
    assert L.nxs_dyn_forcing_ingest(None, 0, C.byref(g), 0, 0, one, 1, izero, izero, None) == -1
    assert L.nxs_dyn_set_forcing_time_rows(None, C.byref(t)) == -1
    assert L.nxs_dyn_set_element_depth(None, one) == -1
    assert L.nxs_dyn_forcing_get(None, 0, C.byref(rows)) == -1
    # a NULL argument beside a handle is refused before the handle is looked at: a fake, non-NULL handle is never dereferenced
    fake = C.c_void_p(8)
    assert L.nxs_dyn_forcing_targets(fake, 0, None, one) == -1 and L.nxs_dyn_forcing_targets(fake, 0, one, None) == -1
    for args in ((None, 0, 0, one, 1, izero, izero, C.byref(v)), (C.byref(g), 0, 0, None, 1, izero, izero, None), (C.byref(g), 0, 0, one, 1, None, izero, None),
                 (C.byref(g), 0, 0, one, 1, izero, None, None), (C.byref(g), 0, 0, one, 1, izero, izero, None)):      # (the last: the descriptor's axes are NULL)
        assert L.nxs_dyn_forcing_ingest(fake, 0, *args) == -1, args
    assert L.nxs_dyn_set_forcing_time_rows(fake, None) == -1
    assert L.nxs_dyn_set_element_depth(fake, None) == -1
    assert L.nxs_dyn_forcing_get(fake, 0, None) == -1


def _llvm_tool(name):
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for sub in ("llvm/bin", "lib/llvm/bin"):
        if os.path.exists(os.path.join(root, sub, name)):
            return os.path.join(root, sub, name)
    raise AssertionError(f"{name} not found beside hipcc ({root})")


def test_the_kernels_use_no_scratch_memory_and_no_lds(tmp_path):
    """read from the gfx950 code object inside the built library: every new kernel streams through registers"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    found = {}
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\S+)$", block, flags=re.M))
        for k in KERNELS:
            if re.search(r"\d" + k + r"(?![a-z_])", f.get("name", "")):
                found[k] = f
    assert sorted(found) == sorted(KERNELS), sorted(found)
    for k, f in found.items():
        print(k, f)
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0 and int(f["group_segment_fixed_size"]) == 0, f
