"""thermo()'s element forcing at the C ABI (include/nxs_dyn.h: nxs_dyn_thermo_forcing_*): exported and declared, the ctypes mirrors match the header, the enum
values are the fixed order of the rows, the ABI version stays 2, and what the entry points refuse without a handle (so without a device) -- plus the resources of
the two kernels read from the built library."""
import ctypes as C
import os
import re
import subprocess

from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
NEW = ("nxs_dyn_thermo_forcing_pair", "nxs_dyn_thermo_forcing_time", "nxs_dyn_thermo_forcing_targets", "nxs_dyn_thermo_forcing_ingest", "nxs_dyn_thermo_forcing_get")
ORDER = ("TAIR", "MSLP", "QSW_IN", "HUMIDITY", "LONGWAVE", "PRECIP", "SNOW", "OCEAN_TEMP", "OCEAN_SALT", "MLD")


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("thermo_forcing_pair", "thermo_forcing_time", "thermo_forcing_targets", "thermo_forcing_ingest", "thermo_forcing_get"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))


def test_layouts_and_enums_match_the_header(tmp_path):
    types = {"nxs_dyn_thermo_forcing_rows": _abi.ThermoForcingRows, "struct nxs_dyn_thermo_forcing_time": _abi.ThermoForcingTime, "nxs_dyn_forcing_grid": _abi.ForcingGrid}
    members = {s: [k for k, _ in T._fields_] for s, T in types.items()}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms) + 'printf("\\n");' for s, ms in members.items())
    enums = ["NXS_TF_" + k for k in ORDER] + ["NXS_TF_ROWS", "NXS_TF_SETS", "NXS_TF_MAX_COLUMNS", "NXS_TF_OFF", "NXS_TF_LINEAR", "NXS_TF_STEP",
                                              "NXS_INTERP_TRIANGLE", "NXS_INTERP_BILINEAR", "NXS_INTERP_NEAREST"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\n#include "nxs_interp.h"\nint main(void){' + body + "".join(f'printf("%d ", {e});' for e in enums)
                   + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])      # (as C: the tag and the entry point share a name)
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    for row, (s, ms) in zip(rows, members.items()):
        assert [int(v) for v in row.split()] == [C.sizeof(types[s])] + [getattr(types[s], m).offset for m in ms], s
    assert [int(v) for v in rows[3].split()] == list(range(10)) + [10, 4, 32, 0, 1, 2, 0, 1, 2]
    assert (_abi.NXS_TF_ROWS, _abi.NXS_TF_SETS, _abi.NXS_TF_MAX_COLUMNS, _abi.NXS_TF_OFF, _abi.NXS_TF_LINEAR, _abi.NXS_TF_STEP) == (10, 4, 32, 0, 1, 2)
    assert tuple(k.upper() for k in _abi.TF_ROWS) == ORDER                      # the mirror's names in the header's order ...
    assert _abi.TF_ROWS[:5] == _abi.FLUX_ATMOSPHERE and _abi.TF_ROWS[5:] == _abi.COL_FORCING      # ... which is d_flux_atm[0..4], d_col_forcing[0..4]
    assert _abi.TF_MODES == {"off": 0, "linear": 1, "step": 2}


def test_the_header_compiles_as_cxx_too(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "nxs_dyn.h"\nint main(){ struct nxs_dyn_thermo_forcing_time t = {}; nxs_dyn_forcing_grid g = {}; return t.mode[0] + g.M + (&nxs_dyn_thermo_forcing_time == 0); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_arguments_are_invalid():
    L = dynamics.load_library()
    rows, t, g = _abi.ThermoForcingRows(), _abi.ThermoForcingTime(), _abi.ForcingGrid()
    one = (C.c_double * 1)(0.)
    izero = (C.c_int32 * 1)(0)
    assert L.nxs_dyn_thermo_forcing_pair(None, C.byref(rows), C.byref(rows)) == -1
    assert L.nxs_dyn_thermo_forcing_time(None, C.byref(t)) == -1
    assert L.nxs_dyn_thermo_forcing_targets(None, 0, one, one) == -1
    assert L.nxs_dyn_thermo_forcing_ingest(None, 0, C.byref(g), one, 1, izero, izero) == -1
    assert L.nxs_dyn_thermo_forcing_get(None, 0, C.byref(rows)) == -1
    # a NULL argument beside a handle is refused before the handle is looked at: a fake, non-NULL handle is never dereferenced
    fake = C.c_void_p(8)
    assert L.nxs_dyn_thermo_forcing_pair(fake, None, None) == -1
    assert L.nxs_dyn_thermo_forcing_time(fake, None) == -1
    assert L.nxs_dyn_thermo_forcing_targets(fake, 0, None, one) == -1 and L.nxs_dyn_thermo_forcing_targets(fake, 0, one, None) == -1
    for args in ((None, one, 1, izero, izero), (C.byref(g), None, 1, izero, izero), (C.byref(g), one, 1, None, izero), (C.byref(g), one, 1, izero, None),
                 (C.byref(g), one, 1, izero, izero)):      # (the last: the descriptor's axes are NULL)
        assert L.nxs_dyn_thermo_forcing_ingest(fake, 0, *args) == -1, args
    assert L.nxs_dyn_thermo_forcing_get(fake, 0, None) == -1


def _llvm_tool(name):
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for sub in ("llvm/bin", "lib/llvm/bin"):
        if os.path.exists(os.path.join(root, sub, name)):
            return os.path.join(root, sub, name)
    raise AssertionError(f"{name} not found beside hipcc ({root})")


def test_the_two_kernels_use_no_scratch_memory_and_no_lds(tmp_path):
    """read from the gfx950 code object inside the built library: both stream rows through registers"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    found = {}
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\S+)$", block, flags=re.M))
        if "k_thermo_forcing_" in f.get("name", ""):
            found[f["name"]] = f
    assert len(found) == 2 and any("blend" in k for k in found) and any("ingest" in k for k in found), found
    for f in found.values():
        print(f)
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0 and int(f["group_segment_fixed_size"]) == 0, f
