"""The coupler's outgoing side at the C ABI (include/nxs_dyn.h: nxs_dyn_cpl_out_*, nxs_dyn_fsd_diag_configure, NXS_MEANS_DMAX / NXS_MEANS_DMEAN; include/nxs_interp.h:
nxs_gridmap_send_rows): exported and declared, the new enum values and flags as a C compiler reads the header against _abi, the ABI version and the older ranges
unchanged, the new range overlapping no other, NULL arguments refused before any device work, the new definitions function-try-blocks, the out-of-scope passages
brought up to date, and the send kernel's resources read from the built library.  No device."""
import ctypes as C
import os
import re
import subprocess

import pytest

from nextsim_amd import _abi, dynamics, interp
from test_column_abi import _llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
IHEADER = open(os.path.join(ROOT, "include", "nxs_interp.h")).read()
NEW = ("nxs_dyn_cpl_out_configure", "nxs_dyn_cpl_out_update", "nxs_dyn_cpl_out_get", "nxs_dyn_cpl_out_reset", "nxs_dyn_cpl_out_attach_grid", "nxs_dyn_cpl_out_put",
       "nxs_dyn_cpl_out_reset_grid", "nxs_dyn_fsd_diag_configure")
INVALID = -1


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert "nxs_gridmap_send_rows" in dynamics.INTERP_EXPORTS and " T nxs_gridmap_send_rows\n" in out
    assert re.search(r"NXS_INTERP_API int nxs_gridmap_send_rows\(", IHEADER)
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("cpl_out_configure", "cpl_out_update", "cpl_out_get", "cpl_out_reset", "cpl_out_attach_grid", "cpl_out_put", "cpl_out_reset_grid", "fsd_diag_configure"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name)), name
    assert callable(interp.GridMap.send_rows)
    hpp = open(os.path.join(ROOT, "include", "nxs_dyn.hpp")).read()
    for name in NEW:
        assert name + "(h_" in hpp, name


def test_enum_values_and_flags_match_the_header(tmp_path):
    enums = ("NXS_MEANS_DMAX", "NXS_MEANS_DMEAN", "NXS_MEANS_FSD_BEGIN", "NXS_MEANS_FSD_END", "NXS_CPL_OUT_RESET", "NXS_MEANS_THERMO_BEGIN", "NXS_MEANS_THERMO_END",
             "NXS_MEANS_ELEMENTAL_END", "NXS_MEANS_NODAL_BEGIN", "NXS_MEANS_NODAL_END", "NXS_MEANS_MAX_VARS", "NXS_DYN_ABI_VERSION", "NXS_FSD_MAX_BINS")
    src = tmp_path / "en.c"
    src.write_text('#include <stdio.h>\n#include "nxs_dyn.h"\n#include "nxs_interp.h"\nint main(void){' + "".join(f'printf("%d ", (int){e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "en")])
    v = dict(zip(enums, (int(x) for x in subprocess.check_output([str(tmp_path / "en")], text=True).split())))
    assert (v["NXS_MEANS_DMAX"], v["NXS_MEANS_DMEAN"], v["NXS_MEANS_FSD_BEGIN"], v["NXS_MEANS_FSD_END"]) == (192, 193, 192, 194)
    assert _abi.MEANS_FSD == ("dmax", "dmean") and _abi.MEANS_FSD_ID == {"dmax": v["NXS_MEANS_DMAX"], "dmean": v["NXS_MEANS_DMEAN"]}
    assert (_abi.NXS_MEANS_FSD_BEGIN, _abi.NXS_MEANS_FSD_END, _abi.NXS_CPL_OUT_RESET) == (v["NXS_MEANS_FSD_BEGIN"], v["NXS_MEANS_FSD_END"], v["NXS_CPL_OUT_RESET"]) and v["NXS_CPL_OUT_RESET"] == 1
    assert v["NXS_DYN_ABI_VERSION"] == 2 and v["NXS_MEANS_THERMO_END"] == 190 and v["NXS_MEANS_THERMO_BEGIN"] == _abi.NXS_MEANS_THERMO_BEGIN == 128
    # the older names keep their contents: the new ids live in names of their own
    assert not set(_abi.MEANS_FSD) & set(_abi.MEANS_ID) and len(_abi.MEANS_ID) == len(_abi.MEANS_ELEMENTAL) + len(_abi.MEANS_NODAL) + len(_abi.MEANS_THERMO)
    assert len(_abi.MEANS_ELEMENTAL) == v["NXS_MEANS_ELEMENTAL_END"] and len(_abi.MEANS_THERMO) == v["NXS_MEANS_THERMO_END"] - v["NXS_MEANS_THERMO_BEGIN"]
    ranges = [(0, v["NXS_MEANS_ELEMENTAL_END"]), (v["NXS_MEANS_NODAL_BEGIN"], v["NXS_MEANS_NODAL_END"]), (v["NXS_MEANS_THERMO_BEGIN"], v["NXS_MEANS_THERMO_END"]),
              (v["NXS_MEANS_FSD_BEGIN"], v["NXS_MEANS_FSD_END"])]
    for i, (a, b) in enumerate(ranges):
        assert a < b <= 256                                       # MeansTable::id is an unsigned char
        for c, d in ranges[i + 1:]:
            assert b <= c or d <= a, (a, b, c, d)
    assert v["NXS_FSD_MAX_BINS"] == 16                            # nxs_fsd_diag::MAX_BINS
    assert "constexpr int MAX_BINS = 16;" in open(os.path.join(ROOT, "nextsim_amd", "csrc", "nxs_fsd_diag_body.inl")).read()


def test_null_arguments_are_refused_before_any_device_work():
    L = dynamics.load_library()
    Li = interp._declare_gridmap()
    c = _abi.MeansConfig()
    assert L.nxs_dyn_cpl_out_configure(None, C.byref(c)) == INVALID and L.nxs_dyn_cpl_out_update(None, 1.0) == INVALID
    assert L.nxs_dyn_cpl_out_get(None, None, None, None, None) == INVALID and L.nxs_dyn_cpl_out_reset(None) == INVALID
    assert L.nxs_dyn_cpl_out_attach_grid(None, None, None) == INVALID and L.nxs_dyn_cpl_out_put(None, None, None, None, None, 0) == INVALID
    assert L.nxs_dyn_cpl_out_reset_grid(None) == INVALID and L.nxs_dyn_fsd_diag_configure(None, 0.1, 1000., 10.) == INVALID
    assert Li.nxs_gridmap_send_rows(None, 1, None, None, 0, None) == INVALID and "NULL" in Li.nxs_interp_last_error().decode()


def test_the_new_definitions_are_function_try_blocks():
    csrc = os.path.join(ROOT, "nextsim_amd", "csrc")
    seen = set()
    for fn, names in (("nxs_interp.hip", ("nxs_gridmap_send_rows",)), ("nxs_cpl_out.inl", NEW)):
        lines = open(os.path.join(csrc, fn)).read().split("\n")
        for i, line in enumerate(lines):
            m = re.match(r'^(?:extern "C" )?int (nxs_\w+)\(', line)
            if not m or m.group(1) not in names:
                continue
            j = i
            while not lines[j].split("//")[0].rstrip().endswith(("{", ";")):
                j += 1
            assert lines[j].split("//")[0].rstrip().endswith("try {"), f"{fn}:{j + 1}: {m.group(1)} is not a function-try-block"
            k = j + 1
            while not lines[k].startswith("}"):
                k += 1
            assert "catch (...)" in lines[k] and m.group(1) in lines[k], f"{fn}:{k + 1}: handler of {m.group(1)}"
            seen.add(m.group(1))
    assert seen == set(NEW) | {"nxs_gridmap_send_rows"}
    assert '#include "nxs_cpl_out.inl"' in open(os.path.join(csrc, "nxs_dyn.hip")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "nxs_cpl_out.inl" in mk and "nxs_fsd_diag_body.inl" in mk


def test_one_statement_of_the_launch_logic_and_of_the_body():
    """nxs_dyn_means_update and nxs_dyn_cpl_out_update call ONE helper; the put writes no second locator and no copy of the per-point body"""
    csrc = os.path.join(ROOT, "nextsim_amd", "csrc")
    dyn, cpl = open(os.path.join(csrc, "nxs_dyn.hip")).read(), open(os.path.join(csrc, "nxs_cpl_out.inl")).read()
    assert dyn.count("hipLaunchKernelGGL(k_means_elements_thermo<true>") == 1 and dyn.count("hipLaunchKernelGGL(k_means_nodes<true>") == 1
    assert dyn.count("means_update_set(h, ") == 1 and cpl.count("means_update_set(h, ") == 1 and "hipLaunchKernelGGL" not in cpl
    assert "nxs_drifters::means_points_update(" in cpl and "nxs_gridmap_send_rows(" in cpl
    body = open(os.path.join(csrc, "nxs_fsd_diag_body.inl")).read()
    code = "\n".join(line.split("//")[0] for line in body.split("\n"))
    assert not re.search(r"\b(pow|exp|log|sqrt|hypot|fabs|fmin|fmax|std::)\s*\(?", code)      # + - * / and the two selects only: bit for bit


def test_the_out_of_scope_sentences_were_brought_up_to_date():
    assert "a second set of accumulators for the coupler's means (M_cpl_out) beside the Moorings'" not in HEADER
    assert "M_cpl_out's accumulators and the OASIS put, dmax / dmean" not in HEADER
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "6o" in design and "a second set of accumulators for `M_cpl_out`" not in design
    for f in ("README.md", "INTEGRATION.md"):
        assert "nxs_dyn_cpl_out_put" in open(os.path.join(ROOT, f)).read(), f


def test_the_send_kernel_uses_no_scratch_memory_and_no_lds(tmp_path):
    """the sums of up to twelve variables stay in registers (the builds for at most 4, 8 and 12 variables)"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    blob, magic, notes = open(fat, "rb").read(), b"__CLANG_OFFLOAD_BUNDLE__", ""
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]          # one bundle per translation unit of the library
    assert starts
    for i, lo in enumerate(starts):
        part = str(tmp_path / f"fat{i}.bin")
        open(part, "wb").write(blob[lo:starts[i + 1] if i + 1 < len(starts) else len(blob)])
        subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"])
        notes += subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    found = []
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\S+)$", block, flags=re.M))
        if "k_gridmap_send" in f.get("name", "") or "k_means_elements_thermo" in f.get("name", ""):
            found.append(f)
    assert len([f for f in found if "k_gridmap_send" in f["name"]]) == 3 and len(found) == 5, [f.get("name") for f in found]
    for f in found:
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, f
        if "k_gridmap_send" in f["name"]:
            assert int(f["group_segment_fixed_size"]) == 0, f
    print(sorted((f["name"], f["vgpr_count"]) for f in found))
