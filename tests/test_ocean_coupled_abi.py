"""A coupled ocean at the C ABI (include/nxs_dyn.h: nxs_ocean_coupled_*, nxs_dyn_ocean_coupled_*; include/nxs_interp.h: nxs_gridmap_receive_rows): exported and
declared, the ctypes mirrors match the header, every NXS_ERR_INVALID / NXS_ERR_STATE reachable without a device names what is wrong, the column's configuration
still refuses NXS_COL_OCEAN_COUPLED, the three "out of scope: OceanType::COUPLED" sentences are gone from the header, the new definitions are function-try-blocks
and the resources of the receive kernel read from the built library.  No device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nextsim_amd import _abi, dynamics, interp
from test_column_abi import _llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
IHEADER = open(os.path.join(ROOT, "include", "nxs_interp.h")).read()
NEW = ("nxs_ocean_coupled_default_config", "nxs_ocean_coupled_config_check", "nxs_dyn_ocean_coupled_attach", "nxs_dyn_ocean_coupled_receive",
       "nxs_dyn_ocean_coupled_put_rows", "nxs_dyn_ocean_coupled_get")
INEW = ("nxs_gridmap_receive_rows", "nxs_gridmap_debug_receive_lists")
INVALID = -1


def _err():
    return dynamics.load_library().nxs_dyn_last_error(None).decode()


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    for name in INEW:
        assert name in dynamics.INTERP_EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_INTERP_API int " + name + r"\(", IHEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("ocean_coupled_attach", "ocean_coupled_detach", "ocean_coupled_receive", "ocean_coupled_put_rows", "ocean_coupled_get"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name)), name
    assert callable(interp.GridMap.receive_rows) and callable(dynamics.ocean_coupled_default_config) and callable(dynamics.ocean_coupled_config_check)
    hpp = open(os.path.join(ROOT, "include", "nxs_dyn.hpp")).read()
    for name in NEW[2:]:
        assert name + "(h_" in hpp, name


def test_layouts_and_enum_values_match_the_header(tmp_path):
    types = {"nxs_dyn_ocean_coupled_config": _abi.OceanCoupledConfig, "nxs_dyn_ocean_coupled_rows": _abi.OceanCoupledRows}
    members = {s: [k for k, _ in T._fields_] for s, T in types.items()}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms) + 'printf("\\n");' for s, ms in members.items())
    enums = ("NXS_OC_OCEAN_TEMP", "NXS_OC_OCEAN_SALT", "NXS_OC_QSRML", "NXS_OC_MLD", "NXS_OC_WLBK", "NXS_OC_ROWS", "NXS_GRIDMAP_MAX_RECEIVE", "NXS_REGRID_IN_DEVICE",
             "NXS_REGRID_OUT_DEVICE")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\n#include "nxs_interp.h"\nint main(void){' + body
                   + "".join(f'printf("%d ", {e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    for row, (s, ms) in zip(rows, members.items()):
        assert [int(v) for v in row.split()] == [C.sizeof(types[s])] + [getattr(types[s], m).offset for m in ms], s
    assert [int(v) for v in rows[2].split()] == [_abi.OC_ROWS.index(k) for k in ("ocean_temp", "ocean_salt", "qsrml", "mld", "wlbk")] + [
        _abi.NXS_OC_ROWS, _abi.NXS_GRIDMAP_MAX_RECEIVE, interp.GridMap.IN_DEVICE, interp.GridMap.OUT_DEVICE]


def test_the_default_configuration_is_the_references_receive():
    """dataset.cpp's ocean_cpl_elements with coupler.rcv_first_layer_depth off: I_SST, I_SSS, I_FrcQsr, a = 1, b = 0; no wave model, so no I_wlbk"""
    d = dynamics.ocean_coupled_default_config()
    assert d == {"rows": ("ocean_temp", "ocean_salt", "qsrml"), "a": [1.] * 3, "b": [0.] * 3, "factor": [1.] * 3, "bias": [0.] * 3}
    assert dynamics.load_library().nxs_ocean_coupled_default_config(None) == INVALID


def test_what_the_attach_refuses_in_a_configuration():
    chk = dynamics.ocean_coupled_config_check
    for ok in (("ocean_temp", "ocean_salt", "qsrml"), ("wlbk",), ("qsrml", "ocean_salt", "ocean_temp", "mld", "wlbk"), (4, 3, 2, 1, 0)):
        assert chk(ok) == 0, ok
    assert chk(()) == INVALID and "n_fields = 0" in _err()
    assert chk((0, 1, 2, 3, 4, 0)) == INVALID and "n_fields = 6" in _err()
    assert chk((0, 5)) == INVALID and "unknown row 5" in _err() and "field 1" in _err()
    assert chk((0, -1)) == INVALID and "unknown row -1" in _err()
    assert chk(("qsrml", "mld", "qsrml")) == INVALID and "qsrml" in _err() and "field 2" in _err()
    assert dynamics.load_library().nxs_ocean_coupled_config_check(None) == INVALID and "no configuration" in _err()


def test_null_arguments_are_refused_before_any_device_work():
    L = dynamics.load_library()
    Li = interp._declare_gridmap()
    c = _abi.ocean_coupled_config_struct(("ocean_temp",))
    r = _abi.OceanCoupledRows()
    assert L.nxs_dyn_ocean_coupled_attach(None, None, C.byref(c)) == INVALID and L.nxs_dyn_ocean_coupled_attach(None, None, None) == INVALID
    assert L.nxs_dyn_ocean_coupled_receive(None, None, 0) == INVALID
    assert L.nxs_dyn_ocean_coupled_put_rows(None, C.byref(r)) == INVALID
    assert L.nxs_dyn_ocean_coupled_get(None, None, None) == INVALID
    one = np.ones(1)
    ptrs = (C.c_void_p * 1)(one.ctypes.data)
    D = _abi.dptr
    assert Li.nxs_gridmap_receive_rows(None, 1, ptrs, D(one), D(one), D(one), D(one), ptrs, 0, None) == INVALID
    assert "NULL" in Li.nxs_interp_last_error().decode()
    prev = C.c_int32(-1)
    assert Li.nxs_gridmap_debug_receive_lists(2, C.byref(prev)) == INVALID and Li.nxs_gridmap_debug_receive_lists(-1, None) == INVALID
    assert Li.nxs_gridmap_debug_receive_lists(1, C.byref(prev)) == 0 and prev.value == 1               # the library's choice: copies in transposed order


def test_the_column_configuration_still_refuses_the_coupled_ocean():
    """the coupled ocean is an attachment (nxs_dyn_ocean_coupled_attach), not an option of nxs_dyn_column_configure"""
    assert dynamics.column_config_check(ocean_type="coupled") == INVALID and "OASIS" in _err()


def test_the_out_of_scope_sentences_were_brought_up_to_date():
    assert "the OceanType::COUPLED term" not in HEADER                                  # the fluxes' (6e)
    assert "tracers), OceanType::COUPLED (#ifdef OASIS)" not in HEADER                 # the column's (6f)
    assert "each needs the coupled ocean's received fields, which no entry point carries" not in HEADER   # the coupled slab's (6h)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "which no entry point carries" not in design and "6n" in design
    for f in ("README.md", "INTEGRATION.md"):
        assert "nxs_dyn_ocean_coupled_receive" in open(os.path.join(ROOT, f)).read(), f


def test_the_new_definitions_are_function_try_blocks():
    csrc = os.path.join(ROOT, "nextsim_amd", "csrc")
    seen = set()
    for fn, names in (("nxs_interp.hip", INEW), ("nxs_ocean_coupled.inl", NEW)):
        lines = open(os.path.join(csrc, fn)).read().split("\n")
        for i, line in enumerate(lines):
            m = re.match(r'^(?:extern "C" )?int (nxs_\w+)\(', line)
            if not m or m.group(1) not in names:
                continue
            j = i
            while not lines[j].split("//")[0].rstrip().endswith(("{", ";")):
                j += 1
            head = lines[j].split("//")[0].rstrip()
            assert head.endswith("try {"), f"{fn}:{j + 1}: {m.group(1)} is not a function-try-block"
            k = j + 1
            while not lines[k].startswith("}"):
                k += 1
            assert "catch (...)" in lines[k] and m.group(1) in lines[k], f"{fn}:{k + 1}: handler of {m.group(1)}"
            seen.add(m.group(1))
    assert seen == set(NEW) | set(INEW)
    assert '#include "nxs_ocean_coupled.inl"' in open(os.path.join(csrc, "nxs_dyn.hip")).read()
    assert "nxs_ocean_coupled.inl" in open(os.path.join(csrc, "Makefile")).read()


def test_the_receive_kernel_uses_no_scratch_memory_and_no_lds(tmp_path):
    """the accumulators of up to five variables stay in registers (the builds for 1 .. 5 variables, both ways of reading the lists)"""
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
        if "k_gridmap_receive" in f.get("name", ""):
            found.append(f)
    assert len(found) == 10, [f.get("name") for f in found]
    for f in found:
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0 and int(f["group_segment_fixed_size"]) == 0, f
    print(sorted((f["name"], f["vgpr_count"]) for f in found))
