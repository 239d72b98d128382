"""Nesting and the slab ocean's diffusion at the C ABI (include/nxs_dyn.h: nxs_dyn_nesting_*, nxs_dyn_diffusion_configure, nxs_dyn_diffuse): exported and declared,
the ctypes mirrors match the header, the enum values are the fixed order of forcingNesting()'s rows, the ABI version stays 2, and what the entry points refuse without
a handle (so without a device) -- plus the resources of the kernels read from the built library."""
import ctypes as C
import os
import re
import subprocess

import pytest

from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
NEW = ("nxs_nesting_config_check", "nxs_dyn_nesting_configure", "nxs_dyn_nesting_pair", "nxs_dyn_nesting_time", "nxs_dyn_nesting_ice", "nxs_dyn_nesting_dynamics",
       "nxs_dyn_nesting_get", "nxs_dyn_diffusion_configure", "nxs_dyn_diffuse", "nxs_dyn_flux_device_rows")
METHODS = ("nesting_configure", "nesting_pair", "nesting_time", "nesting_ice", "nesting_dynamics", "nesting_get", "diffusion_configure", "diffuse", "flux_device_rows")


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
        assert getattr(L, name).argtypes is not None, name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in METHODS:
        assert callable(getattr(dynamics.FiniteElementDynamics, name))
    assert callable(dynamics.nesting_config_check)


def test_layouts_and_enums_match_the_header(tmp_path):
    types = {"nxs_dyn_nesting_config": _abi.NestingConfig, "nxs_dyn_nesting_rows": _abi.NestingRows, "struct nxs_dyn_nesting_time": _abi.NestingTime}
    members = {s: [k for k, _ in T._fields_] for s, T in types.items()}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms) + 'printf("\\n");' for s, ms in members.items())
    enums = (["NXS_NEST_" + k.upper() for k in _abi.NEST_ELEMENT_ROWS] + ["NXS_NEST_" + k.upper() for k in _abi.NEST_NODE_ROWS]
             + ["NXS_NEST_DS_" + k.upper() for k in _abi.NEST_DATASETS]
             + ["NXS_NEST_ELEMENT_ROWS", "NXS_NEST_NODE_ROWS", "NXS_NEST_DATASETS", "NXS_NUDGE_LINEAR", "NXS_NUDGE_EXPONENTIAL", "NXS_TF_OFF", "NXS_TF_LINEAR", "NXS_TF_STEP"])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){' + body + "".join(f'printf("%d ", {e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])      # (as C: the tag and the entry point share a name)
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    for row, (s, ms) in zip(rows, members.items()):
        assert [int(v) for v in row.split()] == [C.sizeof(types[s])] + [getattr(types[s], m).offset for m in ms], s
    assert [int(v) for v in rows[3].split()] == list(range(12)) + list(range(3)) + list(range(5)) + [12, 3, 5, 0, 1, 0, 1, 2]
    # the order of forcingNesting() (FE.cpp:11062-11121)
    assert _abi.NEST_ELEMENT_ROWS == ("dist", "thick", "conc", "snow_thick", "h_young", "conc_young", "hs_young", "sigma1", "sigma2", "sigma3", "damage", "ridge_ratio")
    assert _abi.NEST_NODE_ROWS == ("dist_nodes", "VT1", "VT2")
    assert _abi.NUDGE_FUNCTIONS == {"linear": 0, "exponential": 1}


def test_the_header_compiles_as_cxx_too(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "nxs_dyn.h"\nint main(){ struct nxs_dyn_nesting_time t = {}; nxs_dyn_nesting_config c = {}; nxs_dyn_nesting_rows r = {};'
                   ' return t.mode[0] + c.time_step + (r.node[2] != 0) + (&nxs_dyn_nesting_time == 0); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


GOOD = dict(nudge_function="exponential", nudge_timescale=86400., nudge_scale=2e4, nest_dynamic_vars=True, time_step=900, dtime_step=900.)
BAD = [("nudge_function", 2), ("nudge_function", -1), ("nudge_timescale", 0.), ("nudge_timescale", -5.), ("nudge_timescale", float("nan")), ("nudge_timescale", float("inf")),
       ("nudge_scale", 0.), ("nudge_scale", -1.), ("nudge_scale", float("nan")), ("nudge_scale", float("inf")), ("dtime_step", float("nan")), ("dtime_step", float("-inf"))]


def test_the_config_check_accepts_both_functions():
    assert dynamics.nesting_config_check(**GOOD) == (0, "")
    assert dynamics.nesting_config_check(**dict(GOOD, nudge_function="linear", nest_dynamic_vars=False)) == (0, "")
    assert dynamics.load_library().nxs_nesting_config_check(None) == -1


@pytest.mark.parametrize("field,value", BAD)
def test_the_config_check_refuses_each_bad_field_and_names_it(field, value):
    rc, text = dynamics.nesting_config_check(**dict(GOOD, **{field: value}))
    assert rc == -1 and field in text, (rc, text)
    if field == "nudge_function":
        assert "use exponential or linear" in text                          # the reference's own words (FE.cpp:4888)


def test_null_arguments_are_invalid():
    L = dynamics.load_library()
    rows, t, c = _abi.NestingRows(), _abi.NestingTime(), dynamics._nesting_config(**GOOD)
    dev = (C.c_void_p * 8)()
    assert L.nxs_dyn_nesting_configure(None, C.byref(c)) == -1
    assert L.nxs_dyn_nesting_pair(None, C.byref(rows), C.byref(rows)) == -1
    assert L.nxs_dyn_nesting_time(None, C.byref(t)) == -1
    assert L.nxs_dyn_nesting_ice(None) == -1 and L.nxs_dyn_nesting_dynamics(None) == -1
    assert L.nxs_dyn_nesting_get(None, 0, C.byref(rows)) == -1
    assert L.nxs_dyn_diffusion_configure(None, 1., 1., 1., 1.) == -1 and L.nxs_dyn_diffuse(None) == -1
    assert L.nxs_dyn_flux_device_rows(None, dev) == -1
    # a NULL argument beside a handle is refused before the handle is looked at: a fake, non-NULL handle is never dereferenced
    fake = C.c_void_p(8)
    assert L.nxs_dyn_nesting_pair(fake, None, None) == -1
    assert L.nxs_dyn_nesting_time(fake, None) == -1
    assert L.nxs_dyn_nesting_get(fake, 0, None) == -1
    assert L.nxs_dyn_flux_device_rows(fake, None) == -1


def _llvm_tool(name):
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for sub in ("llvm/bin", "lib/llvm/bin"):
        if os.path.exists(os.path.join(root, sub, name)):
            return os.path.join(root, sub, name)
    raise AssertionError(f"{name} not found beside hipcc ({root})")


def test_the_kernels_use_no_scratch_memory_and_no_lds(tmp_path):
    """read from the gfx950 code object inside the built library: all four stream rows through registers"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    found = {}
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\S+)$", block, flags=re.M))
        if "k_nesting_" in f.get("name", "") or "k_diffuse" in f.get("name", ""):
            found[f["name"]] = f
    assert len(found) == 4 and all(any(k in n for n in found) for k in ("k_nesting_ice", "k_nesting_dynamics", "k_diffuse_pack", "k_diffuse")), found
    for f in found.values():
        print(f)
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0 and int(f["group_segment_fixed_size"]) == 0, f
