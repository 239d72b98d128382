"""thermo()'s slab loop from new ice to tracers at the C ABI (include/nxs_dyn.h: nxs_slab_*, nxs_dyn_slab_*, nxs_dyn_slab): exported and declared, the ctypes
mirrors match the header, the defaults and the constants are the reference's (tests/golden/reference_constants.json), what nxs_dyn_slab_configure refuses --
through nxs_slab_config_check, the same check without a handle, so without a device -- and the resources of k_slab read from the built library."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import slab_ref as R
from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_constants.json")))
NEW = ("nxs_slab_default_config", "nxs_slab_config_check", "nxs_slab_constants", "nxs_dyn_slab_configure", "nxs_dyn_slab_put", "nxs_dyn_slab_get_state", "nxs_dyn_slab",
       "nxs_dyn_slab_get")


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("slab_configure", "slab_put", "slab_get", "slab", "slab_rows"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))
    assert callable(dynamics.slab_default_config) and callable(dynamics.slab_config_check) and callable(dynamics.slab_constants) and callable(dynamics.slab_clock)


def test_layouts_match_the_header(tmp_path):
    types = {"nxs_dyn_slab_config": _abi.SlabConfig, "nxs_dyn_slab_state": _abi.SlabState, "nxs_dyn_slab_clock": _abi.SlabClock, "nxs_dyn_slab_rows": _abi.SlabRows}
    members = {s: [k for k, _ in T._fields_] for s, T in types.items()}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms) + 'printf("\\n");' for s, ms in members.items())
    enums = (["NXS_SLAB_ROWS", "NXS_SLAB_CONST_COUNT"] + ["NXS_SLAB_CONST_" + k.upper() for k in _abi.SLAB_CONSTANTS] + ["NXS_SLAB_" + k.upper() for k in _abi.SLAB_ROWS]
             + ["NXS_SLAB_BR_" + k.upper() for k in _abi.SLAB_BRANCHES])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){' + body + "".join(f'printf("%d ", {e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    for row, (s, ms) in zip(rows, members.items()):
        assert [int(v) for v in row.split()] == [C.sizeof(types[s])] + [getattr(types[s], m).offset for m in ms], s
    assert [int(v) for v in rows[4].split()] == ([_abi.NXS_SLAB_ROWS, len(_abi.SLAB_CONSTANTS)] + list(range(len(_abi.SLAB_CONSTANTS))) + list(range(_abi.NXS_SLAB_ROWS))
                                                 + [1 << i for i in range(len(_abi.SLAB_BRANCHES))])
    assert _abi.SLAB_ROWS == R.ROWS and _abi.SLAB_CONSTANTS == R.CONSTANTS and set(R.IN_PLACE) >= set(_abi.SLAB_STATE) - {"conc_upd"}


def test_the_defaults_are_the_fixtures():
    """model/options.cpp:329-331, 397-403, 428-449, 543-548 as tests/golden/reference_constants.json holds it"""
    opt = FIX["options"]
    got = dynamics.slab_default_config()
    for member, option in (("hnull", "thermo.hnull"), ("PhiF", "thermo.PhiF"), ("PhiM", "thermo.PhiM"), ("h_young_min", "thermo.h_young_min"),
                           ("h_young_max", "thermo.h_young_max"), ("assim_flux_exponent", "thermo.assim_flux_exponent"), ("reset_freeze_days", "age.reset_freeze_days"),
                           ("meltpond_runoff_fraction", "thermo.meltpond_runoff_fraction"), ("meltpond_depth_to_fraction", "thermo.meltpond_depth_to_fraction"),
                           ("deltaT_relaxation_damage", "dynamics.deltaT_relaxation_damage")):
        assert got[member] == float.fromhex(opt[option]["hex"]) == opt[option]["value"], member
    days = float.fromhex(FIX["members"]["days_in_sec"]["hex"])
    assert got["time_relaxation_damage"] == days * opt["dynamics.time_relaxation_damage"]["value"] == 25 * 86400.
    for member, option in (("newice_type", "thermo.newice_type"), ("melt_type", "thermo.melt_type"), ("use_assim_flux", "thermo.use_assim_flux"),
                           ("temp_dep_healing", "dynamics.use_temperature_dependent_healing"), ("use_meltponds", "thermo.use_meltponds"),
                           ("reset_by_date", "age.reset_by_date"), ("include_young_ice", "age.include_young_ice"), ("equal_melting", "age.equal_melting")):
        assert got[member] == int(opt[option]["value"]), member
    assert (got["newice_type"], got["melt_type"], got["include_young_ice"], got["equal_melting"]) == (4, 2, 1, 1)
    assert got == R.default_config() and FIX["string_options"]["age.reset_date"] == "0915"


def test_the_constants_are_the_references():
    phys = FIX["physical"]
    got = dynamics.slab_constants()
    assert tuple(got) == R.CONSTANTS == _abi.SLAB_CONSTANTS
    for k, v in got.items():
        if k == "days_in_sec":
            assert v == float.fromhex(FIX["members"]["days_in_sec"]["hex"]) == float(R.days_in_sec)
        else:
            assert v == float.fromhex(phys[k]["hex"]) == float(getattr(R, k)), k


def test_what_configure_refuses():
    chk = dynamics.slab_config_check
    err = lambda: dynamics.load_library().nxs_dyn_last_error(None)
    assert chk() == 0
    bad = [dict(newice_type=0), dict(newice_type=5), dict(newice_type=-1), dict(melt_type=0), dict(melt_type=3), dict(melt_type=4), dict(melt_type=-1)]
    for k in ("hnull", "PhiF", "h_young_min", "meltpond_depth_to_fraction", "time_relaxation_damage", "deltaT_relaxation_damage"):
        bad += [{k: 0.}, {k: -1.}, {k: float("nan")}]
    bad += [dict(h_young_max=0.05), dict(h_young_max=0.01), dict(h_young_max=float("nan")), dict(h_young_min=0.5)]
    for b in bad:
        assert chk(**b) == -1, b
        text = err()
        assert next(iter(b)).encode() in text or (b"h_young_max" in text and "h_young_min" in b), (b, text)
        assert b"must be" in text or b"1 .. " in text or b"OASIS" in text, text
    assert chk(melt_type=3) == -1 and b"OASIS" in err() and b"melt_type = 3" in err()
    assert chk(newice_type=5) == -1 and b"newice_type = 5 (1 .. 4" in err()
    assert chk(hnull=0.) == -1 and b"hnull = 0 must be positive" in err()
    assert chk(h_young_max=0.05) == -1 and b"must be larger than h_young_min" in err()
    for ok in ([dict(newice_type=k) for k in (1, 2, 3, 4)] + [dict(melt_type=1), dict(use_assim_flux=1, assim_flux_exponent=2.), dict(temp_dep_healing=1), dict(use_meltponds=1),
               dict(reset_by_date=1, include_young_ice=0), dict(equal_melting=0), dict(PhiM=0.), dict(meltpond_runoff_fraction=0.), dict(reset_freeze_days=0.)]):
        assert chk(**ok) == 0, ok
    assert dynamics.load_library().nxs_slab_config_check(None) == -1


def test_the_python_mirror_refuses_an_unknown_option():
    with pytest.raises(KeyError):
        dynamics.slab_config_check(h_null=0.3)
    with pytest.raises(KeyError):
        dynamics.slab_config_check(freezingpoint_mu=0.05)         # the column's: one copy


def _llvm_tool(name):
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for sub in ("llvm/bin", "lib/llvm/bin"):
        if os.path.exists(os.path.join(root, sub, name)):
            return os.path.join(root, sub, name)
    raise AssertionError(f"{name} not found beside hipcc ({root})")


def test_the_slab_kernel_uses_no_scratch_memory_and_no_lds(tmp_path):
    """a long divergent fp64 body, everything of an element in registers: read from the gfx950 code object inside the built library (the VGPR count is printed; it
    is in DESIGN.md 6g and is not bounded here)"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    found = []
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\S+)$", block, flags=re.M))
        if "k_slab" in f.get("name", ""):
            found.append(f)
    assert len(found) == 1, found
    f = found[0]
    print(f)
    assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0 and int(f["group_segment_fixed_size"]) == 0, f
