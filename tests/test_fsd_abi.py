"""The floe-size distribution at the C ABI (include/nxs_dyn.h, nxs_fsd_bins and nxs_dyn_fsd_*): exported and declared, the ctypes mirrors match the header,
the new enums are the reference's, and what nxs_dyn_fsd_configure refuses -- through nxs_fsd_config_check, the same check without a handle, so without a device."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fsd_ref as R
from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
NEW = ("nxs_fsd_bins", "nxs_fsd_config_check", "nxs_dyn_fsd_configure", "nxs_dyn_fsd_put", "nxs_dyn_fsd_get", "nxs_dyn_fsd_init", "nxs_dyn_fsd_update",
       "nxs_dyn_fsd_breakup", "nxs_dyn_fsd_weld")


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive, like the earlier additions: the version stays
    for name in ("fsd_configure", "fsd_put", "fsd_get", "fsd_init", "fsd_update", "fsd_breakup", "fsd_weld"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))
    assert callable(dynamics.fsd_bins)


def test_layouts_match_the_header(tmp_path):
    members = {"nxs_fsd_tables": [k for k, _ in _abi.FsdTables._fields_], "nxs_dyn_fsd_config": [k for k, _ in _abi.FsdConfig._fields_],
               "nxs_dyn_fsd_state": [k for k, _ in _abi.FsdState._fields_]}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms) + 'printf("\\n");' for s, ms in members.items())
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){' + body + 'printf("%d\\n", NXS_FSD_MAX_BINS);return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    for row, (s, ms), T in zip(rows, members.items(), (_abi.FsdTables, _abi.FsdConfig, _abi.FsdState)):
        assert [int(v) for v in row.split()] == [C.sizeof(T)] + [getattr(T, m).offset for m in ms], s
    assert int(rows[3]) == _abi.NXS_FSD_MAX_BINS == 16


def test_the_enums_are_the_references():
    """setup::FSDType / WeldingType / BreakupType as tests/golden/reference_constants.json holds them: its generator prints every enum class of
    model/enums.hpp, these three included, so the fixture needed no addition."""
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_constants.json")))["enums"]
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    enums = {}
    for body in re.findall(r"enum\s*\{([^}]*)\}", text):
        for item in body.split(","):
            name, _, val = item.strip().partition("=")
            if val.strip():
                enums[name.strip()] = int(val)
    for prefix, kind, mirror in (("NXS_FSD_", "FSDType", _abi.FSD_TYPES), ("NXS_WELDING_", "WeldingType", _abi.WELDING_TYPES), ("NXS_BREAKUP_", "BreakupType", _abi.BREAKUP_TYPES)):
        assert len(mirror) == len(ref[kind])
        for name, value in ref[kind].items():
            assert enums[prefix + name] == value == mirror[name.lower()] == getattr(_abi, prefix + name), (kind, name)
    assert (R.NONE, R.UNIFORM_SIZE, R.ZHANG, R.DUMONT) == tuple(ref["BreakupType"][k] for k in ("NONE", "UNIFORM_SIZE", "ZHANG", "DUMONT"))
    phys = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_constants.json")))["physical"]
    assert float.fromhex(phys["g"]["hex"]) == R.G and float.fromhex(phys["rhow"]["hex"]) == R.RHOW
    assert re.search(r"#define NXS_FSD_G 9\.8\b", open(os.path.join(ROOT, "nextsim_amd", "csrc", "nxs_fsd_kernels.inl")).read())


def _check(n, attached, tables=None, **over):
    cfg = R.default_config(n, R.standard_tables(max(n, 1)) if tables is None else tables, True, **over)
    return dynamics.fsd_config_check(n, cfg["tables"], attached, **R.library_options(cfg))


def test_what_configure_refuses():
    assert _check(12, 12) == 0 and _check(1, 1) == 0 and _check(_abi.NXS_FSD_MAX_BINS, _abi.NXS_FSD_MAX_BINS) == 0
    assert _check(12, 11) == -1 and _check(12, 0) == -1                       # not the attached conc_fsd's
    assert _check(0, 0) == -1 and _check(-1, -1) == -1                        # below 1
    assert _check(_abi.NXS_FSD_MAX_BINS + 1, _abi.NXS_FSD_MAX_BINS + 1) == -1 # above the cap
    for bad in (dict(breakup_type=4), dict(breakup_type=-1), dict(welding_type=2), dict(welding_type=-1), dict(fsd_damage_type=3), dict(fsd_damage_type=-1),
                dict(breakup_prob_type=1)):
        assert _check(12, 12, **bad) == -1, bad
    for ok in (dict(breakup_type=k) for k in range(4)):
        assert _check(12, 12, **ok) == 0
    # a merge-table entry outside [1, num_bins] for a ky <= kx; above the diagonal the reference's -999 is fine
    for kx, ky, v in ((5, 2, -999), (11, 11, 0), (3, 0, 13), (0, 0, -1)):
        t = R.standard_tables(12)
        t["alpha_merge"][kx, ky] = v
        assert _check(12, 12, t) == -1, (kx, ky, v)
        L = dynamics.load_library()
        assert f"alpha_merge[{kx}][{ky}] = {v}".encode() in L.nxs_dyn_last_error(None)
    t = R.standard_tables(12)
    assert (t["alpha_merge"][np.triu_indices(12, 1)] == -999).all()
    t["alpha_merge"][2, 7] = 40
    assert _check(12, 12, t) == 0
    t = R.standard_tables(12)
    t["bin_centres"] = None
    assert _check(12, 12, t) == -1                                            # a NULL table
    t = R.standard_tables(12)
    t["area_scaled_low"] = None
    assert _check(12, 12, t) == 0                                             # (no loop reads it)
    assert dynamics.load_library().nxs_fsd_config_check(None, 3) == -1


def test_the_python_mirror_refuses_an_unknown_option():
    with pytest.raises(KeyError):
        _abi.fsd_config_struct(3, R.standard_tables(3), breakup_coef4=1.)


def _llvm_tool(name):
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for sub in ("llvm/bin", "lib/llvm/bin"):
        if os.path.exists(os.path.join(root, sub, name)):
            return os.path.join(root, sub, name)
    raise AssertionError(f"{name} not found beside hipcc ({root})")


def test_no_fsd_kernel_uses_scratch_memory(tmp_path):
    """A thread keeps its bins in registers.  The source asks for that with fully unrolled loops, but for 12 and 16 bins the optimizer leaves the break-up's loop
    over the bins rolled, so what holds is what the backend emitted: read it from the gfx950 code object inside the built library."""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    kernels = {}
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\S+)$", block, flags=re.M))
        if "k_fsd_" in f.get("name", ""):
            kernels[f["name"]] = f
    builds = [k for k in kernels if re.search(r"k_fsd_(update|breakup|weld)ILi(2|6|12|16)E", k)]
    assert len(builds) == 12 and any("k_fsd_init" in k for k in kernels), sorted(kernels)
    for name, f in kernels.items():
        print(name, f)
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0, (name, f)
        assert int(f["vgpr_count"]) <= 256, (name, f)                # (two waves per SIMD at least)
