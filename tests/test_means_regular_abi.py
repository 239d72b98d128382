"""The Moorings means on the regular grid at the C ABI (include/nxs_dyn.h: nxs_dyn_means_regular_*): exported and declared, the ctypes mirror matches the header (a compiled
offsetof program), the enum values, the ABI version stays 2, what the entry points refuse without a handle (so without a device) -- plus the resources of the new
kernels read from the built library: no scratch memory, no spills."""
import ctypes as C
import os
import re
import shutil
import subprocess

from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
NEW = ("nxs_dyn_means_regular_set", "nxs_dyn_means_regular_lsm", "nxs_dyn_means_regular_update", "nxs_dyn_means_regular_get", "nxs_dyn_means_regular_reset")
KERNELS = ("k_means_regular_hits", "k_means_regular_gather", "k_means_regular_lsm")


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("means_regular_set", "means_regular_lsm", "means_regular_update", "means_regular_get", "means_regular_reset"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))
    hpp = open(os.path.join(ROOT, "include", "nxs_dyn.hpp")).read()
    for name in NEW:
        assert name + "(h_" in hpp, name


def test_layout_and_enums_match_the_header(tmp_path):
    T, s = _abi.MeansRegular, "nxs_dyn_means_regular"
    members = [k for k, _ in T._fields_]
    body = f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in members) + 'printf("\\n");'
    enums = ["NXS_MEANS_ROTATE_NONE", "NXS_MEANS_ROTATE_NORTH_EAST", "NXS_MEANS_ROTATE_GRID_THETA", "NXS_MEANS_MAX_PAIRS", "NXS_MEANS_MAX_VARS"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){' + body + "".join(f'printf("%d ", {e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    assert [int(v) for v in rows[0].split()] == [C.sizeof(T)] + [getattr(T, m).offset for m in members]
    assert [int(v) for v in rows[1].split()] == [0, 1, 2, 12, 24]
    assert (_abi.NXS_MEANS_ROTATE_NONE, _abi.NXS_MEANS_ROTATE_NORTH_EAST, _abi.NXS_MEANS_ROTATE_GRID_THETA, _abi.NXS_MEANS_MAX_PAIRS, _abi.NXS_MEANS_MAX_VARS) == (0, 1, 2, 12, 24)
    assert T.pair_first.size == T.pair_second.size == 12 * C.sizeof(C.c_int32)


def test_the_header_compiles_as_cxx_too(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "nxs_dyn.hpp"\nint main(){ nxs_dyn_means_regular p = {}; return p.ncols + p.nrows + p.n_pairs + p.pair_first[11] + (&nxs_dyn_means_regular_update == 0); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_errors_without_a_device():
    L = dynamics.load_library()
    p = _abi.MeansRegular()
    one = (C.c_int32 * 1)(0)
    d = (C.c_double * 1)(0.)
    assert L.nxs_dyn_means_regular_set(None, C.byref(p)) == -1 and L.nxs_dyn_means_regular_set(None, None) == -1
    assert L.nxs_dyn_means_regular_lsm(None, one, one) == -1 and L.nxs_dyn_means_regular_lsm(None, None, None) == -1
    assert L.nxs_dyn_means_regular_update(None) == -1
    assert L.nxs_dyn_means_regular_get(None, 0, d, d, None, None) == -1
    assert L.nxs_dyn_means_regular_reset(None) == -1


def _llvm_tool(name):
    root = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for sub in ("llvm/bin", "lib/llvm/bin"):
        if os.path.exists(os.path.join(root, sub, name)):
            return os.path.join(root, sub, name)
    raise AssertionError(f"{name} not found beside hipcc ({root})")


def test_the_kernels_use_no_scratch_memory_and_spill_nothing(tmp_path):
    """read from the gfx950 code objects inside the built library (one bundle per translation unit; the kernels live in nxs_dyn.hip's)"""
    fat = str(tmp_path / "fat.bin")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)] + [len(blob)]
    found = {}
    for n, (lo, hi) in enumerate(zip(starts[:-1], starts[1:])):
        part, co = str(tmp_path / f"fat{n}.bin"), str(tmp_path / f"dev{n}.co")
        with open(part, "wb") as f:
            f.write(blob[lo:hi])
        subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"])
        if not os.path.getsize(co):
            continue
        notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
        for block in notes.split("- .agpr_count:")[1:]:
            f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\S+)$", block, flags=re.M))
            for k in KERNELS:
                if re.search(r"\d" + k, f.get("name", "")):      # (no name is the start of another)
                    found[k] = f
    assert sorted(found) == sorted(KERNELS), sorted(found)
    for k, f in found.items():
        print(k, f)
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, f
        assert int(f["group_segment_fixed_size"]) == 0      # (k_means_regular_gather's interp_out is DYNAMIC LDS: 256 * n_nod doubles, nothing without nodal variables)
