"""thermo()'s slab loop with floe-size bins attached at the C ABI (include/nxs_dyn.h: nxs_slab_coupled_config_check, nxs_dyn_slab_coupled*): exported and declared,
the ctypes mirrors match the header, what nxs_slab_coupled_config_check refuses (host only, so without a device), and the resources of the kernels read from the
built library: no scratch memory and no spilled vector register in the two new kernels (their VGPR counts are printed; they are in DESIGN.md 6h and are not
bounded here), and k_slab and every k_fsd_* build exactly as the commit before this one built them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from nextsim_amd import _abi, dynamics
from test_slab_abi import _llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
NEW = ("nxs_slab_coupled_config_check", "nxs_dyn_slab_coupled_configure", "nxs_dyn_slab_coupled", "nxs_dyn_slab_coupled_info")
# (vgpr_count, sgpr_count, private_segment_fixed_size) of the gfx950 code object as commit 25fa963 ("Run the rest of thermo()'s slab loop on the device: new ice to
# tracers"), the parent of the change that made k_slab's body and k_fsd_weld's welding shared device functions, builds them (ROCm 7.2): the refactoring must not
# move them
PARENT = {
    "k_slab": (128, 106, 0), "k_fsd_init": (10, 19, 0),
    "k_fsd_updateILi2E": (20, 44, 0), "k_fsd_updateILi6E": (56, 49, 0), "k_fsd_updateILi12E": (96, 98, 0), "k_fsd_updateILi16E": (84, 106, 0),
    "k_fsd_breakupILi2E": (66, 106, 0), "k_fsd_breakupILi6E": (95, 106, 0), "k_fsd_breakupILi12E": (167, 106, 0), "k_fsd_breakupILi16E": (180, 106, 0),
    "k_fsd_weldILi2E": (38, 68, 0), "k_fsd_weldILi6E": (61, 106, 0), "k_fsd_weldILi12E": (94, 106, 0), "k_fsd_weldILi16E": (104, 106, 0),
}


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("slab_coupled_configure", "slab_coupled", "slab_coupled_info"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))
    assert callable(dynamics.slab_coupled_config_check)


def test_layouts_match_the_header(tmp_path):
    enums = ["NXS_SLAB_FSD_BR_" + k.upper() for k in _abi.SLAB_FSD_BRANCHES]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){printf("%zu %zu\\n", sizeof(struct nxs_dyn_slab_coupled_info), '
                   'offsetof(struct nxs_dyn_slab_coupled_info, thermo_fsd_crash));' + "".join(f'printf("%d ", {e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    assert [int(v) for v in rows[0].split()] == [C.sizeof(_abi.SlabCoupledInfo), _abi.SlabCoupledInfo.thermo_fsd_crash.offset]
    assert [int(v) for v in rows[1].split()] == [1 << i for i in range(len(_abi.SLAB_FSD_BRANCHES))]
    assert not set(e[len("NXS_SLAB_FSD_BR_"):].lower() for e in enums) & set(_abi.SLAB_BRANCHES)             # NXS_SLAB_BR_* keeps its numbers: a word of its own


def test_what_the_coupled_check_accepts_and_refuses():
    chk = dynamics.slab_coupled_config_check
    err = lambda: dynamics.load_library().nxs_dyn_last_error(None)
    for melt_type, bins in ((1, 0), (2, 0), (1, 12), (2, 1), (3, 1), (3, 16)):
        assert chk(melt_type, bins) == 0, (melt_type, bins)
    assert chk(3, 12, melt_type=1) == 0 and chk(1, 0, melt_type=2, newice_type=1) == 0                      # the slab's own melt_type is replaced
    assert chk(3, 0) == -1 and b"melt_type = 3" in err() and b"attached_bins = 0" in err()                   # the throw of FE.cpp:5595
    assert chk(3, -1) == -1 and b"attached_bins = -1" in err()
    for bad in (0, 4, -1):
        assert chk(bad, 12) == -1 and f"melt_type = {bad} (1 .. 3".encode() in err()
    # everything else is the slab's own check, the message naming the field
    for b in (dict(newice_type=0), dict(newice_type=5), dict(hnull=0.), dict(PhiF=-1.), dict(h_young_min=0.), dict(h_young_max=0.01), dict(meltpond_depth_to_fraction=0.),
              dict(time_relaxation_damage=float("nan")), dict(deltaT_relaxation_damage=0.)):
        for melt_type in (1, 2, 3):
            assert chk(melt_type, 12, **b) == -1, b
            assert next(iter(b)).encode() in err(), (b, err())
    assert dynamics.load_library().nxs_slab_coupled_config_check(None, 2, 0) == -1
    assert dynamics.slab_config_check(melt_type=3) == -1 and b"OASIS" in err()                               # nxs_slab_config_check is as it was
    with pytest.raises(KeyError):
        chk(3, 12, h_null=0.3)


def _kernels():
    fat, co = "fat.bin", "dev.co"
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, fat), os.path.join(d, co)
        subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
        subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
        notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    found = {}
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count|sgpr_count):\s+(\S+)$", block, flags=re.M))
        found[f.get("name", "")] = f
    return found


@pytest.fixture(scope="module")
def kernels():
    dynamics.load_library()
    return _kernels()


def test_the_new_kernels_use_no_scratch_memory_and_spill_no_vector_register(kernels):
    new = {k: f for k, f in kernels.items() if "k_coupled_" in k}
    assert len(new) == 5 and sum("k_coupled_thermo" in k for k in new) == 1, sorted(new)
    assert {m.group(1) for k in new for m in [re.search(r"k_coupled_binsILi(\d+)E", k)] if m} == {"2", "6", "12", "16"}
    for k, f in sorted(new.items()):
        print(k, f)
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["group_segment_fixed_size"]) == 0, (k, f)
    assert not any("k_slab" in k or "k_fsd_" in k for k in new)                                              # the counts of tests/test_slab_abi.py, test_fsd_abi.py stay


def test_k_slab_and_the_fsd_kernels_build_as_the_parent_commit_built_them(kernels):
    seen = set()
    for name, f in kernels.items():
        for key, want in PARENT.items():
            if re.search(r"\d+" + re.escape(key) + r"(E|v|\d)", name):
                seen.add(key)
                got = (int(f["vgpr_count"]), int(f["sgpr_count"]), int(f["private_segment_fixed_size"]))
                assert got == want, (name, got, want)
    assert seen == set(PARENT), set(PARENT) - seen
