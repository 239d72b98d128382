"""The grid map (nxs_gridmap_*, include/nxs_interp.h) and nxs_dyn_means_to_grid_conservative at the C ABI: exported and declared, the argument checks
that come before any device work, the function-try-block rule for the new definitions, and -- on a box without a GPU -- an error instead of a CPU
path.  No device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nextsim_amd import _abi, dynamics, interp
from test_abi import _has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDMAP = ("nxs_gridmap_create", "nxs_gridmap_destroy", "nxs_gridmap_info", "nxs_gridmap_mesh_to_grid", "nxs_gridmap_grid_to_mesh", "nxs_gridmap_export",
           "nxs_gridmap_import", "nxs_gridmap_restrict", "nxs_gridmap_debug_chunk")
INVALID, NO_DEVICE = -1, -2


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "nxs_interp.h")).read()
    for name in GRIDMAP:
        assert name in dynamics.INTERP_EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_INTERP_API int %s\(" % name, header), name
    name = "nxs_dyn_means_to_grid_conservative"
    assert name in dynamics.EXPORTS and f" T {name}\n" in out
    dh = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
    assert f"NXS_API int {name}(" in dh and "#define NXS_DYN_ABI_VERSION 2\n" in dh and L.nxs_dyn_abi_version() == 2
    assert "ConservativeRemappingMeshToGrid, rotateVectors" not in dh          # the OUT OF SCOPE comment was brought up to date
    for m in ("weights", "import_", "mesh_to_grid", "grid_to_mesh", "restrict", "export", "info"):
        assert callable(getattr(interp.GridMap, m)), m
    assert callable(dynamics.FiniteElementDynamics.means_to_grid_conservative)


def test_the_header_compiles_as_c(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "nxs_dyn.h"\n#include "nxs_interp.h"\nint main(void){ nxs_gridmap *m = 0; return nxs_gridmap_destroy(m) + (NXS_REGRID_OUT_DEVICE - 2); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "h.o")])


def test_argument_checks_before_any_device_work():
    L = interp._declare_gridmap()
    h = C.c_void_p()
    one, z = np.zeros(4), np.zeros(1, np.int32)
    D, I = _abi.dptr, _abi.iptr
    assert L.nxs_gridmap_create(None, D(one), D(one), D(one), D(one), 1, C.byref(h)) == INVALID and not h.value
    assert L.nxs_gridmap_create(None, D(one), D(one), D(one), D(one), 0, C.byref(h)) == INVALID
    assert L.nxs_gridmap_create(None, D(one), D(one), D(one), D(one), 1, None) == INVALID
    assert L.nxs_gridmap_destroy(None) == 0
    assert L.nxs_gridmap_info(None, None, None, None, None, None, None) == INVALID
    assert L.nxs_gridmap_mesh_to_grid(None, one.ctypes.data, one.ctypes.data, 1, 0., 0) == INVALID
    assert L.nxs_gridmap_grid_to_mesh(None, one.ctypes.data, one.ctypes.data, 1, 0) == INVALID
    assert L.nxs_gridmap_export(None, None, None, None, None, None, None) == INVALID
    assert L.nxs_gridmap_restrict(None, I(z), 1, C.byref(h)) == INVALID
    assert L.nxs_gridmap_debug_chunk(-1, None) == INVALID and L.nxs_gridmap_debug_chunk(0, None) == 0
    # import: sizes and lists are checked on the host, before a device is looked for
    gp, off, tr, w = np.array([0], np.int32), np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.ones(2)
    cx = np.zeros(8)
    imp = lambda nels, G, rows, gp_, off_, tr_: L.nxs_gridmap_import(0, nels, G, rows, I(gp_), I(off_), I(tr_), D(w), D(cx), D(cx), C.byref(h))  # noqa: E731
    assert imp(2, 0, 0, gp, off, tr) == INVALID                                  # G = 0
    assert imp(0, 2, 1, gp, off, tr) == INVALID                                  # no element
    assert imp(2, 2, 3, gp, off, tr) == INVALID                                  # more rows than cells
    assert imp(1, 2, 1, gp, off, tr) == INVALID                                  # a triangle beyond the mesh (a map of another mesh)
    assert imp(2, 2, 1, np.array([2], np.int32), off, tr) == INVALID             # a cell beyond the grid
    assert imp(2, 2, 1, gp, np.array([0, 0], np.int32), tr) == INVALID           # an empty row
    assert imp(2, 2, 1, gp, np.array([1, 2], np.int32), tr) == INVALID           # off[0] != 0
    assert L.nxs_gridmap_import(0, 2, 2, 1, I(gp), None, I(tr), D(w), D(cx), D(cx), C.byref(h)) == INVALID
    assert L.nxs_gridmap_import(0, 2, 2, 1, I(gp), I(off), I(tr), D(w), D(cx), D(cx), None) == INVALID
    assert not h.value
    Ld = dynamics.load_library()
    assert Ld.nxs_dyn_means_to_grid_conservative(None, None, 0., None) == INVALID


@pytest.mark.skipif(_has_gpu(), reason="a GPU is present: the no-device path cannot be exercised")
def test_no_gpu_means_error_not_cpu_fallback():
    lists = {"gridP": [0], "off": [0, 2], "tris": [0, 1], "w": [1., 1.], "cornerX": np.zeros((2, 4)), "cornerY": np.zeros((2, 4)), "nels": 2, "grid_size": 2}
    with pytest.raises(dynamics.NxsError) as e:
        interp.GridMap.import_(lists)
    assert e.value.code == NO_DEVICE and "no CPU path" in str(e.value)


def test_the_new_definitions_are_function_try_blocks():
    csrc = os.path.join(ROOT, "nextsim_amd", "csrc")
    seen = set()
    for fn, names in (("nxs_interp.hip", GRIDMAP), ("nxs_dyn.hip", ("nxs_dyn_means_to_grid_conservative",))):
        lines = open(os.path.join(csrc, fn)).read().split("\n")
        for i, line in enumerate(lines):
            m = re.match(r'^(?:extern "C" )?int (nxs_\w+)\(', line)
            if not m or m.group(1) not in names:
                continue
            j = i
            while not lines[j].split("//")[0].rstrip().endswith(("{", ";")):
                j += 1
            head = lines[j].split("//")[0].rstrip()
            if head.endswith(";"):
                continue
            assert head.endswith("try {"), f"{fn}:{j + 1}: {m.group(1)} is not a function-try-block"
            k = j + 1
            while not lines[k].startswith("}"):
                k += 1
            assert "catch (...)" in lines[k] and m.group(1) in lines[k], f"{fn}:{k + 1}: handler of {m.group(1)}"
            seen.add(m.group(1))
    assert seen == set(GRIDMAP) | {"nxs_dyn_means_to_grid_conservative"}
    # the kernels hold no entry point of their own
    assert 'extern "C"' not in open(os.path.join(csrc, "nxs_gridmap_kernels.inl")).read()
