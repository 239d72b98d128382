"""Forcing given on a triangulated source at the C ABI (include/nxs_interp.h: nxs_nodemap_load_rows, nxs_nodemap_debug_load; include/nxs_dyn.h:
nxs_dyn_forcing_*_mesh, nxs_dyn_thermo_forcing_*_mesh): exported and declared, nxs_nodemap_load as a C compiler reads the header against _abi, the ABI version
unchanged, NULL and out-of-range arguments refused before any device work, the no-device answer, the new definitions function-try-blocks, the Makefile's list, ONE
copy of the east/north body, the files that must not move, and the new kernels' resources read from the built library.  No device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from nextsim_amd import _abi, dynamics, interp
from test_column_abi import _llvm_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextsim_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
IHEADER = open(os.path.join(ROOT, "include", "nxs_interp.h")).read()
MAP = ("nxs_nodemap_load_rows", "nxs_nodemap_debug_load")
DYN = ("nxs_dyn_forcing_attach_mesh", "nxs_dyn_forcing_ingest_mesh", "nxs_dyn_thermo_forcing_attach_mesh", "nxs_dyn_thermo_forcing_ingest_mesh")
INVALID, NO_DEVICE = -1, -2


def last():
    return interp._declare_nodemap().nxs_interp_last_error().decode()


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in MAP:
        assert name in dynamics.INTERP_EXPORTS and f" T {name}\n" in out and re.search(r"NXS_INTERP_API int " + name + r"\(", IHEADER), name
    for name in DYN:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out and re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("load_rows", "debug_load"):
        assert callable(getattr(interp.NodeMap, name)), name
    for name in ("forcing_attach_mesh", "forcing_ingest_mesh", "thermo_forcing_attach_mesh", "thermo_forcing_ingest_mesh"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name)), name
    hpp = open(os.path.join(ROOT, "include", "nxs_dyn.hpp")).read()
    for name in DYN:
        assert name + "(h_" in hpp, name


def test_the_struct_layout_matches_the_header(tmp_path):
    enums = ("NXS_NODEMAP_MAX_LOAD", "NXS_NODEMAP_MAX_RECEIVE", "NXS_REGRID_IN_DEVICE", "NXS_REGRID_OUT_DEVICE", "NXS_NF_SETS", "NXS_TF_SETS", "NXS_NF_ROWS", "NXS_TF_ROWS",
             "NXS_DYN_ABI_VERSION")
    members = ("n_var", "n_step", "fields", "scale_factor", "add_offset", "a", "b", "pairs")
    sizes = ("sizeof(nxs_nodemap_load)",) + tuple(f"offsetof(nxs_nodemap_load, {m})" for m in members)
    src = tmp_path / "en.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_interp.h"\n#include "nxs_dyn.h"\nint main(void){'
                   + "".join(f'printf("%d ", (int){e});' for e in enums + sizes) + 'return 0;}\n')      # nxs_interp.h FIRST: it stands without nxs_dyn.h
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "en")])
    v = dict(zip(enums + sizes, (int(x) for x in subprocess.check_output([str(tmp_path / "en")], text=True).split())))
    assert v["NXS_NODEMAP_MAX_LOAD"] == _abi.NXS_NODEMAP_MAX_LOAD == 8 == 2 * v["NXS_NODEMAP_MAX_RECEIVE"] and v["NXS_DYN_ABI_VERSION"] == 2
    assert (interp.NodeMap.IN_DEVICE, interp.NodeMap.OUT_DEVICE) == (v["NXS_REGRID_IN_DEVICE"], v["NXS_REGRID_OUT_DEVICE"])
    assert v["NXS_NF_SETS"] == _abi.NXS_NF_SETS and v["NXS_NF_ROWS"] == len(_abi.NF_ROWS) and v["NXS_TF_ROWS"] == len(_abi.TF_ROWS)
    S = _abi.NodemapLoad
    assert C.sizeof(S) == v["sizeof(nxs_nodemap_load)"]
    for m in members:
        assert getattr(S, m).offset == v[f"offsetof(nxs_nodemap_load, {m})"], m
    # nxs_dyn.h alone: the load is an incomplete type there, and the two headers agree on its tag
    alone = tmp_path / "alone.c"
    alone.write_text('#include "nxs_dyn.h"\n#include "nxs_interp.h"\nint main(void){ nxs_nodemap_load l; l.n_var = 1; return nxs_dyn_forcing_ingest_mesh(0, 0, &l, 0, 0) == 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(alone)])
    kern = open(os.path.join(CSRC, "nxs_nodemap_load_kernels.inl")).read()
    assert "kMaxLoad = 8" in kern and "NXS_NODEMAP_MAX_LOAD == nodemap::kMaxLoad" in open(os.path.join(CSRC, "nxs_interp.hip")).read()
    host = open(os.path.join(ROOT, "tests", "mesh_forcing_host_kernel.cpp")).read()      # the host program restates the two enums the load kernels' file continues
    base = open(os.path.join(CSRC, "nxs_nodemap_kernels.inl")).read()
    for line in ("enum { kMaxVar = 4, kMaxPairs = 2 };", "enum { ROTATE_NONE = 0, ROTATE_UNIFORM = 1, ROTATE_GRID_THETA = 2 };"):
        assert line in base and line in host, line


def test_null_and_out_of_range_arguments_are_refused_before_any_device_work():
    L = dynamics.load_library()
    Li = interp._declare_nodemap()
    assert Li.nxs_nodemap_load_rows(None, None, None, 0, None) == INVALID and "nodemap_load_rows: NULL argument" in last()
    assert Li.nxs_nodemap_debug_load(None, None, 1) == INVALID and "nodemap_debug_load: NULL argument" in last()
    l, out = _abi.NodemapLoad(), (C.c_void_p * 8)()
    fake = C.c_void_p(8)      # (never dereferenced: a NULL load or rows array is refused first)
    assert Li.nxs_nodemap_load_rows(fake, None, out, 0, None) == INVALID and "NULL argument" in last()
    assert Li.nxs_nodemap_load_rows(fake, C.byref(l), None, 0, None) == INVALID and "NULL argument" in last()
    assert Li.nxs_nodemap_load_rows(fake, C.byref(l), out, 0, None) == INVALID and "NULL argument (fields)" in last()
    f = np.zeros(4)
    src = (C.c_void_p * 8)(*([f.ctypes.data] * 8))
    l.fields = C.cast(src, C.POINTER(C.c_void_p))
    for n_var, n_step, text in ((0, 1, "n_var = 0 (1 .. 4)"), (5, 1, "n_var = 5 (1 .. 4)"), (2, 0, "n_step = 0 (1 or 2)"), (2, 3, "n_step = 3 (1 or 2)")):
        l.n_var, l.n_step = n_var, n_step
        assert Li.nxs_nodemap_load_rows(fake, C.byref(l), out, 0, None) == INVALID and text in last(), text
    l.n_var, l.n_step = 2, 2
    for k in range(8):
        l.scale_factor[k], l.a[k] = 1., 1.
    src[3] = None
    assert Li.nxs_nodemap_load_rows(fake, C.byref(l), out, 0, None) == INVALID and "field 3 (forcing step 1, variable 1) is NULL" in last()
    src[3] = f.ctypes.data
    l.add_offset[2] = float("inf")
    assert Li.nxs_nodemap_load_rows(fake, C.byref(l), out, 0, None) == INVALID and "of column 2 is not finite" in last()
    l.add_offset[2] = 0.
    l.b[7] = float("nan")      # beyond the four columns of this load: not read
    assert Li.nxs_nodemap_load_rows(fake, C.byref(l), out, 0, None) == INVALID and "every column is skipped" in last()
    out[1] = f.ctypes.data
    for pairs, text in (((0, -1, -1, -1), "pairs[0] = 0 is not another variable"), ((2, -1, -1, -1), "pairs[0] = 2 is not another variable (0 .. 1)"), ((1, 0, -1, -1), "named by two pairs")):
        for k in range(4):
            l.pairs[k] = pairs[k]
        assert Li.nxs_nodemap_load_rows(fake, C.byref(l), out, 0, None) == INVALID and text in last(), text
    # the handle's entries: NULL before anything else
    ip = np.zeros(3, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.nxs_dyn_forcing_attach_mesh(None, 0, None) == INVALID and L.nxs_dyn_thermo_forcing_attach_mesh(None, 0, None) == INVALID
    assert L.nxs_dyn_forcing_ingest_mesh(None, 0, C.byref(l), ip, 0) == INVALID and L.nxs_dyn_thermo_forcing_ingest_mesh(None, 0, C.byref(l), ip, 0) == INVALID


def test_a_machine_without_a_device_says_so_and_never_falls_back():
    """a map cannot be made without a device (nxs_nodemap_import answers NXS_ERR_NO_DEVICE: tests/test_nodal_receive_abi.py), so the load's own answer is reached
    only behind its argument checks; the source states it, and there is no CPU path to fall back to"""
    Li = interp._declare_nodemap()
    h, v, a = C.c_void_p(), np.zeros(4, np.int32), np.full(4, 1. / 3.)
    rc = Li.nxs_nodemap_import(0, 4, 2, _abi.iptr(v), _abi.iptr(v), _abi.iptr(v), _abi.dptr(a), _abi.dptr(a), _abi.dptr(a), C.byref(h))
    if rc == 0:      # a machine with a device: the map is made
        assert h.value and Li.nxs_nodemap_destroy(h) == 0
    else:
        assert rc == NO_DEVICE and "no CPU path" in last() and not h.value
    src = open(os.path.join(CSRC, "nxs_interp.hip")).read()
    body = src.split('extern "C" int nxs_nodemap_load_rows(')[1].split("} catch (...)")[0]
    assert 'return fail(NXS_ERR_NO_DEVICE, "no HIP device visible: the node map has no CPU path")' in body
    assert body.index("NXS_ERR_NO_DEVICE") < body.index("hipSetDevice") < body.index("hipLaunchKernelGGL")


def test_the_new_definitions_are_function_try_blocks():
    seen = set()
    for fn, names in (("nxs_interp.hip", MAP), ("nxs_mesh_forcing.inl", DYN)):
        lines = open(os.path.join(CSRC, fn)).read().split("\n")
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
            assert "catch (...)" in lines[k] and m.group(1) in lines[k] and ("entry_caught(" in lines[k] or "dyn_caught(h, " in lines[k]), f"{fn}:{k + 1}: handler of {m.group(1)}"
            seen.add(m.group(1))
    assert seen == set(MAP) | set(DYN)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    dep = mk.split("libnxsdyn.so:")[1].split("\n")[0]
    for f in ("nxs_nodemap_load_kernels.inl", "nxs_mesh_forcing.inl", "nxs_nodemap_kernels.inl", "nxs_east_north_body.inl"):
        assert f" {f} " in dep, f


def test_one_copy_of_every_shared_body_and_where_the_new_code_lives():
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".inl", ".hip", ".hpp", ".cpp"))}
    everything = "\n".join(text.values())
    assert len(re.findall(r"void nf_east_north_point\(", everything)) == 1 and "void nf_east_north_point(" in text["nxs_east_north_body.inl"]
    load = text["nxs_nodemap_load_kernels.inl"]
    assert load.count("nf_east_north_point(s.map, s.Re,") == 1 and '#include "nxs_east_north_body.inl"' not in load      # called once, in a loop that is not unrolled
    code = "\n".join(line.split("//")[0] for line in load.split("\n"))
    assert not re.search(r"\b(cos|sin)\s*\(", code) and "atomic" not in code and "__shared__" not in code
    assert code.count("#pragma unroll 1") == 2 and "fstep" in code.split("k_nodemap_load(LoadArgs s)")[1].split("struct ColsArgs")[0]
    gather = code.split("k_nodemap_cols_gather(")[1]
    assert "factor" not in gather and "bias" not in gather      # ExternalData::get is the time blend's
    # included behind the node map's kernels, which stay as they are
    assert text["nxs_interp.hip"].index('#include "nxs_nodemap_kernels.inl"\n#include "nxs_nodemap_load_kernels.inl"') > text["nxs_interp.hip"].index("int locate(const InterpDev")
    assert text["nxs_dyn.hip"].index('#include "nxs_nodes_coupled.inl"\n#include "nxs_mesh_forcing.inl"') > 0
    assert "hipLaunchKernelGGL" not in text["nxs_mesh_forcing.inl"] and "hipMalloc" not in text["nxs_mesh_forcing.inl"]      # no kernel, no buffer of its own
    assert "release_mesh_forcing(h);" in text["nxs_dyn.hip"].split("void release_mesh(nxs_dyn_handle *h) {")[1].split("\n}")[0]      # set_mesh and regrid both detach
    # the staging buffer is made by the first load, not by set_source
    set_source = text["nxs_interp.hip"].split('extern "C" int nxs_nodemap_set_source(')[1].split("} catch (...)")[0]
    assert "dload" not in set_source and "m->dload.alloc(" in text["nxs_interp.hip"].split('extern "C" int nxs_nodemap_load_rows(')[1].split("} catch (...)")[0]
    for doc, mark in (("DESIGN.md", "## 6q."), ("DESIGN.md", "mesh-forcing-measurement:begin"), ("INTEGRATION.md", "nxs_dyn_forcing_ingest_mesh"), ("INTEGRATION.md", "nxs_dyn_thermo_forcing_ingest_mesh")):
        assert mark in open(os.path.join(ROOT, doc)).read(), (doc, mark)


def test_the_kernels_resources(tmp_path):
    """the two new kernels at every instantiation: no scratch, no LDS, no VGPR spilled to memory; the gather keeps three vertices, three weights and its sums in
    registers and spills no SGPR either.  The kernels the change does not touch keep the figures they had (DESIGN 6q's table)."""
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
    found = {}
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\S+)$", block, flags=re.M))
        for key in ("k_nodemap_cols_gatherILi", "k_nodemap_loadE", "k_nodemap_gatherILi", "k_nodemap_sourceE", "k_interpE", "k_nf_east_north"):
            if key in f.get("name", ""):
                found.setdefault(key, []).append(f)
    assert len(found["k_nodemap_cols_gatherILi"]) == 8 and len(found["k_nodemap_loadE"]) == 1 and len(found["k_nodemap_gatherILi"]) == 4, {k: len(v) for k, v in found.items()}
    for f in found["k_nodemap_cols_gatherILi"]:
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["group_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, f
        assert int(f["vgpr_count"]) <= 32, f
    f = found["k_nodemap_loadE"][0]
    assert int(f["private_segment_fixed_size"]) == 0 and int(f["group_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0, f
    assert int(f["vgpr_count"]) <= 128, f      # one copy of the east/north body: k_nodemap_source carries two at 108
    untouched = {"k_interpE": [50], "k_nf_east_north": [66], "k_nodemap_sourceE": [108], "k_nodemap_gatherILi": [20, 26, 26, 28]}
    for key, want in untouched.items():
        assert sorted(int(f["vgpr_count"]) for f in found[key]) == want, (key, [f["vgpr_count"] for f in found[key]])
        for f in found[key]:
            assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0, f
    print({k: [(f["vgpr_count"], f["sgpr_spill_count"]) for f in v] for k, v in found.items()})
