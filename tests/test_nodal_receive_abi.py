"""The nodal half of a coupled run's receive at the C ABI (include/nxs_interp.h: nxs_nodemap_*; include/nxs_dyn.h: nxs_dyn_nodes_coupled_*): exported and declared,
the constants as a C compiler reads the headers against _abi, the ABI version unchanged, NULL and malformed arguments refused before any device work with the
messages the headers promise, the new definitions function-try-blocks, ONE copy of the east/north body and of the host's cos / sin rows, the out-of-scope passages
brought up to date, and the kernels' resources read from the built library.  No device."""
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
MAP = ("nxs_nodemap_create", "nxs_nodemap_destroy", "nxs_nodemap_info", "nxs_nodemap_device", "nxs_nodemap_export", "nxs_nodemap_import", "nxs_nodemap_set_source", "nxs_nodemap_receive_rows",
       "nxs_nodemap_debug_source")
DYN = ("nxs_nodes_coupled_default_config", "nxs_dyn_nodes_coupled_attach", "nxs_dyn_nodes_coupled_receive", "nxs_dyn_nodes_coupled_get")
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
    for name in ("weights", "import_", "export", "info", "set_source", "receive_rows", "debug_source", "close"):
        assert callable(getattr(interp.NodeMap, name)), name
    for name in ("nodes_coupled_attach", "nodes_coupled_detach", "nodes_coupled_receive", "nodes_coupled_get"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name)), name
    hpp = open(os.path.join(ROOT, "include", "nxs_dyn.hpp")).read()
    for name in DYN[1:]:
        assert name + "(h_" in hpp, name


def test_constants_and_struct_layouts_match_the_headers(tmp_path):
    enums = ("NXS_NODEMAP_MAX_RECEIVE", "NXS_NODEMAP_GET", "NXS_REGRID_IN_DEVICE", "NXS_REGRID_OUT_DEVICE", "NXS_NODEMAP_ROTATE_NONE", "NXS_NODEMAP_ROTATE_UNIFORM",
             "NXS_NODEMAP_ROTATE_GRID_THETA", "NXS_NC_OCEAN", "NXS_NC_WAVE", "NXS_NC_DATASETS", "NXS_NC_MAX_FIELDS", "NXS_DYN_ABI_VERSION")
    sizes = ("sizeof(nxs_nodemap_source)", "offsetof(nxs_nodemap_source, reduced)", "offsetof(nxs_nodemap_source, cos_m_diff_angle)", "offsetof(nxs_nodemap_source, theta)",
             "offsetof(nxs_nodemap_source, map)", "offsetof(nxs_nodemap_source, delta_t)", "sizeof(nxs_dyn_nodes_coupled_config)", "offsetof(nxs_dyn_nodes_coupled_config, bias)")
    src = tmp_path / "en.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_interp.h"\n#include "nxs_dyn.h"\nint main(void){'
                   + "".join(f'printf("%d ", (int){e});' for e in enums + sizes) + 'return 0;}\n')      # nxs_interp.h FIRST: it stands without nxs_dyn.h
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "en")])
    v = dict(zip(enums + sizes, (int(x) for x in subprocess.check_output([str(tmp_path / "en")], text=True).split())))
    assert v["NXS_NODEMAP_MAX_RECEIVE"] == _abi.NXS_NODEMAP_MAX_RECEIVE == 4 and v["NXS_NODEMAP_GET"] == _abi.NXS_NODEMAP_GET == interp.NodeMap.GET
    assert v["NXS_NODEMAP_GET"] & (v["NXS_REGRID_IN_DEVICE"] | v["NXS_REGRID_OUT_DEVICE"]) == 0      # a flag of its own
    assert (interp.NodeMap.IN_DEVICE, interp.NodeMap.OUT_DEVICE) == (v["NXS_REGRID_IN_DEVICE"], v["NXS_REGRID_OUT_DEVICE"])
    assert _abi.NODEMAP_ROTATE == {"none": v["NXS_NODEMAP_ROTATE_NONE"], "uniform": v["NXS_NODEMAP_ROTATE_UNIFORM"], "grid_theta": v["NXS_NODEMAP_ROTATE_GRID_THETA"]}
    assert _abi.NC_DATASETS.index("ocean") == v["NXS_NC_OCEAN"] and _abi.NC_DATASETS.index("wave") == v["NXS_NC_WAVE"] and len(_abi.NC_DATASETS) == v["NXS_NC_DATASETS"]
    assert _abi.NXS_NC_MAX_FIELDS == v["NXS_NC_MAX_FIELDS"] == max(len(f) for f in _abi.NC_FIELDS.values()) and v["NXS_DYN_ABI_VERSION"] == 2
    S, K = _abi.NodemapSource, _abi.NodesCoupledConfig
    assert C.sizeof(S) == v["sizeof(nxs_nodemap_source)"] and C.sizeof(K) == v["sizeof(nxs_dyn_nodes_coupled_config)"] and K.bias.offset == v["offsetof(nxs_dyn_nodes_coupled_config, bias)"]
    for k in ("reduced", "cos_m_diff_angle", "theta", "map", "delta_t"):
        assert getattr(S, k).offset == v[f"offsetof(nxs_nodemap_source, {k})"], k
    kern = open(os.path.join(CSRC, "nxs_nodemap_kernels.inl")).read()
    assert "kMaxVar = 4" in kern and "ROTATE_NONE = 0, ROTATE_UNIFORM = 1, ROTATE_GRID_THETA = 2" in kern


def test_null_and_malformed_arguments_are_refused_before_any_device_work():
    L = dynamics.load_library()
    Li = interp._declare_nodemap()
    h, x = C.c_void_p(), np.zeros(3)
    assert Li.nxs_nodemap_create(None, _abi.dptr(x), _abi.dptr(x), 3, 0, C.byref(h)) == INVALID and "nodemap_create: NULL argument" in last() and not h.value
    assert Li.nxs_nodemap_create(None, None, None, 3, 0, None) == INVALID and "out is NULL" in last()
    assert Li.nxs_nodemap_destroy(None) == 0
    assert Li.nxs_nodemap_info(None, None, None, None) == INVALID and Li.nxs_nodemap_export(None, None, None, None, None, None, None) == INVALID
    assert Li.nxs_nodemap_device(None, None) == INVALID and "nodemap_device: NULL argument" in last()
    assert Li.nxs_nodemap_set_source(None, None) == INVALID and "nodemap_set_source: NULL argument" in last()
    assert Li.nxs_nodemap_receive_rows(None, 1, None, None, None, None, None, None, None, 0, None) == INVALID and "nodemap_receive_rows: NULL argument" in last()
    assert Li.nxs_nodemap_debug_source(None, None, 1) == INVALID
    v, a = np.zeros(4, np.int32), np.full(4, 1. / 3.)
    args = lambda vv, N=4, R=2: (0, N, R, _abi.iptr(vv), _abi.iptr(v), _abi.iptr(v), _abi.dptr(a), _abi.dptr(a), _abi.dptr(a), C.byref(h))  # noqa: E731
    bad = v.copy(); bad[2] = 2
    assert Li.nxs_nodemap_import(*args(bad)) == INVALID and "v0[2] = 2 is not a source node (0 .. 1)" in last()
    bad[2] = -1
    assert Li.nxs_nodemap_import(*args(bad)) == INVALID and "v0[2] = -1" in last()
    assert Li.nxs_nodemap_import(*args(v, N=0)) == INVALID and "must be positive" in last()
    assert Li.nxs_nodemap_import(0, 4, 2, None, _abi.iptr(v), _abi.iptr(v), _abi.dptr(a), _abi.dptr(a), _abi.dptr(a), C.byref(h)) == INVALID and "NULL argument" in last()
    assert Li.nxs_nodemap_import(0, 4, 2, _abi.iptr(v), _abi.iptr(v), _abi.iptr(v), _abi.dptr(a), _abi.dptr(a), _abi.dptr(a), None) == INVALID
    c = _abi.NodesCoupledConfig()
    assert L.nxs_nodes_coupled_default_config(None) == INVALID and L.nxs_nodes_coupled_default_config(C.byref(c)) == 0
    assert list(c.a) == [1.] * 3 and list(c.b) == [0.] * 3 and list(c.factor) == [1.] * 3 and list(c.bias) == [0.] * 3
    assert L.nxs_dyn_nodes_coupled_attach(None, 0, None, C.byref(c)) == INVALID and L.nxs_dyn_nodes_coupled_receive(None, 0, None, 3, 0) == INVALID
    assert L.nxs_dyn_nodes_coupled_get(None, 0, None, None) == INVALID


def test_a_machine_without_a_device_says_so_and_never_falls_back():
    Li = interp._declare_nodemap()
    h, v, a = C.c_void_p(), np.zeros(4, np.int32), np.full(4, 1. / 3.)
    rc = Li.nxs_nodemap_import(0, 4, 2, _abi.iptr(v), _abi.iptr(v), _abi.iptr(v), _abi.dptr(a), _abi.dptr(a), _abi.dptr(a), C.byref(h))
    if rc == 0:      # a machine with a device: the map is made
        assert h.value and Li.nxs_nodemap_destroy(h) == 0
        return
    assert rc == NO_DEVICE and "no CPU path" in last() and not h.value


def test_the_unmappable_source_is_one_the_completion_refuses():
    """the precondition of tests/test_gpu_nodal_receive.py::test_a_source_without_completion_is_refused, on the host: both constructions refuse the source, each
    with its own reason, so nxs_nodemap_create meets a context without completion there"""
    import pytest
    import nodal_receive_ref as R
    x, y, tri, why = R.unmappable_source()
    for mode, texts in ((0, ("several outer boundary loops", why)), (1, (why,)), (2, ("several outer boundary loops",))):
        with pytest.raises(dynamics.NxsError) as e:
            interp.convex_completion(tri + 1, x, y, mode)
        assert e.value.code == INVALID and "no convex completion" in str(e.value) and all(t in str(e.value) for t in texts), (mode, str(e.value))
    full = R.source("full")
    fill, hull = interp.convex_completion(full["tri"] + 1, full["x"], full["y"])      # ... and one copy alone completes
    assert hull.shape[0] >= 4
    src = open(os.path.join(CSRC, "nxs_interp.hip")).read()
    assert "if (!locp->comp.ok || locp->d.nhull < 1)" in src and "a map never holds stand-in weights" in src


def test_the_new_definitions_are_function_try_blocks():
    seen = set()
    for fn, names in (("nxs_interp.hip", MAP), ("nxs_nodes_coupled.inl", DYN)):
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
            assert "catch (...)" in lines[k] and m.group(1) in lines[k], f"{fn}:{k + 1}: handler of {m.group(1)}"
            seen.add(m.group(1))
    assert seen == set(MAP) | set(DYN)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    for f in ("nxs_nodemap_kernels.inl", "nxs_nodes_coupled.inl", "nxs_east_north_body.inl", "nxs_angles.hpp"):
        assert f in mk, f


def test_one_copy_of_every_shared_body():
    """the east/north point, the host's cos / sin rows, the locator and the wave stress's attachment are each stated once and used from both sides"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".inl", ".hip", ".hpp", ".cpp"))}
    everything = "\n".join(text.values())
    assert len(re.findall(r"void nf_east_north_point\(", everything)) == 1 and "void nf_east_north_point(" in text["nxs_east_north_body.inl"]
    assert "nf_east_north_point(a.map, a.R," in text["nxs_nodal_forcing_kernels.inl"] and "nf_east_north_point(s.map, s.Re," in text["nxs_nodemap_kernels.inl"]
    assert len(re.findall(r"void nxs_cos_sin_of_difference\(", everything)) == 1
    assert "nxs_cos_sin_of_difference(" in text["nxs_means_points.inl"] and "nxs_cos_sin_of_difference(s->rotation, s->theta[i]" in text["nxs_interp.hip"]
    assert "std::cos(" not in text["nxs_means_points.inl"] and not re.search(r"\b(cos|sin)\s*\(", "\n".join(line.split("//")[0] for line in text["nxs_nodemap_kernels.inl"].split("\n")))
    assert len(re.findall(r"int locate\(const InterpDev", everything)) == 1 and "locate(d, x, y, dd, Bx, By)" in text["nxs_nodemap_kernels.inl"]
    assert everything.count("h->dw.tau_wi = h->d_tau_wi") == 1 and text["nxs_nodes_coupled.inl"].count("wave_stress_attach(h, was)") == 1
    assert "wave_stress_attach(h, was)" in text["nxs_dyn.hip"] and "hipLaunchKernelGGL" not in text["nxs_nodes_coupled.inl"]
    assert "release_nodes_coupled(h);" in text["nxs_dyn.hip"].split("void release_mesh(nxs_dyn_handle *h) {")[1].split("\n}")[0]      # set_mesh and regrid both detach
    gather = text["nxs_nodemap_kernels.inl"].split("k_nodemap_gather(")[1]
    assert "atomic" not in gather and "__shared__" not in gather


def test_the_out_of_scope_sentences_were_brought_up_to_date():
    assert "OUT OF SCOPE: the nodal half of the receive" not in HEADER
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 6p." in design and "**Out of scope.**  The nodal half of the receive" not in design and "the nodal half of the receive (§6n)" not in design
    assert "the nodal half of a coupled ocean's receive and, of its outgoing side" not in design
    assert "nodal-receive-measurement:begin" in design
    assert "## 5r." in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for f in ("README.md", "INTEGRATION.md"):
        assert "nxs_dyn_nodes_coupled_receive" in open(os.path.join(ROOT, f)).read(), f


def test_the_kernels_resources(tmp_path):
    """the gather keeps three vertices, three weights and its sums in registers: no scratch, no LDS, no spill, in all four builds; k_interp, which the change does not touch, and k_nf_east_north,
    whose point body moved into a file of its own, keep the resources they had"""
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
        for key in ("k_nodemap_gather", "k_nodemap_source", "k_nodemap_weights", "k_interpE", "k_nf_east_north"):
            if key in f.get("name", ""):
                found.setdefault(key, []).append(f)
    assert len(found["k_nodemap_gather"]) == 4 and len(found["k_nodemap_source"]) == 1 and len(found["k_nodemap_weights"]) == 1 and len(found["k_interpE"]) == 1, {k: len(v) for k, v in found.items()}
    for f in found["k_nodemap_gather"]:
        assert int(f["private_segment_fixed_size"]) == 0 and int(f["group_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, f
        assert int(f["vgpr_count"]) <= 32, f
    for key in ("k_nodemap_source", "k_nodemap_weights", "k_interpE", "k_nf_east_north"):
        for f in found[key]:
            assert int(f["private_segment_fixed_size"]) == 0 and int(f["group_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0, f
    assert int(found["k_interpE"][0]["vgpr_count"]) == 50 and int(found["k_nf_east_north"][0]["vgpr_count"]) == 66      # as before: k_interp is untouched, k_nf_east_north calls the point body where it now lives
    print({k: [(f["vgpr_count"], f["sgpr_spill_count"]) for f in v] for k, v in found.items()})
