"""thermo()'s atmospheric bulk fluxes at the C ABI (include/nxs_dyn.h: nxs_flux_*, nxs_dyn_flux_*, nxs_dyn_fluxes): exported and declared, the ctypes mirrors
match the header, the defaults and the constants are the reference's (tests/golden/thermo_flux_options.json, reference_constants.json), and what
nxs_dyn_flux_configure refuses -- through nxs_flux_config_check, the same check without a handle, so without a device."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import fluxes_ref as R
from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
NEW = ("nxs_flux_default_config", "nxs_flux_config_check", "nxs_flux_constants", "nxs_dyn_flux_configure", "nxs_dyn_flux_set_atmosphere", "nxs_dyn_flux_put",
       "nxs_dyn_flux_get", "nxs_dyn_fluxes", "nxs_dyn_fluxes_get")


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("flux_configure", "flux_set_atmosphere", "flux_put", "flux_get", "fluxes", "fluxes_get"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))
    assert callable(dynamics.flux_default_config) and callable(dynamics.flux_config_check)


def test_layouts_match_the_header(tmp_path):
    types = {"nxs_dyn_flux_config": _abi.FluxConfig, "nxs_dyn_flux_atmosphere": _abi.FluxAtmosphere, "nxs_dyn_flux_state": _abi.FluxState, "nxs_dyn_flux_rows": _abi.FluxRows}
    members = {s: [k for k, _ in T._fields_] for s, T in types.items()}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms) + 'printf("\\n");' for s, ms in members.items())
    enums = ("NXS_FLUX_ROWS", "NXS_FLUX_CONST_COUNT", "NXS_FLUX_HUM_DEWPOINT", "NXS_FLUX_HUM_SPHUMA", "NXS_FLUX_HUM_MIXRAT", "NXS_FLUX_LW_QLW_IN", "NXS_FLUX_LW_TCC",
             "NXS_FLUX_QOW", "NXS_FLUX_TAU_OW", "NXS_FLUX_QIA", "NXS_FLUX_ALBEDO", "NXS_FLUX_QIA_YOUNG", "NXS_FLUX_ALBEDO_YOUNG")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){' + body + "".join(f'printf("%d ", {e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    for row, (s, ms) in zip(rows, members.items()):
        assert [int(v) for v in row.split()] == [C.sizeof(types[s])] + [getattr(types[s], m).offset for m in ms], s
    rows_of = _abi.FLUX_ROWS.index
    assert [int(v) for v in rows[4].split()] == [_abi.NXS_FLUX_ROWS, len(_abi.FLUX_CONSTANTS), _abi.NXS_FLUX_HUM_DEWPOINT, _abi.NXS_FLUX_HUM_SPHUMA, _abi.NXS_FLUX_HUM_MIXRAT,
                                                 _abi.NXS_FLUX_LW_QLW_IN, _abi.NXS_FLUX_LW_TCC, rows_of("Qow"), rows_of("tau_ow"), rows_of("Qia"), rows_of("albedo"),
                                                 rows_of("Qia_young"), rows_of("albedo_young")]
    assert _abi.FLUX_ROWS == R.ROWS and _abi.FLUX_HUMIDITY == R.HUM and _abi.FLUX_LONGWAVE == R.LW


def test_the_defaults_are_the_fixtures():
    """model/options.cpp:388-438 as tests/golden/thermo_flux_options.json holds it, copied by hand with the line of each option"""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "thermo_flux_options.json")))["options"]
    got = dynamics.flux_default_config()
    names = {"ocean_albedo": "thermo.albedoW"}
    for k in _abi.FLUX_CONFIG_REALS + ("alb_scheme", "force_neutral_atmosphere"):
        o = fx[names.get(k, "thermo." + k)]
        assert 388 <= o["line"] <= 438
        assert got[k] == o["value"], k
        if o["type"] == "double":
            assert got[k] == float.fromhex(o["hex"]), k
    assert got["longwave_source"] == (_abi.NXS_FLUX_LW_TCC if fx["thermo.use_parameterised_long_wave_radiation"]["value"] else _abi.NXS_FLUX_LW_QLW_IN)
    assert got["humidity_source"] == _abi.NXS_FLUX_HUM_DEWPOINT
    ref = R.default_config()
    assert {k: got[k] for k in _abi.FLUX_CONFIG_REALS} == {k: ref[k] for k in _abi.FLUX_CONFIG_REALS} and got["alb_scheme"] == ref["alb_scheme"]


def test_the_constants_are_the_references():
    phys = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_constants.json")))["physical"]
    got = dynamics.flux_constants()
    assert tuple(got) == R.CONSTANTS == _abi.FLUX_CONSTANTS
    for k, v in got.items():
        assert v == float.fromhex(phys[k]["hex"]) == getattr(R, k), k


def test_what_configure_refuses():
    chk = dynamics.flux_config_check
    assert chk() == 0
    for scheme in (1, 2, 3, 4):
        assert chk(alb_scheme=scheme) == 0
    for bad in (dict(alb_scheme=0), dict(alb_scheme=5), dict(alb_scheme=-1), dict(zref_wind=0.), dict(zref_wind=-10.), dict(zref_temp=0.), dict(zref_temp=-2.),
                dict(zref_temp=float("nan")), dict(limiting_lengthscale=0.), dict(limiting_lengthscale=-1.), dict(humidity_source=3), dict(humidity_source=-1),
                dict(longwave_source=2), dict(longwave_source=-1)):
        assert chk(**bad) == -1, bad
        assert next(iter(bad)).encode() in dynamics.load_library().nxs_dyn_last_error(None), bad
    for ok in (dict(humidity_source="sphuma"), dict(humidity_source="mixrat"), dict(longwave_source="tcc"), dict(force_neutral_atmosphere=1), dict(zref_temp=10., zref_wind=2.)):
        assert chk(**ok) == 0, ok
    assert dynamics.load_library().nxs_flux_config_check(None) == -1


def test_the_python_mirror_refuses_an_unknown_option():
    with pytest.raises(KeyError):
        dynamics.flux_config_check(alb_snow=0.8)


def _llvm_tool(name):
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for sub in ("llvm/bin", "lib/llvm/bin"):
        if os.path.exists(os.path.join(root, sub, name)):
            return os.path.join(root, sub, name)
    raise AssertionError(f"{name} not found beside hipcc ({root})")


def test_the_flux_kernel_uses_no_scratch_memory_and_no_lds(tmp_path):
    """a streaming fp64 kernel: everything of an element in registers; read from the gfx950 code object inside the built library"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    found = []
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\S+)$", block, flags=re.M))
        if "k_fluxes" in f.get("name", ""):
            found.append(f)
    assert len(found) == 1, found
    f = found[0]
    print(f)
    assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["group_segment_fixed_size"]) == 0, f
    assert int(f["vgpr_count"]) <= 128, f                 # (four waves per SIMD at least)
