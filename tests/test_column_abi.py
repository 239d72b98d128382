"""thermo()'s ice columns at the C ABI (include/nxs_dyn.h: nxs_col_*, nxs_dyn_column_*, nxs_dyn_column): exported and declared, the ctypes mirrors match the
header, the defaults, the enum values and the constants are the reference's (tests/golden/reference_constants.json), what nxs_dyn_column_configure refuses --
through nxs_col_config_check, the same check without a handle, so without a device -- and the resources of k_column read from the built library."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import column_ref as R
from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
FIX = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_constants.json")))
NEW = ("nxs_col_default_config", "nxs_col_config_check", "nxs_col_constants", "nxs_dyn_column_configure", "nxs_dyn_column_set_forcing", "nxs_dyn_column_put",
       "nxs_dyn_column_get_state", "nxs_dyn_column", "nxs_dyn_column_get")


def test_the_entry_points_are_exported_and_declared():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NEW:
        assert name in dynamics.EXPORTS and hasattr(L, name) and f" T {name}\n" in out, name
        assert re.search(r"NXS_API int " + name + r"\(", HEADER), name
    assert L.nxs_dyn_abi_version() == 2 and re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)      # additive: the version stays
    for name in ("column_configure", "column_set_forcing", "column_put", "column_get", "column", "column_rows"):
        assert callable(getattr(dynamics.FiniteElementDynamics, name))
    assert callable(dynamics.column_default_config) and callable(dynamics.column_config_check) and callable(dynamics.column_constants)


def test_layouts_match_the_header(tmp_path):
    types = {"nxs_dyn_column_config": _abi.ColumnConfig, "nxs_dyn_column_forcing": _abi.ColumnForcing, "nxs_dyn_column_state": _abi.ColumnState,
             "nxs_dyn_column_rows": _abi.ColumnRows}
    members = {s: [k for k, _ in T._fields_] for s, T in types.items()}
    body = "".join(f'printf("%zu", sizeof({s}));' + "".join(f'printf(" %zu", offsetof({s}, {m}));' for m in ms) + 'printf("\\n");' for s, ms in members.items())
    enums = ("NXS_COL_ROWS", "NXS_COL_CONST_COUNT", "NXS_COL_THERMO_ZERO_LAYER", "NXS_COL_THERMO_WINTON", "NXS_COL_QIO_BASIC", "NXS_COL_QIO_EXCHANGE",
             "NXS_COL_FREEZINGPOINT_LINEAR", "NXS_COL_FREEZINGPOINT_UNESCO", "NXS_COL_OCEAN_CONSTANT", "NXS_COL_OCEAN_NUDGED", "NXS_COL_OCEAN_COUPLED",
             "NXS_COL_SNOWFALL_PRECIP_SNOWFR", "NXS_COL_SNOWFALL_SNOWFALL", "NXS_COL_SNOWFALL_PRECIP_TAIR", "NXS_COL_MLD_CONSTANT", "NXS_COL_MLD_ROW",
             "NXS_COL_SNOWFALL", "NXS_COL_TFRW", "NXS_COL_QIO", "NXS_COL_DEL_HI_S2I", "NXS_COL_QIO_YOUNG", "NXS_COL_DEL_HI_S2I_YOUNG")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){' + body + "".join(f'printf("%d ", {e});' for e in enums) + 'return 0;}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    rows = subprocess.check_output([str(tmp_path / "sz")], text=True).split("\n")
    for row, (s, ms) in zip(rows, members.items()):
        assert [int(v) for v in row.split()] == [C.sizeof(types[s])] + [getattr(types[s], m).offset for m in ms], s
    E, rows_of = _abi.COL_ENUMS, _abi.COL_ROWS.index
    assert [int(v) for v in rows[4].split()] == [
        _abi.NXS_COL_ROWS, len(_abi.COL_CONSTANTS), E["thermo_type"]["zero_layer"], E["thermo_type"]["winton"], E["qio_type"]["basic"], E["qio_type"]["exchange"],
        E["freezingpoint_type"]["linear"], E["freezingpoint_type"]["unesco"], E["ocean_type"]["constant"], E["ocean_type"]["nudged"], E["ocean_type"]["coupled"],
        E["snowfall_source"]["precip_snowfr"], E["snowfall_source"]["snowfall"], E["snowfall_source"]["precip_tair"], E["mld_source"]["constant"], E["mld_source"]["row"],
        rows_of("snowfall"), rows_of("tfrw"), rows_of("Qio"), rows_of("del_hi_s2i"), rows_of("Qio_young"), rows_of("del_hi_s2i_young")]
    assert _abi.COL_ROWS == R.ROWS and _abi.COL_CONSTANTS == R.CONSTANTS


def test_the_enum_values_are_the_references():
    """setup:: of model/enums.hpp as tests/golden/reference_constants.json holds it"""
    ref, E = FIX["enums"], _abi.COL_ENUMS
    assert E["thermo_type"] == {"zero_layer": ref["ThermoType"]["ZERO_LAYER"], "winton": ref["ThermoType"]["WINTON"]}
    assert E["qio_type"] == {"basic": ref["OceanHeatfluxScheme"]["BASIC"], "exchange": ref["OceanHeatfluxScheme"]["EXCHANGE"]}
    assert E["freezingpoint_type"] == {"linear": ref["FreezingPointType"]["LINEAR"], "unesco": ref["FreezingPointType"]["UNESCO"]}
    assert E["ocean_type"]["constant"] == ref["OceanType"]["CONSTANT"] and E["ocean_type"]["coupled"] == ref["OceanType"]["COUPLED"]
    assert E["ocean_type"]["nudged"] == ref["OceanType"]["TOPAZ4R"]               # (every dataset ocean is nudged alike: FE.cpp:5359-5366)


def test_the_defaults_are_the_fixtures():
    """model/options.cpp:112, 291-293, 383-420 as tests/golden/reference_constants.json holds it"""
    opt, sopt, E = FIX["options"], FIX["string_options"], _abi.COL_ENUMS
    got = dynamics.column_default_config()
    for member, option in (("freezingpoint_mu", "thermo.freezingpoint_mu"), ("snow_cond", "thermo.snow_cond"), ("Csens_io", "thermo.Csens_io"),
                           ("constant_mld", "ideal_simul.constant_mld"), ("Qdw_const", "ideal_simul.constant_Qdw"), ("Fdw_const", "ideal_simul.constant_Fdw")):
        assert got[member] == float.fromhex(opt[option]["hex"]) == opt[option]["value"], member
    days = float.fromhex(FIX["members"]["days_in_sec"]["hex"])
    assert got["nudge_timeT"] == days * opt["thermo.ocean_nudge_timeT_days"]["value"] and got["nudge_timeS"] == days * opt["thermo.ocean_nudge_timeS_days"]["value"]
    assert got["flooding"] == int(opt["thermo.flooding"]["value"])
    assert got["thermo_type"] == E["thermo_type"][sopt["setup.thermo-type"]] and got["qio_type"] == E["qio_type"][sopt["thermo.Qio-type"]]
    assert got["freezingpoint_type"] == E["freezingpoint_type"][sopt["thermo.freezingpoint-type"]] and got["ocean_type"] == E["ocean_type"][sopt["setup.ocean-type"]]
    assert got["snowfall_source"] == E["snowfall_source"]["precip_snowfr"] and got["mld_source"] == E["mld_source"]["constant"]
    ref = R.default_config()
    assert {k: got[k] for k in _abi.COL_CONFIG_REALS} == {k: ref[k] for k in _abi.COL_CONFIG_REALS}
    assert all(got[k] == E[k][ref[k]] for k in E) and got["flooding"] == ref["flooding"]


def test_the_constants_are_the_references():
    phys = FIX["physical"]
    got = dynamics.column_constants()
    assert tuple(got) == R.CONSTANTS == _abi.COL_CONSTANTS
    for k, v in got.items():
        assert v == float.fromhex(phys[k]["hex"]) == float(getattr(R, k)), k


def test_what_configure_refuses():
    chk = dynamics.column_config_check
    assert chk() == 0
    bad = [dict(thermo_type=2), dict(thermo_type=-1), dict(qio_type=2), dict(qio_type=-1), dict(freezingpoint_type=2), dict(freezingpoint_type=-1),
           dict(ocean_type=2), dict(ocean_type=-1), dict(ocean_type="coupled"), dict(snowfall_source=3), dict(snowfall_source=-1), dict(mld_source=2), dict(mld_source=-1)]
    for k in ("snow_cond", "constant_mld", "nudge_timeT", "nudge_timeS"):
        bad += [{k: 0.}, {k: -1.}, {k: float("nan")}]
    for b in bad:
        assert chk(**b) == -1, b
        assert next(iter(b)).encode() in dynamics.load_library().nxs_dyn_last_error(None), b
    assert b"OASIS" in (chk(ocean_type="coupled"), dynamics.load_library().nxs_dyn_last_error(None))[1]
    for ok in (dict(thermo_type="zero_layer"), dict(qio_type="exchange"), dict(freezingpoint_type="unesco"), dict(ocean_type="nudged"), dict(snowfall_source="snowfall"),
               dict(snowfall_source="precip_tair"), dict(mld_source="row"), dict(flooding=0), dict(Qdw_const=-3., Fdw_const=1e-6), dict(freezingpoint_mu=0.06)):
        assert chk(**ok) == 0, ok
    assert dynamics.load_library().nxs_col_config_check(None) == -1


def test_the_python_mirror_refuses_an_unknown_option():
    with pytest.raises(KeyError):
        dynamics.column_config_check(snow_conductivity=0.3)
    with pytest.raises(KeyError):
        dynamics.column_config_check(reserved=1)


def _llvm_tool(name):
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc"))))
    for sub in ("llvm/bin", "lib/llvm/bin"):
        if os.path.exists(os.path.join(root, sub, name)):
            return os.path.join(root, sub, name)
    raise AssertionError(f"{name} not found beside hipcc ({root})")


def test_the_column_kernel_uses_no_scratch_memory_and_no_lds(tmp_path):
    """long divergent fp64 bodies, everything of an element in registers: read from the gfx950 code object inside the built library (the VGPR count is in
    DESIGN.md 6f and is not bounded here)"""
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "dev.co")
    subprocess.check_call([_llvm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", dynamics._LIB_PATH, fat])
    subprocess.check_call([_llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.check_output([_llvm_tool("llvm-readelf"), "--notes", co], text=True)
    found = []
    for block in notes.split("- .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(name|private_segment_fixed_size|group_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\S+)$", block, flags=re.M))
        if "k_column" in f.get("name", ""):
            found.append(f)
    assert len(found) == 1, found
    f = found[0]
    print(f)
    assert int(f["private_segment_fixed_size"]) == 0 and int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0 and int(f["group_segment_fixed_size"]) == 0, f
