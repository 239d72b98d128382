"""nxs_dyn_regrid_carry_thermo at the C ABI, the part that needs no GPU: the ctypes mirrors have the C structs' sizes and member offsets, the library exports the
two entry points and refuses a call without a handle, and dynamics.py names the carried columns with the kinds and bounds of model/model_variable.cpp."""
import ctypes as C
import os
import re
import subprocess

from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()


def test_ctypes_layouts_match_the_header(tmp_path):
    structs = {"nxs_dyn_regrid_thermo": _abi.RegridThermo, "nxs_dyn_regrid_thermo_info": _abi.RegridThermoInfo,
               "nxs_dyn_regrid_args": _abi.RegridArgs, "nxs_dyn_regrid_info": _abi.RegridInfo}        # (the last two: their layout has not moved)
    probes = [("nxs_dyn_regrid_thermo", "carry"), ("nxs_dyn_regrid_thermo", "drag_ice_t"), ("nxs_dyn_regrid_thermo_info", "flux_carried"),
              ("nxs_dyn_regrid_thermo_info", "col_carried"), ("nxs_dyn_regrid_thermo_info", "slab_carried"), ("nxs_dyn_regrid_thermo_info", "flux_remade"),
              ("nxs_dyn_regrid_thermo_info", "nb_var_element"), ("nxs_dyn_regrid_thermo_info", "tiled")]
    body = "".join(f'printf("%zu\\n", sizeof({s}));' for s in structs) + "".join(f'printf("%zu\\n", offsetof({s}, {f}));' for s, f in probes)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert vals == [C.sizeof(t) for t in structs.values()] + [getattr(structs[s], f).offset for s, f in probes]
    assert vals[:4] == [16, 24, 96, 64]
    L = dynamics.load_library()
    assert {"nxs_dyn_regrid_carry_thermo", "nxs_dyn_regrid_thermo_info_get"} <= set(dynamics.EXPORTS) and L.nxs_dyn_abi_version() == 2
    assert L.nxs_dyn_regrid_carry_thermo(None, None) == -1 and L.nxs_dyn_regrid_thermo_info_get(None, None) == -1     # no handle: refused before any device call
    assert re.search(r"NXS_API\s+int\s+nxs_dyn_regrid_carry_thermo\s*\(\s*nxs_dyn_handle\s*\*h,\s*const\s+nxs_dyn_regrid_thermo\s*\*o\)", HEADER)
    assert re.search(r"NXS_API\s+int\s+nxs_dyn_regrid_thermo_info_get\s*\(\s*nxs_dyn_handle\s*\*h,\s*nxs_dyn_regrid_thermo_info\s*\*out\)", HEADER)


def test_the_column_table_is_model_variable_cpps():
    none = lambda lo=None, hi=None: ("none", lo, hi)   # noqa: E731
    want = {"tice0": none(), "tice1": ("enthalpy", None, None), "tice2": ("thick", None, None),
            "tsurf_young": none(), "sst": none(), "sss": none(), "lid_volume": none(), "pond_volume": none(), "del_vi_tend": none(),
            "conc_upd": none(-1., 1.),
            "freeze_onset": none(0., 1.), "conc_summer": none(0., 1.), "fyi_fraction": none(0., 1.),
            "freeze_days": none(0.), "thick_summer": none(0.), "age_det": none(0.), "age": none(0.)}
    table = dynamics.REGRID_THERMO_COLUMNS
    assert {c[0]: tuple(c[1:4]) for c in table} == want and len(table) == len(want) == 17
    assert {c[0] for c in table if c[4]} == {"tice0", "tice1", "tice2"}                                  # the M_tice no-ice rule
    assert all(c[1] in _abi.TRANSFORMATIONS for c in table)
    # sortPrognosticVars: kind by kind, so that the carried columns stand in front of the caller's extras of the same kind
    kinds = [_abi.TRANSFORMATIONS[c[1]] for c in table]
    assert kinds == sorted(kinds)
    # every row of the three state structs is either carried or re-made, none twice
    rows = _abi.FLUX_STATE + _abi.COL_STATE + _abi.SLAB_STATE
    assert sorted([c[0] for c in table] + list(dynamics.REGRID_THERMO_REMADE)) == sorted(rows) and len(set(rows)) == 20
    assert dynamics.REGRID_THERMO_REMADE == ("drag_ti", "drag_ti_young", "pond_fraction")
    assert callable(dynamics.FiniteElementDynamics.regrid_carry_thermo) and callable(dynamics.FiniteElementDynamics.regrid_thermo_info)
