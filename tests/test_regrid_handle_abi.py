"""nxs_dyn_regrid (interpFields + assignVariables on the live handle), the part that needs no GPU: the header declares it, the library exports it, the ABI
version is unchanged, the ctypes mirrors match the C structs, and bad arguments are refused on the host -- by the Python wrapper before any library call, and
by the library before it touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cases
from nextsim_amd import _abi, dynamics, mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()


def test_header_declares_the_entry_and_the_enum():
    assert re.search(r"NXS_API\s+int\s+nxs_dyn_regrid\s*\(\s*nxs_dyn_handle\s*\*h,\s*const\s+nxs_dyn_regrid_args\s*\*a,\s*nxs_dyn_regrid_info\s*\*info", HEADER)
    for name, val in (("NXS_TRANSFORM_NONE", 0), ("NXS_TRANSFORM_CONC", 1), ("NXS_TRANSFORM_THICK", 2), ("NXS_TRANSFORM_ENTHALPY", 3)):
        assert re.search(rf"\b{name}\s*=\s*{val}\b", HEADER), name
        assert getattr(_abi, name) == val
    assert re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", HEADER)
    for name in ("HAS_MIN", "HAS_MAX", "IS_TICE", "OLD_ON_DEVICE", "NEW_ON_DEVICE"):
        m = re.search(rf"NXS_REGRID_VAR_{name}\s*=\s*(\d+)", HEADER)
        assert m and int(m.group(1)) == getattr(_abi, "NXS_REGRID_VAR_" + name)


def test_library_exports_the_symbol_and_the_version_is_still_2():
    assert "nxs_dyn_regrid" in dynamics.EXPORTS
    L = dynamics.load_library()
    assert hasattr(L, "nxs_dyn_regrid") and L.nxs_dyn_abi_version() == 2
    # no handle: refused before any device call (this box may have no GPU at all)
    assert L.nxs_dyn_regrid(None, None, None) == -1
    # the constants of the enthalpy transformation are the reference's (model/constants.hpp:68, 44, 17)
    out = (C.c_double * 11)()
    assert L.nxs_dyn_physical_constants(out, 11) == 0
    assert list(out)[8:] == [5., 333.55e3, 2100.]


def test_ctypes_layouts_match_the_header(tmp_path):
    structs = {"nxs_dyn_regrid_var": _abi.RegridVar, "nxs_dyn_regrid_args": _abi.RegridArgs, "nxs_dyn_regrid_info": _abi.RegridInfo}
    probes = [("nxs_dyn_regrid_var", "max_val"), ("nxs_dyn_regrid_var", "flags"), ("nxs_dyn_regrid_args", "extra"), ("nxs_dyn_regrid_args", "freezingpoint_mu"),
              ("nxs_dyn_regrid_args", "drag_ui_young"), ("nxs_dyn_regrid_args", "num_extra"), ("nxs_dyn_regrid_info", "nb_var_element"), ("nxs_dyn_regrid_info", "total_ms")]
    body = "".join(f'printf("%zu\\n", sizeof({s}));' for s in structs) + "".join(f'printf("%zu\\n", offsetof({s}, {f}));' for s, f in probes)
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "nxs_dyn.h"\nint main(void){{{body}return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert vals == [C.sizeof(t) for t in structs.values()] + [getattr(structs[s], f).offset for s, f in probes]


def _new_mesh():
    x, y, tri, ng = cases.rect_mesh(6, 1)
    on_b = np.zeros(x.size, bool); on_b[:ng] = True
    gm = M.GlobalMesh(x=x, y=y, tri=tri, dirichlet=on_b, neumann=np.zeros(x.size, bool), lat=M.polar_stereographic_lat(x, y), name="regrid-abi")
    return M.localize(gm, 1)[0], ng


def test_python_wrapper_refuses_bad_arguments_without_a_device():
    """regrid_args is the host half of FiniteElementDynamics.regrid: no handle, no library call."""
    lm, ng = _new_mesh()
    Ne, Nn = lm.num_elements, lm.num_nodes
    inputs = {k: np.ones(Ne) for k in dynamics.REGRID_INPUTS}
    moved = (lm.coord_x.copy(), lm.coord_y.copy())
    ok = dict(old=np.zeros(Ne), transformation="thick")
    a, keep, res = dynamics.regrid_args(lm, None, ng, inputs, [ok], moved=moved, num_nodes_old=Nn, num_elements_old=Ne)
    assert a.num_extra == 1 and a.extra[0].transformation == _abi.NXS_TRANSFORM_THICK and res[0].shape == (Ne,) and a.new_mesh.contents.num_elements == Ne
    with pytest.raises(ValueError, match="unknown transformation"):
        dynamics.regrid_args(lm, None, ng, inputs, [dict(old=np.zeros(Ne), transformation=7)], moved=moved)
    with pytest.raises(ValueError, match="unknown transformation"):
        dynamics.regrid_args(lm, None, ng, inputs, [dict(old=np.zeros(Ne), transformation="salinity")], moved=moved)
    with pytest.raises(ValueError, match="num_extra"):
        dynamics.regrid_args(lm, None, ng, inputs, -1, moved=moved)
    with pytest.raises(ValueError, match="drag_ui_young"):
        dynamics.regrid_args(lm, None, ng, {k: v for k, v in inputs.items() if k != "drag_ui_young"}, moved=moved)
    with pytest.raises(ValueError, match="neither a context nor the moved coordinates"):
        dynamics.regrid_args(lm, None, ng, inputs)
    with pytest.raises(ValueError, match="no 'old' values"):
        dynamics.regrid_args(lm, None, ng, inputs, [dict(transformation="none")], moved=moved)
    with pytest.raises(ValueError, match="shape"):
        dynamics.regrid_args(lm, None, ng, {k: np.ones(Ne + 1) for k in dynamics.REGRID_INPUTS}, moved=moved)
    with pytest.raises(ValueError, match="previous_numbering"):
        dynamics.regrid_args(lm, np.zeros(Nn + 2), ng, inputs, moved=moved)
    # a device address is flagged, a host array is not
    a, keep, res = dynamics.regrid_args(lm, None, ng, inputs, [dict(old=0x1000, new=0x2000, min=0., max=None, is_tice=True)], moved=moved)
    assert a.extra[0].flags == (_abi.NXS_REGRID_VAR_OLD_ON_DEVICE | _abi.NXS_REGRID_VAR_NEW_ON_DEVICE | _abi.NXS_REGRID_VAR_HAS_MIN | _abi.NXS_REGRID_VAR_IS_TICE)


def test_cpp_wrapper_has_the_method():
    text = open(os.path.join(ROOT, "include", "nxs_dyn.hpp")).read()
    assert re.search(r"nxs_dyn_regrid_info\s+regrid\(const nxs_dyn_regrid_args &a\)", text)
    src = "#include \"nxs_dyn.hpp\"\nint main() { return sizeof(&nxs::FiniteElementDynamics::regrid) ? 0 : 1; }\n"
    subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"], input=src, text=True, check=True)
