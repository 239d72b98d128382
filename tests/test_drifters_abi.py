"""The drifter entry points of the C ABI (include/nxs_dyn.h, nxs_dyn_drifters_*): exported, declared to ctypes as the header declares them."""
import ctypes as C
import os
import re
import subprocess

from nextsim_amd import _abi, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nxs_dyn_drifters_set", "nxs_dyn_drifters_clear", "nxs_dyn_drifters_mesh_bbox", "nxs_dyn_drifters_move", "nxs_dyn_drifters_conc",
         "nxs_dyn_drifters_mask", "nxs_dyn_drifters_get")
CTYPE = {"h": C.c_void_p, "i32": C.c_int32, "f64": C.c_double, "pf64": _abi.c_double_p, "pi32": _abi.c_int32_p}


def test_the_seven_symbols_are_exported():
    L = dynamics.load_library()
    out = subprocess.check_output(["nm", "-D", "--defined-only", dynamics._LIB_PATH], text=True)
    for name in NAMES:
        assert name in dynamics.EXPORTS and hasattr(L, name), name
        assert re.search(r"\bT %s$" % name, out, re.M), name
    assert not re.search(r"nxs_drifters", out)      # the interface between the two translation units is not part of the ABI


def test_ctypes_signatures_agree_with_the_header(tmp_path):
    """A C++ probe compiled against the header prints every parameter type of the seven declarations; ctypes must have declared the same."""
    probe = r'''
#include <cstdio>
#include <cstdint>
#include "nxs_dyn.h"
template <typename T> struct N;
template <> struct N<nxs_dyn_handle *> { static const char *s() { return "h"; } };
template <> struct N<int32_t> { static const char *s() { return "i32"; } };
template <> struct N<double> { static const char *s() { return "f64"; } };
template <> struct N<double *> { static const char *s() { return "pf64"; } };
template <> struct N<const double *> { static const char *s() { return "pf64"; } };
template <> struct N<int32_t *> { static const char *s() { return "pi32"; } };
template <> struct N<const int32_t *> { static const char *s() { return "pi32"; } };
template <typename... A> void show(const char *name, int (*)(A...)) {
    std::printf("%s", name);
    const char *t[] = {N<A>::s()...};
    for (const char *q : t) std::printf(" %s", q);
    std::printf("\n");
}
int main() {
''' + "".join(f'    show("{n}", &{n});\n' for n in NAMES) + '    std::printf("sets %d\\n", NXS_DRIFTER_SETS);\n    return 0;\n}\n'
    src = tmp_path / "probe.cpp"
    src.write_text(probe)
    exe = tmp_path / "probe"
    # (only addresses are taken: the library is linked so that they resolve)
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), dynamics._LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(dynamics._LIB_PATH), "-Wl,--unresolved-symbols=ignore-in-shared-libs"])
    lines = subprocess.check_output([str(exe)], text=True).strip().split("\n")
    L = dynamics.load_library()
    seen = {}
    for line in lines:
        name, *types = line.split()
        seen[name] = types
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [CTYPE[t] for t in seen[name]], (name, seen[name], fn.argtypes)
    assert seen["sets"] == [str(_abi.NXS_DRIFTER_SETS)] == ["8"]


def test_drifter_sets_constant_has_the_headers_value():
    text = open(os.path.join(ROOT, "include", "nxs_dyn.h")).read()
    m = re.search(r"#define\s+NXS_DRIFTER_SETS\s+(\d+)", text)
    assert m and int(m.group(1)) == _abi.NXS_DRIFTER_SETS == 8
    assert re.search(r"#define\s+NXS_DYN_ABI_VERSION\s+2\b", text)      # additive: the ABI version stays


def test_wrapper_methods_exist():
    for m in ("drifters_set", "drifters_clear", "drifters_mesh_bbox", "drifters_move", "drifters_conc", "drifters_mask", "drifters_get", "drifters_update"):
        assert callable(getattr(dynamics.FiniteElementDynamics, m)), m
