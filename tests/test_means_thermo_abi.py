"""The thermodynamic range of enum nxs_means_var at the C ABI: every NXS_MEANS_* value of the range as a C compiler reads the header equals _abi's, the range
overlaps neither the elemental ids 0..19 nor the nodal ids 64..74, the cap per list and the ABI version are what they were, and the restatement names the same
variables in the same order."""
import os
import subprocess

from nextsim_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_values(tmp_path, exprs):
    src = tmp_path / "ids.c"
    src.write_text('#include <stdio.h>\n#include "nxs_dyn.h"\nint main(void){' + "".join(f'printf("%d\\n", (int)({e}));' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "ids"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]


def test_the_header_values_are_abis(tmp_path):
    names = [f"NXS_MEANS_{k.upper()}" for k in _abi.MEANS_THERMO]
    vals = _header_values(tmp_path, names + ["NXS_MEANS_THERMO_BEGIN", "NXS_MEANS_THERMO_END"])
    assert vals[:-2] == [_abi.MEANS_ID[k] for k in _abi.MEANS_THERMO]
    assert vals[:-2] == list(range(_abi.NXS_MEANS_THERMO_BEGIN, _abi.NXS_MEANS_THERMO_BEGIN + len(_abi.MEANS_THERMO)))
    assert vals[-2] == _abi.NXS_MEANS_THERMO_BEGIN == 128
    assert vals[-1] == _abi.NXS_MEANS_THERMO_BEGIN + len(_abi.MEANS_THERMO) <= 256        # the kernel's id table entry is an unsigned char
    assert len(set(k.upper() for k in _abi.MEANS_THERMO)) == len(_abi.MEANS_THERMO)         # no two names fall on one C identifier


def test_the_range_overlaps_no_other(tmp_path):
    el_end, nod_begin, nod_end, begin, end = _header_values(tmp_path, ["NXS_MEANS_ELEMENTAL_END", "NXS_MEANS_NODAL_BEGIN", "NXS_MEANS_NODAL_END", "NXS_MEANS_THERMO_BEGIN",
                                                                        "NXS_MEANS_THERMO_END"])
    assert (el_end, nod_begin, nod_end) == (20, 64, 75)
    thermo = set(range(begin, end))
    assert not thermo & set(range(0, el_end)) and not thermo & set(range(nod_begin, nod_end))
    ids = [_abi.MEANS_ID[k] for k in _abi.MEANS_ELEMENTAL + _abi.MEANS_NODAL + _abi.MEANS_THERMO]
    assert len(set(ids)) == len(ids) == len(_abi.MEANS_ID)
    assert not set(_abi.MEANS_THERMO) & set(_abi.MEANS_ELEMENTAL + _abi.MEANS_NODAL)


def test_the_cap_and_the_abi_version_are_unchanged(tmp_path):
    assert _header_values(tmp_path, ["NXS_MEANS_MAX_VARS", "NXS_DYN_ABI_VERSION"]) == [24, 2]
    assert _abi.NXS_MEANS_MAX_VARS == 24
    assert _abi.MEANS_ELEMENTAL[0] == "conc" and _abi.MEANS_ELEMENTAL[-1] == "ice_mask" and len(_abi.MEANS_ELEMENTAL) == 20


def test_the_restatement_names_the_same_variables():
    import means_thermo_ref as T
    assert T.THERMO == _abi.MEANS_THERMO
    assert set(T.NEGATED) | set(T.YEARS) | set(T.LIBM) <= set(T.THERMO)


def test_the_wrapper_takes_the_names():
    from nextsim_amd import dynamics
    ids, masks = dynamics.FiniteElementDynamics._means_list(["conc", ("sst", True), "QNoSw", 189], 0, 0)
    assert list(ids) == [0, 128, _abi.MEANS_ID["QNoSw"], 189] and list(masks) == [0, 1, 0, 0]
