"""tests/means_thermo_ref.py on a hand-made five-element input whose answers are worked out here by hand: the sign of the five negated variables, the quotient
of the two ages, D_tsurf in both ice categories, drag_ti in both, the ghost row, and the plain case.  No device."""
import numpy as np
import pytest

import means_thermo_ref as T

NE, NEO = 5, 4                                   # four owned elements and one ghost


def _src():
    one = np.arange(1., 6.)                      # 1 .. 5
    src = {k: one * (3 + i) for i, k in enumerate(sorted({v for _, v in T.SOURCE if v}))}
    src.update(conc=np.array([0.5, 0.25, 0., 1., 0.5]), conc_young=np.array([0.25, 0.25, 0., 0., 0.5]),
               tice0=np.array([-8., -4., -2., -16., -1.]), tsurf_young=np.array([-2., -6., -1., -3., -1.]), sst=np.array([-1., 0.5, 2., -1.5, 1.]),
               drag_ti=np.array([1., 2., 3., 4., 5.]) * 1e-3, drag_ti_young=np.array([3., 2., 1., 8., 5.]) * 1e-3,
               wind=np.array([3., 0., -5., 8., 4., 0., 12., 6.]))                  # four nodes: |w| = 5, 0, 13, 10
    tri = np.array([[0, 1, 2], [1, 2, 3], [0, 2, 3], [3, 1, 0], [2, 1, 0]])
    return src, tri


def test_the_five_negated_variables_carry_the_reversed_sign():
    src, tri = _src()
    ref = T.ThermoMeansRef(NE, NEO, True, T.NEGATED + ("Qa",))
    ref.update(0.5, src); ref.update(0.25, src)
    for k, name in enumerate(T.NEGATED):
        row = src[dict(T.SOURCE)[name]]
        assert np.array_equal(ref.el[:NEO, k], -(row[:NEO] * 0.5) - row[:NEO] * 0.25) and (ref.el[:NEO, k] < 0).all(), name
    assert np.array_equal(ref.el[:NEO, -1], src["Qa"][:NEO] * 0.75) and (ref.el[:NEO, -1] > 0).all()
    assert not ref.el[NEO:].any()                                                  # the ghost row
    assert {dict(T.SOURCE)[n] for n in T.NEGATED} == {"fwflux_ice", "fwflux", "Qnosun", "Qsw_ocean", "brine"}


def test_the_ages_are_a_product_then_a_quotient():
    src, tri = _src()
    assert T.YEARS_IN_SEC == 365.25 * 86400. == 31557600.
    src["age"] = np.array([1., 2., 3., 4., 5.]) * T.YEARS_IN_SEC
    src["age_det"] = np.full(5, 0.1 * T.YEARS_IN_SEC)
    ref = T.ThermoMeansRef(NE, NEO, False, ("age", "age_det"))
    ref.update(0.5, src)
    assert np.array_equal(ref.el[:NEO, 0], [0.5, 1., 1.5, 2.])
    want = (0.1 * T.YEARS_IN_SEC) * 0.5 / T.YEARS_IN_SEC
    assert np.array_equal(ref.el[:NEO, 1], np.full(NEO, want))
    # the order matters at the last bit: for some x, (x * tf) / y is not x * (tf / y)
    x = np.linspace(1., 2., 1001) * 1e7
    assert np.any(x * (1. / 3.) / T.YEARS_IN_SEC != x * ((1. / 3.) / T.YEARS_IN_SEC))
    src["age"] = x[:5].copy()
    ref = T.ThermoMeansRef(NE, 5, False, ("age",))
    ref.update(1. / 3., src)
    assert np.array_equal(ref.el[:, 0], x[:5] * (1. / 3.) / T.YEARS_IN_SEC)


@pytest.mark.parametrize("young", [True, False])
def test_tsurf_and_drag_ti_in_both_categories(young):
    src, tri = _src()
    ref = T.ThermoMeansRef(NE, NEO, young, ("tsurf", "drag_ti"))
    ref.update(1.0, src)
    if young:   # conc*tice0 + conc_young*tsurf_young + (1 - conc - conc_young)*sst
        tsurf = [0.5 * -8. + 0.25 * -2. + 0.25 * -1., 0.25 * -4. + 0.25 * -6. + 0.5 * 0.5, 2., -16.]
        drag = [(1e-3 * 0.5 + 3e-3 * 0.25) / 0.75, (2e-3 * 0.25 + 2e-3 * 0.25) / 0.5, np.nan, (4e-3 * 1. + 8e-3 * 0.) / 1.]
    else:       # conc*tice0 + (1 - conc)*sst; the young rows are not read
        tsurf = [0.5 * -8. + 0.5 * -1., 0.25 * -4. + 0.75 * 0.5, 2., -16.]
        drag = [1e-3, 2e-3, 3e-3, 4e-3]
    assert np.array_equal(ref.el[:NEO, 0], tsurf)
    assert np.array_equal(ref.el[:NEO, 1], drag, equal_nan=True)
    assert np.isnan(ref.el[2, 1]) == young                                         # 0 / 0 on the ice-free element, as in the reference
    assert not ref.el[NEO:].any()


def test_wspeed_and_the_plain_case():
    src, tri = _src()
    ref = T.ThermoMeansRef(NE, NEO, True, ("wspeed", "sst", "t2", "snowfr", "snowfall", "d2m", "tcc"))
    ref.update(2.0, src, tri)
    assert np.array_equal(ref.el[:NEO, 0], np.array([(5. + 0. + 13.) / 3., (0. + 13. + 10.) / 3., (5. + 13. + 10.) / 3., (10. + 0. + 5.) / 3.]) * 2.)
    assert np.array_equal(ref.el[:NEO, 1], src["sst"][:NEO] * 2.) and np.array_equal(ref.el[:NEO, 2], src["tice2"][:NEO] * 2.)
    assert np.array_equal(ref.el[:, 3], ref.el[:, 4]) and np.array_equal(ref.el[:NEO, 5], src["humidity"][:NEO] * 2.)      # the aliases read one row
    assert np.array_equal(ref.el[:NEO, 6], src["longwave"][:NEO] * 2.)
    with pytest.raises(KeyError):
        T.ThermoMeansRef(NE, NEO, True, ("conc",))
