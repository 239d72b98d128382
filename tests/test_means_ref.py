"""tests/means_ref.py (the numpy restatement of updateMeans the GPU tests compare the device with) against a hand-computed known answer: two triangles on
four nodes, the second triangle a ghost, every number below worked out by hand from FE.cpp:8518-9024."""
import numpy as np

import means_ref as R

NAN = float("nan")
# nodes 0..3; triangle 0 = (0, 1, 2) owned, triangle 1 = (1, 3, 2) ghost.  NodalElementConnectivity (1-based, width 3): NaN padding, and for node 2 a
# NEGATIVE entry between its two elements (FE.cpp:9008 "Skip negative elt_num": elt_num = entry - 1 < 0)
NEC = np.array([[1., NAN, NAN],
                [1., 2., NAN],
                [2., -3., 1.],
                [2., NAN, NAN]])
STATE = {"conc": np.array([0.5, 0.25]), "thick": np.array([2., 0.]), "conc_young": np.array([0.25, 0.5]), "h_young": np.array([0.5, 0.]),
         "VT": np.array([1., 2., 3., 4., -1., -2., -3., -4.])}
DIAG = {"surface": np.array([2., 6.]), "D_tau_w": np.array([0.5, 0.5, 3., 0.5, 0.25, 0.25, 4., 0.25])}
WIND = np.array([3., 3., 3., 0., 4., 4., 4., 5.])
TAU_OW = np.array([0.5, 0.25])
DRAG, DRAG_YOUNG = np.array([2., 2.]), np.array([4., 4.])


def _ref(young, elemental=(), nodal=(), local=1):
    return R.MeansRef(4, 2, local, young, elemental, nodal, NEC)


def test_stress_gather_with_a_negative_and_nan_entries():
    tau_a, conc = R.stress_gather(NEC, TAU_OW, DIAG["surface"], STATE["conc"])
    # node 0: element 0 only: (0.5*2)/2, (0.5*2)/2.  node 1: elements 0, 1: (0.5*2 + 0.25*6)/8 = 2.5/8, (0.5*2 + 0.25*6)/8
    # node 2: element 1, [skipped], element 0: (0.25*6 + 0.5*2)/8.  node 3: element 1 only: 0.25, 0.25
    assert tau_a.tolist() == [0.5, 0.3125, 0.3125, 0.25]
    assert conc.tolist() == [0.5, 0.3125, 0.3125, 0.25]


def test_taux_tauy_taumod_known_answer():
    m = _ref(True, nodal=("taux", "tauy", "taumod", "VT_y"))
    m.update(0.5, STATE, diag=DIAG, wind=WIND, tau_ow=TAU_OW)
    # node 0: |wind| = hypot(3, 4) = 5, conc = tau_a = 0.5
    #   taux   = (0.5*0.5 + 0.5*(5*3)*(1 - 0.5)) * 0.5 = (0.25 + 3.75) * 0.5 = 2
    #   tauy   = (0.25*0.5 + 0.5*(5*4)*0.5) * 0.5      = (0.125 + 5) * 0.5   = 2.5625
    #   taumod = (hypot(0.5, 0.25)*0.5 + 0.5*25*0.5) * 0.5
    assert m.nod[0, 0] == 2.0 and m.nod[0, 1] == 2.5625
    assert m.nod[0, 2] == (np.hypot(0.5, 0.25) * 0.5 + 0.5 * 25. * 0.5) * 0.5
    # node 2: D_tau_w = (3, 4) -> modulus 5; conc = tau_a = 0.3125: taumod = (5*0.3125 + 0.3125*25*0.6875) * 0.5
    assert m.nod[2, 2] == (5. * 0.3125 + 0.3125 * 25. * 0.6875) * 0.5
    # node 3 (a ghost node in a real partition: nodal rows are filled for ALL nodes): wind (0, 5): taux = (0.5*0.25 + 0.25*(5*0)*0.75)*0.5
    assert m.nod[3, 0] == 0.0625
    assert m.nod[:, 3].tolist() == [-0.5, -1., -1.5, -2.]
    m.update(0.5, STATE, diag=DIAG, wind=WIND, tau_ow=TAU_OW)      # the second half of the mean
    assert m.nod[0, 0] == 4.0 and m.nod[3, 0] == 0.125


def test_drag_ui_with_and_without_the_young_category():
    y = _ref(True, elemental=("drag_ui",), local=2)
    y.update(0.5, STATE, drag_ui=DRAG, drag_ui_young=DRAG_YOUNG)
    # element 0: (2*0.5 + 4*0.25) / 0.75 = 8/3; element 1: (2*0.25 + 4*0.5) / 0.75 = 10/3
    assert y.el[:, 0].tolist() == [(2. / 0.75) * 0.5, (2.5 / 0.75) * 0.5]
    c = _ref(False, elemental=("drag_ui",), local=2)
    c.update(0.5, STATE, drag_ui=DRAG, drag_ui_young=DRAG_YOUNG)
    assert c.el[:, 0].tolist() == [1., 1.]


def test_ice_mask_in_both_category_types_is_not_scaled_by_the_time_factor():
    st = dict(STATE, thick=np.array([0., 0.]), h_young=np.array([0.5, 0.]))
    y = _ref(True, elemental=("ice_mask",), local=2)
    y.update(0.25, st); y.update(0.25, st)
    assert y.el[:, 0].tolist() == [2., 0.]          # young ice counts: M_thick + M_h_young > 0; += 1 per call, whatever time_factor
    c = _ref(False, elemental=("ice_mask",), local=2)
    c.update(0.25, st)
    assert c.el[:, 0].tolist() == [0., 0.]          # classic: M_thick alone
    c.update(0.25, dict(st, thick=np.array([0., 1e-3])))
    assert c.el[:, 0].tolist() == [0., 1.]


def test_ghost_rows_stay_zero_and_reset_zeroes():
    m = _ref(True, elemental=("conc_cons", "ice_mask", "conc_young"), nodal=("VT_x",), local=1)
    m.update(0.5, STATE)
    assert m.el[0].tolist() == [0.25, 1., 0.125]
    assert m.el[1].tolist() == [0., 0., 0.]           # the ghost element
    assert m.nod[:, 0].tolist() == [0.5, 1., 1.5, 2.]
    m.reset()
    assert not m.el.any() and not m.nod.any()


def test_grid_mean_transposes_adds_and_masks():
    ncols, nrows = 3, 2
    # a fake sampler: value = 10 * i + j at "line" i (along x), column j (along y), times the first data value of the rows given
    def sample(rows):
        base = np.add.outer(10. * np.arange(ncols), np.arange(nrows))
        return base[..., None] * np.asarray(rows)[0][None, None, :]
    el_rows = np.array([[1., 0.]]); nod_rows = np.array([[2.]])
    ge, gn = R.grid_mean(sample, 2, 1, np.array([1.]), el_rows, nod_rows, ncols, nrows, -1e14, 1, [1, 0], [1])
    # grid_ind = i + ncols * j: row j = 0 holds i = 0, 1, 2 -> 0, 10, 20; row j = 1 -> 1, 11, 21; the ice mask column is 0 everywhere -> masked variables zeroed
    assert ge[1].tolist() == [0.] * 6 and ge[0].tolist() == [0.] * 6 and gn[0].tolist() == [0.] * 6
    ge, gn = R.grid_mean(sample, 2, 1, np.array([1.]), np.array([[1., 1.]]), nod_rows, ncols, nrows, -1e14, 1, [1, 0], [1])
    assert ge[0].tolist() == [0., 10., 20., 1., 11., 21.]            # (0 where the ice mask is 0: the first cell)
    assert gn[0].tolist() == [0., 200., 800., 2., 242., 882.]         # nodal value 2 * base, times the proc mask (= base)
    ge2, _ = R.grid_mean(sample, 2, 1, np.array([1.]), np.array([[1., 1.]]), nod_rows, ncols, nrows, -1e14, 1, [1, 0], [1], ge.copy(), gn.copy())
    assert ge2[0].tolist() == [0., 20., 40., 2., 22., 42.]            # += on a non-zero grid
