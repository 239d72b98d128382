"""What tests/test_thermo_forcing_host_kernel.py and tests/test_gpu_thermo_forcing.py share: ExternalData::get (model/externaldata.cpp:401-403, 434, 438) as a numpy
expression, per-row tables of modes and coefficients that cover the end points, the first step of a spin-up (factor 0) and a bias, and snapshot rows with the
special values in them.  numpy rounds every product and sum on its own (no contraction), like the library's build."""
import numpy as np

from nextsim_amd import _abi

OFF, LINEAR, STEP = _abi.NXS_TF_OFF, _abi.NXS_TF_LINEAR, _abi.NXS_TF_STEP
# (mode, fcoeff0, fcoeff1, factor, bias) per row: every row its own dataset
TABLE = ((LINEAR, 0.25, 0.75, 1., 0.),              # inside the interval
         (LINEAR, 1., 0., 1., -0.),                 # the two end points (bias -0.0: the only bias that lets a zero keep its sign, so STEP and LINEAR (1, 0) differ there)
         (LINEAR, 0., 1., 1., 0.),
         (STEP, 0., 0., 1., -0.),                   # nearest_daily / constant: snapshot 1 is never read
         (OFF, 0.5, 0.5, 1., 0.),
         (LINEAR, 0.6, 0.4, 0., 0.),                # factor 0: the first step of a spin-up
         (LINEAR, 1. / 3., 2. / 3., 0.37, -1.5),
         (STEP, 0., 0., 2.5, 273.15),
         (STEP, 0., 0., 0., 0.),
         (OFF, 1., 0., 1., 0.))


def table(shift=0):
    """TABLE rotated by `shift` rows: another mode on every row"""
    return tuple(TABLE[(k + shift) % len(TABLE)] for k in range(len(TABLE)))


def snapshots(Ne, seed=3):
    """d0, d1 [10, Ne]: ordinary values, -0.0 and +0.0 in both, and in d1 NaN and +-Inf (a STEP row must not see them; a LINEAR row carries them as numpy does)"""
    rng = np.random.default_rng(seed + Ne)
    d0 = rng.normal(size=(10, Ne)) * 10. ** rng.integers(-3, 6, size=(10, 1))
    d1 = rng.normal(size=(10, Ne)) * 10. ** rng.integers(-3, 6, size=(10, 1))
    special0 = (-0., 0., -0., 1e-310, -1e300)
    special1 = (-0., -0., 0., np.nan, np.inf, -np.inf, 1e300)
    for k in range(10):
        for j, v in enumerate(special0):
            d0[k, (3 * k + 7 * j) % Ne] = v
        for j, v in enumerate(special1):
            d1[k, (5 * k + 11 * j + 1) % Ne] = v
    d0[:, Ne - 1] = -0.                                  # the scalar tail of an odd Ne sees a signed zero too
    return np.ascontiguousarray(d0), np.ascontiguousarray(d1)


def blend(row, d0, d1):
    """ExternalData::get for one row: factor*(fcoeff0*d0 + fcoeff1*d1) + bias, or factor*d0 + bias; None for an OFF row"""
    mode, c0, c1, factor, bias = row
    f64 = np.float64
    with np.errstate(all="ignore"):
        if mode == LINEAR:
            return f64(factor) * (f64(c0) * d0 + f64(c1) * d1) + f64(bias)
        if mode == STEP:
            return f64(factor) * d0 + f64(bias)
    return None


def time_rows(tab):
    """the argument of FiniteElementDynamics.thermo_forcing_time for a table"""
    return {name: dict(mode=m, fcoeff0=c0, fcoeff1=c1, factor=f, bias=b) for name, (m, c0, c1, f, b) in zip(_abi.TF_ROWS, tab)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
