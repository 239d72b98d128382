"""numpy / plain-Python restatements for the nodal forcing tests (nxs_mapx_*, nxs_dyn_forcing_*; model/externaldata.cpp:944-1383, contrib/mapx):
  transform()    ExternalData::transformData for the east/north branch, the pole rows and the rotation, with the projection passed in (the fixture's maker passes the
                 REAL forward_mapx, the tests pass the library's host body); libm's cos, hypot and floor through ctypes, so the arithmetic beside the projection is the
                 reference's (CPython's own math.hypot is not glibc's)
  wrap()         interpolateDataset's cyclic copy (:1336-1383) and the appended centre
  blend()        ExternalData::get for one group (:401-403 + 438, :434 + 438)
  bound_*()      the ONE tolerance of the device's east/north transform against the host body

THE TOLERANCE (u = 2^-53; every figure below is a bound on the DIFFERENCE between the device's and the host's value, to first order).
The host and the device run the same source without contraction; +, -, *, / and sqrt are correctly rounded on both.  They differ only where sin, cos, pow and hypot
are called: the device's are taken to be within 2 ulp of the true value (OCML documents 1-2 ulp for these four), glibc's within 1 ulp, so two results
from the SAME argument differ by at most 3 ulp = tau = 6 u relative.  An operation that is correctly rounded on both sides and whose operands differ relatively by
eps gives results that differ by at most eps + 2 u (two independent roundings of u each).
 polar_stereographic.c:155-174 for one point, s = sin(phi):
   s                                   tau
   1.0 - s                             tau s/(1-s) + 2u          <- the cancellation near the pole
   1.0 + s                             tau + 2u
   (1-s)/(1+s)                         tau s/(1-s) + tau + 6u
   e s                                 tau + 2u;  1 +- e s: (tau + 2u) e/(1-e) + 2u = 2.71u with e = 0.0818;  their quotient: 2 * 2.71u + 2u = 7.43u
   pow(quotient, e)                    e * 7.43u + tau = 6.61u
   the product under the root          tau s/(1-s) + 20.61u;   t = sqrt(..): half of it + 2u = (tau/2) s/(1-s) + 12.3u
   rho = Rg*m1*t/t1                    + 4u  (Rg*m1 and t1 are the host's constants on both sides) = 3u s/(1-s) + 16.3u
   lam = (lon - lon0)*PI/180           the same bits on both sides
   x = rho sin(lam), y = -rho cos(lam) the RADIAL error of the point is rho (3u s/(1-s) + 16.3u); sin and cos add a vector of norm <= rho tau = 6u rho, the two products 2u rho
 mapx.c:1112-1113: a rotation (norm-preserving) of four products and two sums and the shift by (u0, v0): <= 9u rho in norm.
 So the position of ONE point differs by a vector of norm at most
   delta = u rho (C1 + C2/(1 - sin(phi))),   C1 = 34 (16.3 + 6 + 2 + 9, rounded up),  C2 = 3 (s <= 1),
 and each component of nxs_mapx_forward alone by at most that: |got - want| <= u hypot(x, y) (C1 + C2/(1 - sin(phi))), hypot(x, y) = rho because (u0, v0) = 0 for a
 map centred on the pole.  At the pole itself t = sqrt(0 * pow) = 0 on both sides: bit for bit.
 externaldata.cpp:1165-1199: the two projected points p, p' of one grid point differ from the host's by delta each, delta taken with the larger rho and the larger
 latitude of the two (rho_max, phi).  cos(lat*PI/180) differs by tau, so the displaced longitude moves p' along d = p' - p by at most (tau + 6u)|d|; the subtraction
 adds 2u|d| per component.  Hence |Delta d| <= 2 delta + 17u |d|.  The result is n = d/|d| * speed: to first order |Delta n| <= speed |Delta d|/|d|, plus the two
 hypots (tau + 2u each), the quotient and the product (2u each): 35u speed.  Together
   |Delta n| <= speed (2 delta/|d| + 52u)  <=  speed K delta/|d|  with K = 2.5   wherever   rho_max >= 4|d|   (0.5 * 34 * rho/|d| >= 52),
 which the tests assert for every point they hold to the bound (the others -- lat == 90 -- are bit for bit: d = 0 there).  With speed ~ |d| this is 6.5e-7 at 89 N
 (1 - sin = 1.5e-4, rho = 1.1e5 m) and 5e-8 at 60 N, below the cap of 1e-6 speed the tests put on every point with lat <= 89 and speed >= 1 m/s.
 A pole row is the mean of N transformed values: its difference is at most the largest bound of that row + N * 2u * the largest |value| (the sequential sum).
 A node's value is a convex combination of four (bilinear) grid values with weights that are the same bits on both sides: its difference is at most the same
 combination of the four bounds, plus 16u * the combination of their |values| for the roundings of the sum."""
import ctypes as C
import ctypes.util

import numpy as np

U = 2.0 ** -53
C1, C2, K = 34., 3., 2.5
PI = 3.141592653589793          # contrib/mapx/include/mapx.h:47
RE_KM = 6371.228                # mapx_Re_km, mapx.h:55
OFF, LINEAR, STEP = 0, 1, 2

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f, _n in (("cos", 1), ("sin", 1), ("floor", 1), ("hypot", 2)):
    getattr(_libm, _f).restype = C.c_double
    getattr(_libm, _f).argtypes = [C.c_double] * _n

MPP = {   # what the reference's two .mpp files hold (mesh/NpsNextsim.mpp, mesh/NpsASR.mpp): lat0 lon0 lat1, rotation, scale, centre, radius, eccentricity
    "NpsNextsim": dict(lat0=90., lon0=0., lat1=60., rotation=-45., scale=0.001, center_lat=90., center_lon=135., equatorial_radius=6378.273, eccentricity=0.081816153),
    "NpsASR": dict(lat0=90., lon0=0., lat1=60., rotation=-175., scale=0.001, center_lat=90., center_lon=135., equatorial_radius=6378.273, eccentricity=0.081816153),
}


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).view(np.uint64) == np.ascontiguousarray(b, np.float64).view(np.uint64)


def transform(data, lat, lon, grid_y, pairs, forward, rotation_angle=0., per_point=False, details=None):
    """transformData on data [M, N, N_data] (a copy is returned).  lat [M], lon [N] (or [M*N] each with per_point), grid_y [M] the grid's y axis (the pole test),
    pairs = [(j0, j1, east_west_oriented)], forward(lat, lon) -> (x, y) for scalars.  details: a dict that receives, per east/north pair k, arrays [M*N] of
    |d|, rho_max, the larger latitude of the two projected points, the speed, the point's own latitude -- what bound_east_north() takes."""
    import math
    out = np.array(data, np.float64, copy=True)
    M, N = out.shape[:2]
    R = RE_KM * 1000.
    delta_t = 1.
    cos_m, sin_m = math.cos(-rotation_angle), math.sin(-rotation_angle)
    for k, (j0, j1, ew) in enumerate(pairs):
        if ew:
            dd, rr, ll, ss, lp = (np.zeros(M * N) for _ in range(5))
            for i in range(M * N):
                yi, xi = divmod(i, N)
                lat_tmp, lon_tmp = (float(lat[i]), float(lon[i])) if per_point else (float(lat[yi]), float(lon[xi]))
                t0, t1 = float(out[yi, xi, j0]), float(out[yi, xi, j1])
                if lat_tmp < 90.:
                    t0_deg = t0 / (R * _libm.cos(lat_tmp * PI / 180.)) * 180. / PI
                    t1_deg = t1 / R * 180. / PI
                else:
                    t0_deg = 0.
                    t1_deg = 0.
                lat_bis = lat_tmp + t1_deg * delta_t
                lon_bis = lon_tmp + t0_deg * delta_t
                lon_bis = lon_bis - 360. * _libm.floor(lon_bis / (360.))
                x, y = forward(lat_tmp, lon_tmp)
                xb, yb = forward(lat_bis, lon_bis)
                n0 = (xb - x) / delta_t
                n1 = (yb - y) / delta_t
                speed = _libm.hypot(t0, t1)
                new_speed = _libm.hypot(n0, n1)
                dd[i], rr[i], ll[i], ss[i], lp[i] = new_speed, max(_libm.hypot(x, y), _libm.hypot(xb, yb)), max(lat_tmp, lat_bis), speed, lat_tmp
                if new_speed > 0.:
                    n0 = n0 / new_speed * speed
                    n1 = n1 / new_speed * speed
                out[yi, xi, j0], out[yi, xi, j1] = n0, n1
            if details is not None:
                details[k] = dict(d=dd, rho=rr, lat=ll, speed=ss, lat_point=lp)
            pole = None
            if grid_y[0] == 90.:
                pole = (0, 1)
            if grid_y[M - 1] == 90.:
                pole = (M - 1, M - 2)
            if pole is not None:
                a0 = a1 = 0.
                for xi in range(N):
                    a0 = a0 + float(out[pole[1], xi, j0])
                    a1 = a1 + float(out[pole[1], xi, j1])
                a0 = a0 / N
                a1 = a1 / N
                out[pole[0], :, j0] = a0
                out[pole[0], :, j1] = a1
        if rotation_angle != 0.:
            a, b = out[:, :, j0].copy(), out[:, :, j1].copy()
            out[:, :, j0] = cos_m * a + sin_m * b
            out[:, :, j1] = -sin_m * a + cos_m * b
    return out


def wrap(data, x, y, cyclic_x, cyclic_y):
    """interpolateDataset (:1315-1373) on data [M, N, N_data] and the centres x [N], y [M]: the wrapped data (zero-initialised, as the reference's vector), x, y."""
    M, N, nd = data.shape
    cM, cN = M + int(bool(cyclic_y)), N + int(bool(cyclic_x))
    x, y = np.array(x, np.float64), np.array(y, np.float64)
    if cyclic_y:
        y = np.append(y, y[M - 1] + (y[M - 1] - y[M - 2]))
    if cyclic_x:
        x = np.append(x, x[N - 1] + (x[N - 1] - x[N - 2]))
    out = np.zeros((cM, cN, nd))
    out[:M, :N] = data
    if cyclic_y:
        out[cM - 1, :N] = data[0, :N]
    if cyclic_x:
        out[:M, cN - 1] = data[:M, 0]
    return out, x, y


def blend(mode, c0, c1, factor, bias, d0, d1):
    """ExternalData::get; None for an OFF group"""
    if mode == OFF:
        return None
    with np.errstate(all="ignore"):
        if mode == LINEAR:
            return factor * (c0 * d0 + c1 * d1) + bias
        return factor * d0 + bias


def bound_forward(x, y, lat):
    """|got - want| per component of nxs_mapx_forward: u hypot(x, y) (C1 + C2/(1 - sin(phi))); 0 at the pole"""
    one_minus = 1. - np.sin(np.asarray(lat) * PI / 180.)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = U * np.hypot(x, y) * (C1 + C2 / one_minus)
    return np.where(one_minus > 0., b, 0.)


def bound_east_north(det):
    """|got - want| per component of the transformed vector from transform()'s details of one pair: speed K delta/|d|, delta = u rho_max (C1 + C2/(1 - sin(phi)));
    0 where d == 0 (the zero vector, lat == 90)"""
    one_minus = 1. - np.sin(det["lat"] * PI / 180.)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = U * det["rho"] * (C1 + C2 / one_minus)
        b = det["speed"] * K * delta / det["d"]
    return np.where(det["d"] > 0., b, 0.)


def forward_points():
    """The (lat, lon) of tests/golden/mapx_forward.npz, seeded: 2 000 over 20 .. 90 N, longitudes outside [0, 360), the lon0 meridian and its antimeridian, the
    pole itself, latitudes close under it, and pairs 1e-5 degrees apart (the size of transformData's finite difference)."""
    rng = np.random.default_rng(2025)
    lat = [rng.uniform(20., 90., 2000)]
    lon = [rng.uniform(-180., 360., 2000)]
    lat.append(rng.uniform(20., 90., 100)); lon.append(np.concatenate([rng.uniform(-900., -180., 50), rng.uniform(360., 1080., 50)]))
    lat.append(np.linspace(20., 90., 29)); lon.append(np.zeros(29))
    lat.append(np.linspace(20., 90., 29)); lon.append(np.full(29, 180.))
    lat.append(np.full(9, 90.)); lon.append(np.linspace(-180., 360., 9))
    lat.append(np.array([89., 89.9, 89.99, 89.999, 89.9999, 20., 45.])); lon.append(np.array([10., -75., 135., 200., 359.5, 0., -45.]))
    a, o = rng.uniform(20., 89.9, 100), rng.uniform(0., 360., 100)
    lat += [a, a + 1e-5 * rng.uniform(-1., 1., 100)]; lon += [o, o + 1e-5 * rng.uniform(-1., 1., 100)]
    return np.concatenate(lat), np.concatenate(lon)


def transform_cases():
    """The seeded inputs of the fixture's transformData results: name -> dict(data [M, N, N_data], lat, lon, grid_y, pairs, rotation_angle, per_point, map)."""
    rng = np.random.default_rng(77)
    cases = {}

    def field(M, N, nd, zero_at=None):
        d = rng.uniform(-30., 30., (M, N, nd))
        if zero_at is not None:
            d[zero_at] = 0.                                   # a zero vector (every column of that point), at a longitude in [0, 360): the floor wrap leaves it
                                                              # alone, both projections are one point and the result is +0., +0. whatever the sine
        return d
    lat = np.array([89., 90.])
    cases["g2x2_pole_last"] = dict(data=field(2, 2, 2), lat=lat, lon=np.array([0., 180.]), grid_y=lat, pairs=[(0, 1, True)], rotation_angle=0., per_point=False, map="NpsNextsim")
    lat = np.array([90., 87.5, 85., 82.5, 80.])
    cases["g5x8_pole_first_rotated"] = dict(data=field(5, 8, 5, (2, 3)), lat=lat, lon=45. * np.arange(8), grid_y=lat, pairs=[(0, 1, True), (3, 2, True)], rotation_angle=0.3,
                                            per_point=False, map="NpsNextsim")
    lat = np.array([60., 65., 70., 75., 80.])
    cases["g5x8_no_pole"] = dict(data=field(5, 8, 5, (0, 2)), lat=lat, lon=45. * np.arange(8) - 90., grid_y=lat, pairs=[(0, 1, True), (2, 3, False)], rotation_angle=0.,
                                 per_point=False, map="NpsASR")
    lat = np.linspace(10., 90., 33)
    lon = -180. + 5. * np.arange(72)
    cases["g33x72_pole_last"] = dict(data=field(33, 72, 5, (7, 40)), lat=lat, lon=lon, grid_y=lat, pairs=[(0, 1, True), (2, 3, True)], rotation_angle=0., per_point=False,
                                     map="NpsNextsim")
    cases["g33x72_rotation_only"] = dict(data=field(33, 72, 5), lat=lat, lon=lon, grid_y=lat, pairs=[(0, 1, False), (4, 2, False)], rotation_angle=(-45. + 175.) * PI / 180.,
                                         per_point=False, map="NpsNextsim")
    latp, lonp = rng.uniform(70., 89.5, 40), rng.uniform(-180., 180., 40)
    latp[13] = 90.                                            # a point at the pole on a grid without a pole row (an x-y grid: its y axis is in metres)
    cases["g5x8_per_point_pole_point"] = dict(data=field(5, 8, 3), lat=latp, lon=lonp, grid_y=1e5 * np.arange(-2., 3.), pairs=[(0, 1, True)], rotation_angle=-0.7, per_point=True,
                                              map="NpsASR")
    return cases
