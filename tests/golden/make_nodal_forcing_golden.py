"""Generates tests/golden/mapx_forward.npz with the REAL contrib/mapx (oracle/_ref/libmapx_ref.so, built by `python __graft_entry__.py` where the reference is
present) and the reference's two .mpp files:
    python tests/golden/make_nodal_forcing_golden.py

  lat, lon                  nodal_forcing_ref.forward_points(): 20 .. 90 N, longitudes outside [0, 360), the lon0 meridian, the pole, pairs 1e-5 degrees apart
  x_<map>, y_<map>          forward_mapx of every point for NpsNextsim.mpp and NpsASR.mpp
  polar_<map>               the derived constants of the real mapx_class in the order _abi.MAPX_POLAR_FIELDS (what nxs_mapx_polar_north has to reproduce)
  t_<case>                  the complete transformData result of nodal_forcing_ref.transform_cases(): the Python restatement nodal_forcing_ref.transform() whose only
                            projection is the real library's forward_mapx
  constants                 mapx_Re_km and PI as a translation unit that includes the reference's mapx.h prints them (%.17g)"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nodal_forcing_ref as R  # noqa: E402

REF = os.environ.get("NXS_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "mapx_forward.npz")


class MapxClass(C.Structure):      # the head of mapx_class (contrib/mapx/include/mapx.h:82-118), down to t2
    _fields_ = ([(k, C.c_double) for k in ("lat0", "lon0", "lat1", "lon1", "rotation", "scale", "south", "north", "west", "east", "center_lat", "center_lon", "label_lat",
                                           "label_lon", "lat_interval", "lon_interval")]
                + [(k, C.c_int) for k in ("cil_detail", "bdy_detail", "riv_detail", "dummy1")]
                + [(k, C.c_double) for k in ("equatorial_radius", "polar_radius", "eccentricity", "e2", "x0", "y0", "false_easting", "false_northing", "center_scale",
                                             "maximum_error")]
                + [(k, C.c_int) for k in ("utm_zone", "isin_nzone", "isin_justify", "dummy2")]
                + [(k, C.c_double) for k in ("T00", "T01", "T10", "T11", "u0", "v0")]
                + [(k, C.c_int) for k in ("map_stradles_180", "dummy3")]
                + [(k, C.c_double) for k in ("e4", "e6", "e8", "qp", "Rq", "q0", "q1", "q2", "Rg", "sin_phi0", "sin_phi1", "sin_phi2", "sin_lam1", "cos_phi0", "cos_phi1",
                                             "cos_phi2", "cos_lam1", "beta1", "sin_beta1", "cos_beta1", "D", "phis", "kz", "rho0", "n", "C", "F", "m0", "m1", "m2", "t0", "t1",
                                             "t2")])


def main():
    L = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libmapx_ref.so"))
    L.init_mapx.restype = C.POINTER(MapxClass); L.init_mapx.argtypes = [C.c_char_p]
    L.forward_mapx.argtypes = [C.POINTER(MapxClass), C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.close_mapx.argtypes = [C.POINTER(MapxClass)]
    maps = {}
    for name in R.MPP:
        m = L.init_mapx(os.path.join(REF, "mesh", name + ".mpp").encode())
        assert m, name
        assert m.contents.maximum_error == 0. and m.contents.lat0 == 90.
        maps[name] = m
    a, b = C.c_double(), C.c_double()

    def forward(name):
        def f(lat, lon):
            L.forward_mapx(maps[name], float(lat), float(lon), C.byref(a), C.byref(b))
            return a.value, b.value
        return f
    out = {}
    lat, lon = R.forward_points()
    out["lat"], out["lon"] = lat, lon
    for name in R.MPP:
        xy = np.array([forward(name)(la, lo) for la, lo in zip(lat, lon)])
        out["x_" + name], out["y_" + name] = xy[:, 0].copy(), xy[:, 1].copy()
        c = maps[name].contents
        out["polar_" + name] = np.array([c.lon0, c.Rg, c.m1, c.t1, c.eccentricity, c.scale, c.lat1, c.T00, c.T01, c.T10, c.T11, c.u0, c.v0, c.false_easting, c.false_northing])
    for name, case in R.transform_cases().items():
        out["t_" + name] = R.transform(case["data"], case["lat"], case["lon"], case["grid_y"], case["pairs"], forward(case["map"]), case["rotation_angle"], case["per_point"])
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "c.c")
        open(src, "w").write('#include <stdio.h>\n#include <stdbool.h>\n#include "mapx.h"\nint main(void){ printf("%.17g %.17g\\n", (double)mapx_Re_km, (double)PI); return 0; }\n')
        subprocess.check_call(["gcc", "-I", os.path.join(REF, "contrib", "mapx", "include"), src, "-o", os.path.join(tmp, "c")])
        out["constants"] = np.array([float(v) for v in subprocess.check_output([os.path.join(tmp, "c")], text=True).split()])
    for m in maps.values():
        L.close_mapx(m)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes;", lat.size, "points")


if __name__ == "__main__":
    main()
