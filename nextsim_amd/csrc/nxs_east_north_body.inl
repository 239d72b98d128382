// nxs_east_north_body.inl -- transformData's east/north branch for ONE point (model/externaldata.cpp:1157-1203): the ONE copy of it.  Textually included by
// nxs_nodal_forcing_kernels.inl (k_nf_east_north behind nxs_dyn_forcing_ingest) and by nxs_nodemap_kernels.inl (k_nodemap_source behind nxs_nodemap_receive_rows);
// it compiles for the host with the HIP qualifiers defined away.  delta_t is the reference's constant 1. (externaldata.cpp:956).  Uncontracted build.

#include "nxs_mapx_body.inl"

// externaldata.cpp:1157-1203 for one point
__device__ __forceinline__ void nf_east_north_point(const nxs_mapx_polar &map, double R, double lat0, double lon0, double *p0, double *p1) {
    const double PI = NXS_MAPX_PI, dt = 1.;
    const double east = *p0, north = *p1;
    double east_deg, north_deg;
    if (lat0 < 90.) {
        east_deg = east / (R * cos(lat0 * PI / 180.)) * 180. / PI;
        north_deg = north / R * 180. / PI;
    } else {
        east_deg = 0.;
        north_deg = 0.;
    }
    const double lat1 = lat0 + north_deg * dt;
    double lon1 = lon0 + east_deg * dt;
    lon1 = lon1 - 360. * floor(lon1 / (360.));
    double x0, y0, x1, y1;
    nxs_mapx_forward_point(map, lat0, lon0, &x0, &y0);
    nxs_mapx_forward_point(map, lat1, lon1, &x1, &y1);
    double vx = (x1 - x0) / dt;
    double vy = (y1 - y0) / dt;
    const double speed = hypot(east, north);
    const double moved = hypot(vx, vy);
    if (moved > 0.) {
        vx = vx / moved * speed;
        vy = vy / moved * speed;
    }
    *p0 = vx;
    *p1 = vy;
}
