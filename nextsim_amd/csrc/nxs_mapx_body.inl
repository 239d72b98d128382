// nxs_mapx_body.inl -- forward_mapx for a north-aspect "Polar Stereographic Ellipsoid" map (contrib/mapx/src/polar_stereographic.c:136-186 followed by the rotation
// and shift of contrib/mapx/src/mapx.c:1112-1113) for ONE point: the ONE copy of it.  Textually included by nxs_nodal_forcing_kernels.inl (k_mapx_forward behind
// nxs_mapx_forward, k_nf_east_north behind nxs_dyn_forcing_ingest), by the host side of nxs_mapx_forward / nxs_mapx_polar_north (nxs_nodal_forcing.inl) and by
// tests/nodal_forcing_host_kernel.cpp, which compiles it for the host with the HIP qualifiers defined away.  Operand order is the reference's (RADIANS(t) is
// ((t) * PI/180): the product first); the build is uncontracted (-ffp-contract=off).  Needs nxs_mapx_polar (include/nxs_dyn.h) and <math.h>.

#define NXS_MAPX_PI 3.141592653589793      // contrib/mapx/include/mapx.h:47
#define NXS_MAPX_RE_KM 6371.228            // mapx_Re_km, contrib/mapx/include/mapx.h:55

// polar_stereographic_ellipsoid with lat0 == 90 (both lat1 branches): the unrotated map coordinates
__host__ __device__ __forceinline__ void nxs_mapx_polar_xy(const nxs_mapx_polar &m, double lat, double lon, double *x, double *y) {
    const double phi = lat * NXS_MAPX_PI / 180;
    const double lam = (lon - m.lon0) * NXS_MAPX_PI / 180;
    const double s = sin(phi);
    double num = 1.0 + m.eccentricity * s;
    double den = 1.0 - m.eccentricity * s;
    const double t = sqrt((1.0 - s) / (1.0 + s) * pow(num / den, m.eccentricity));
    double rho;
    if ((90.0 != m.lat1) && (-90.0 != m.lat1)) {
        rho = m.Rg * m.m1 * t / m.t1;
    } else {
        num = 2 * m.Rg * m.scale * t;
        den = sqrt(pow(1 + m.eccentricity, 1 + m.eccentricity) * pow(1 - m.eccentricity, 1 - m.eccentricity));
        rho = num / den;
    }
    *x = rho * sin(lam);
    *y = -rho * cos(lam);
    *x += m.false_easting;
    *y += m.false_northing;
}

// forward_mapx (maximum_error == 0: forward_xy_mapx_check does nothing)
__host__ __device__ __forceinline__ void nxs_mapx_forward_point(const nxs_mapx_polar &m, double lat, double lon, double *u, double *v) {
    double x, y;
    nxs_mapx_polar_xy(m, lat, lon, &x, &y);
    *u = m.T00 * x + m.T01 * y - m.u0;
    *v = m.T10 * x + m.T11 * y - m.v0;
}
