// nxs_wind_speed.inl -- windSpeedElement(i), FE.cpp:6359-6370 (FE.cpp = model/finiteelement.cpp): the mean over the element's three nodes of hypot(u, v) of
// M_wind ([2 * Nn]: u, then v).  ONE statement of it for k_fluxes, k_slab (newice_type 3) and the Moorings mean `wspeed` (k_means_elements), so that the three
// give the same bits from the same wind.  Textually included by each of the three kernel files.
#ifndef NXS_WIND_SPEED_INL
#define NXS_WIND_SPEED_INL
__device__ __forceinline__ double wind_speed_element(const double *wind, int Nn, int n0, int n1, int n2) {
    const int nd[3] = {n0, n1, n2};
    double wspd = 0.;
#pragma unroll
    for (int j = 0; j < 3; ++j) wspd += hypot(wind[nd[j]], wind[nd[j] + Nn]);
    return wspd / 3.;
}
#endif
