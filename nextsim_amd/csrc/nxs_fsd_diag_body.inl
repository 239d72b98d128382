// nxs_fsd_diag_body.inl -- D_dmax / D_dmean of ONE element: the "FSD relative parameters" block of updateIceDiagnostics() in a coupled build (FE.cpp:7902-7951),
// line by line in the reference's operand order.  __host__ __device__ text: means_elements_body (nxs_dyn_kernels.inl) calls it per thread for NXS_MEANS_DMAX /
// NXS_MEANS_DMEAN, and tests/cpl_out_host_kernel.cpp compiles the same text with g++ -O2 -ffp-contract=off.  Only + - * /, std::min and std::max (as the selects
// libstdc++ makes of them: (b < a) ? b : a and (a < b) ? b : a, so a NaN falls where the reference's falls): no libm call, and the build forbids contraction, so
// the result is bit for bit.
// M_conc_mech_fsd is read where it lies, bin-major ([nb][stride]): neighbouring threads read neighbouring addresses of each bin, and there is no per-thread array.
// The loops run over the bin number, which is the same for every lane (the limits and centres are scalar loads out of the by-value table); the break of
// FE.cpp:7922 is the only lane-dependent branch.
#ifndef NXS_FSD_DIAG_BODY_INL
#define NXS_FSD_DIAG_BODY_INL

namespace nxs_fsd_diag {

constexpr int MAX_BINS = 16;    // NXS_FSD_MAX_BINS

struct Args {   // travels to the kernel by value
    const double *mech;             // M_conc_mech_fsd [nb][stride]
    long long stride;               // M_num_elements
    int nb;                         // M_num_fsd_bins; 0: D_dmax = D_dmean = 0.
    double dmax_c_threshold;        // M_dmax_c_threshold (wave_coupling.dmax_c_threshold)
    double unbroken_floe_size;      // M_fsd_unbroken_floe_size
    double min_floe_size;           // M_fsd_min_floe_size
    double up[MAX_BINS];            // M_fsd_bin_up_limits
    double centres[MAX_BINS];       // M_fsd_bin_centres
};

__host__ __device__ inline double std_min(double a, double b) { return (b < a) ? b : a; }
__host__ __device__ inline double std_max(double a, double b) { return (a < b) ? b : a; }

// i: the element; D_conc: M_conc[i] (+ M_conc_young[i] in the young-ice category) as updateIceDiagnostics forms it just above (FE.cpp:7866-7884)
__host__ __device__ inline void diag(const Args &a, long long i, double D_conc, double &D_dmax, double &D_dmean) {
    const double *const M_conc_mech_fsd = a.mech + i;   // bin j of this element: M_conc_mech_fsd[j * a.stride]
    const int M_num_fsd_bins = a.nb;
    D_dmean = 0.;
    D_dmax = 0.;
    if (M_num_fsd_bins > 0) {
        if (D_conc > 0) {
            D_dmax = 1000.;
            D_dmean = 1000.;
            const double last = M_conc_mech_fsd[(M_num_fsd_bins - 1) * a.stride];
            if (last <= a.dmax_c_threshold * D_conc) {
                double ctot_fsd = last;
                for (int j = M_num_fsd_bins - 2; j > -1; j--) {
                    ctot_fsd += M_conc_mech_fsd[j * a.stride];
                    if (ctot_fsd > a.dmax_c_threshold * D_conc) {
                        D_dmax = a.up[j];
                        break;
                    }
                }
                D_dmean = 0.;
                for (int j = 0; j < M_num_fsd_bins; j++) D_dmean += M_conc_mech_fsd[j * a.stride] * a.centres[j] / D_conc;
            } else {
                D_dmax = (last / D_conc - a.dmax_c_threshold) / (1. - a.dmax_c_threshold) * (a.unbroken_floe_size - a.up[M_num_fsd_bins - 1]) + a.up[M_num_fsd_bins - 1];
                D_dmax = std_min(D_dmax, a.unbroken_floe_size);
                D_dmean = 0.;
                for (int j = 0; j < M_num_fsd_bins - 1; j++) D_dmean += M_conc_mech_fsd[j * a.stride] * a.centres[j] / D_conc;
                D_dmean += last * D_dmax / D_conc;
            }
            D_dmax = std_min(D_dmax, a.unbroken_floe_size);
            D_dmax = std_max(D_dmax, a.min_floe_size);
            D_dmean = std_min(D_dmax, D_dmean);
            D_dmean = std_max(D_dmean, a.min_floe_size);
        } else {
            D_dmax = 0.;
            D_dmean = 0.;
        }
    }
}

}  // namespace nxs_fsd_diag
#endif
