// nxs_nesting_kernels.inl -- the in-place statements of FiniteElement::step() outside thermo() and the dynamics, on the device (textually included by nxs_dyn.hip
// behind the thermo-forcing kernels; include/nxs_dyn.h, nxs_dyn_nesting_* and nxs_dyn_diffuse).  FE.cpp = model/finiteelement.cpp, externaldata.cpp = model/externaldata.cpp.
//   k_nesting_ice       nestingIce(), FE.cpp:4878-4908: M_conc, M_thick, M_snow_thick (and the young-ice trio) relaxed towards the outer model.
//   k_nesting_dynamics  nestingDynamics(), FE.cpp:4915-4958: M_sigma[0..2], M_damage, M_ridge_ratio per element, M_VT per node, in ONE launch (lane i takes the
//              i-th pair of elements and the i-th pair of nodes).  M_sigma / M_damage are nudged where they are current: in their arrays, or in the 4-double
//              records the sub-step loop left behind (k_pack_state's layout), read and written as two 16-byte halves per element; a record slot that is not
//              nudged (the fourth under EVP / mEVP, where M_damage is taken from its array) goes back with its bits.
//   Both evaluate every target in the kernel -- ExternalData::get, externaldata.cpp:401-403 + 438 (LINEAR), :434 + 438 (STEP, which never touches d1) -- so no blended
//   row is stored and each snapshot is read once.  A lane takes two neighbouring entries with one 16-byte access per row (every row is an allocation of its own);
//   the last entry of an odd count is a scalar tail; the second half of M_VT is 16-byte aligned only where Nn is even, else it is walked by scalars.
//   k_diffuse_pack / k_diffuse   diffuse(), FE.cpp:2760-2815, for M_sst and M_sss at once: the first packs {sst, sss} of every element into one 16-byte pair (the
//              OLD copy Jacobi needs anyway), the second does per element one 12-byte index load, up to three 16-byte gathers and one store per field that is on.
// Plain loads and stores, no LDS, no atomics.  The bodies compile for the host (tests/nesting_host_kernel.cpp defines the HIP qualifiers away).  The build is
// uncontracted (-ffp-contract=off): a*b + c is two roundings, and the association is the reference's.

enum { NEST_EL_ROWS = 12, NEST_ND_ROWS = 3, NEST_DATASETS = 5, NEST_ICE_FIELDS = 6 };
static_assert(NEST_EL_ROWS == NXS_NEST_ELEMENT_ROWS && NEST_ND_ROWS == NXS_NEST_NODE_ROWS && NEST_DATASETS == NXS_NEST_DATASETS, "the rows of nxs_dyn_nesting_*");

struct alignas(16) NestPair { double a, b; };   // two neighbouring entries of a row: one 16-byte access

struct NestTime { double c0, c1, factor, bias; int mode; };   // one dataset's ExternalData::get: NXS_TF_LINEAR or NXS_TF_STEP
struct NestRow { const double *d0, *d1; };                    // its snapshots of one variable (d1 is not read under NXS_TF_STEP: it may be NULL)

// ExternalData::get for one entry
__device__ __forceinline__ double nest_target(const NestTime &t, double d0, double d1) {
    return t.mode == NXS_TF_LINEAR ? t.factor * (t.c0 * d0 + t.c1 * d1) + t.bias : t.factor * d0 + t.bias;
}
__device__ __forceinline__ double nest_target_at(const NestTime &t, const NestRow &r, int i) {
    return nest_target(t, r.d0[i], t.mode == NXS_TF_LINEAR ? r.d1[i] : 0.);
}
__device__ __forceinline__ NestPair nest_target_pair(const NestTime &t, const NestRow &r, int i) {
    const NestPair p0 = *reinterpret_cast<const NestPair *>(r.d0 + i);
    NestPair p1{0., 0.};
    if (t.mode == NXS_TF_LINEAR) p1 = *reinterpret_cast<const NestPair *>(r.d1 + i);
    return NestPair{nest_target(t, p0.a, p1.a), nest_target(t, p0.b, p1.b)};
}
// fNudge (FE.cpp:4892-4895) times the step quotient: the product every row of the entry shares.  std::min(1., r) is (r < 1.) ? r : 1.
__device__ __forceinline__ double nest_weight(int fn, double dist, double scale, double q) {
    double fNudge;
    if (fn == NXS_NUDGE_LINEAR) { const double r = dist / scale; fNudge = 1. - (r < 1. ? r : 1.); }
    else fNudge = exp(-dist / scale);
    return fNudge * q;
}
// x += (fNudge*(time_step/nudge_time)*(target - x))
__device__ __forceinline__ double nest_nudge(double x, double w, double target) { return x + (w * (target - x)); }

// one row of stride 1, lane-wise: the pair at i, or the scalar tail
__device__ __forceinline__ void nest_row_pair(double *x, const NestTime &t, const NestRow &r, int i, double wa, double wb) {
    const NestPair tg = nest_target_pair(t, r, i);
    NestPair v = *reinterpret_cast<NestPair *>(x + i);
    v.a = nest_nudge(v.a, wa, tg.a);
    v.b = nest_nudge(v.b, wb, tg.b);
    *reinterpret_cast<NestPair *>(x + i) = v;
}
__device__ __forceinline__ void nest_row_one(double *x, const NestTime &t, const NestRow &r, int i, double w) { x[i] = nest_nudge(x[i], w, nest_target_at(t, r, i)); }

struct NestIce {
    int Ne, nfields, fn;         // nfields: 3, or 6 with the young-ice category
    double scale, q;             // nudge_scale; (double)time_step / nudge_timescale
    NestTime t_dist, t_ice;
    NestRow dist, snap[NEST_ICE_FIELDS];
    double *x[NEST_ICE_FIELDS];  // M_conc, M_thick, M_snow_thick, M_conc_young, M_h_young, M_hs_young
};

__global__ void __launch_bounds__(BLOCK) k_nesting_ice(NestIce a) {
    const int i = 2 * (blockIdx.x * BLOCK + threadIdx.x);   // this lane's first element
    if (i + 1 < a.Ne) {
        const NestPair d = nest_target_pair(a.t_dist, a.dist, i);
        const double wa = nest_weight(a.fn, d.a, a.scale, a.q), wb = nest_weight(a.fn, d.b, a.scale, a.q);
        for (int f = 0; f < a.nfields; ++f) nest_row_pair(a.x[f], a.t_ice, a.snap[f], i, wa, wb);
    } else if (i < a.Ne) {   // odd Ne: the last element alone
        const double w = nest_weight(a.fn, nest_target_at(a.t_dist, a.dist, i), a.scale, a.q);
        for (int f = 0; f < a.nfields; ++f) nest_row_one(a.x[f], a.t_ice, a.snap[f], i, w);
    }
}

struct NestDyn {
    int Ne, Nn, fn;
    int rec;                     // M_sigma is current in the records S4 ([Ne][4]: sigma0, sigma1, sigma2, slot 3), else in s[0..2]
    int dmg_rec;                 // ... and slot 3 is M_damage (BBM); else M_damage is its array
    double scale, q, qvt;        // qvt: dtime_step / nudge_timescale (FE.cpp:4954-4955)
    NestTime t_dist, t_dyn, t_dist_n, t_nodes;
    NestRow dist, sig[3], dmg, ridge, dist_n, vt[2];
    double *S4, *s[3], *damage, *ridge_x, *VT;
};

// one element's record: two 16-byte halves in, two out
__device__ __forceinline__ void nest_record(const NestDyn &a, int e, double w) {
    NestPair *S = reinterpret_cast<NestPair *>(a.S4) + 2 * (size_t)e;
    NestPair lo = S[0], hi = S[1];
    lo.a = nest_nudge(lo.a, w, nest_target_at(a.t_dyn, a.sig[0], e));
    lo.b = nest_nudge(lo.b, w, nest_target_at(a.t_dyn, a.sig[1], e));
    hi.a = nest_nudge(hi.a, w, nest_target_at(a.t_dyn, a.sig[2], e));
    if (a.dmg_rec) hi.b = nest_nudge(hi.b, w, nest_target_at(a.t_dyn, a.dmg, e));
    S[0] = lo; S[1] = hi;
}

__global__ void __launch_bounds__(BLOCK) k_nesting_dynamics(NestDyn a) {
    const int i = 2 * (blockIdx.x * BLOCK + threadIdx.x);   // this lane's first element and first node
    if (i + 1 < a.Ne) {
        const NestPair d = nest_target_pair(a.t_dist, a.dist, i);
        const double wa = nest_weight(a.fn, d.a, a.scale, a.q), wb = nest_weight(a.fn, d.b, a.scale, a.q);
        if (a.rec) {
            const NestPair t0 = nest_target_pair(a.t_dyn, a.sig[0], i), t1 = nest_target_pair(a.t_dyn, a.sig[1], i), t2 = nest_target_pair(a.t_dyn, a.sig[2], i);
            NestPair t3{0., 0.};
            if (a.dmg_rec) t3 = nest_target_pair(a.t_dyn, a.dmg, i);
            NestPair *S = reinterpret_cast<NestPair *>(a.S4) + 2 * (size_t)i;   // the two records lie side by side: four halves
            NestPair lo0 = S[0], hi0 = S[1], lo1 = S[2], hi1 = S[3];
            lo0.a = nest_nudge(lo0.a, wa, t0.a); lo0.b = nest_nudge(lo0.b, wa, t1.a); hi0.a = nest_nudge(hi0.a, wa, t2.a);
            lo1.a = nest_nudge(lo1.a, wb, t0.b); lo1.b = nest_nudge(lo1.b, wb, t1.b); hi1.a = nest_nudge(hi1.a, wb, t2.b);
            if (a.dmg_rec) { hi0.b = nest_nudge(hi0.b, wa, t3.a); hi1.b = nest_nudge(hi1.b, wb, t3.b); }
            S[0] = lo0; S[1] = hi0; S[2] = lo1; S[3] = hi1;
        } else {
            for (int k = 0; k < 3; ++k) nest_row_pair(a.s[k], a.t_dyn, a.sig[k], i, wa, wb);
        }
        if (!a.dmg_rec) nest_row_pair(a.damage, a.t_dyn, a.dmg, i, wa, wb);
        nest_row_pair(a.ridge_x, a.t_dyn, a.ridge, i, wa, wb);
    } else if (i < a.Ne) {   // odd Ne: the last element alone
        const double w = nest_weight(a.fn, nest_target_at(a.t_dist, a.dist, i), a.scale, a.q);
        if (a.rec) nest_record(a, i, w);
        else for (int k = 0; k < 3; ++k) nest_row_one(a.s[k], a.t_dyn, a.sig[k], i, w);
        if (!a.dmg_rec) nest_row_one(a.damage, a.t_dyn, a.dmg, i, w);
        nest_row_one(a.ridge_x, a.t_dyn, a.ridge, i, w);
    }
    // M_VT: u at [i], v at [i + Nn] (FE.cpp:4941-4957)
    double *u = a.VT, *v = a.VT + a.Nn;
    if (i + 1 < a.Nn) {
        const NestPair d = nest_target_pair(a.t_dist_n, a.dist_n, i);
        const double wa = nest_weight(a.fn, d.a, a.scale, a.qvt), wb = nest_weight(a.fn, d.b, a.scale, a.qvt);
        nest_row_pair(u, a.t_nodes, a.vt[0], i, wa, wb);
        if ((a.Nn & 1) == 0) nest_row_pair(v, a.t_nodes, a.vt[1], i, wa, wb);
        else { nest_row_one(v, a.t_nodes, a.vt[1], i, wa); nest_row_one(v, a.t_nodes, a.vt[1], i + 1, wb); }   // (v + i is 8 bytes off a 16-byte boundary)
    } else if (i < a.Nn) {
        const double w = nest_weight(a.fn, nest_target_at(a.t_dist_n, a.dist_n, i), a.scale, a.qvt);
        nest_row_one(u, a.t_nodes, a.vt[0], i, w);
        nest_row_one(v, a.t_nodes, a.vt[1], i, w);
    }
}

// ---- diffuse(), FE.cpp:2760-2815
struct DiffTri { int n[3]; };   // bamgmesh->ElementConnectivity of one element, 0-based, -1 on the boundary: column j the triangle across the edge of vertices (j+1)%3, (j+2)%3

__global__ void __launch_bounds__(BLOCK) k_diffuse_pack(int Ne, const double *__restrict__ sst, const double *__restrict__ sss, NestPair *__restrict__ old) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= Ne) return;
    old[e] = NestPair{sst[e], sss[e]};   // std::vector<double> old_variable_elt = variable_elt_root (FE.cpp:2776), for both fields
}

// fluxes_source[0] + fluxes_source[1] + fluxes_source[2] added to the field (FE.cpp:2790-2809): every flux reads the OLD row; a missing neighbour gives 0.
__device__ __forceinline__ double diffuse_sum(double factor, double me, bool h0, double n0, bool h1, double n1, bool h2, double n2) {
    const double f0 = h0 ? factor * (n0 - me) : 0., f1 = h1 ? factor * (n1 - me) : 0., f2 = h2 ? factor * (n2 - me) : 0.;
    return me + (f0 + f1 + f2);
}

__global__ void __launch_bounds__(BLOCK) k_diffuse(int Ne, const DiffTri *__restrict__ ec, const NestPair *__restrict__ old, double factor_sst, double factor_sss, int on_sst, int on_sss,
                                                   double *sst, double *sss) {
    const int e = blockIdx.x * BLOCK + threadIdx.x;
    if (e >= Ne) return;
    const DiffTri t = ec[e];
    const NestPair me = old[e];
    const bool h0 = t.n[0] >= 0, h1 = t.n[1] >= 0, h2 = t.n[2] >= 0;
    // three unconditional 16-byte gathers: a missing neighbour reads the element's own pair (in the cache already) and its flux is 0. below
    const NestPair n0 = old[h0 ? t.n[0] : e], n1 = old[h1 ? t.n[1] : e], n2 = old[h2 ? t.n[2] : e];
    if (on_sst) sst[e] = diffuse_sum(factor_sst, me.a, h0, n0.a, h1, n1.a, h2, n2.a);
    if (on_sss) sss[e] = diffuse_sum(factor_sss, me.b, h0, n0.b, h1, n1.b, h2, n2.b);
}
