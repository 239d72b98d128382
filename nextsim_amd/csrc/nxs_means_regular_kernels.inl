// nxs_means_regular_kernels.inl -- updateGridMean() on the REGULAR grid as two launches on the handle's stream (nxs_dyn_means_regular_update) and setLSM on the mesh
// at rest (nxs_dyn_means_regular_lsm).  Textually included by nxs_dyn.hip behind the nodal forcing's kernels; the host side is nxs_means_regular.inl, the
// arithmetic nxs_means_regular_body.inl.
//
// Reference: contrib/bamg/src/InterpFromMeshToGridx.cpp:94-181, model/gridoutput.cpp:360-378, 387-415, 486-538, 558-574, 578-623.  The reference interpolates three
// times (proc mask, elemental variables, nodal variables) in the same mesh at the same points; the winner of a point -- the LAST element in ascending order that
// holds it -- is the same each time and is found once.  No search table: the mesh moves every step, a table would be rebuilt per call.
//   k_means_regular_hits    one thread per element, the reference's own loop: the mesh is x0 + M_UM formed here, the window of :120-130 is walked, and every
//                    point the triangle holds takes atomicMax(hit[point], n).  An integer maximum does not depend on the order of arrival: the result is
//                    deterministic and equals "the last in ascending order wins".  hit is -1 everywhere before the launch (a memset of 0xFF on the stream).  atomicMax
//                    on global memory is device-scope; the gather runs in the next launch, behind the kernel boundary.  With triangles much smaller than the spacing
//                    most threads find no point and write nothing.
//   k_means_regular_gather  one thread per grid point in GRID order, so neighbouring threads read-modify-write neighbouring addresses of the [var][G] rows.  It
//                    recomputes its winner's area coordinates (the same function, the same bits), gathers, rotates, accumulates and applies the ice-mask rule.
//                    The nodal leg's interp_out row is staged in dynamic LDS ([n_nod][256], one column per thread: conflict-free) because rotateVectors indexes
//                    it by run-time column numbers -- a per-thread array would go to scratch memory.
//   k_means_regular_lsm     setLSM: 1 where any triangle, ghosts included, holds the point.

__global__ void __launch_bounds__(BLOCK) k_means_regular_hits(nxs_mr::Args a) {
    const int n = blockIdx.x * BLOCK + threadIdx.x;
    if (n >= a.Ne) return;
    int *hit = a.hit;
    nxs_mr::element_hits(a, n, [hit, n](int g) { atomicMax(hit + g, n); });
}

__global__ void __launch_bounds__(BLOCK) k_means_regular_gather(nxs_mr::Args a) {
    extern __shared__ double mr_interp_out[];   // [n_nod][BLOCK]
    const int g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= a.m.G) return;
    nxs_mr::point(a, g, mr_interp_out + threadIdx.x, BLOCK);
}

__global__ void __launch_bounds__(BLOCK) k_means_regular_lsm(int G, const int *__restrict__ hit, int *__restrict__ lsm) {
    const int g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= G) return;
    lsm[g] = hit[g] >= 0 ? 1 : 0;
}
