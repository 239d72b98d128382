// nxs_drifters.hpp -- internal interface (hidden visibility, not part of the ABI) between the dynamics handle (nxs_dyn.hip) and the drifter code
// that lives next to the exact point locator (nxs_drifters.inl, textually included by nxs_interp.hip: locate() exists once).
//
// Reference: FiniteElement::checkMoveDrifters / checkUpdateDrifters (FE.cpp:8375-8437) and Drifters::move / updateConc / maskXY
// (model/drifters.cpp:468-579).  The handle owns a State: up to NXS_DRIFTER_SETS sets (x, y, id, conc, found; double-buffered for the ordered
// compaction of maskXY) and two locators over the handle's OWN device arrays -- the undisplaced mesh (built once per set_mesh) and the mesh
// displaced by M_UM (rebuilt after a step or put_state).  Every pointer of a MeshView is a device pointer; every launch goes on `st`.
#ifndef NXS_DRIFTERS_HPP
#define NXS_DRIFTERS_HPP

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "nxs_means_points_body.inl"   // nxs_mp::Args

namespace nxs_drifters {

struct MeshView {
    int Nn = 0, Ne = 0, Neo = 0;            // nodes, elements, owned elements (they come first)
    const int *t0 = nullptr, *t1 = nullptr, *t2 = nullptr;   // 0-based triangles, one array per corner
    const double *x0 = nullptr, *y0 = nullptr;               // undisplaced coordinates
};

struct State;
State *create();
void destroy(State *s);
void mesh_changed(State *s);     // nxs_dyn_set_mesh: both locators are gone, the sets stay
void state_changed(State *s);    // a step or put_state: M_UM may have changed, the displaced locator is stale
void set_timing(State *s, bool on);
bool timing(const State *s, double ms[4]);   // last locator build, move kernels, conc kernel, mask kernels [ms]; false: nothing timed yet

bool any_set(const State *s);
bool has_set(const State *s, int set);
// every function below returns an NXS_* status and, on failure, the text in `err`
int set(State *s, hipStream_t st, int set, int32_t n, const double *x, const double *y, const int32_t *id, std::string &err);
int clear(State *s, int set);
int mesh_bbox(State *s, hipStream_t st, const MeshView &m, const double *UM /* NULL: undisplaced */, double out[4], std::string &err);
int move(State *s, hipStream_t st, const MeshView &m, const double *UT, const double *bbox, std::string &err);
int conc(State *s, hipStream_t st, const MeshView &m, const double *UM, const double *conc, int set, const double *bbox, double *conc_host, std::string &err);
int mask(State *s, hipStream_t st, int set, double conc_lim, const int32_t *keepers, int32_t n_keepers, int32_t *n_left, std::string &err);
int get(State *s, hipStream_t st, int set, int32_t *n, double *x, double *y, int32_t *id, double *conc, int32_t *found, std::string &err);

// the Moorings means on a loaded grid (nxs_dyn_means_points_*, nxs_means_points_kernels.inl): they use the two locators above and build none of their own
int means_points_update(State *s, hipStream_t st, const MeshView &m, const double *UM, const nxs_mp::Args &a, std::string &err);   // one launch, asynchronous
int means_points_lsm(State *s, hipStream_t st, const MeshView &m, int G, const double *gx, const double *gy, int *lsm /* device, [G] */, std::string &err);
bool means_points_timing(const State *s, double ms[2]);   // of the last means_points_update: its locator build (0: the locator was current), its kernel [ms]

}  // namespace nxs_drifters
#endif
