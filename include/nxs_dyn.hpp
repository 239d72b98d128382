// nxs_dyn.hpp -- header-only C++ convenience layer over the C ABI of nxs_dyn.h, with the reference's own
// method names and error behaviour: every failure throws std::runtime_error, as FiniteElement does
// (uncaught -> terminate, FE.cpp:14653).  Nothing here computes; it only forwards to libnxsdyn.so.
#ifndef NXS_DYN_HPP
#define NXS_DYN_HPP

#include <stdexcept>
#include <string>
#include <vector>

#include "nxs_dyn.h"

namespace nxs {

class FiniteElementDynamics {
public:
    explicit FiniteElementDynamics(const nxs_dyn_params &p, int device = 0) {
        if (nxs_dyn_create(&p, device, &h_) != 0) throw std::runtime_error(std::string("nxs_dyn_create: ") + nxs_dyn_last_error(nullptr));
    }
    ~FiniteElementDynamics() { nxs_dyn_destroy(h_); }
    FiniteElementDynamics(const FiniteElementDynamics &) = delete;
    FiniteElementDynamics &operator=(const FiniteElementDynamics &) = delete;

    void setMesh(const nxs_dyn_mesh &m) { check(nxs_dyn_set_mesh(h_, &m), "set_mesh"); }      // distributedMeshProcessing, FE.cpp:50-143
    void setHalo(const nxs_dyn_halo &hl) { check(nxs_dyn_set_halo(h_, &hl), "set_halo"); }    // initUpdateGhosts, FE.cpp:14003-14088
    void setHaloExchange(nxs_dyn_halo_fn fn, void *ctx) { check(nxs_dyn_set_halo_exchange_fn(h_, fn, ctx), "set_halo_exchange_fn"); }   // the caller's own M_comm.send / recv, FE.cpp:13981-13985
    void putState(const nxs_dyn_state &s) { check(nxs_dyn_put_state(h_, &s), "put_state"); }
    void getState(nxs_dyn_state &s) { check(nxs_dyn_get_state(h_, &s), "get_state"); }
    void setForcing(const nxs_dyn_forcing &f) { check(nxs_dyn_set_forcing(h_, &f), "set_forcing"); }
    // ExternalData's two snapshots resident + the per-step time coefficients (externaldata.cpp:360-401)
    void setForcingPair(const nxs_dyn_forcing &f0, const nxs_dyn_forcing &f1) { check(nxs_dyn_set_forcing_pair(h_, &f0, &f1), "set_forcing_pair"); }
    void setForcingTime(double fcoeff0, double fcoeff1, const double *factor = nullptr, const double *bias = nullptr) {
        check(nxs_dyn_set_forcing_time(h_, fcoeff0, fcoeff1, factor, bias), "set_forcing_time");
    }
    // the same snapshots made on the device from a dataset's source grid: transformData, the cyclic wrap, InterpFromGridToMeshx at the nodes (externaldata.cpp:461-940);
    // the time blend with coefficients per dataset; M_element_depth alone
    void forcingTargets(int set, const double *RX, const double *RY) { check(nxs_dyn_forcing_targets(h_, set, RX, RY), "forcing_targets"); }
    void forcingIngest(int set, const nxs_dyn_forcing_grid &g, bool cyclic_x, bool cyclic_y, const double *data, int N_data, const int32_t *row, const int32_t *snapshot,
                       const nxs_dyn_forcing_vectors *vectors = nullptr) {
        check(nxs_dyn_forcing_ingest(h_, set, &g, cyclic_x ? 1 : 0, cyclic_y ? 1 : 0, data, N_data, row, snapshot, vectors), "forcing_ingest");
    }
    void setForcingTimeRows(const struct nxs_dyn_forcing_time_rows &t) { check(nxs_dyn_set_forcing_time_rows(h_, &t), "set_forcing_time_rows"); }
    void setElementDepth(const double *depth) { check(nxs_dyn_set_element_depth(h_, depth), "set_element_depth"); }
    void forcingGet(int which, const nxs_dyn_forcing_rows &out) { check(nxs_dyn_forcing_get(h_, which, &out), "forcing_get"); }
    void setOption(const char *key, long long value) { check(nxs_dyn_set_option(h_, key, value), "set_option"); }
    void getDiag(nxs_dyn_diag &d) { check(nxs_dyn_get_diag(h_, &d), "get_diag"); }
    // the coupled build's terms (#ifdef OASIS): M_tau_wi into explicitSolve(), M_cum_damage / M_conc_fsd through the sub-steps and update()
    void setWaveStress(const double *tau_wi) { check(nxs_dyn_set_wave_stress(h_, tau_wi), "set_wave_stress"); }
    void putCoupled(const nxs_dyn_coupled &c) { check(nxs_dyn_put_coupled(h_, &c), "put_coupled"); }
    void getCoupled(nxs_dyn_coupled &c) { check(nxs_dyn_get_coupled(h_, &c), "get_coupled"); }

    void explicitSolve() { check(nxs_dyn_explicit_solve(h_), "explicitSolve"); }               // FE.cpp:10182-10643
    void update() { check(nxs_dyn_update(h_), "update"); }                                     // FE.cpp:3919-4132
    void step() { check(nxs_dyn_step(h_), "step"); }                                           // FE.cpp:8197-8214
    void synchronize() { check(nxs_dyn_synchronize(h_), "synchronize"); }

    bool checkRegridding(double *min_angle = nullptr) {                                        // FE.cpp:8298-8309 (local part)
        double ang = 0; int32_t flip = 0, rg = 0;
        check(nxs_dyn_check_regridding(h_, &ang, &flip, &rg), "checkRegridding");
        if (min_angle) *min_angle = ang;
        return rg != 0;
    }
    void checkFieldsFast() {                                                                   // FE.cpp:14536-14655: throws on a bad field
        int32_t crash = 0;
        check(nxs_dyn_check_fields_fast(h_, &crash), "checkFieldsFast");
        if (crash) throw std::runtime_error("FiniteElement::checkFieldsFast: Check failed");
    }
    // FE.cpp:7860-7905: the element diagnostics of checkOutputs() / exportResults().  Host arrays of `d` that are not NULL are filled; the return value
    // is the DEVICE address of the same diagnostics as [Ne][NXS_ICE_DIAG_FIELDS] rows (what nxs_interp_mesh_to_grid_device samples for a Moorings record).
    const double *updateIceDiagnostics(nxs_dyn_ice_diag *d = nullptr) {
        const double *rows = nullptr;
        check(nxs_dyn_ice_diagnostics(h_, d, &rows), "updateIceDiagnostics");
        return rows;
    }
    // The drifters (checkMoveDrifters / checkUpdateDrifters, FE.cpp:8375-8437; Drifters::move / updateConc / maskXY, drifters.cpp:468-579) on the device-resident
    // arrays.  bbox: NULL on one rank, the min / max-reduced driftersMeshBbox of all ranks otherwise.
    void driftersSet(int set, int n, const double *x, const double *y, const int32_t *id) { check(nxs_dyn_drifters_set(h_, set, n, x, y, id), "drifters_set"); }
    void driftersClear(int set) { check(nxs_dyn_drifters_clear(h_, set), "drifters_clear"); }                               // drifters.cpp:456-459
    void driftersMeshBbox(bool displaced, double out[4]) { check(nxs_dyn_drifters_mesh_bbox(h_, displaced ? 1 : 0, out), "drifters_mesh_bbox"); }
    void checkMoveDrifters(const double *bbox = nullptr) { check(nxs_dyn_drifters_move(h_, bbox), "checkMoveDrifters"); }   // FE.cpp:8375-8397, M_UT = 0 included
    void driftersUpdateConc(int set, const double *bbox = nullptr, double *conc_host = nullptr) { check(nxs_dyn_drifters_conc(h_, set, bbox, conc_host), "drifters_conc"); }
    int driftersMaskXY(int set, double conc_lim, const int32_t *keepers = nullptr, int n_keepers = 0) {                    // drifters.cpp:548-579; returns how many are left
        int32_t left = 0;
        check(nxs_dyn_drifters_mask(h_, set, conc_lim, keepers, n_keepers, &left), "drifters_mask");
        return left;
    }
    int driftersGet(int set, double *x = nullptr, double *y = nullptr, int32_t *id = nullptr, double *conc = nullptr, int32_t *found = nullptr) {
        int32_t n = 0;
        check(nxs_dyn_drifters_get(h_, set, &n, x, y, id, conc, found), "drifters_get");
        return n;
    }
    // The Moorings means on a LOADED grid (moorings.grid_type=from_file): GridOutput::updateGridMean / setLSM / applyLSM / resetGridMean (gridoutput.cpp:387-415,
    // 470-485, 558-651) on the device-resident accumulators.  The grid, its mask and its accumulators survive setMesh and regrid.
    void meansPointsSet(const nxs_dyn_means_points *p) { check(nxs_dyn_means_points_set(h_, p), "means_points_set"); }       // NULL or G == 0: removed
    void meansPointsSetLSM(const int32_t *lsm_in = nullptr, int32_t *lsm_out = nullptr) { check(nxs_dyn_means_points_lsm(h_, lsm_in, lsm_out), "means_points_lsm"); }
    void meansPointsUpdateGridMean() { check(nxs_dyn_means_points_update(h_), "means_points_update"); }
    void meansPointsGet(bool apply_lsm, double *grid_elemental, double *grid_nodal, const double **elemental_dev = nullptr, const double **nodal_dev = nullptr) {
        check(nxs_dyn_means_points_get(h_, apply_lsm ? 1 : 0, grid_elemental, grid_nodal, elemental_dev, nodal_dev), "means_points_get");
    }
    void meansPointsResetGridMean() { check(nxs_dyn_means_points_reset(h_), "means_points_reset"); }
    // The Moorings means on the REGULAR grid (moorings.grid_type=regular): the same five on the M_is_regular_grid branch (gridoutput.cpp:486-538), InterpFromMeshToGridx
    // restated on the device.  The grid, its mask and its accumulators survive setMesh and regrid.
    void meansRegularSet(const nxs_dyn_means_regular *p) { check(nxs_dyn_means_regular_set(h_, p), "means_regular_set"); }   // NULL, ncols == 0 or nrows == 0: removed
    void meansRegularSetLSM(const int32_t *lsm_in = nullptr, int32_t *lsm_out = nullptr) { check(nxs_dyn_means_regular_lsm(h_, lsm_in, lsm_out), "means_regular_lsm"); }
    void meansRegularUpdateGridMean() { check(nxs_dyn_means_regular_update(h_), "means_regular_update"); }
    void meansRegularGet(bool apply_lsm, double *grid_elemental, double *grid_nodal, const double **elemental_dev = nullptr, const double **nodal_dev = nullptr) {
        check(nxs_dyn_means_regular_get(h_, apply_lsm ? 1 : 0, grid_elemental, grid_nodal, elemental_dev, nodal_dev), "means_regular_get");
    }
    void meansRegularResetGridMean() { check(nxs_dyn_means_regular_reset(h_), "means_regular_reset"); }
    // The coupler's outgoing fields, M_cpl_out: updateMeans(M_cpl_out, cpl_time_factor), M_cpl_out.updateGridMean, resetMeshMean, resetGridMean (FE.cpp:8012-8052,
    // 8226-8266) on a second accumulator set; the exchange grid's accumulators survive setMesh and regrid, the map is attached again after either.
    void cplOutConfigure(const nxs_dyn_means_config &c) { check(nxs_dyn_cpl_out_configure(h_, &c), "cpl_out_configure"); }
    void cplOutUpdateMeans(double cpl_time_factor) { check(nxs_dyn_cpl_out_update(h_, cpl_time_factor), "cpl_out_update"); }
    void cplOutGet(double *elemental, double *nodal, const double **elemental_dev = nullptr, const double **nodal_dev = nullptr) {
        check(nxs_dyn_cpl_out_get(h_, elemental, nodal, elemental_dev, nodal_dev), "cpl_out_get");
    }
    void cplOutResetMeshMean() { check(nxs_dyn_cpl_out_reset(h_), "cpl_out_reset"); }
    void cplOutAttachGrid(struct nxs_gridmap *map, const nxs_dyn_means_points *points = nullptr) { check(nxs_dyn_cpl_out_attach_grid(h_, map, points), "cpl_out_attach_grid"); }
    void cplOutUpdateGridMean(double *grid_elemental, double *grid_nodal, const double **elemental_dev = nullptr, const double **nodal_dev = nullptr, int32_t flags = 0) {
        check(nxs_dyn_cpl_out_put(h_, grid_elemental, grid_nodal, elemental_dev, nodal_dev, flags), "cpl_out_put");
    }
    void cplOutResetGridMean() { check(nxs_dyn_cpl_out_reset_grid(h_), "cpl_out_reset_grid"); }
    void fsdDiagConfigure(double dmax_c_threshold = 0.1, double fsd_unbroken_floe_size = 1000., double fsd_min_floe_size = 10.) {
        check(nxs_dyn_fsd_diag_configure(h_, dmax_c_threshold, fsd_unbroken_floe_size, fsd_min_floe_size), "fsd_diag_configure");
    }
    // interpFields() + assignVariables() on the device-resident state (FE.cpp:3071-3154, 553-572): the handle goes on with a.new_mesh; forcing is the next setForcing
    nxs_dyn_regrid_info regrid(const nxs_dyn_regrid_args &a) {
        nxs_dyn_regrid_info info{};
        check(nxs_dyn_regrid(h_, &a, &info), "regrid");
        return info;
    }
    // ... with the thermodynamic rows carried across (nxs_dyn_regrid_carry_thermo), and what the last regrid did with them
    void regridCarryThermo(bool carry, double drag_ice_t) {
        const nxs_dyn_regrid_thermo o{carry ? 1 : 0, 0, drag_ice_t};
        check(nxs_dyn_regrid_carry_thermo(h_, &o), "regridCarryThermo");
    }
    nxs_dyn_regrid_thermo_info regridThermoInfo() {
        nxs_dyn_regrid_thermo_info info{};
        check(nxs_dyn_regrid_thermo_info_get(h_, &info), "regridThermoInfo");
        return info;
    }
    // A coupled ocean (OceanType::COUPLED, #ifdef OASIS): the receive of ocean_cpl_elements / wave_cpl_elements onto the device rows thermo() reads, and the
    // COUPLED statements of thermo() (FE.cpp:5150-5157, 5348-5358, 5826-5841) for as long as it is attached.  cfg == nullptr detaches.
    void oceanCoupledAttach(struct nxs_gridmap *map, const nxs_dyn_ocean_coupled_config *cfg) { check(nxs_dyn_ocean_coupled_attach(h_, map, cfg), "ocean_coupled_attach"); }
    void oceanCoupledReceive(const double *const *fields, int32_t flags = 0) { check(nxs_dyn_ocean_coupled_receive(h_, fields, flags), "ocean_coupled_receive"); }
    void oceanCoupledPutRows(const nxs_dyn_ocean_coupled_rows &rows) { check(nxs_dyn_ocean_coupled_put_rows(h_, &rows), "ocean_coupled_put_rows"); }
    void oceanCoupledGet(const nxs_dyn_ocean_coupled_rows *out, const double **device_rows = nullptr) { check(nxs_dyn_ocean_coupled_get(h_, out, device_rows), "ocean_coupled_get"); }
    void nodesCoupledAttach(int32_t which, struct nxs_nodemap *map, const nxs_dyn_nodes_coupled_config *cfg) { check(nxs_dyn_nodes_coupled_attach(h_, which, map, cfg), "nodes_coupled_attach"); }
    void nodesCoupledReceive(int32_t which, const double *const *fields, int32_t n_fields, int32_t flags = 0) { check(nxs_dyn_nodes_coupled_receive(h_, which, fields, n_fields, flags), "nodes_coupled_receive"); }
    void nodesCoupledGet(int32_t which, double *const *out, const double **device_rows = nullptr) { check(nxs_dyn_nodes_coupled_get(h_, which, out, device_rows), "nodes_coupled_get"); }
    // Forcing given on a triangulated source (topaz4r_nodes, topaz4r_elements): one loadDataset through a node map (nxs_nodemap_load of include/nxs_interp.h); map == nullptr detaches
    void forcingAttachMesh(int32_t set, struct nxs_nodemap *map) { check(nxs_dyn_forcing_attach_mesh(h_, set, map), "forcing_attach_mesh"); }
    void forcingIngestMesh(int32_t set, const struct nxs_nodemap_load *l, const int32_t *row, int32_t flags = 0) { check(nxs_dyn_forcing_ingest_mesh(h_, set, l, row, flags), "forcing_ingest_mesh"); }
    void thermoForcingAttachMesh(int32_t set, struct nxs_nodemap *map) { check(nxs_dyn_thermo_forcing_attach_mesh(h_, set, map), "thermo_forcing_attach_mesh"); }
    void thermoForcingIngestMesh(int32_t set, const struct nxs_nodemap_load *l, const int32_t *row, int32_t flags = 0) { check(nxs_dyn_thermo_forcing_ingest_mesh(h_, set, l, row, flags), "thermo_forcing_ingest_mesh"); }
    nxs_dyn_handle *handle() { return h_; }

private:
    void check(int rc, const char *what) {
        if (rc != 0) throw std::runtime_error(std::string(what) + ": " + nxs_dyn_last_error(h_));
    }
    nxs_dyn_handle *h_ = nullptr;
};

}  // namespace nxs
#endif
