/*
 * nxs_dyn.h -- C ABI of libnxsdyn.so: the MI355X (gfx950) implementation of neXtSIM's
 * per-time-step sea-ice dynamics hot path.
 *
 * The reference (nansencenter/nextsim) has no plugin / FFI interface for this path: it is two
 * member functions of class FiniteElement that work on ~40 member vectors
 * (model/finiteelement.hpp:386-838).  This header *creates* the boundary: one entry point per
 * reference call site, taking exactly the arrays that call site reads and writes, as plain
 * pointers + sizes (no C++ types, no torch types).  "FE.cpp" = model/finiteelement.cpp.
 *
 *   reference call site                         replaced by
 *   ------------------------------------------  ------------------------------------------
 *   FiniteElement::initOptAndParam/init         nxs_dyn_create          (FE.cpp:1066-1209, 6993-6999)
 *   distributedMeshProcessing (per (re)mesh)    nxs_dyn_set_mesh        (FE.cpp:50-143, 150-271)
 *   initUpdateGhosts                            nxs_dyn_set_halo        (FE.cpp:14003-14088)
 *   ExternalData::getVector() snapshots         nxs_dyn_set_forcing     (model/externaldata.cpp:441-459)
 *   member vectors M_VT, M_conc, ...            nxs_dyn_put_state / nxs_dyn_get_state
 *   step(): UM_P=M_UM; explicitSolve(); update  nxs_dyn_step            (FE.cpp:8197-8214)
 *   explicitSolve()                             nxs_dyn_explicit_solve  (FE.cpp:10182-10643)
 *   update(UM_P)                                nxs_dyn_update          (FE.cpp:3919-4132)
 *   updateFreeDriftVelocity()                   (inside nxs_dyn_step)   (FE.cpp:10140-10176)
 *   checkRegridding()                           nxs_dyn_check_regridding(FE.cpp:8298-8309)
 *   checkFieldsFast()                           nxs_dyn_check_fields_fast (FE.cpp:14536-14655)
 *   M_surface, D_tau_a, D_tau_w, ...            nxs_dyn_get_diag
 *   #ifdef OASIS: M_tau_wi in explicitSolve()   nxs_dyn_set_wave_stress (FE.cpp:10353-10354, 10408-10414, 10509-10518)
 *   #ifdef OASIS: M_cum_damage, M_conc_fsd      nxs_dyn_put_coupled / nxs_dyn_get_coupled (FE.cpp:4233-4238, 3991-3994)
 *   updateMeans(M_moorings, time_factor)        nxs_dyn_means_update    (FE.cpp:8518-9024; configure / get / to_grid / reset beside it)
 *   M_moorings.updateGridMean() on a loaded grid nxs_dyn_means_points_update (gridoutput.cpp:387-415, 470-485; set / lsm / get / reset beside it)
 *   M_moorings.updateGridMean() on the regular grid nxs_dyn_means_regular_update (gridoutput.cpp:387-415, 486-538; set / lsm / get / reset beside it)
 *   interpFields() + assignVariables()          nxs_dyn_regrid          (FE.cpp:3071-3154, 2120-2151, 2196-2258, 3161-3297, 553-572)
 *   #ifdef OASIS: initFsd / updateFSD / redistributeFSD / weldingRoach   nxs_fsd_bins, nxs_dyn_fsd_* (FE.cpp:7408-7576, 4674-4732, 4268-4483, 4737-4870, 5888-5896)
 *   thermo(): OWBulkFluxes + IABulkFluxes       nxs_dyn_fluxes, nxs_dyn_flux_* (FE.cpp:5214-5277, 5032-5159, 6148-6353, 4966-5019, 6359-6389, 6454-6535)
 *   thermo(): thermoWinton / thermoIce0 columns nxs_dyn_column, nxs_dyn_column_* (FE.cpp:5306-5411, 6396-6448, 6633-6962)
 *   thermo(): the slab loop from new ice to tracers nxs_dyn_slab, nxs_dyn_slab_*, nxs_slab_* (FE.cpp:5413-6133, 6538-6627)
 *   thermo() under OceanType::COUPLED + the receive nxs_dyn_ocean_coupled_*, nxs_gridmap_receive_rows (FE.cpp:5150-5157, 5348-5358, 5826-5841; externaldata.cpp:163-236)
 *   ... and its nodal half: I_Uocn, I_Vocn, I_SSH, I_tauwix / y   nxs_dyn_nodes_coupled_*, nxs_nodemap_* (dataset.cpp:11157-11175; externaldata.cpp:498-509, 1246-1281, 1457-1463)
 *   loadDataset of a dataset on a triangulated source (topaz4r_*)   nxs_dyn_forcing_*_mesh, nxs_dyn_thermo_forcing_*_mesh, nxs_nodemap_load_rows (externaldata.cpp:886-931, 944-1288, 1334-1383, 1442-1448)
 *   BamgConvertMeshx connectivity tables        nxs_mesh_connectivity   (contrib/bamg/src/Mesh.cpp:495-865)
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (never throws across the ABI; the reference
 *     throws std::runtime_error and aborts, FE.cpp:14653).  nxs_dyn_last_error() gives the text.
 *   - all reals are fp64, all indices int32.  Nodal vectors are [u(0..Nn-1) | v(0..Nn-1)]
 *     (FE.cpp:10152-10153).  Element indices are 1-based local node ids (core/include/entities.hpp:151).
 *   - caller owns every host buffer; the library owns the device mirrors.
 *   - a handle is driven by one host thread and one HIP stream; handles are independent.
 *   - there is NO CPU fallback: without a HIP device nxs_dyn_create fails with NXS_ERR_NO_DEVICE.
 */
#ifndef NXS_DYN_H
#define NXS_DYN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NXS_DYN_ABI_VERSION 2

/* error codes */
#define NXS_OK 0
#define NXS_ERR_INVALID (-1)   /* bad argument / inconsistent sizes */
#define NXS_ERR_NO_DEVICE (-2) /* no HIP device: the product path never falls back to the CPU */
#define NXS_ERR_HIP (-3)       /* a HIP runtime call failed */
#define NXS_ERR_STATE (-4)     /* call order (e.g. step before set_mesh) */
#define NXS_ERR_COMM (-5)      /* RCCL failure */
#define NXS_ERR_NOMEM (-6)     /* host memory exhausted (a std::bad_alloc inside the library, caught at the boundary) */
#define NXS_ERR_INTERNAL (-7)  /* any other C++ exception inside the library, caught at the boundary; the text names it */

/* setup::DynamicsType, model/enums.hpp:142-149 */
enum { NXS_DYN_BBM = 0, NXS_DYN_NO_MOTION = 1, NXS_DYN_FREE_DRIFT = 2, NXS_DYN_EVP = 3, NXS_DYN_MEVP = 4 };
/* setup::BasalStressType, model/enums.hpp:82-86 */
enum { NXS_BASAL_NONE = 0, NXS_BASAL_LEMIEUX = 1 };
/* setup::IceCategoryType, model/enums.hpp:88-93 */
enum { NXS_ICECAT_CLASSIC = 0, NXS_ICECAT_YOUNG_ICE = 1 };

/* Everything explicitSolve()/update() read from vm[] or from members set in initOptAndParam/init.
 * Defaults: model/options.cpp:43,80,314-376.  compr_strength is the value AFTER the scale_coef
 * multiplication of FE.cpp:6996-6999 (cohesion arrives per element in nxs_dyn_state). */
typedef struct nxs_dyn_params {
    double dtime_step;                      /* simul.timestep [s] (FE.cpp: dtime_step) */
    int32_t substeps;                       /* dynamics.substeps (options.cpp:363) */
    int32_t dynamics_type;                  /* NXS_DYN_* */
    int32_t basal_stress_type;              /* NXS_BASAL_* */
    int32_t ice_cat_type;                   /* NXS_ICECAT_* (thermo.newice_type==4 -> YOUNG_ICE, FE.cpp:1206-1209) */
    int32_t newice_type;                    /* thermo.newice_type (FE.cpp:3943).  The reference ties 4 to YOUNG_ICE (FE.cpp:1212-1215); with the classic category
                                             * update() still bounds conc_myi by conc + conc_young as FE.cpp:4126-4128 is written: the array as put_state left it, so
                                             * with use_young_ice_in_myi_reset the caller of a classic build has to put meaningful values into conc_young */
    int32_t equal_ridging;                  /* age.equal_ridging (FE.cpp:3942) */
    int32_t use_young_ice_in_myi_reset;     /* age.include_young_ice (FE.cpp:3944) */
    int32_t reserved0;
    double young;                           /* dynamics.young */
    double nu0;                             /* dynamics.nu0 */
    double tan_phi;                         /* dynamics.tan_phi */
    double compr_strength;                  /* dynamics.compr_strength * scale_coef */
    double compaction_param;                /* dynamics.compaction_param */
    double undamaged_time_relaxation_sigma; /* dynamics.undamaged_time_relaxation_sigma */
    double exponent_relaxation_sigma;       /* dynamics.exponent_relaxation_sigma */
    double compression_factor;              /* dynamics.compression_factor */
    double exponent_compression_factor;     /* dynamics.exponent_compression_factor */
    double min_h;                           /* dynamics.min_h */
    double min_c;                           /* dynamics.min_c (used by update() only, FE.cpp:4063) */
    double quad_drag_coef_water;            /* dynamics.quad_drag_coef_water */
    double lin_drag_coef_water;             /* dynamics.lin_drag_coef_water (free drift only) */
    double quad_drag_coef_air;              /* <atm>_quad_drag_coef_air (free drift only; BBM uses state.drag_ui) */
    double lin_drag_coef_air;               /* dynamics.lin_drag_coef_air (free drift only) */
    double ocean_turning_angle_rad;         /* FE.cpp:1167-1172 */
    double basal_k1, basal_k2, basal_Cb, basal_u_0; /* dynamics.Lemieux_basal_* */
    double evp_e, evp_Pstar, evp_C, evp_dmin;       /* dynamics.evp.* */
    double mevp_alpha, mevp_beta;                   /* dynamics.mevp.* */
    double regrid_angle;                    /* numerics.regrid_angle [deg] */
} nxs_dyn_params;

/* The per-rank mesh as FiniteElement holds it after distributedMeshProcessing().
 * Ordering contract (core/src/gmshmesh.cpp:1165-1169, 1379-1417): nodes [0,local_ndof) are owned,
 * then ghosts; elements [0,local_nelements) are owned, then ghost elements.  Every owned node has
 * its complete element fan locally. */
typedef struct nxs_dyn_mesh {
    int32_t num_nodes;              /* M_num_nodes  (owned + ghost) */
    int32_t num_elements;           /* M_num_elements (owned + ghost) */
    int32_t local_ndof;             /* M_local_ndof (owned nodes) */
    int32_t local_nelements;        /* M_local_nelements (owned elements) */
    const int32_t *indices;         /* [3*Ne] M_elements[e].indices[k], 1-based local node ids */
    const uint8_t *ghost_nodes;     /* [3*Ne] M_elements[e].ghostNodes[k] (gmshmesh.cpp:1289-1301) */
    const double *coord_x;          /* [Nn] M_mesh.coordX()  (undisplaced) */
    const double *coord_y;          /* [Nn] M_mesh.coordY() */
    const double *lat;              /* [Nn] M_mesh.lat() in degrees (gmshmesh.cpp:1800-1824) */
    const uint8_t *mask_dirichlet;  /* [Nn] M_mask_dirichlet (false on ghosts, FE.cpp:228-234) */
    int32_t num_neumann_flags;      /* M_neumann_flags.size() */
    int32_t reserved0;
    const int32_t *neumann_flags;   /* sorted, 0-based local node ids incl. ghosts (FE.cpp:236-252) */
    /* bamgmesh tables exactly as BamgConvertMeshx leaves them (doubles, 1-based, NaN / 0 padded).
     * Either may be NULL: the library then builds an identical table with nxs_mesh_connectivity(). */
    const double *nodal_element_connectivity;  /* bamgmesh->NodalElementConnectivity [Nn*nec_width] */
    const double *nodal_connectivity;          /* bamgmesh->NodalConnectivity [Nn*nc_width], last col = count */
    int32_t nec_width;                         /* NodalElementConnectivitySize[1] */
    int32_t nc_width;                          /* NodalConnectivitySize[1] */
} nxs_dyn_mesh;

/* Halo lists of initUpdateGhosts() (FE.hpp:615-618), flattened CSR-style.
 * send_index = M_extract_local_index[q][], recv_index = M_local_ghosts_local_index[q][]; send_procs = M_recipients_proc_id,
 * recv_procs = M_local_ghosts_proc_id -- VERBATIM, as FE.cpp:14003-14088 leaves them.  On a ragged partition (Gmsh / METIS) a rank may send a node to a rank it
 * receives nothing from; the device-direct mailboxes need every link in both directions (below), so nxs_dyn_set_halo itself adds the missing direction as an
 * empty segment -- APPENDED behind the caller's neighbours, so that the caller's neighbour numbers k and its offsets (the layout of nxs_dyn_halo_fn's buffers)
 * stay what they were.  Both ranks of such a link do the same without talking to each other: one has the link in its send list, the other in its receive list. */
typedef struct nxs_dyn_halo {
    int32_t rank, nranks;
    int32_t num_send_procs;        /* M_recipients_proc_id.size() */
    int32_t num_recv_procs;        /* M_local_ghosts_proc_id.size() */
    const int32_t *send_procs;     /* [num_send_procs] */
    const int32_t *send_offsets;   /* [num_send_procs+1] into send_index */
    const int32_t *send_index;     /* 0-based local node ids */
    const int32_t *recv_procs;     /* [num_recv_procs] */
    const int32_t *recv_offsets;   /* [num_recv_procs+1] into recv_index */
    const int32_t *recv_index;     /* 0-based local (ghost) node ids */
} nxs_dyn_halo;

/* Prognostic state touched by the path (FE.hpp:712-746).  put: host -> device, get: device -> host.
 * A NULL member is skipped on get; on put every non-const member must be non-NULL. */
typedef struct nxs_dyn_state {
    double *VT, *UM, *UT;                 /* [2*Nn] M_VT, M_UM, M_UT */
    double *conc, *thick, *snow_thick;    /* [Ne] M_conc, M_thick, M_snow_thick */
    double *damage, *ridge_ratio;         /* [Ne] M_damage, M_ridge_ratio */
    double *sigma[3];                     /* [Ne] M_sigma[0..2] = s11, s22, s12 */
    double *conc_young, *h_young, *hs_young; /* [Ne] young-ice category */
    double *conc_myi, *thick_myi;         /* [Ne] multi-year ice */
    /* inputs only (written by thermo / calcCohesion in the reference) */
    const double *cohesion;               /* [Ne] M_Cohesion (FE.cpp:3909-3914) */
    const double *time_relaxation_damage; /* [Ne] M_time_relaxation_damage [s] */
    const double *drag_ui;                /* [Ne] M_drag_ui */
    const double *drag_ui_young;          /* [Ne] M_drag_ui_young */
} nxs_dyn_state;

/* Flat per-step forcing snapshot (ExternalData::getVector semantics). */
typedef struct nxs_dyn_forcing {
    const double *wind;          /* [2*Nn] M_wind */
    const double *ocean;         /* [2*Nn] M_ocean */
    const double *ssh;           /* [Nn]   M_ssh */
    const double *element_depth; /* [Ne]   M_element_depth */
} nxs_dyn_forcing;

/* The element variables of the coupled build (#ifdef OASIS: a wave- or ocean-coupled neXtSIM) that the loops of this path touch:
 *   M_cum_damage[cpt] += del_damage   inside the damage branch of every BBM sub-step (updateSigmaDamage, FE.cpp:4233-4238)
 *   M_conc_fsd[k][cpt] *= surf_ratio  for every floe-size bin, where update() scales the other element variables (FE.cpp:3991-3994)
 * updateFSD, the wave break-up (with the second M_cum_damage += of FE.cpp:4470) and the welding work on the same bins through nxs_dyn_fsd_* below; the statements of
 * thermo() that need thermo's own intermediates -- redistributeThermoFSD (lateral melt / growth, FE.cpp:4487-4670) and the melt-out branch (FE.cpp:5729-5764) -- stay
 * with the host. */
typedef struct nxs_dyn_coupled {
    double *cum_damage;      /* [Ne] M_cum_damage; NULL = not carried */
    double *conc_fsd;        /* [num_fsd_bins][Ne], bin-major like M_conc_fsd[k][cpt]; NULL = none */
    int32_t num_fsd_bins;    /* M_num_fsd_bins; 0 with conc_fsd == NULL */
    int32_t reserved0;
} nxs_dyn_coupled;

/* Side outputs other parts of the model consume (moorings, coupler, exporter). NULL = skip. */
typedef struct nxs_dyn_diag {
    double *surface;            /* [Ne] M_surface */
    double *delta_x;            /* [Ne] M_delta_x */
    double *D_tau_a;            /* [2*Nn] */
    double *D_tau_w;            /* [2*Nn] */
    double *D_del_ci_ridge_myi; /* [Ne] */
} nxs_dyn_diag;

/* updateIceDiagnostics() (FE.cpp:7860-7905), the element diagnostics checkOutputs() / exportResults() feed to the Moorings and the Exporter:
 * totals over the ice categories, the principal stresses, the divergence of the velocity on the displaced mesh.  NULL = skip.
 * (D_tsurf mixes thermodynamic variables -- M_tice, M_tsurf_young, M_sst -- that never cross this boundary: it stays with the host;
 * D_dmean / D_dmax are 0 without OASIS, FE.cpp:7903-7904.) */
typedef struct nxs_dyn_ice_diag {
    double *D_conc;         /* [Ne] M_conc (+ M_conc_young with the young-ice category) */
    double *D_thick;        /* [Ne] M_thick (+ M_h_young) */
    double *D_snow_thick;   /* [Ne] M_snow_thick (+ M_hs_young) */
    double *D_sigma0;       /* [Ne] (sigma11 + sigma22) / 2 */
    double *D_sigma1;       /* [Ne] hypot((sigma11 - sigma22) / 2, sigma12) */
    double *D_divergence;   /* [Ne] sum_j dxN_j u_j + dyN_j v_j with shapeCoeff on x0 + M_UM */
} nxs_dyn_ice_diag;
#define NXS_ICE_DIAG_FIELDS 6   /* order of the interleaved device rows: D_conc, D_thick, D_snow_thick, D_sigma0, D_sigma1, D_divergence */

/* Per-phase device time of nxs_dyn_step, averaged over the steps since the last "timing_reset"
 * option (HIP events on the handle's stream; steps stay asynchronous), named after the reference's
 * Timer rows (FE.cpp:8197-8221, 10217-10642). Milliseconds per step. */
typedef struct nxs_dyn_timing {
    double prep_ms;        /* "prep elements" + "prep nodes" */
    double substeps_ms;    /* "sub-time stepping" (all sub-steps, halo included) */
    double smoother_ms;    /* "OW smoother" (+ open-water mesh move) */
    double update_ms;      /* "update" */
    double total_ms;       /* "dynamics" */
    int32_t substep_launches; /* kernel launches inside substeps_ms */
    int32_t steps_averaged;   /* number of steps the averages cover */
    double ring_flush_ms;     /* (ABI 2) the part of substeps_ms spent in the step's last k_move_ring -- the deferred M_UM / M_UT += dt * M_VT of FE.cpp:10543-10550
                               * for all the sub-steps the velocity ring holds; 0 where the mesh move is inside the sub-step kernel */
} nxs_dyn_timing;

typedef struct nxs_dyn_handle nxs_dyn_handle;

#if defined(__GNUC__)
#define NXS_API __attribute__((visibility("default")))
#else
#define NXS_API
#endif

NXS_API int nxs_dyn_abi_version(void);
NXS_API const char *nxs_dyn_last_error(const nxs_dyn_handle *h); /* h may be NULL: last create() error */

NXS_API int nxs_dyn_default_params(nxs_dyn_params *p); /* model/options.cpp defaults, bbm */
/* The physical constants compiled into the kernels, in the order NXS_CONST_* names them: physical::rhoi, rhow, rhos, rhoa, gravity, omega
 * (model/constants.hpp:56-87), PI (contrib/bamg/include/OppositeAngle.h:4), days_in_sec (model/finiteelement.hpp:549).  Host only; lets a
 * caller (and tests/test_reference_constants.py, against values printed by a translation unit that includes the reference's headers) check
 * that library and model agree before the first step. */
enum { NXS_CONST_RHOI = 0, NXS_CONST_RHOW, NXS_CONST_RHOS, NXS_CONST_RHOA, NXS_CONST_GRAVITY, NXS_CONST_OMEGA, NXS_CONST_PI, NXS_CONST_DAYS_IN_SEC,
       NXS_CONST_SI /* physical::si */, NXS_CONST_LF /* physical::Lf */, NXS_CONST_C /* physical::C: model/constants.hpp:17-68, the enthalpy transformation of nxs_dyn_regrid */, NXS_CONST_COUNT };
NXS_API int nxs_dyn_physical_constants(double *out, int32_t count);
/* Self-test of one arithmetic short-cut of the sub-step kernels (no reference call site).  The six shape coefficients of a triangle (FE.cpp:1951-1964) are six
 * quotients by ONE divisor, the Jacobian; where every operand of a step lies in a range the prep kernels check once per step (|coordinate| zero or in
 * [1e-100, 1e100], |Jacobian| in [1e-100, 1e100]) the kernels refine the divisor's reciprocal once and finish every quotient with the three operations the
 * compiler's own division sequence ends in -- the same instructions on the same operands, hence the same bits as six divisions; outside that range they divide.
 * This entry point computes n pseudo-random sextuples both ways on `device` and returns in *mismatches the number of quotients whose bits differ (0 expected):
 * mode 0 = triangles of the size and position meshes have, mode 1 = operands spread over the whole admitted range, zeros among the numerators.
 * mode 2 tests the second short-cut: the strain-rate and stress-increment sums of updateSigmaDamage (FE.cpp:4167-4176, 4204-4210) are formed without the terms
 * that are products with a LITERAL zero of M_B0T / M_Dunit (adding +-0 to a sum that cannot be -0 returns it unchanged); n random operand sets, zeros of both signs
 * among the velocities and stresses, computed with and without those terms: *mismatches = values whose bits differ (0 expected). */
NXS_API int nxs_dyn_selftest_quotients(int32_t device, int64_t n, uint64_t seed, int32_t mode, int64_t *mismatches);
NXS_API int nxs_dyn_create(const nxs_dyn_params *p, int device, nxs_dyn_handle **out);
NXS_API int nxs_dyn_destroy(nxs_dyn_handle *h);
NXS_API int nxs_dyn_set_params(nxs_dyn_handle *h, const nxs_dyn_params *p);

NXS_API int nxs_dyn_set_mesh(nxs_dyn_handle *h, const nxs_dyn_mesh *m);
NXS_API int nxs_dyn_set_halo(nxs_dyn_handle *h, const nxs_dyn_halo *halo);
/* RCCL communicator for the halo exchange: every rank passes the same 128-byte ncclUniqueId
 * (nxs_dyn_comm_unique_id on rank 0, broadcast by the host launcher). */
NXS_API int nxs_dyn_comm_unique_id(void *id128);
NXS_API int nxs_dyn_comm_init(nxs_dyn_handle *h, const void *id128, int rank, int nranks);
/* One exchange of coded payloads through that communicator (collective): a grouped ncclSend/ncclRecv of the rank to itself and,
 * when halo lists are set, updateGhosts' grouped send/recv with checked contents.  *errors = wrong values received. */
NXS_API int nxs_dyn_comm_selftest(nxs_dyn_handle *h, int32_t *errors);

/* Device-direct transport: updateGhosts through peer-mapped mailboxes (stores over xGMI, flags, no RCCL
 * launch, replayable from a hipGraph).  Collective setup driven by the host launcher:
 *   1. every rank: nxs_dyn_ipc_export(h, blob)                 -> NXS_IPC_BLOB_BYTES bytes to publish
 *   2. the launcher all-gathers the blobs and each rank's receive lists
 *   3. every rank: nxs_dyn_ipc_connect(h, blobs_of_my_send_neighbours, ...)
 *   4. every rank: nxs_dyn_ipc_selftest(h, rounds, &errors)    -> use it only if errors == 0 everywhere
 * Takes precedence over RCCL once connected; the host-staged callback below overrides both. */
/* The mailbox must be uncached device memory (the in-kernel exchange takes no acquire after its flag wait): ipc_export fails when
 * the runtime refuses it, and the caller stays on RCCL or its own communicator.  Neighbour handles may live in other processes
 * (hipIpc) or in this one (a host that drives several GPUs from one process); ipc_connect checks the tables it is given against
 * what each neighbour published, and a second connect replaces the first.  The self-test pushes checked payloads through every
 * link with both publishing protocols the step can use (one release per block / one per launch).
 * NEIGHBOURS IN BOTH DIRECTIONS: a mailbox has two buffers per link, which is safe because "a neighbour cannot start exchange x + 2 before it has received my
 * exchange x + 1, which I send only after my pull of exchange x" -- a hand-shake that needs every rank I send to to send to me as well.  A ragged partition can
 * send a node to a rank it receives nothing from: nxs_dyn_set_halo adds that direction itself as an empty segment (its flag is still raised and waited for: that
 * is the hand-shake), on both ranks, without communication.  The LOW-LEVEL nxs_dyn_ipc_connect below takes tables for the caller's own send neighbours only, so on
 * such a partition it returns NXS_ERR_INVALID and names the rank (round 4: found as one wrong payload in the self-test of a 4-rank mosaic): use the record form,
 * which finds the added direction in the neighbours' records.  RCCL and the host-staged transport do not need the pairing; they skip segments without nodes. */
#define NXS_IPC_BLOB_BYTES 128
NXS_API int nxs_dyn_ipc_export(nxs_dyn_handle *h, void *blob);
NXS_API int nxs_dyn_ipc_connect(nxs_dyn_handle *h, const void *blobs, const int32_t *peer_recv_offset,
                                const int32_t *peer_recv_total, const int32_t *peer_flag_slot);
NXS_API int nxs_dyn_ipc_selftest(nxs_dyn_handle *h, int rounds, int32_t *errors);
/* The same set-up WITHOUT bookkeeping on the caller's side (round 5) -- what INTEGRATION.md section 3 shows, and the only form that works on a partition with
 * one-directional neighbours (the direction nxs_dyn_set_halo added is not in any list the caller holds):
 *   1. every rank: nxs_dyn_ipc_record_bytes(h, &n)         the size of its record: the blob of nxs_dyn_ipc_export + its receive lists as the library holds them
 *   2. the launcher: stride = MPI_Allreduce(MAX) of n
 *   3. every rank: nxs_dyn_ipc_export_record(h, rec, stride)   (exports the mailbox, like nxs_dyn_ipc_export; the tail of rec is zeroed)
 *   4. the launcher: MPI_Allgather of the records, `stride` bytes each, in rank order
 *   5. every rank: nxs_dyn_ipc_connect_records(h, records, stride, nranks)   finds its segment, the totals and its flag slot in every neighbour's record itself
 *   6. every rank: nxs_dyn_ipc_selftest
 * connect_records returns NXS_ERR_INVALID when the records disagree with this rank's lists (a neighbour that does not list this rank, a segment of another length). */
NXS_API int nxs_dyn_ipc_record_bytes(nxs_dyn_handle *h, int32_t *bytes);
NXS_API int nxs_dyn_ipc_export_record(nxs_dyn_handle *h, void *record, int32_t capacity);
NXS_API int nxs_dyn_ipc_connect_records(nxs_dyn_handle *h, const void *records, int64_t stride, int32_t nranks);
/* Profiling aid (no reference call site): the mailboxes of this handle connected to THEMSELVES, so that a rank's partition can be stepped alone on a device with the
 * exchange inside its kernels -- every flag a kernel waits for is raised by the rank's own launches (rocprofv3's counter collection serialises the kernels of a
 * device: two ranks whose kernels wait for each other cannot be profiled together, a looped-back rank can; bench.py's roofline.traffic at N > 1 and its
 * aux_partition_floor).  The ghosts receive meaningless velocities -- results are NOT the model's --, the launches walk the same tables and move the same bytes.
 * NXS_ERR_INVALID when the lists do not allow it (no neighbour). */
NXS_API int nxs_dyn_ipc_loopback(nxs_dyn_handle *h);

/* Test door "ipc_delay" (option of nxs_dyn_set_option; compiled in, off by default, no reference call site): ONE named rank sleeps at ONE named point of the exchange
 * protocols -- value = rank << 16 | point << 8 | units, a unit = 10 us, units 1..255; 0 = off.  The blocking send / recv of the reference (FE.cpp:13981-13985) cannot
 * reorder; the flag protocols of the device-direct transport can, in windows a few microseconds wide that a bitwise test only sees when the race is lost.  A delay at
 * the right point makes the race lose every time: tests/test_gpu_protocol_delays.py walks (variant x point x delayed rank) on ragged 3- and 4-rank partitions and
 * requires the bits of the undelayed separate kernels -- and, with the test door "halo_one_directional" (= 1 BEFORE nxs_dyn_set_halo: the lists are taken as given, no
 * direction is added, nxs_dyn_ipc_connect does not refuse), shows round 4's defect fail deterministically. */
enum { NXS_DELAY_NONE = 0,
       NXS_DELAY_PULL_READ = 1,          /* k_halo_pull: flags seen, before the mailbox half is read */
       NXS_DELAY_PUSH_STORE = 2,         /* k_halo_push: before the stores into the neighbours' mailboxes */
       NXS_DELAY_PUSH_FLAG = 3,          /* k_halo_push: stores drained, before the flags are raised */
       NXS_DELAY_STAGE_READ = 4,         /* k_substep_fused / k_substep_pair<HALO> / k_substep_resident*: flags seen, before the ghosts are staged from the mailbox half */
       NXS_DELAY_SEND_STORE = 5,         /* the same kernels: before the (first) store of the sent nodes */
       NXS_DELAY_PAIR_SECOND_STORE = 6,  /* k_substep_pair<HALO>: before the second sub-step's store */
       NXS_DELAY_PUBLISH_FLAG = 7,       /* the same kernels: stores drained, before the (first) flag is raised */
       NXS_DELAY_PAIR_MID_READ = 8,      /* k_substep_pair<HALO>: flags x + 1 seen, before the ghosts of N_1 are read */
       NXS_DELAY_SMOOTH_READ = 9,        /* k_smooth_halo: flags seen, before the ghosts' slot is read */
       NXS_DELAY_SMOOTH_STORE = 10,      /* k_smooth_halo: before a sweep's stores */
       NXS_DELAY_SMOOTH_FLAG = 11,       /* k_smooth_halo: before a sweep's publication */
       NXS_DELAY_SMOOTH_PULL_READ = 12,  /* k_smooth_pull: flags seen, before the last slot is read */
       NXS_DELAY_PAIR_SECOND_FLAG = 13,  /* k_substep_pair<HALO>: before the second publication */
       NXS_DELAY_POINTS = 14 };

/* Alternative transport: host-staged exchange through the CALLER's communicator -- the literal
 * M_comm.send / M_comm.recv of FE.cpp:13981-13985.  send holds, per send neighbour k, 2*n_k doubles
 * [u-block | v-block] at offset 2*send_offsets[k]; recv is laid out the same way from recv_offsets.
 * fn must fill recv and return 0.  Takes precedence over RCCL when set; NULL unsets it. */
typedef int (*nxs_dyn_halo_fn)(void *ctx, const double *send, double *recv);
NXS_API int nxs_dyn_set_halo_exchange_fn(nxs_dyn_handle *h, nxs_dyn_halo_fn fn, void *ctx);

/* Host <-> device copies of the prognostic arrays.  The first put after nxs_dyn_set_mesh must bring every member; afterwards a
 * NULL member means "the device copy is current" (put) / "not wanted" (get), so a host whose thermodynamics only touched
 * concentration, thickness and snow moves only those across PCIe instead of the whole state every step. */
NXS_API int nxs_dyn_put_state(nxs_dyn_handle *h, const nxs_dyn_state *s);
NXS_API int nxs_dyn_get_state(nxs_dyn_handle *h, nxs_dyn_state *s);
NXS_API int nxs_dyn_set_forcing(nxs_dyn_handle *h, const nxs_dyn_forcing *f);
/* Forcing that is interpolated linearly in time (ExternalData::get, model/externaldata.cpp:360-401) without a host->device
 * copy per step: the two snapshots of a forcing interval (dataset->variables[].interpolated_data[0] and [1] of M_wind,
 * M_ocean, M_ssh; element_depth of f0, a constant dataset) become resident once per interval, and every step only passes
 *   fcoeff[0] = |t - ftime_range[1]| / fdt,  fcoeff[1] = |t - ftime_range[0]| / fdt,
 * M_factor (spin-up ramp, Q10) and M_bias_correction of {wind, ocean, ssh} (NULL = 1 and 0); the device evaluates
 *   M_factor*(fcoeff[0]*d0[i] + fcoeff[1]*d1[i]) + M_bias_correction      -- the reference's expression, same bits. */
NXS_API int nxs_dyn_set_forcing_pair(nxs_dyn_handle *h, const nxs_dyn_forcing *f0, const nxs_dyn_forcing *f1);
NXS_API int nxs_dyn_set_forcing_time(nxs_dyn_handle *h, double fcoeff0, double fcoeff1, const double factor[3], const double bias[3]);
/* The coupled build's terms.  NOTHING ATTACHED (the state after nxs_dyn_set_mesh) = the library without them, bit for bit and byte for byte: the kernels that
 * carry a term are builds of their own, picked per launch while it is attached.
 *   nxs_dyn_set_wave_stress   M_tau_wi.getVector(), [u | v] like every nodal vector: the wave radiation stress of the momentum equation,
 *                  tau_x = D_tau_a[u] + tau_wi[u] + c_prime * (...) (FE.cpp:10509-10518; the sum associates left, and so does the library's).  Copied to the device and
 *                  ATTACHED until tau_wi == NULL detaches it; NULL is the expression of the build without OASIS, a vector of zeros the coupled build that received
 *                  no wave stress.  D_tau_a of nxs_dyn_get_diag stays drag * wind.  Values on a rank's ghost nodes are never used (only owned nodes are solved,
 *                  FE.cpp:10472).  nxs_dyn_check_fields_fast raises crash_local when tau_wi[i] + tau_wi[i + Nn] is NaN for a node (FE.cpp:14631-14643).
 *   nxs_dyn_put_coupled       host -> device, and ATTACHES: a non-NULL member is copied and carried by the following steps, a NULL member is detached (both NULL:
 *                  the library without them).  A num_fsd_bins larger than any put before takes a new buffer of that size; the smaller one is kept until
 *                  nxs_dyn_set_mesh / nxs_dyn_destroy (no device memory is freed between two steps), so a caller that grows the number step by step holds them all.
 *   nxs_dyn_get_coupled       device -> host; a NULL member is not wanted; num_fsd_bins must be the attached number when conc_fsd is wanted.
 * nxs_dyn_set_mesh detaches all three (the sizes change: the caller interpolates the element variables through nxs_interp like every other and puts them again).
 * Errors: NXS_ERR_STATE before nxs_dyn_set_mesh; NXS_ERR_INVALID for num_fsd_bins < 0, bins without an array, an array without bins, and a get of a member that
 * is not attached.
 * EVP / mEVP: cum_damage is carried unchanged (there is no damage update).  Free drift / no motion: nothing is touched (step() skips update(), FE.cpp:8197-8214).
 * With cum_damage attached the sub-step loop runs on a kernel family that accumulates it (option "fused" below).  nxs_dyn_step_host keeps its signature: a coupled
 * host calls put_coupled / get_coupled beside it. */
NXS_API int nxs_dyn_set_wave_stress(nxs_dyn_handle *h, const double *tau_wi /* [2*Nn] M_tau_wi, NULL = off */);
NXS_API int nxs_dyn_put_coupled(nxs_dyn_handle *h, const nxs_dyn_coupled *c);
NXS_API int nxs_dyn_get_coupled(nxs_dyn_handle *h, nxs_dyn_coupled *c);
NXS_API int nxs_dyn_get_diag(nxs_dyn_handle *h, nxs_dyn_diag *d);
/* updateIceDiagnostics() on the device-resident state.  d (may be NULL): host arrays to fill.  device_rows (may be NULL): receives a DEVICE
 * pointer to the same diagnostics as [Ne][NXS_ICE_DIAG_FIELDS] interleaved rows (library-owned, valid until the next call on this handle
 * or nxs_dyn_set_mesh) -- the layout nxs_interp_mesh_to_grid_device samples, so a Moorings record needs no round trip of the state. */
NXS_API int nxs_dyn_ice_diagnostics(nxs_dyn_handle *h, nxs_dyn_ice_diag *d, const double **device_rows);

/* ---- Moorings time means on the device: updateMeans() (FE.cpp:8518-9024), GridOutput::updateGridMean() on the regular grid (model/gridoutput.cpp:387-550),
 * resetMeshMean().  checkOutputs() calls updateIceDiagnostics() and updateMoorings() after EVERY step (FE.cpp:8316-8327, 9403-9408); with moorings.snapshot=false
 * that is updateMeans(M_moorings, mooring_time_factor): data_mesh[i] += field[i] * time_factor into one mesh accumulator per output variable.  The accumulators
 * live here as interleaved rows ([Ne][n_el] and [Nn][n_nod], the layout nxs_interp_mesh_to_grid_device samples), one launch per kind and step updates them, and
 * nxs_dyn_means_to_grid samples them at output time -- the state never crosses PCIe for a time-mean Moorings file.
 * The identifiers are named after GridOutput::variableID (model/gridoutput.hpp) and cover the variables whose sources the handle holds.
 * The thermodynamic variables (NXS_MEANS_THERMO_BEGIN ..) read the rows nxs_dyn_fluxes / nxs_dyn_column / nxs_dyn_slab left on the handle: the flux, column and slab
 * state, the slab's D_* rows, the atmosphere and the column's forcing -- a host whose thermodynamics runs here fetches none of them for a time-mean Moorings file.
 * On a LOADED grid with interpMethod::conservative (a coupler's grid; the Moorings with moorings.use_conservative_remapping) the elemental rows go through
 * nxs_dyn_means_to_grid_conservative and a resident nxs_gridmap (include/nxs_interp.h) instead.
 * On a LOADED grid without conservative remapping (moorings.grid_type=from_file) both legs, the proc mask, rotateVectors, the grid accumulators and the
 * land-sea mask are nxs_dyn_means_points_* below.
 * dmax / dmean (NXS_MEANS_FSD_BEGIN ..), the floe-size diagnostics of the coupled build, need nxs_dyn_fsd_diag_configure below.  The coupler's means (M_cpl_out)
 * are a second set of accumulators beside these: nxs_dyn_cpl_out_* below.
 * On the REGULAR grid (moorings.grid_type=regular, the default) nxs_dyn_means_to_grid samples through the host at every call; nxs_dyn_means_regular_* below keep
 * the grid, rotateVectors, the land-sea mask and the grid accumulators on the device. */
enum nxs_means_var {
    /* elemental: accumulated over the owned elements i < M_local_nelements, the rows of ghost elements stay 0 (FE.cpp:8527) */
    NXS_MEANS_CONC = 0,           /* FE.cpp:8526  D_conc */
    NXS_MEANS_THICK = 1,          /* FE.cpp:8531  D_thick */
    NXS_MEANS_SNOW = 2,           /* FE.cpp:8546  D_snow_thick */
    NXS_MEANS_CONC_CONS = 3,      /* FE.cpp:8586  M_conc */
    NXS_MEANS_DAMAGE = 4,         /* FE.cpp:8536  M_damage */
    NXS_MEANS_RIDGE_RATIO = 5,    /* FE.cpp:8541  M_ridge_ratio */
    NXS_MEANS_CONC_YOUNG = 6,     /* FE.cpp:8581  M_conc_young */
    NXS_MEANS_H_YOUNG = 7,        /* FE.cpp:8591  M_h_young */
    NXS_MEANS_HS_YOUNG = 8,       /* FE.cpp:8596  M_hs_young */
    NXS_MEANS_CONC_MYI = 9,       /* FE.cpp:8632  M_conc_myi */
    NXS_MEANS_THICK_MYI = 10,     /* FE.cpp:8636  M_thick_myi */
    NXS_MEANS_DCI_RIDGE_MYI = 11, /* FE.cpp:8660  D_del_ci_ridge_myi */
    NXS_MEANS_SIGMA_11 = 12,      /* FE.cpp:8682  M_sigma[0] */
    NXS_MEANS_SIGMA_22 = 13,      /* FE.cpp:8686  M_sigma[1] */
    NXS_MEANS_SIGMA_12 = 14,      /* FE.cpp:8691  M_sigma[2] */
    NXS_MEANS_SIGMA_N = 15,       /* FE.cpp:8741  D_sigma[0] */
    NXS_MEANS_SIGMA_S = 16,       /* FE.cpp:8746  D_sigma[1] */
    NXS_MEANS_DIVERGENCE = 17,    /* FE.cpp:8751  D_divergence */
    NXS_MEANS_DRAG_UI = 18,       /* FE.cpp:8756-8766  M_drag_ui, concentration-weighted with M_drag_ui_young in the young-ice category */
    NXS_MEANS_ICE_MASK = 19,      /* FE.cpp:8912-8920  += 1 where M_thick (+ M_h_young) > 0 -- NOT multiplied by time_factor */
    NXS_MEANS_ELEMENTAL_END = 20,
    /* elemental, the thermodynamics: the same loop over the owned elements; each reads a row the handle holds (see nxs_dyn_means_update) */
    NXS_MEANS_SST = 128,                 /* FE.cpp:8556  M_sst (nxs_dyn_flux_state) */
    NXS_MEANS_SSS = 129,                 /* FE.cpp:8561  M_sss */
    NXS_MEANS_TSURF_ICE = 130,           /* FE.cpp:8566  M_tice[0] */
    NXS_MEANS_MELTPOND_LID_VOLUME = 131, /* FE.cpp:8626  M_lid_volume */
    NXS_MEANS_MELTPOND_FRACTION = 132,   /* FE.cpp:8779  D_pond_fraction */
    NXS_MEANS_DRAG_TI = 133,             /* FE.cpp:8767-8777  M_drag_ti, concentration-weighted with M_drag_ti_young in the young-ice category */
    NXS_MEANS_T1 = 134,                  /* FE.cpp:8571  M_tice[1] (nxs_dyn_column_state; WINTON) */
    NXS_MEANS_T2 = 135,                  /* FE.cpp:8576  M_tice[2] */
    NXS_MEANS_CONC_UPD = 136,            /* FE.cpp:8616  M_conc_upd (nxs_dyn_slab_state) */
    NXS_MEANS_MELTPOND_VOLUME = 137,     /* FE.cpp:8621  M_pond_volume */
    NXS_MEANS_DEL_VI_TEND = 138,         /* FE.cpp:8656  M_del_vi_tend */
    NXS_MEANS_FREEZE_DAYS = 139,         /* FE.cpp:8640  M_freeze_days */
    NXS_MEANS_FREEZE_ONSET = 140,        /* FE.cpp:8652  M_freeze_onset */
    NXS_MEANS_CONC_SUMMER = 141,         /* FE.cpp:8644  M_conc_summer */
    NXS_MEANS_THICK_SUMMER = 142,        /* FE.cpp:8648  M_thick_summer */
    NXS_MEANS_FYI_FRACTION = 143,        /* FE.cpp:8601  M_fyi_fraction */
    NXS_MEANS_AGE_DET = 144,             /* FE.cpp:8606  M_age_det * time_factor / years_in_sec */
    NXS_MEANS_AGE = 145,                 /* FE.cpp:8611  M_age * time_factor / years_in_sec */
    NXS_MEANS_QA = 146,                  /* FE.cpp:8697  D_Qa (NXS_SLAB_QA; the rows of nxs_dyn_slab from here on) */
    NXS_MEANS_QSW = 147,                 /* FE.cpp:8701  D_Qsw */
    NXS_MEANS_QLW = 148,                 /* FE.cpp:8705  D_Qlw */
    NXS_MEANS_QSH = 149,                 /* FE.cpp:8709  D_Qsh */
    NXS_MEANS_QLH = 150,                 /* FE.cpp:8713  D_Qlh */
    NXS_MEANS_QO = 151,                  /* FE.cpp:8717  D_Qo */
    NXS_MEANS_DELS = 152,                /* FE.cpp:8721  D_delS */
    NXS_MEANS_EVAP = 153,                /* FE.cpp:8725  D_evap */
    NXS_MEANS_RAIN = 154,                /* FE.cpp:8729  D_rain */
    NXS_MEANS_SIALB = 155,               /* FE.cpp:8733  D_sialb */
    NXS_MEANS_ALBEDO = 156,              /* FE.cpp:8737  D_albedo */
    NXS_MEANS_DEL_VI_YOUNG = 157,        /* FE.cpp:8833  D_del_vi_young */
    NXS_MEANS_VICE_MELT = 158,           /* FE.cpp:8837  D_vice_melt */
    NXS_MEANS_DEL_HI = 159,              /* FE.cpp:8841  D_del_hi */
    NXS_MEANS_DEL_HI_YOUNG = 160,        /* FE.cpp:8845  D_del_hi_young */
    NXS_MEANS_NEWICE = 161,              /* FE.cpp:8849  D_newice */
    NXS_MEANS_SNOW2ICE = 162,            /* FE.cpp:8853  D_snow2ice */
    NXS_MEANS_MLT_TOP = 163,             /* FE.cpp:8857  D_mlt_top */
    NXS_MEANS_MLT_BOT = 164,             /* FE.cpp:8861  D_mlt_bot */
    NXS_MEANS_DVI_RPLNT_MYI = 165,       /* FE.cpp:8664  D_del_vi_rplnt_myi */
    NXS_MEANS_DCI_RPLNT_MYI = 166,       /* FE.cpp:8668  D_del_ci_rplnt_myi */
    NXS_MEANS_DVI_MLT_MYI = 167,         /* FE.cpp:8672  D_del_vi_mlt_myi */
    NXS_MEANS_DCI_MLT_MYI = 168,         /* FE.cpp:8676  D_del_ci_mlt_myi */
    NXS_MEANS_FWFLUX_ICE = 169,          /* FE.cpp:8829  -= D_fwflux_ice * time_factor: the reversed sign, here and in the next four */
    NXS_MEANS_FWFLUX = 170,              /* FE.cpp:8894  -= D_fwflux */
    NXS_MEANS_QNOSW = 171,               /* FE.cpp:8898  -= D_Qnosun */
    NXS_MEANS_QSWOCEAN = 172,            /* FE.cpp:8902  -= D_Qsw_ocean */
    NXS_MEANS_SALTFLUX = 173,            /* FE.cpp:8906  -= D_brine */
    NXS_MEANS_TAIR = 174,                /* FE.cpp:8785  M_tair (nxs_dyn_flux_atmosphere) */
    NXS_MEANS_MSLP = 175,                /* FE.cpp:8789  M_mslp */
    NXS_MEANS_QSW_IN = 176,              /* FE.cpp:8805  M_Qsw_in */
    NXS_MEANS_SPHUMA = 177,              /* FE.cpp:8793  M_sphuma: the humidity row under NXS_FLUX_HUM_SPHUMA */
    NXS_MEANS_MIXRAT = 178,              /* FE.cpp:8797  M_mixrat: ... under NXS_FLUX_HUM_MIXRAT */
    NXS_MEANS_D2M = 179,                 /* FE.cpp:8801  M_dair: ... under NXS_FLUX_HUM_DEWPOINT */
    NXS_MEANS_QLW_IN = 180,              /* FE.cpp:8809  M_Qlw_in: the long-wave row under NXS_FLUX_LW_QLW_IN */
    NXS_MEANS_TCC = 181,                 /* FE.cpp:8813  M_tcc: ... under NXS_FLUX_LW_TCC */
    NXS_MEANS_PRECIP = 182,              /* FE.cpp:8825  M_precip (nxs_dyn_column_forcing) */
    NXS_MEANS_SNOWFALL = 183,            /* FE.cpp:8817  M_snowfall: the snow row under NXS_COL_SNOWFALL_SNOWFALL */
    NXS_MEANS_SNOWFR = 184,              /* FE.cpp:8821  M_snowfr: ... under NXS_COL_SNOWFALL_PRECIP_SNOWFR */
    NXS_MEANS_OCEAN_TEMP = 185,          /* FE.cpp:8873  M_ocean_temp */
    NXS_MEANS_OCEAN_SALT = 186,          /* FE.cpp:8877  M_ocean_salt */
    NXS_MEANS_MLD = 187,                 /* FE.cpp:8869  M_mld */
    NXS_MEANS_TSURF = 188,               /* FE.cpp:8551  D_tsurf of updateIceDiagnostics (FE.cpp:7875-7883) */
    NXS_MEANS_WSPEED = 189,              /* FE.cpp:8865  windSpeedElement(i) (FE.cpp:6359-6370) of the wind the step reads */
    NXS_MEANS_THERMO_END = 190,
    /* elemental, the floe-size diagnostics of the coupled build (updateIceDiagnostics, FE.cpp:7902-7951): nxs_dyn_fsd_diag_configure */
    NXS_MEANS_DMAX = 192,                /* FE.cpp:8883  D_dmax */
    NXS_MEANS_DMEAN = 193,               /* FE.cpp:8887  D_dmean */
    NXS_MEANS_FSD_END = 194,
    /* nodal: accumulated over all M_num_nodes, ghosts included */
    NXS_MEANS_VT_X = 64,          /* FE.cpp:8931  M_VT[i] */
    NXS_MEANS_VT_Y = 65,          /* FE.cpp:8936  M_VT[i + M_num_nodes] */
    NXS_MEANS_WIND_X = 66,        /* FE.cpp:8941  M_wind[i] */
    NXS_MEANS_WIND_Y = 67,        /* FE.cpp:8946 */
    NXS_MEANS_TAU_AX = 68,        /* FE.cpp:8951  D_tau_a[i] */
    NXS_MEANS_TAU_AY = 69,        /* FE.cpp:8956 */
    NXS_MEANS_TAUWIX = 70,        /* FE.cpp:8962  M_tau_wi[i]: needs a wave stress attached (nxs_dyn_set_wave_stress) */
    NXS_MEANS_TAUWIY = 71,        /* FE.cpp:8966 */
    NXS_MEANS_TAUX = 72,          /* FE.cpp:8974-9020  D_tau_w and the area-weighted means of D_tau_ow and M_conc over NodalElementConnectivity: */
    NXS_MEANS_TAUY = 73,          /*                   needs nxs_dyn_means_set_tau_ow */
    NXS_MEANS_TAUMOD = 74,
    NXS_MEANS_NODAL_END = 75
};
#define NXS_MEANS_NODAL_BEGIN 64
#define NXS_MEANS_THERMO_BEGIN 128
#define NXS_MEANS_FSD_BEGIN 192
#define NXS_MEANS_MAX_VARS 24   /* entries per list (the list travels to the kernel by value; a workgroup stages 256 rows of it in LDS) */

typedef struct nxs_dyn_means_config {
    int32_t num_elemental;          /* M_elemental_variables.size(), <= NXS_MEANS_MAX_VARS; 0 in both lists = the feature off, buffers freed */
    int32_t num_nodal;              /* M_nodal_variables.size() */
    const int32_t *elemental_ids;   /* [num_elemental] NXS_MEANS_* : the column order of the elemental rows */
    const uint8_t *elemental_mask;  /* [num_elemental] Variable::mask (NULL = none): zeroed on the grid where ice_mask <= 0 (gridoutput.cpp:404-414) */
    const int32_t *nodal_ids;       /* [num_nodal] */
    const uint8_t *nodal_mask;      /* [num_nodal] */
} nxs_dyn_means_config;

/* the regular grid of GridOutput (gridoutput.cpp:496-504): M_xmin, M_ymax, M_mooring_spacing, M_ncols (along x), M_nrows (along y), M_miss_val */
typedef struct nxs_dyn_means_grid {
    double xmin, ymax, mooring_spacing;
    double miss_val;
    int32_t ncols, nrows;
} nxs_dyn_means_grid;

/*   nxs_dyn_means_configure  the two lists (copied).  The configuration survives nxs_dyn_set_mesh: the accumulators are re-sized and zeroed there, which is
 *                  resetMeshMean(bamgmesh, regrid = true, ...).  The elemental list takes the ids below NXS_MEANS_ELEMENTAL_END and those of NXS_MEANS_THERMO_BEGIN
 *                  .. NXS_MEANS_THERMO_END - 1 and of NXS_MEANS_FSD_BEGIN .. NXS_MEANS_FSD_END - 1, in any mixture.  NXS_ERR_INVALID: an unknown id, an elemental id in the nodal list or the reverse, more than
 *                  NXS_MEANS_MAX_VARS entries, a mask flag without NXS_MEANS_ICE_MASK among the elemental ids.  A refused configuration leaves the previous one.
 *   nxs_dyn_means_set_tau_ow  D_tau_ow ([Ne], written by the thermodynamics): the one input of taux / tauy / taumod that is not the handle's; uploaded like
 *                  a forcing member, NULL detaches.  nxs_dyn_set_mesh detaches it (the size changes).
 *   nxs_dyn_means_update   updateMeans(means, time_factor): one launch over the owned elements, one over the nodes; asynchronous on the handle's stream.  It
 *                  includes the part of updateIceDiagnostics() the configured ids need (no nxs_dyn_ice_diagnostics call first) and only READS state and
 *                  diagnostics.  NXS_ERR_STATE: before nxs_dyn_set_mesh / nxs_dyn_put_state, nothing configured, tauwix / tauwiy without a wave stress
 *                  attached, taux / tauy / taumod without tau_ow attached.  For a thermodynamic id, naming the variable: its source row was never given on
 *                  this mesh (nxs_dyn_set_mesh and nxs_dyn_regrid make every such row missing); a row of the slab before the first nxs_dyn_slab /
 *                  nxs_dyn_slab_coupled on this mesh; t1 / t2 without WINTON rows; an alias that is not the configured source (tcc under NXS_FLUX_LW_QLW_IN,
 *                  snowfr under NXS_COL_SNOWFALL_SNOWFALL, mixrat under a dew-point humidity ...); wspeed before a forcing.  A list of ids below
 *                  NXS_MEANS_ELEMENTAL_END launches the kernel it always launched.
 *   nxs_dyn_means_get      synchronised on return.  elemental [Ne][num_elemental], nodal [Nn][num_nodal] host arrays (either may be NULL);
 *                  *elemental_dev / *nodal_dev (either may be NULL) receive the DEVICE pointers of the same interleaved rows (library-owned, valid until
 *                  nxs_dyn_means_configure / nxs_dyn_set_mesh; NULL for an empty list).
 *   nxs_dyn_means_to_grid  updateGridMean() on the regular grid: the coordinates displaced by the device's M_UM; with nodal variables the reference's setProcMask
 *                  (one elemental column, 1 on owned elements, 0 on ghosts, sampled with default 0); both row sets sampled with InterpFromMeshToGridx
 *                  semantics (nxs_interp_mesh_to_grid_device, default value 0); transposed as gridoutput.cpp:526-537 (grid_ind = i + ncols * j) and ADDED to
 *                  the caller's grid_elemental [num_elemental][ncols * nrows] / grid_nodal [num_nodal][ncols * nrows] (nodal values times the proc mask);
 *                  then the ice-mask rule on the variables with `mask`.  Summing the ranks' grids (boost::mpi::reduce, FE.cpp:9476-9487) stays with the caller.
 *   nxs_dyn_means_to_grid_conservative  updateGridMean()'s elemental leg on a loaded grid with interpMethod::conservative: the accumulator rows go straight from
 *                  the device into nxs_gridmap_mesh_to_grid with missing value 0. (gridoutput.cpp:473-476 passes 0., not M_miss_val); the result is ADDED to the
 *                  caller's grid_elemental [num_elemental][G] WITHOUT transposition (:541-545); then the ice-mask rule of :410-414 with miss_val.  `map` is a
 *                  nxs_gridmap (nxs_interp.h) of this mesh on the handle's device -- for a partitioned run the restricted one.  NXS_ERR_STATE: the map's
 *                  element count is not the handle's, no elemental variable is configured, a mask flag is set without NXS_MEANS_ICE_MASK.  A handle that
 *                  never calls it allocates and launches nothing for it.
 *   nxs_dyn_means_reset    resetMeshMean(bamgmesh): zeroes both accumulators on the stream. */
NXS_API int nxs_dyn_means_configure(nxs_dyn_handle *h, const nxs_dyn_means_config *c);
NXS_API int nxs_dyn_means_set_tau_ow(nxs_dyn_handle *h, const double *tau_ow /* [Ne] D_tau_ow, NULL = detach */);
NXS_API int nxs_dyn_means_update(nxs_dyn_handle *h, double time_factor);
NXS_API int nxs_dyn_means_get(nxs_dyn_handle *h, double *elemental /* [Ne][n_el] */, double *nodal /* [Nn][n_nod] */, const double **elemental_dev,
                              const double **nodal_dev);
NXS_API int nxs_dyn_means_to_grid(nxs_dyn_handle *h, const nxs_dyn_means_grid *g, double *grid_elemental, double *grid_nodal);
struct nxs_gridmap;
NXS_API int nxs_dyn_means_to_grid_conservative(nxs_dyn_handle *h, struct nxs_gridmap *map, double miss_val, double *grid_elemental /* [n_el][G] */);
NXS_API int nxs_dyn_means_reset(nxs_dyn_handle *h);

/* ---- The Moorings means on a LOADED grid (moorings.grid_type=from_file: the TOPAZ / NEMO / any curvilinear grid): GridOutput::updateGridMean() through the
 * M_grid.loaded, non-conservative branch of updateGridMeanWorker (model/gridoutput.cpp:387-415, 470-485, 511-545), setLSM / applyLSM (:558-574, :639-651),
 * rotateVectors (:578-623), resetGridMean (:627-635).  The G grid points, their rotation, the land-sea mask and the grid accumulators (data_grid) live on the
 * handle; one launch locates every grid point ONCE in the mesh displaced by the device's M_UM -- the reference's three InterpFromMeshToMesh2dx calls
 * (elemental variables, nodal variables, proc mask; isdefault = true, default 0.) see the same mesh and the same points, so they find the same triangle -- and
 * does the gather, the rotation, the product with the proc mask ("found in an owned element"), the accumulation and the ice-mask rule for that point.
 * The locator is the drifters' (exact, bamg's integer plane); the points, the mask and the accumulators do not depend on the mesh and SURVIVE nxs_dyn_set_mesh and
 * nxs_dyn_regrid: the reference calls updateGridMean just before a regrid and goes on adding after it.  A handle that never calls these functions allocates
 * and launches nothing for them.
 * M_cpl_out's accumulators on its exchange grid: nxs_dyn_cpl_out_* below, whose nodal leg is this section's launch on that set's rows.
 * OUT OF SCOPE: reading and projecting the grid file (initArbitraryGrid), the NetCDF writer, the OASIS put, the
 * reduction over ranks (FE.cpp:9476-9487: ranks fetch with apply_lsm = 0, sum, and mask themselves). */
enum nxs_means_rotation {
    NXS_MEANS_ROTATE_NONE = 0,        /* M_false_easting && thetaName == "": rotateVectors returns at once */
    NXS_MEANS_ROTATE_NORTH_EAST = 1,  /* !M_false_easting: cos / sin(rotation_angle - gridLON[i] * PI / 180) */
    NXS_MEANS_ROTATE_GRID_THETA = 2   /* M_false_easting with a theta variable: cos / sin(rotation_angle - gridTheta[i]) */
};
#define NXS_MEANS_MAX_PAIRS (NXS_MEANS_MAX_VARS / 2)

typedef struct nxs_dyn_means_points {
    int32_t G;                 /* M_grid_size; 0 removes the object */
    int32_t rotation;          /* enum nxs_means_rotation */
    const double *gridX;       /* [G] projected coordinates (forward_mapx stays the caller's, or nxs_mapx_forward) */
    const double *gridY;       /* [G] */
    const double *gridLON;     /* [G] degrees; NXS_MEANS_ROTATE_NORTH_EAST */
    const double *gridTheta;   /* [G] radians; NXS_MEANS_ROTATE_GRID_THETA */
    double rotation_angle;     /* radians: mapNextsim->rotation * PI / 180 */
    double miss_val;           /* M_miss_val */
    int32_t n_pairs;           /* M_vectorial_variables.size(), <= NXS_MEANS_MAX_PAIRS */
    int32_t pair_first[NXS_MEANS_MAX_PAIRS];    /* components_Id.first: a column of the configured nodal list */
    int32_t pair_second[NXS_MEANS_MAX_PAIRS];   /* components_Id.second */
} nxs_dyn_means_points;

/*   nxs_dyn_means_points_set     everything is copied.  cosang / sinang (gridoutput.cpp:602-614) are evaluated here, once, on the host with std::cos / std::sin of
 *                  the reference's own expressions and uploaded; the device does the four products and two sums of :617-618 without contraction, so the rotation is
 *                  bit for bit.  A new set replaces the previous one (mask and accumulators included).  G == 0 or p == NULL removes the object and frees its
 *                  memory.  nxs_dyn_means_configure with other list sizes drops the accumulators; they are made again, zeroed, at the new sizes by the next
 *                  nxs_dyn_means_points_update / _get / _reset.  NXS_ERR_INVALID: G < 0, a NULL coordinate array, a non-finite coordinate, an unknown rotation
 *                  mode or its angle array missing (or holding a non-finite value), n_pairs outside 0 .. NXS_MEANS_MAX_PAIRS, a pair index outside the
 *                  configured nodal list.
 *   nxs_dyn_means_points_lsm     setLSM.  lsm_in == NULL: computed on the handle's own mesh AT REST (M_UM = 0): 1 where the point lies in any triangle, ghosts
 *                  included, else 0 (needs nxs_dyn_set_mesh).  lsm_in != NULL: [G] uploaded (a partitioned run's root computes it on the root mesh, which no
 *                  handle holds).  lsm_out ([G], may be NULL) receives it.  Without this call there is no mask (M_use_lsm = false).
 *   nxs_dyn_means_points_update  updateGridMean(): asynchronous on the handle's stream.  Per grid point: the isdefault box test of InterpFromMeshToMesh2dx.cpp:92
 *                  against the displaced mesh's OWN box (the rank's, as the reference's per-rank call), the exact location; data_grid[nv][j] += the accumulator
 *                  row of the found element (P0; ghost elements included, their rows are 0), 0. when none holds the point; the nodal variables P1 in the operand
 *                  order of :157-159 (0. when not found), rotateVectors per pair in list order with the skip interp_out[first] == miss_val, then
 *                  data_grid[nv][j] += value * proc_mask (a NaN times 0 stays a NaN); the ice-mask rule of :404-414, nodal variables first.
 *                  NXS_ERR_STATE: before nxs_dyn_set_mesh / nxs_dyn_put_state, without points, nothing configured, a pair index outside the nodal list as
 *                  configured NOW.
 *   nxs_dyn_means_points_get     synchronised on return.  grid_elemental [num_elemental][G], grid_nodal [num_nodal][G] host arrays (either may be NULL), NOT
 *                  transposed (:541-545).  apply_lsm != 0 with a mask present: applyLSM on the copy handed out (miss_val where the mask is 0); the resident rows
 *                  stay as they are.  *elemental_dev / *nodal_dev (either may be NULL) receive the DEVICE pointers of the resident rows (library-owned, valid
 *                  until nxs_dyn_means_points_set / nxs_dyn_means_configure; NULL for an empty list).
 *   nxs_dyn_means_points_reset   resetGridMean(): the grid accumulators to zero, on the stream. */
NXS_API int nxs_dyn_means_points_set(nxs_dyn_handle *h, const nxs_dyn_means_points *p);
NXS_API int nxs_dyn_means_points_lsm(nxs_dyn_handle *h, const int32_t *lsm_in /* [G] or NULL */, int32_t *lsm_out /* [G] or NULL */);
NXS_API int nxs_dyn_means_points_update(nxs_dyn_handle *h);
NXS_API int nxs_dyn_means_points_get(nxs_dyn_handle *h, int32_t apply_lsm, double *grid_elemental /* [n_el][G] */, double *grid_nodal /* [n_nod][G] */,
                                     const double **elemental_dev, const double **nodal_dev);
NXS_API int nxs_dyn_means_points_reset(nxs_dyn_handle *h);

/* ---- The Moorings means on the REGULAR grid (moorings.grid_type=regular, the reference's default): GridOutput::updateGridMean() through the M_is_regular_grid
 * branch of updateGridMeanWorker (model/gridoutput.cpp:387-415, 486-505, 511-538), setProcMask (:360-378), setLSM / applyLSM (:558-574, :639-651), rotateVectors
 * (:578-623), resetGridMean (:627-635) and the arithmetic of contrib/bamg/src/InterpFromMeshToGridx.cpp, bit for bit.  The grid, its rotation, the land-sea mask
 * and the grid accumulators (data_grid) live on the handle.  nxs_dyn_means_regular_update is two launches on the handle's stream and nothing else: the mesh is
 * x0 + M_UM formed on the device; the reference's three InterpFromMeshToGridx calls (proc mask, elemental variables, nodal variables) see the same mesh and the same
 * points, so the winner of every point -- the HIGHEST element number that holds it, the reference's element loop overwrites -- is found once (one thread per
 * element, an integer atomic maximum per held point), and one thread per grid point then gathers, rotates, accumulates in grid order and applies the ice-mask rule.
 * No copy in either direction, no host loop, no synchronisation.  The object, its mask and its accumulators SURVIVE nxs_dyn_set_mesh and nxs_dyn_regrid: the
 * reference calls updateGridMean just before a regrid (FE.cpp:8005-8010) and goes on adding after it.  A handle that never calls these functions allocates and
 * launches nothing for them.  nxs_dyn_means_to_grid stays what it was.
 * rotateVectors indexes interp_out in BAMG order (b = i * M_nrows + j for column i, row j) and M_grid.gridLON by the SAME number, although initRegularGrid fills
 * gridLON in grid order (i + M_ncols * j): a point is rotated by the longitude of whichever point has the grid index b.  That is restated as it stands; a
 * square grid hides it.
 * OUT OF SCOPE: inverse_mapx for gridLAT / gridLON (the caller passes gridLON), the NetCDF writer, the reduction over ranks (FE.cpp:9476-9487: ranks fetch with
 * apply_lsm = 0, sum, and mask with the root's LSM). */
typedef struct nxs_dyn_means_regular {
    int32_t ncols, nrows;      /* M_ncols (along x), M_nrows (along y); 0 in either removes the object */
    double xmin, ymax;         /* M_xmin, M_ymax */
    double mooring_spacing;    /* M_mooring_spacing > 0 */
    double miss_val;           /* M_miss_val */
    int32_t rotation;          /* NXS_MEANS_ROTATE_NONE or NXS_MEANS_ROTATE_NORTH_EAST; NXS_MEANS_ROTATE_GRID_THETA is refused: M_grid = Grid() has no theta */
    const double *gridLON;     /* [ncols * nrows] degrees, as initRegularGrid fills it (gridoutput.cpp:199-213: entry i + ncols * j); NORTH_EAST only */
    double rotation_angle;     /* radians: mapNextsim->rotation * PI / 180 */
    int32_t n_pairs;           /* M_vectorial_variables.size(), <= NXS_MEANS_MAX_PAIRS */
    int32_t pair_first[NXS_MEANS_MAX_PAIRS];    /* components_Id.first: a column of the configured nodal list */
    int32_t pair_second[NXS_MEANS_MAX_PAIRS];   /* components_Id.second */
} nxs_dyn_means_regular;

/*   nxs_dyn_means_regular_set     everything is copied.  x_grid[i] = xmin + spacing * i and y_grid[nrows - 1 - i] = ymax - spacing * i are built as
 *                  InterpFromMeshToGridx.cpp:78, 88 builds them (the second is not ymin + spacing * j in its last bit); cosang / sinang (gridoutput.cpp:608-609)
 *                  are evaluated here, once, on the host with std::cos / std::sin of the reference's own expression, entry k from gridLON[k].  A new set replaces
 *                  the previous one (mask and accumulators included).  ncols == 0, nrows == 0 or p == NULL removes the object and frees its memory.
 *                  nxs_dyn_means_configure with other list sizes drops the accumulators; they are made again, zeroed, at the new sizes by the next
 *                  nxs_dyn_means_regular_update / _get / _reset.  NXS_ERR_INVALID: a negative ncols or nrows, more than 2^31 - 1 grid points, a spacing that is
 *                  not positive and finite, a non-finite xmin / ymax, an unknown rotation mode, NXS_MEANS_ROTATE_GRID_THETA, NORTH_EAST without gridLON or with
 *                  a non-finite angle, n_pairs outside 0 .. NXS_MEANS_MAX_PAIRS, a pair index outside the configured nodal list.
 *   nxs_dyn_means_regular_lsm     setLSM.  lsm_in == NULL: computed on the handle's own mesh AT REST (M_UM = 0) with the arithmetic of the update's search: 1
 *                  where any triangle, ghosts included, holds the point, else 0 (needs nxs_dyn_set_mesh).  lsm_in != NULL: [ncols * nrows] in grid order, taken
 *                  as given (a partitioned run's root computes it on the root mesh, which no handle holds).  lsm_out (may be NULL) receives it.  Without
 *                  this call there is no mask (M_use_lsm = false).
 *   nxs_dyn_means_regular_update  updateGridMean(): asynchronous on the handle's stream.  Per grid point: the winner is the highest-numbered element whose box holds
 *                  the point (:143, :148) and whose area_1, area_2, area_3 of :152-158 are all > -10e-12; data_grid[nv][i + ncols * j] += the accumulator row of
 *                  the winner, 0. when none holds the point; the nodal variables area_1 * d0, += area_2 * d1, += area_3 * d2 without contraction; a NaN value
 *                  becomes the default 0. (:175) BEFORE the proc mask -- unlike the loaded grid, where NaN * 0. stays a NaN; rotateVectors per pair in list
 *                  order with the skip interp_out[first] == miss_val; the nodal value times the proc mask (1. for a winner below M_local_nelements, else 0.);
 *                  the ice-mask rule of :404-414, nodal variables first.  NXS_ERR_STATE: before nxs_dyn_set_mesh / nxs_dyn_put_state, without a grid, nothing
 *                  configured, a pair index outside the nodal list as configured NOW.
 *   nxs_dyn_means_regular_get     synchronised on return.  grid_elemental [num_elemental][ncols * nrows], grid_nodal [num_nodal][ncols * nrows] host arrays in
 *                  grid order (either may be NULL).  apply_lsm != 0 with a mask present: applyLSM on the copy handed out (miss_val where the mask is 0); the
 *                  resident rows stay as they are.  *elemental_dev / *nodal_dev (either may be NULL) receive the DEVICE pointers of the resident rows
 *                  (library-owned, valid until nxs_dyn_means_regular_set / nxs_dyn_means_configure; NULL for an empty list).
 *   nxs_dyn_means_regular_reset   resetGridMean(): the grid accumulators to zero, on the stream.
 * Option "means_timing" 1 puts events around the two launches: nxs_dyn_debug_array "means_regular_ms" returns [the search, the gather] of the last update in ms. */
NXS_API int nxs_dyn_means_regular_set(nxs_dyn_handle *h, const nxs_dyn_means_regular *p);
NXS_API int nxs_dyn_means_regular_lsm(nxs_dyn_handle *h, const int32_t *lsm_in /* [ncols * nrows] or NULL */, int32_t *lsm_out /* [ncols * nrows] or NULL */);
NXS_API int nxs_dyn_means_regular_update(nxs_dyn_handle *h);
NXS_API int nxs_dyn_means_regular_get(nxs_dyn_handle *h, int32_t apply_lsm, double *grid_elemental /* [n_el][ncols * nrows] */, double *grid_nodal /* [n_nod][ncols * nrows] */,
                                      const double **elemental_dev, const double **nodal_dev);
NXS_API int nxs_dyn_means_regular_reset(nxs_dyn_handle *h);

/* ---- The coupler's outgoing fields: M_cpl_out, the second GridOutput of a coupled build.  FiniteElement::step() runs, every time step ("coupler put",
 * FE.cpp:8226-8266): updateIceDiagnostics(); updateMeans(M_cpl_out, cpl_time_factor); and, when a coupling step ends, M_cpl_out.updateGridMean(bamgmesh,
 * M_local_nelements, M_UM), the reduction over ranks, OASIS3::put_2d per variable, resetMeshMean(bamgmesh), resetGridMean() -- and updateGridMean once more in
 * front of every regrid (FE.cpp:8012-8052).  Here that is a SECOND accumulator set on the handle beside the Moorings' (the two do not see each other), the
 * exchange grid's accumulators (data_grid) on the device, and one put that chains the conservative elemental leg (nxs_gridmap_send_rows, include/nxs_interp.h)
 * and the nodal leg of nxs_dyn_means_points_update (exact locator in the mesh displaced by M_UM, P1 gather, rotateVectors, proc mask) on the handle's stream:
 * nothing crosses PCIe but the fields the host asks for.  A handle that never configures this set allocates and launches nothing for it.
 *
 *   nxs_dyn_cpl_out_configure  the struct and the id space of nxs_dyn_means_configure.  A set `mask` flag is NXS_ERR_INVALID: initOASIS sets none
 *                  (FE.cpp:7596-7684) and the ice-mask rule is not built for this set.  The configuration survives nxs_dyn_set_mesh / nxs_dyn_regrid: the mesh
 *                  accumulators are made again, zeroed, there (resetMeshMean(regrid = true)).  Other list sizes drop the grid accumulators (made again, zeroed,
 *                  by the next put / reset_grid).  Both lists empty frees everything of the set, the attached grid included.
 *   nxs_dyn_cpl_out_update     updateMeans(M_cpl_out, time_factor): the kernels of nxs_dyn_means_update with this set's tables and destinations; its refusals, with
 *                  "cpl_out_update" in the message; asynchronous.  time_factor is the host's (pcpt == 0) ? 1 : dtime_step / (double)cpl_time_step (FE.cpp:8230).
 *   nxs_dyn_cpl_out_get / nxs_dyn_cpl_out_reset   as nxs_dyn_means_get / nxs_dyn_means_reset (resetMeshMean(bamgmesh)) on this set.
 *   nxs_dyn_cpl_out_attach_grid  `map`: the nxs_gridmap of THIS mesh on the exchange grid (a partitioned run: the restricted one, which gives this rank's
 *                  partial sums); borrowed, and dropped by nxs_dyn_set_mesh / nxs_dyn_regrid like the ocean attachment (FE.cpp:8033: new weights after a regrid)
 *                  -- attach the new map again.  `points`: the P-points, the rotation and the pairs of the nodal variables, copied, cos / sin evaluated on the
 *                  host as nxs_dyn_means_points_set does; needed only when the set has nodal variables (else may be NULL).  The grid accumulators data_grid
 *                  ([n_el][G], [n_nod][G]) are NOT the mesh's: they survive nxs_dyn_set_mesh / nxs_dyn_regrid (the reference puts before a regrid and adds
 *                  again after it) and a new attach on a grid of the same size.  NXS_ERR_INVALID: G of map and points differ, what nxs_dyn_means_points_set
 *                  refuses; NXS_ERR_STATE: the map's element count is not the handle's, nothing configured, nodal variables without points.
 *   nxs_dyn_cpl_out_put        M_cpl_out.updateGridMean() (gridoutput.cpp:387-415) on the handle's stream: the elemental leg, then the nodal leg (n_el = 0, no ice
 *                  mask).  grid_elemental [n_el][G] / grid_nodal [n_nod][G] host arrays (either may be NULL) are copied AFTER the launches and the call is
 *                  synchronised only then; with both NULL it is asynchronous and *elemental_dev / *nodal_dev (either may be NULL) are what a host hands to its
 *                  reduction over ranks (FE.cpp:8236-8247 stays the caller's) and to OASIS.  flags & NXS_CPL_OUT_RESET queues resetMeshMean + resetGridMean behind
 *                  the copies (FE.cpp:8262-8263); without a host array that is NXS_ERR_INVALID: the values would be gone.
 *   nxs_dyn_cpl_out_reset_grid resetGridMean() alone. */
#define NXS_CPL_OUT_RESET 1
NXS_API int nxs_dyn_cpl_out_configure(nxs_dyn_handle *h, const nxs_dyn_means_config *c);
NXS_API int nxs_dyn_cpl_out_update(nxs_dyn_handle *h, double time_factor);
NXS_API int nxs_dyn_cpl_out_get(nxs_dyn_handle *h, double *elemental /* [Ne][n_el] */, double *nodal /* [Nn][n_nod] */, const double **elemental_dev,
                                const double **nodal_dev);
NXS_API int nxs_dyn_cpl_out_reset(nxs_dyn_handle *h);
NXS_API int nxs_dyn_cpl_out_attach_grid(nxs_dyn_handle *h, struct nxs_gridmap *map, const nxs_dyn_means_points *points);
NXS_API int nxs_dyn_cpl_out_put(nxs_dyn_handle *h, double *grid_elemental /* [n_el][G] */, double *grid_nodal /* [n_nod][G] */, const double **elemental_dev,
                                const double **nodal_dev, int32_t flags);
NXS_API int nxs_dyn_cpl_out_reset_grid(nxs_dyn_handle *h);
/* The three options of D_dmax / D_dmean (FE.cpp:1387, 1410-1411; defaults 0.1, 1000, 10: options.cpp:510-518): wave_coupling.dmax_c_threshold,
 * fsd_unbroken_floe_size, fsd_min_floe_size.  NXS_MEANS_DMAX / NXS_MEANS_DMEAN are the block of updateIceDiagnostics at FE.cpp:7902-7951 (+ * / min max only: bit
 * for bit) on M_conc_mech_fsd (nxs_dyn_fsd_put) with the bin limits and centres of nxs_dyn_fsd_configure and D_conc = M_conc (+ M_conc_young).  Without bins
 * attached (M_num_fsd_bins == 0) both accumulate 0; with bins but M_conc_mech_fsd, the FSD configuration or this one missing, the update is NXS_ERR_STATE naming
 * the variable.  NXS_ERR_INVALID: a value that is not finite. */
NXS_API int nxs_dyn_fsd_diag_configure(nxs_dyn_handle *h, double dmax_c_threshold, double fsd_unbroken_floe_size, double fsd_min_floe_size);

/* ---- The drifters on the device: the three statements of checkUpdateDrifters() (FE.cpp:8403-8437) that touch the handle's arrays -- Drifters::move with
 * M_UT and the reset of M_UT (checkMoveDrifters, FE.cpp:8375-8397), Drifters::updateConc on the mesh displaced by M_UM, Drifters::maskXY.  drifters.cpp's file
 * input and output, its timing logic and initFromSpacing's grid stay with the host.  A handle holds up to NXS_DRIFTER_SETS sets (M_drifters is a vector of
 * Drifters), each with x, y, id (M_X, M_Y, M_i) and conc on the device.  The sets are the handle's: they survive nxs_dyn_set_mesh (positions do not depend on the
 * mesh), so a host that regrids calls nxs_dyn_drifters_move BEFORE it replaces the mesh, as regrid() does (FE.cpp:3609).  Both interpolations locate the drifters
 * with bamg's integer predicates (include/nxs_interp.h), isdefault = true and default 0.: inside the mesh the bits are InterpFromMeshToMesh2dx's.
 *   bbox           NULL, or xmin, xmax, ymin, ymax of the mesh whose integer plane (Mesh::SetIntCoor) and isdefault box (InterpFromMeshToMesh2dx.cpp:92) are to be
 *                  used.  One rank: NULL.  Several ranks: every rank passes the box of the GLOBAL mesh -- the ranks' nxs_dyn_drifters_mesh_bbox results reduced
 *                  with min / max -- so that a shared node has the same integer coordinates on every rank and the rank that finds a drifter computes what the
 *                  reference's root computes on the gathered mesh.  Every rank holds the full sets; nothing is exchanged between handles.
 *   found          per drifter, from the last move or conc: 0 = in no triangle of this handle's mesh, 1 = in an owned element, 2 = in a ghost element.  move
 *                  displaces the drifters with found == 1 only; the host takes each drifter from the rank that reports 1 and sets the merged positions again.
 *   nxs_dyn_drifters_set    replaces set `set` (initFromSpacing / initFromTextFile / initFromNetCDF / a restart: drifters.cpp:27-71, 100-330); n == 0 is legal:
 *                  the set then exists and is empty
 *   nxs_dyn_drifters_clear  removes it (Drifters::reset, drifters.cpp:456-459)
 *   nxs_dyn_drifters_mesh_bbox  xmin, xmax, ymin, ymax of this handle's nodes, of coord_x / coord_y (displaced == 0) or displaced by M_UM (!= 0): a device reduction
 *   nxs_dyn_drifters_move   checkMoveDrifters(): with no set nothing happens and M_UT is left alone (FE.cpp:8383-8384); otherwise M_UT is interpolated at the
 *                  drifters of every set in the UNDISPLACED mesh (drifters.cpp:490-496), x += du, y += dv (drifters.cpp:499-503), then M_UT = 0 on every
 *                  node of the handle, ghosts included (FE.cpp:8390).  Asynchronous on the handle's stream
 *   nxs_dyn_drifters_conc   Drifters::updateConc (drifters.cpp:512-542): M_conc of the element that holds the drifter in the mesh displaced by M_UM
 *                  (FE.cpp:8433-8434), default 0., then std::max(0., std::min(1., v)); kept in the set, and copied to conc_host [n] unless that is NULL
 *   nxs_dyn_drifters_mask   Drifters::maskXY (drifters.cpp:548-579): drifter i stays iff conc[i] > conc_lim and id[i] occurs in keepers [n_keepers]; keepers
 *                  NULL keeps every id (the one-argument overload, drifters.hpp:231-237).  The survivors keep their order; *n_left = how many
 *   nxs_dyn_drifters_get    the set as it is now: *n and x, y, id, conc, found [n]; any output may be NULL
 * Errors: NXS_ERR_INVALID for a set outside 0 .. NXS_DRIFTER_SETS - 1 or a NaN coordinate in the mesh, NXS_ERR_STATE before set_mesh / put_state and for conc,
 * mask or get on a set that does not exist.  conc and move on an empty set succeed and do nothing (drifters.cpp:476-477, 518-519). */
#define NXS_DRIFTER_SETS 8
NXS_API int nxs_dyn_drifters_set(nxs_dyn_handle *h, int32_t set, int32_t n, const double *x, const double *y, const int32_t *id);
NXS_API int nxs_dyn_drifters_clear(nxs_dyn_handle *h, int32_t set);
NXS_API int nxs_dyn_drifters_mesh_bbox(nxs_dyn_handle *h, int32_t displaced, double *out /* [4] */);
NXS_API int nxs_dyn_drifters_move(nxs_dyn_handle *h, const double *bbox /* [4] or NULL */);
NXS_API int nxs_dyn_drifters_conc(nxs_dyn_handle *h, int32_t set, const double *bbox /* [4] or NULL */, double *conc_host /* [n] or NULL */);
NXS_API int nxs_dyn_drifters_mask(nxs_dyn_handle *h, int32_t set, double conc_lim, const int32_t *keepers, int32_t n_keepers, int32_t *n_left);
NXS_API int nxs_dyn_drifters_get(nxs_dyn_handle *h, int32_t set, int32_t *n, double *x, double *y, int32_t *id, double *conc, int32_t *found);

/* ---- A regrid on the live handle: FiniteElement::interpFields() + assignVariables() (FE.cpp:3071-3154, 553-572) without the prognostic state leaving the device.
 * The remesher stays the host's; what lies between the handle and the two interpolation kernels of include/nxs_interp.h happens here:
 *   1. collectVariables (FE.cpp:2120-2151)   the element variables as interleaved [Ne_old][nb_var] rows, the interpTransformation of every variable applied
 *      (operand order of FE.cpp:2139-2145).  Column order = sortPrognosticVars (FE.cpp:2087-2111): every variable of kind `none` first -- the handle's own in the
 *      order of nxs_dyn_state (conc, thick, snow_thick, damage, ridge_ratio, sigma[0..2], conc_young, h_young, hs_young, conc_myi, thick_myi), then cum_damage and
 *      the FSD bins while attached (nxs_dyn_put_coupled; with M_conc_mech_fsd / M_cum_wave_damage attached see nxs_dyn_fsd_put), then the caller's extras of kind none -- then the extras of kind conc, thick, enthalpy, each kind in
 *      the caller's order.  cohesion, time_relaxation_damage and drag_ui* are not prognostic in the reference and are no columns.
 *   2. ConservativeRemappingMeshToMesh through the context (nxs_regrid_remap_elements on device rows).
 *   3. redistributeVariables with apply_maxima = true (FE.cpp:2196-2258): one thread per new element walks the columns in order -- the inverse transformation
 *      with the clamped new M_conc / M_thick, the no_old_ice rule (M_tice: -mu * si, FE.cpp:2243-2245), max(minVal, .) then min(maxVal, .), and after the last
 *      column the young-ice cap conc_young = 1 - conc (FE.cpp:2253-2256) when ice_cat_type is NXS_ICECAT_YOUNG_ICE.  The handle's own bounds are
 *      model_variable.cpp's: conc, ridge_ratio, conc_young, conc_myi and every FSD bin in [0, 1]; thick, snow_thick, h_young, hs_young, thick_myi, cum_damage
 *      >= 0; damage in [0, 1 - 1e-10]; sigma unbounded.  A row the remapping left NaN (num_failed) stays NaN in every variable: the caller decides, where the
 *      reference asserts.
 *   4. gatherFieldsNode / scatterFieldsNode (FE.cpp:3174-3198, 3273-3293): [Nn_old][6] = VT.u, VT.v, UM.u, UM.v, UT.u, UT.v through InterpFromMeshToMesh2dx
 *      (isdefault = false) at the new nodes; M_VT from columns 0 and 1; M_UM = M_UT = 0 (assignVariables, FE.cpp:553-560), D_tau_w = D_tau_a = 0.
 *   5. the new mesh through nxs_dyn_set_mesh's own path; the new state rows take the place of the old ones on the device.  Forcing is the caller's next
 *      nxs_dyn_set_forcing, and the means / drifters attached to the handle see what they see after nxs_dyn_set_mesh.  cum_damage / FSD bins stay attached.
 * Errors: everything is checked on the host before the first launch -- NXS_ERR_INVALID for a NULL required pointer, num_extra < 0, an unknown transformation, no
 * context and no moved coordinates, a new mesh nxs_dyn_set_mesh would refuse; NXS_ERR_STATE before nxs_dyn_put_state and on a handle with halo lists (nranks > 1:
 * the reference does this step on its root rank from gathered state; the gather / scatter of a partitioned run is not done here).  A failure before step 5
 * leaves the handle on the old mesh with its state as it was (an extra's new_values may have been written). */
/* ModelVariable::interpTransformation, model_variable.hpp */
enum { NXS_TRANSFORM_NONE = 0, NXS_TRANSFORM_CONC = 1, NXS_TRANSFORM_THICK = 2, NXS_TRANSFORM_ENTHALPY = 3 };
/* nxs_dyn_regrid_var::flags */
enum { NXS_REGRID_VAR_HAS_MIN = 1,        /* ModelVariable::hasMinVal (FE.cpp:2247) */
       NXS_REGRID_VAR_HAS_MAX = 2,        /* ModelVariable::hasMaxVal (FE.cpp:2249) */
       NXS_REGRID_VAR_IS_TICE = 4,        /* varID() == M_tice: -mu * si where there is no ice (FE.cpp:2243-2245) */
       NXS_REGRID_VAR_OLD_ON_DEVICE = 8,  /* old_values is a device pointer on the handle's device: used in place */
       NXS_REGRID_VAR_NEW_ON_DEVICE = 16  /* new_values is: written in place */ };

/* one element variable the HOST owns (thermodynamics: M_tice[k], M_sst, M_sss, M_tsurf_young, ...) that rides along */
typedef struct nxs_dyn_regrid_var {
    const double *old_values;   /* [Ne_old] (*vptr)[i] of collectVariables (FE.cpp:2135) */
    double *new_values;         /* [Ne_new] (*vptr)[i] of redistributeVariables (FE.cpp:2250) */
    int32_t transformation;     /* NXS_TRANSFORM_*: vptr->getInterpTransformation() (FE.cpp:2136, 2217-2241) */
    int32_t flags;              /* NXS_REGRID_VAR_* */
    double min_val, max_val;    /* vptr->minVal(), maxVal() (FE.cpp:2247-2249); read only with the HAS_ flag */
} nxs_dyn_regrid_var;

typedef struct nxs_dyn_regrid_args {
    const nxs_dyn_mesh *new_mesh;            /* as for nxs_dyn_set_mesh: the adapted mesh after distributedMeshProcessing (FE.cpp:3743-3752) */
    struct nxs_regrid *context;              /* nxs_regrid_create of the OLD mesh at x0 + M_UM (M_mesh_root.move(um_root, 1.), FE.cpp:3668-3671), on the handle's device; NULL = built and destroyed inside */
    const double *x_old_moved, *y_old_moved; /* [Nn_old] those coordinates; needed when context == NULL (the host has them: it just ran the remesher on them) */
    const double *previous_numbering;        /* [Nn_new] bamgmesh_root->PreviousNumbering as nxs_regrid_remap_elements takes it (ConservativeRemapping.cpp:263-289); may be NULL */
    int32_t n_geom_vertices;                 /* bamgmesh_root->VerticesOnGeomVertexSize[0] */
    int32_t num_extra;                       /* entries of `extra` */
    const nxs_dyn_regrid_var *extra;         /* [num_extra] M_prognostic_variables_elt beyond the handle's own (FE.cpp:7127-7222); NULL with num_extra == 0 */
    double freezingpoint_mu;                 /* thermo.freezingpoint_mu (FE.cpp:1238); physical::si, Lf, C are the library's own (NXS_CONST_SI, _LF, _C) */
    /* inputs that are NOT prognostic in the reference and are re-made after a regrid (assignVariables, calcCohesion, thermo): [Ne_new] each, required */
    const double *cohesion;                  /* M_Cohesion (calcCohesion, FE.cpp:3909-3914) */
    const double *time_relaxation_damage;    /* M_time_relaxation_damage (FE.cpp:648-649) */
    const double *drag_ui;                   /* M_drag_ui */
    const double *drag_ui_young;             /* M_drag_ui_young */
} nxs_dyn_regrid_args;

typedef struct nxs_dyn_regrid_info {
    int32_t num_failed;       /* new elements the conservative remapping could not do (nxs_regrid_remap_elements): their rows are NaN */
    int32_t num_exterior;     /* new nodes in no triangle of the old mesh (nxs_regrid_interp_nodes) */
    int32_t nb_var_element;   /* columns of the element rows: M_prognostic_variables_elt.size() (FE.cpp:2123) */
    int32_t reserved0;
    double collect_ms, remap_ms, redistribute_ms, nodes_ms, set_mesh_ms, total_ms;   /* host wall clock of the five phases (uploads of extras in collect_ms, their way back and the re-made inputs in set_mesh_ms) and of the call */
} nxs_dyn_regrid_info;

NXS_API int nxs_dyn_regrid(nxs_dyn_handle *h, const nxs_dyn_regrid_args *a, nxs_dyn_regrid_info *info /* may be NULL */);

/* ---- The thermodynamic state across a regrid (opt-in).  In the reference the rows of nxs_dyn_flux_state, nxs_dyn_column_state and nxs_dyn_slab_state are ordinary
 * members of M_prognostic_variables_elt (FE.cpp:7137-7237) and pass through the same collectVariables -> ConservativeRemappingMeshToMesh -> redistributeVariables
 * as M_conc.  With carry != 0, nxs_dyn_regrid appends one column for every such row that is PRESENT on the old mesh (given by nxs_dyn_flux_put / _column_put /
 * _slab_put); within each kind the carried columns come before the caller's extras, columns 0 and 1 stay conc and thick.  interpTransformation and bounds are
 * model/model_variable.cpp's:
 *     tice0 none, tice1 enthalpy, tice2 thick (all three M_tice: -mu * si where the new mesh has no ice)
 *     tsurf_young, sst, sss, lid_volume, pond_volume, del_vi_tend     none, unbounded
 *     conc_upd                                                        none, [-1, 1]
 *     freeze_onset, conc_summer, fyi_fraction                         none, [0, 1]
 *     freeze_days, thick_summer, age_det, age                         none, >= 0
 * Three flux rows are not interpolated by the reference and are RE-MADE on the new mesh whenever carry is on: drag_ti = drag_ti_young = drag_ice_t everywhere
 * (assignVariables, FE.cpp:566-571) and pond_fraction = 0 (D_pond_fraction is a diagnostic: scatterFieldsElement assigns 0, FE.cpp:3012-3015).
 * After the call the rows present on the new mesh are exactly the carried and the re-made ones; a row that was missing stays missing; the forcing rows
 * (nxs_dyn_flux_set_atmosphere, nxs_dyn_column_set_forcing, the nxs_dyn_thermo_forcing_* pool) are missing as after nxs_dyn_set_mesh -- the reference sets
 * interpolated = false -- and so are the output rows of nxs_dyn_fluxes / _column / _slab: the chain starts again with nxs_dyn_fluxes.  A row of a new element the
 * remapping marked failed is NaN in the carried rows too.  The enthalpy constants use nxs_dyn_regrid_args::freezingpoint_mu; if the handle has a column
 * configuration whose freezingpoint_mu differs, nxs_dyn_regrid answers NXS_ERR_INVALID naming both values before its first launch.  A failure before the mesh swap
 * leaves every thermodynamic row of the old mesh as it was.
 *   nxs_dyn_regrid_carry_thermo      the setting is the handle's and survives nxs_dyn_set_mesh; carry = 0 restores the default (every row missing after a regrid).
 *                                    NXS_ERR_INVALID: carry != 0 with a NaN drag_ice_t
 *   nxs_dyn_regrid_thermo_info_get   what the last nxs_dyn_regrid did (all zero before the first) */
typedef struct nxs_dyn_regrid_thermo {
    int32_t carry;        /* != 0: nxs_dyn_regrid carries the thermodynamic state */
    int32_t reserved;
    double drag_ice_t;    /* thermo.drag_ice_t (FE.cpp:566): what drag_ti and drag_ti_young become on the new mesh */
} nxs_dyn_regrid_thermo;
NXS_API int nxs_dyn_regrid_carry_thermo(nxs_dyn_handle *h, const nxs_dyn_regrid_thermo *o);
typedef struct nxs_dyn_regrid_thermo_info {
    uint32_t flux_carried, col_carried, slab_carried;   /* bit k: member k of nxs_dyn_flux_state / _column_state / _slab_state was a column */
    uint32_t flux_remade;                               /* bit k: that member of nxs_dyn_flux_state was re-made */
    int32_t nb_var_element;                             /* columns of the element rows, the carried ones included (= nxs_dyn_regrid_info::nb_var_element) */
    int32_t tiled;                                      /* 1: rows wider than 31 columns went through LDS in column tiles (option "regrid_tile"); 0: staged whole, or walked in global memory */
} nxs_dyn_regrid_thermo_info;
NXS_API int nxs_dyn_regrid_thermo_info_get(nxs_dyn_handle *h, nxs_dyn_regrid_thermo_info *out);

/* ---- The floe-size distribution on the device (#ifdef OASIS, M_num_fsd_bins > 0): the per-element loops a wave-coupled step() runs between two dynamics steps --
 * updateFSD() after update(), after thermo() and after a regrid (FE.cpp:8144-8147, 8216-8219), redistributeFSD() on every coupling step (FE.cpp:8156-8168),
 * weldingRoach() and the mechanical healing inside thermo() (FE.cpp:5783-5796, 5888-5896) -- on the bins nxs_dyn_put_coupled attached, so that a resident host no
 * longer pulls the bins, conc, conc_young, thick, h_young and damage and pushes bins, damage and cum_damage every step.  Every loop is per element without a
 * stencil, ghost elements included: no exchange, and a partitioned handle runs them unchanged.  Each entry point is ONE kernel over M_num_elements, a thread holds
 * its element's bins in registers (bin-major rows: a wave reads and writes whole lines), asynchronous on the handle's stream.  Built uncontracted like the rest.
 * NOT AMONG nxs_dyn_fsd_*: redistributeThermoFSD (FE.cpp:4487-4670, lateral melt and growth, called with thermo's lat_melt_rate / young_ice_growth / old_conc) and
 * the melt-out branch of thermo() (FE.cpp:5729-5764) need intermediates of thermo(): they run inside nxs_dyn_slab_coupled, where those exist on the device.
 *   nxs_fsd_bins   HOST ONLY: the tables of initFsd() (FE.cpp:7408-7533) for FSDType CONSTANT_SIZE / CONSTANT_AREA, M_floe_shape = 0.66.  std::pow(x, 2) is
 *                  written x * x (what GCC and clang make of it at -O1 and above; a libm pow may differ in the last bit); everything else is + - * / sqrt.
 *                  alpha_merge is M_alpha_fsd_merge[m][n], row-major [n][n], -999 where no bin matches.  Any output of nxs_fsd_tables may be NULL.
 *   nxs_fsd_config_check  HOST ONLY: what nxs_dyn_fsd_configure refuses, without a handle (attached_bins = the bins of the attached conc_fsd).
 *   nxs_dyn_fsd_configure  copies the tables (the caller's own or nxs_fsd_bins') and the options of the loops.  NXS_ERR_INVALID: num_bins different from the
 *                  attached conc_fsd's, < 1 or > NXS_FSD_MAX_BINS; an unknown breakup_type / welding_type / fsd_damage_type / breakup_prob_type; a NULL table;
 *                  an alpha_merge[kx][ky] outside [1, num_bins] for a ky <= kx (weldingRoach indexes tmp_conc_fsd[a - 1] with it, FE.cpp:4780).  A refused
 *                  configuration leaves the previous one.  Everything that does not depend on the element is computed HERE with the host's libm and uploaded:
 *                  P = P_inf * (1 - exp(-P_inf * cpl_time_step / tau_w)) (FE.cpp:4335), the redistributors beta[j][k] of ZHANG and UNIFORM_SIZE
 *                  (FE.cpp:4361, 4380-4381), pow(PI, 4) * floes_flex_young and 48 * rhow * g * (1 - pow(poisson, 2)) of d_flex (FE.cpp:4312-4313; physical::g =
 *                  9.8, not physical::gravity), log(ksi).  The configuration is the handle's and survives nxs_dyn_set_mesh; the kernels refuse
 *                  (NXS_ERR_STATE) while the attached number of bins is not the configured one.
 *   nxs_dyn_fsd_put / _get  M_conc_mech_fsd [num_fsd_bins][Ne] and M_cum_wave_damage [Ne]; NULL = detached (put) / not wanted (get), as nxs_dyn_put_coupled.
 *                  conc_fsd and cum_damage stay with nxs_dyn_put_coupled.  nxs_dyn_set_mesh detaches both.  get also reports and clears weld_crash (below).
 *                  nxs_dyn_regrid carries them as further columns of kind none: the mechanical bins in [0, 1] behind M_conc_fsd, cum_wave_damage >= 0 behind
 *                  cum_damage, which is where initModelVariables puts them (FE.cpp:7193-7212): with one of them attached the coupled columns are
 *                  M_conc_fsd[..], M_conc_mech_fsd[..], M_cum_damage, M_cum_wave_damage; with neither the order is what it was (cum_damage, M_conc_fsd[..]).
 *   nxs_dyn_fsd_init     the distribution at the end of initFsd() (FE.cpp:7562-7576): everything in the highest bin.
 *   nxs_dyn_fsd_update   updateFSD() (FE.cpp:4674-4732), M_conc_mech_fsd included with distinguish_mech_fsd; the ctot2 == 0 < ctot branch and the division by
 *                  a zero ctot2 where ctot >= 1 are the reference's.
 *   nxs_dyn_fsd_breakup  redistributeFSD() (FE.cpp:4268-4483).  wlbk: M_wlbk [Ne], a host pointer or (flags & NXS_FSD_WLBK_ON_DEVICE) a device pointer.
 *                  *breakup_in_dt = M_breakup_in_dt, *crash = the mini check of FE.cpp:4426-4436 under debug_fsd -- a flag, not an exception; both are reduced
 *                  on the device; with both NULL the call stays asynchronous.  The reference's oddities are kept: the thickness is 0 before the max with
 *                  breakup_thick_min when neither breakup_cell_average_thickness nor the young-ice category applies; every type redistributes within the
 *                  broken bin too (k <= j); fsd_damage_type 1 falls through into 2 (no break at FE.cpp:4454); damage is written only where M_thick > 0;
 *                  the bins are cleared in the else of ctot > 0.  M_damage is written where the sub-step loop keeps it (its records after a step, like
 *                  update()), M_cum_damage / M_cum_wave_damage where attached.  fsd_damage_type 1 / 2 read M_conc_mech_fsd: NXS_ERR_STATE without it.
 *                  tanh / pow / log are the device's: against a host libm the bins and damage of broken elements agree to 1e-15 with UNIFORM_SIZE and ZHANG and to
 *                  3e-14 with DUMONT, whose redistributor divides differences of powers with exponents down to 1e-6; everything else is bitwise.
 *   nxs_dyn_fsd_weld     weldingRoach(i, ddt) (FE.cpp:4737-4870) where welding_type is ROACH, then the mechanical healing (FE.cpp:5888-5896) where
 *                  distinguish_mech_fsd, both only where freezing[i] != 0 (thermo's del_hi > 0; [Ne] uint8 on the host).  ndt_mrg = round(stability + 0.5),
 *                  subdt = ddt / (float)ndt_mrg as written; the sums of sum_mergers and coag_pos in the reference's order: no libm call, the same bits.  The
 *                  loop over ndt_mrg is per element and data-dependent: lanes diverge, no cap.  The reference's crash conditions (the sanity checks of the
 *                  sub-steps under debug_fsd; |conc_loss| > 1e-6 and a bin below -1e-12 always, as written) raise weld_crash, which the next nxs_dyn_fsd_get
 *                  reports; the element is finished as the arithmetic says.  Healing reads M_time_relaxation_damage as the handle holds it at the call.
 * NXS_FSD_MAX_BINS = 16 is a CHOSEN cap: the kernels are builds for at most 2, 6, 12 and 16 bins in which the index into a thread's bins is meant to be a
 * compile-time constant (the data-dependent tmp_conc_fsd[a - 1] of the welding is a chain of selects).  Measured for gfx950 (ROCm 7.2) at 16 bins: welding 104,
 * break-up 180, update 84 VGPRs of the 512 a wave of a 256-thread workgroup may have, no scratch memory and no VGPR spill in any build; the 12- and 16-bin
 * builds spill 63-79 SGPRs, which the compiler keeps in VGPR lanes, not in memory.  No build above 16 was tried.  tests/test_fsd_abi.py reads these figures from
 * the built library and fails when a build uses scratch memory.
 * M_damage: the kernels find it where the handle says it is after ANY family of the sub-step loop (the arrays, or the records of the last step), resident loop
 * and data-flow launch included; tests/test_gpu_fsd.py runs the residency check on each family.
 * abs(conc_loss) (FE.cpp:4831) is written unqualified in the reference; here it is the floating-point absolute value (what <cmath>'s overloads give a C++11
 * build).  Were it C's int abs, that check could never fire; only weld_crash depends on it. */
#define NXS_FSD_MAX_BINS 16
/* setup::FSDType, WeldingType, BreakupType: model/enums.hpp:99-116 */
enum { NXS_FSD_CONSTANT_SIZE = 0, NXS_FSD_CONSTANT_AREA = 1 };
enum { NXS_WELDING_NONE = 0, NXS_WELDING_ROACH = 1 };
enum { NXS_BREAKUP_NONE = 0, NXS_BREAKUP_UNIFORM_SIZE = 1, NXS_BREAKUP_ZHANG = 2, NXS_BREAKUP_DUMONT = 3 };
enum { NXS_FSD_WLBK_ON_DEVICE = 1 };   /* nxs_dyn_fsd_breakup flags */

typedef struct nxs_fsd_tables {      /* [num_bins] each */
    double *bin_widths;              /* M_fsd_bin_widths */
    double *bin_low_limits;          /* M_fsd_bin_low_limits */
    double *bin_up_limits;           /* M_fsd_bin_up_limits */
    double *bin_centres;             /* M_fsd_bin_centres */
    double *area_scaled_up;          /* M_fsd_area_scaled_up */
    double *area_scaled_low;         /* M_fsd_area_scaled_low */
    double *area_scaled_centered;    /* M_fsd_area_scaled_centered */
    double *area_scaled_binwidth;    /* M_fsd_area_scaled_binwidth */
    int32_t *alpha_merge;            /* [num_bins][num_bins] M_alpha_fsd_merge[m][n] */
} nxs_fsd_tables;

typedef struct nxs_dyn_fsd_config {
    int32_t num_bins;                          /* M_num_fsd_bins */
    int32_t breakup_type;                      /* NXS_BREAKUP_*: wave_coupling.breakup_type */
    int32_t breakup_prob_type;                 /* wave_coupling.breakup_prob_type: only 0 exists (FE.cpp:4331-4341) */
    int32_t fsd_damage_type;                   /* wave_coupling.fsd_damage_type: 0, 1, 2 */
    int32_t welding_type;                      /* NXS_WELDING_* */
    int32_t distinguish_mech_fsd;              /* wave_coupling.distinguish_mech_fsd */
    int32_t debug_fsd;                         /* wave_coupling.debug_fsd */
    int32_t breakup_cell_average_thickness;    /* wave_coupling.breakup_cell_average_thickness */
    double breakup_coef1, breakup_coef2, breakup_coef3;   /* FE.cpp:4274-4276 */
    double breakup_prob_cutoff;                /* FE.cpp:4277 */
    double breakup_timescale_tuning;           /* tau_w, FE.cpp:4329 */
    double cpl_time_step;                      /* coupler.timestep [s] */
    double floes_flex_young;                   /* M_floes_flex_young */
    double breakup_thick_min;                  /* M_breakup_thick_min */
    double fsd_damage_max;                     /* wave_coupling.fsd_damage_max */
    double welding_kappa;                      /* M_welding_kappa */
    nxs_fsd_tables tables;                     /* read, not written; area_scaled_low may be NULL (no loop reads it) */
} nxs_dyn_fsd_config;

typedef struct nxs_dyn_fsd_state {
    double *conc_mech_fsd;     /* [num_fsd_bins][Ne] M_conc_mech_fsd, bin-major; NULL = none */
    double *cum_wave_damage;   /* [Ne] M_cum_wave_damage; NULL = none */
    int32_t num_fsd_bins;      /* with conc_mech_fsd: the number of bins of the attached conc_fsd */
    int32_t weld_crash;        /* written by nxs_dyn_fsd_get: != 0 when a crash condition of weldingRoach was met since the last get */
} nxs_dyn_fsd_state;

NXS_API int nxs_fsd_bins(int32_t fsd_type, int32_t num_bins, double min_floe_size, double bin_cst_width, int32_t welding_use_scaled_area, nxs_fsd_tables *out);
NXS_API int nxs_fsd_config_check(const nxs_dyn_fsd_config *c, int32_t attached_bins);
NXS_API int nxs_dyn_fsd_configure(nxs_dyn_handle *h, const nxs_dyn_fsd_config *c);
NXS_API int nxs_dyn_fsd_put(nxs_dyn_handle *h, const nxs_dyn_fsd_state *s);
NXS_API int nxs_dyn_fsd_get(nxs_dyn_handle *h, nxs_dyn_fsd_state *s);
NXS_API int nxs_dyn_fsd_init(nxs_dyn_handle *h);
NXS_API int nxs_dyn_fsd_update(nxs_dyn_handle *h);
NXS_API int nxs_dyn_fsd_breakup(nxs_dyn_handle *h, const double *wlbk /* [Ne] M_wlbk */, int32_t flags, int32_t *breakup_in_dt /* may be NULL */, int32_t *crash /* may be NULL */);
NXS_API int nxs_dyn_fsd_weld(nxs_dyn_handle *h, double ddt, const uint8_t *freezing /* [Ne] del_hi > 0 */);

/* ---- The atmospheric bulk fluxes of thermo() on the device: its "fluxes" timer (FE.cpp:5214-5277) -- OWBulkFluxes (the `nextsim` formula, FE.cpp:5096-5132, and the
 * radiative loop, FE.cpp:5138-5158), IABulkFluxes (FE.cpp:6148-6353: the constants block, the Grachev stability functions, thermo.force_neutral_atmosphere, the
 * pond-fraction rule) for the old ice and, in the young-ice category, for the young ice, with specificHumidity (FE.cpp:4966-5019, all three schemes), albedo
 * (FE.cpp:6454-6535, schemes 1-4), windSpeedElement (FE.cpp:6359-6370) and incomingLongwave (FE.cpp:6376-6389, both sources).  One launch, a thread per element,
 * ghost elements included.  It reads M_conc, M_snow_thick, M_conc_young, M_hs_young and the wind the step's prep kernels read (nxs_dyn_set_forcing, or the pair
 * blended by nxs_dyn_set_forcing_time) -- all resident --, the atmosphere and the thermodynamic rows below, and writes 25 rows for the slab loop, D_tau_ow into
 * the row nxs_dyn_means_update reads (so no nxs_dyn_means_set_tau_ow) and M_drag_ui / M_drag_ti and their _young twins IN PLACE (the next call and the next step
 * read them: no upload of drag_ui / drag_ui_young through nxs_dyn_put_state).
 * While a coupled ocean is attached (nxs_dyn_ocean_coupled_attach, below) Qow += Qsw * M_qsrml replaces Qow += Qsw (FE.cpp:5150-5157); NXS_FLUX_QSW_OW stays the
 * total short wave.  OUT OF SCOPE: the #ifdef AEROBULK branch of OWBulkFluxes (a Fortran library; only the `nextsim` formula is built), and thermo() from
 * FE.cpp:5279 on (the slab loop), which consumes the rows of nxs_dyn_fluxes_get.
 *   nxs_flux_default_config   model/options.cpp:388-438; humidity from the dew point, long wave from Qlw_in
 *   nxs_flux_config_check     what nxs_dyn_flux_configure refuses, without a handle (so without a device): alb_scheme outside 1..4, zref_wind, zref_temp or
 *                  limiting_lengthscale <= 0 (or NaN), an unknown humidity or long-wave source; NXS_ERR_INVALID, the text in nxs_dyn_last_error(NULL)
 *   nxs_flux_constants        TEST DOOR, like nxs_dyn_physical_constants: the physical:: constants compiled into the kernel, in the order NXS_FLUX_CONST_* names them
 *                  (host only), so that a caller and tests/test_fluxes_abi.py can check that library and model agree; no reference call site
 *   nxs_dyn_flux_configure    the configuration is the handle's and survives nxs_dyn_set_mesh; quad_drag_coef_air (z0, FE.cpp:6170) is nxs_dyn_params'
 *   nxs_dyn_flux_set_atmosphere   [Ne] host rows; a NULL row means "the device copy is current" (a row never given stays missing)
 *   nxs_dyn_flux_put / _get   the thermodynamic rows the fluxes read or write; NULL members as in nxs_dyn_put_state / nxs_dyn_get_state (put: the device copy is
 *                  current; get: not wanted).  sss is carried for the slab loop: specificHumidity(WATER) assigns it and never reads it (FE.cpp:4990-4993)
 *   nxs_dyn_fluxes            the launch, asynchronous on the handle's stream.  NXS_ERR_STATE: before nxs_dyn_flux_configure, before nxs_dyn_put_state and a
 *                  forcing, while an atmosphere or flux row is missing -- which is the state after nxs_dyn_set_mesh AND, by default, after nxs_dyn_regrid.
 *                  With nxs_dyn_regrid_carry_thermo the rows of nxs_dyn_flux_state cross a regrid on the device (drag_ti, drag_ti_young and pond_fraction
 *                  are re-made, as in the reference); the atmosphere is the host's to give again on the new mesh in either case
 *   nxs_dyn_fluxes_get        synchronised on return.  out (may be NULL): host pointers, a NULL row is skipped.  device_rows (may be NULL): receives the
 *                  NXS_FLUX_ROWS DEVICE pointers of the same rows ([Ne] each, library-owned, valid until nxs_dyn_set_mesh), for the slab loop or a host that
 *                  lives on the GPU.  In the classic category the nine _young rows are zero (FE.cpp:5266-5272).  NXS_ERR_STATE before the first nxs_dyn_fluxes */
enum { NXS_FLUX_HUM_DEWPOINT = 0 /* M_dair */, NXS_FLUX_HUM_SPHUMA = 1 /* M_sphuma */, NXS_FLUX_HUM_MIXRAT = 2 /* M_mixrat */ };
enum { NXS_FLUX_LW_QLW_IN = 0 /* M_Qlw_in */, NXS_FLUX_LW_TCC = 1 /* M_tcc: thermo.use_parameterised_long_wave_radiation */ };
enum { NXS_FLUX_CONST_TFRWK = 0, NXS_FLUX_CONST_RA_DRY, NXS_FLUX_CONST_RA_VAP, NXS_FLUX_CONST_CPA, NXS_FLUX_CONST_CPV, NXS_FLUX_CONST_LV0, NXS_FLUX_CONST_EPS,
       NXS_FLUX_CONST_SIGMA_SB, NXS_FLUX_CONST_VONKARMAN, NXS_FLUX_CONST_GAMMA_D, NXS_FLUX_CONST_RHOA, NXS_FLUX_CONST_LF, NXS_FLUX_CONST_G, NXS_FLUX_CONST_COUNT };
typedef struct nxs_dyn_flux_config {
    int32_t alb_scheme;                /* thermo.alb_scheme, 1..4 */
    int32_t humidity_source;           /* NXS_FLUX_HUM_*: which of M_dair, M_sphuma, M_mixrat the dataset initialised (FE.cpp:4980-4985) */
    int32_t longwave_source;           /* NXS_FLUX_LW_* (FE.cpp:6378) */
    int32_t force_neutral_atmosphere;  /* thermo.force_neutral_atmosphere: the drags are left as they are */
    double alb_ice, alb_sn, alb_ponds; /* thermo.alb_ice, alb_sn, alb_ponds */
    double I_0;                        /* thermo.I_0 */
    double ocean_albedo;               /* thermo.albedoW (M_ocean_albedo) */
    double drag_ocean_t, drag_ocean_q; /* thermo.drag_ocean_t, drag_ocean_q */
    double zref_wind, zref_temp;       /* thermo.zref_wind, zref_temp [m] */
    double limiting_lengthscale;       /* thermo.limiting_lengthscale [m] */
} nxs_dyn_flux_config;
typedef struct nxs_dyn_flux_atmosphere {
    const double *tair, *mslp, *Qsw_in; /* [Ne] M_tair, M_mslp, M_Qsw_in */
    const double *humidity;             /* [Ne] M_dair, M_sphuma or M_mixrat, as humidity_source says */
    const double *longwave;             /* [Ne] M_Qlw_in or M_tcc, as longwave_source says */
} nxs_dyn_flux_atmosphere;
typedef struct nxs_dyn_flux_state {
    double *tice0, *tsurf_young;        /* [Ne] M_tice[0], M_tsurf_young */
    double *sst, *sss;                  /* [Ne] M_sst, M_sss */
    double *drag_ti, *drag_ti_young;    /* [Ne] M_drag_ti, M_drag_ti_young (M_drag_ui and M_drag_ui_young are members of nxs_dyn_state) */
    double *pond_fraction, *lid_volume; /* [Ne] D_pond_fraction, M_lid_volume */
} nxs_dyn_flux_state;
enum { NXS_FLUX_QOW = 0, NXS_FLUX_QLW_OW, NXS_FLUX_QSW_OW, NXS_FLUX_QLH_OW, NXS_FLUX_QSH_OW, NXS_FLUX_EVAP, NXS_FLUX_TAU_OW,
       NXS_FLUX_QIA, NXS_FLUX_QLWI, NXS_FLUX_QSWI, NXS_FLUX_QLHI, NXS_FLUX_QSHI, NXS_FLUX_I, NXS_FLUX_SUBL, NXS_FLUX_DQIADT, NXS_FLUX_ALBEDO,
       NXS_FLUX_QIA_YOUNG, NXS_FLUX_QLW_YOUNG, NXS_FLUX_QSW_YOUNG, NXS_FLUX_QLH_YOUNG, NXS_FLUX_QSH_YOUNG, NXS_FLUX_I_YOUNG, NXS_FLUX_SUBL_YOUNG,
       NXS_FLUX_DQIADT_YOUNG, NXS_FLUX_ALBEDO_YOUNG };
#define NXS_FLUX_ROWS 25
typedef struct nxs_dyn_flux_rows { double *row[NXS_FLUX_ROWS]; } nxs_dyn_flux_rows;   /* [Ne] each, indexed by NXS_FLUX_* */

NXS_API int nxs_flux_default_config(nxs_dyn_flux_config *c);
NXS_API int nxs_flux_config_check(const nxs_dyn_flux_config *c);
NXS_API int nxs_flux_constants(double *out, int32_t count);
NXS_API int nxs_dyn_flux_configure(nxs_dyn_handle *h, const nxs_dyn_flux_config *c);
NXS_API int nxs_dyn_flux_set_atmosphere(nxs_dyn_handle *h, const nxs_dyn_flux_atmosphere *a);
NXS_API int nxs_dyn_flux_put(nxs_dyn_handle *h, const nxs_dyn_flux_state *s);
NXS_API int nxs_dyn_flux_get(nxs_dyn_handle *h, nxs_dyn_flux_state *s);
NXS_API int nxs_dyn_fluxes(nxs_dyn_handle *h);
NXS_API int nxs_dyn_fluxes_get(nxs_dyn_handle *h, const nxs_dyn_flux_rows *out /* may be NULL */, const double **device_rows /* [NXS_FLUX_ROWS], may be NULL */);

/* ---- The ice columns of thermo()'s slab loop on the device: its sections 3.2 to 5 (FE.cpp:5306-5411) -- the snowfall rule (FE.cpp:5321-5332), the ocean nudging
 * flux (FE.cpp:5343-5366), iceOceanHeatflux (FE.cpp:6396-6428, BASIC and EXCHANGE), freezingPoint (FE.cpp:6432-6448, LINEAR and UNESCO), thermoWinton
 * (FE.cpp:6633-6853) or thermoIce0 (FE.cpp:6860-6962) for the old ice and, in the young-ice category, thermoIce0 for the young ice with the stores
 * M_h_young = hi_young*old_conc_young, M_hs_young = hs_young*old_conc_young (FE.cpp:5409-5410).  One launch, a thread per element, ghost elements included.  It
 * reads the rows of nxs_dyn_fluxes (Qia, dQiadT, I, subl and their _young twins), M_conc, M_thick, M_snow_thick, M_conc_young, M_h_young, M_hs_young (resident),
 * M_tice[0], M_tsurf_young, M_sst, M_sss (the device copies of nxs_dyn_flux_state: ONE copy that both launches use), M_tair (nxs_dyn_flux_set_atmosphere), and under
 * EXCHANGE M_VT and M_ocean at the element's three nodes.  It writes NXS_COL_ROWS rows for sections 6 to 10 and, IN PLACE, M_tice[0] (under WINTON also M_tice[1],
 * M_tice[2]) and in the young-ice category M_tsurf_young, M_h_young, M_hs_young -- the last two are rows of nxs_dyn_state, so the next nxs_dyn_step reads them.
 * While a coupled ocean is attached (nxs_dyn_ocean_coupled_attach, below) the launch runs the reference's OceanType::COUPLED branch (FE.cpp:5348-5358) whatever
 * ocean_type was configured: Qdw = Fdw = 0 and M_sst, M_sss are reset IN PLACE to the received ocean_temp, ocean_salt before iceOceanHeatflux and freezingPoint read
 * them; the configuration itself still refuses NXS_COL_OCEAN_COUPLED (the coupled ocean is an attachment, not an option).
 * OUT OF SCOPE: thermo() from FE.cpp:5413 on (the assimilation flux, new ice, lateral melt, redistributeThermoFSD, meltPonds, the slab ocean, healing, diagnostics,
 * tracers), Winton's LOG(WARNING) and assert.
 *   nxs_col_default_config    model/options.cpp:112, 291-293, 383-420; snowfall from precip*snowfr, the constant mixed layer depth
 *   nxs_col_config_check      what nxs_dyn_column_configure refuses, without a handle: an unknown enum value, snow_cond, constant_mld, nudge_timeT or nudge_timeS
 *                  <= 0 (or NaN), the coupled ocean; NXS_ERR_INVALID, the text in nxs_dyn_last_error(NULL)
 *   nxs_col_constants         TEST DOOR like nxs_flux_constants: the physical:: constants compiled into the kernel, in the order NXS_COL_CONST_* names them
 *   nxs_dyn_column_configure  the configuration is the handle's and survives nxs_dyn_set_mesh
 *   nxs_dyn_column_set_forcing   [Ne] host rows; a NULL row means "the device copy is current" (a row never given stays missing).  Which rows the launch NEEDS
 *                  follows from the configuration: precip unless snowfall_source is SNOWFALL, snow unless it is PRECIP_TAIR, ocean_temp and ocean_salt under a
 *                  nudged ocean, mld under NXS_COL_MLD_ROW
 *   nxs_dyn_column_put / nxs_dyn_column_get_state   the rows of M_tice the fluxes do not carry (tice1, tice2); NULL members as in nxs_dyn_flux_put / _get
 *   nxs_dyn_column            the launch, asynchronous on the handle's stream; dt is thermo()'s integer argument (ddt = double(dt); BASIC divides by it as
 *                  FE.cpp:6410 does).  NXS_ERR_INVALID: dt <= 0.  NXS_ERR_STATE: before nxs_dyn_column_configure, before the first nxs_dyn_fluxes since the last
 *                  nxs_dyn_set_mesh / nxs_dyn_regrid, while a needed row is missing (again the state after set_mesh and after regrid: the forcing rows
 *                  always, tice1 / tice2 unless nxs_dyn_regrid_carry_thermo carried them), under WINTON without tice1 / tice2
 *   nxs_dyn_column_get        exactly like nxs_dyn_fluxes_get.  In the classic category the nine _young rows are zero.  NXS_ERR_STATE before the first nxs_dyn_column */
enum { NXS_COL_THERMO_ZERO_LAYER = 0, NXS_COL_THERMO_WINTON = 1 };                 /* setup::ThermoType */
enum { NXS_COL_QIO_BASIC = 0, NXS_COL_QIO_EXCHANGE = 1 };                          /* setup::OceanHeatfluxScheme */
enum { NXS_COL_FREEZINGPOINT_LINEAR = 0, NXS_COL_FREEZINGPOINT_UNESCO = 1 };       /* setup::FreezingPointType */
enum { NXS_COL_OCEAN_CONSTANT = 0, NXS_COL_OCEAN_NUDGED = 1, NXS_COL_OCEAN_COUPLED = 7 };   /* setup::OceanType: CONSTANT, any nudged dataset (TOPAZ4R = 1 ...), COUPLED (refused as an option: nxs_dyn_ocean_coupled_attach) */
enum { NXS_COL_SNOWFALL_PRECIP_SNOWFR = 0 /* M_precip*M_snowfr */, NXS_COL_SNOWFALL_SNOWFALL = 1 /* M_snowfall */, NXS_COL_SNOWFALL_PRECIP_TAIR = 2 /* M_precip where M_tair < 0 */ };
enum { NXS_COL_MLD_CONSTANT = 0 /* ideal_simul.constant_mld */, NXS_COL_MLD_ROW = 1 /* M_mld */ };
enum { NXS_COL_CONST_RHOW = 0, NXS_COL_CONST_CPW, NXS_COL_CONST_RHOI, NXS_COL_CONST_RHOS, NXS_COL_CONST_LF, NXS_COL_CONST_C, NXS_COL_CONST_KI, NXS_COL_CONST_SI,
       NXS_COL_CONST_HMIN, NXS_COL_CONST_COUNT };
typedef struct nxs_dyn_column_config {
    int32_t thermo_type;               /* NXS_COL_THERMO_*: setup.thermo-type */
    int32_t qio_type;                  /* NXS_COL_QIO_*: thermo.Qio-type */
    int32_t freezingpoint_type;        /* NXS_COL_FREEZINGPOINT_*: thermo.freezingpoint-type */
    int32_t ocean_type;                /* NXS_COL_OCEAN_*: setup.ocean-type */
    int32_t snowfall_source;           /* NXS_COL_SNOWFALL_*: which of M_snowfr, M_snowfall the dataset initialised (FE.cpp:5323-5329) */
    int32_t mld_source;                /* NXS_COL_MLD_* (FE.cpp:5335) */
    int32_t flooding;                  /* thermo.flooding */
    int32_t reserved;
    double freezingpoint_mu;           /* thermo.freezingpoint_mu */
    double snow_cond;                  /* thermo.snow_cond (M_ks) */
    double Csens_io;                   /* thermo.Csens_io */
    double constant_mld;               /* ideal_simul.constant_mld [m] */
    double nudge_timeT, nudge_timeS;   /* days_in_sec * thermo.ocean_nudge_timeT_days, _timeS_days [s] */
    double Qdw_const, Fdw_const;       /* ideal_simul.constant_Qdw, constant_Fdw */
} nxs_dyn_column_config;
typedef struct nxs_dyn_column_forcing {
    const double *precip;               /* [Ne] M_precip */
    const double *snow;                 /* [Ne] M_snowfr or M_snowfall, as snowfall_source says */
    const double *ocean_temp, *ocean_salt; /* [Ne] M_ocean_temp, M_ocean_salt */
    const double *mld;                  /* [Ne] M_mld */
} nxs_dyn_column_forcing;
typedef struct nxs_dyn_column_state {
    double *tice1, *tice2;              /* [Ne] M_tice[1], M_tice[2] (WINTON) */
} nxs_dyn_column_state;
enum { NXS_COL_SNOWFALL = 0, NXS_COL_QDW, NXS_COL_FDW, NXS_COL_TFRW,
       NXS_COL_QIO, NXS_COL_HI, NXS_COL_HS, NXS_COL_HI_OLD, NXS_COL_DEL_HI, NXS_COL_DEL_HS_MLT, NXS_COL_MLT_HI_TOP, NXS_COL_MLT_HI_BOT, NXS_COL_DEL_HI_S2I,
       NXS_COL_QIO_YOUNG, NXS_COL_HI_YOUNG, NXS_COL_HS_YOUNG, NXS_COL_HI_YOUNG_OLD, NXS_COL_DEL_HI_YOUNG, NXS_COL_DEL_HS_YOUNG_MLT, NXS_COL_MLT_HI_TOP_YOUNG,
       NXS_COL_MLT_HI_BOT_YOUNG, NXS_COL_DEL_HI_S2I_YOUNG };
#define NXS_COL_ROWS 22
typedef struct nxs_dyn_column_rows { double *row[NXS_COL_ROWS]; } nxs_dyn_column_rows;   /* [Ne] each, indexed by NXS_COL_* */

NXS_API int nxs_col_default_config(nxs_dyn_column_config *c);
NXS_API int nxs_col_config_check(const nxs_dyn_column_config *c);
NXS_API int nxs_col_constants(double *out, int32_t count);
NXS_API int nxs_dyn_column_configure(nxs_dyn_handle *h, const nxs_dyn_column_config *c);
NXS_API int nxs_dyn_column_set_forcing(nxs_dyn_handle *h, const nxs_dyn_column_forcing *f);
NXS_API int nxs_dyn_column_put(nxs_dyn_handle *h, const nxs_dyn_column_state *s);
NXS_API int nxs_dyn_column_get_state(nxs_dyn_handle *h, nxs_dyn_column_state *s);
NXS_API int nxs_dyn_column(nxs_dyn_handle *h, int32_t dt);
NXS_API int nxs_dyn_column_get(nxs_dyn_handle *h, const nxs_dyn_column_rows *out /* may be NULL */, const double **device_rows /* [NXS_COL_ROWS], may be NULL */);

/* ---- thermo()'s element forcing on the device: the ten rows of nxs_dyn_flux_atmosphere and nxs_dyn_column_forcing without a host -> device copy per step.  A
 * dataset interpolated linearly in time changes its bits EVERY model step (M_tair.getVector() evaluates ExternalData::get, model/externaldata.cpp:324-439, for the
 * current time), so a host that goes through nxs_dyn_flux_set_atmosphere / nxs_dyn_column_set_forcing uploads ten [Ne] rows per step.  Here both snapshots of a
 * forcing interval (dataset->variables[].interpolated_data[0] and [1]) become resident once per interval -- from host rows (nxs_dyn_thermo_forcing_pair) or from
 * the source grid by the device's InterpFromGridToMeshx at the element barycentres (nxs_dyn_thermo_forcing_targets + _ingest: the arithmetic of
 * nxs_interp_grid_to_mesh, the same bits) -- and every step one launch (nxs_dyn_thermo_forcing_time) evaluates ExternalData::get's expression into the SAME device
 * rows the two old calls fill: nxs_dyn_fluxes, nxs_dyn_column, nxs_dyn_slab, nxs_dyn_slab_coupled and nxs_dyn_means_update read them unchanged, and a handle that
 * never calls these entry points is the library without them.  Rows in the fixed order NXS_TF_*: the first five are nxs_dyn_flux_atmosphere's members, the last
 * five nxs_dyn_column_forcing's; what humidity, longwave and snow MEAN is still chosen by the flux and column configurations.
 * MEMORY: the snapshots, the targets and the uploaded grid (axes and data) are one pool of their own that goes with the mesh: nxs_dyn_set_mesh and nxs_dyn_regrid
 * drop it (the reference sets interpolated = false after a regrid too) and the host gives targets and snapshots again on the new mesh.  Twenty snapshot rows are
 * 20 * 8 B * Ne: 233 MB on the 2 km mesh (Ne = 1 456 798).
 *   nxs_dyn_thermo_forcing_pair     [Ne] host rows of snapshot 0 (s0) and 1 (s1).  A NULL row means "that snapshot's device copy is current"; s1 may be NULL as
 *                  a whole.  A row may exist with snapshot 0 only (a `constant` or `nearest_daily` dataset); a row never given stays missing.
 *                  NXS_ERR_INVALID: h or s0 NULL.  NXS_ERR_STATE before nxs_dyn_set_mesh
 *   nxs_dyn_thermo_forcing_time     per row its own mode, coefficients, M_factor and M_bias_correction (every ExternalData has its own dataset, so its own
 *                  ftime_range): NXS_TF_OFF leaves the row alone (the host still gives it through the old calls), NXS_TF_LINEAR writes
 *                  factor*(fcoeff0*d0[i] + fcoeff1*d1[i]) + bias (externaldata.cpp:401-403, 438), NXS_TF_STEP writes factor*d0[i] + bias (externaldata.cpp:434, 438)
 *                  and never reads d1 -- it is NOT LINEAR with (1, 0): those differ in the sign of zero and where d1 holds NaN or Inf.  One asynchronous launch on
 *                  the handle's stream; the written rows then count as given on this mesh, exactly as after an upload.  NXS_ERR_INVALID: h or t NULL, an
 *                  unknown mode.  NXS_ERR_STATE: before nxs_dyn_set_mesh, a LINEAR row without both snapshots, a STEP row without snapshot 0 (which is every
 *                  row after nxs_dyn_set_mesh / nxs_dyn_regrid)
 *   nxs_dyn_thermo_forcing_targets  [Ne] element barycentres in the coordinates of dataset `set` (0 .. NXS_TF_SETS - 1: atmosphere, ocean, a third product) --
 *                  what convertTargetXY made: the projection stays the host's.  Resident until the mesh changes.  NXS_ERR_INVALID: a NULL argument, a set out
 *                  of range.  NXS_ERR_STATE before nxs_dyn_set_mesh
 *   nxs_dyn_thermo_forcing_ingest   the grid descriptor and data ([M][N][N_data], or [N][M][N_data] with row_major) mean exactly what nxs_interp_grid_to_mesh's
 *                  arguments mean (include/nxs_interp.h).  Column j goes to snapshot snapshot[j] (0 or 1) of row row[j] (NXS_TF_*); row[j] = -1 skips the
 *                  column: the nb_var*nb_forcing_step columns of one InterpFromGridToMeshx call of loadDataset are taken as they lie.  One launch, a thread
 *                  per element, one contiguous [Ne] stream per column; the host arrays are free on return, the launch is asynchronous.  NXS_ERR_INVALID: a
 *                  NULL argument, a set out of range, M or N < 2, N_data outside 1 .. NXS_TF_MAX_COLUMNS, axes that are neither centres nor contours, an unknown
 *                  interpolation, a row outside -1 .. NXS_TF_ROWS - 1, a snapshot other than 0 / 1, two columns for one snapshot of one row.  NXS_ERR_STATE:
 *                  before nxs_dyn_set_mesh, before nxs_dyn_thermo_forcing_targets of that set on this mesh
 *   nxs_dyn_thermo_forcing_get      which = 0 / 1: the snapshots; which = 2: the rows as the launches will read them (blended or uploaded, whichever came
 *                  last).  Synchronised on return; NULL rows are skipped; a missing row that is asked for is NXS_ERR_STATE.  The tests' door and a restart
 *                  writer's.  NXS_ERR_INVALID: h or out NULL, which outside 0 .. 2 */
enum { NXS_TF_TAIR = 0, NXS_TF_MSLP, NXS_TF_QSW_IN, NXS_TF_HUMIDITY, NXS_TF_LONGWAVE, NXS_TF_PRECIP, NXS_TF_SNOW, NXS_TF_OCEAN_TEMP, NXS_TF_OCEAN_SALT, NXS_TF_MLD };
#define NXS_TF_ROWS 10
#define NXS_TF_SETS 4
#define NXS_TF_MAX_COLUMNS 32
enum { NXS_TF_OFF = 0, NXS_TF_LINEAR = 1, NXS_TF_STEP = 2 };
typedef struct nxs_dyn_thermo_forcing_rows { double *row[NXS_TF_ROWS]; } nxs_dyn_thermo_forcing_rows;   /* [Ne] each, indexed by NXS_TF_* (read by _pair, written by _get) */
/* (a struct TAG only: the entry point of the same name is the ordinary identifier, so C and C++ callers write `struct nxs_dyn_thermo_forcing_time`) */
struct nxs_dyn_thermo_forcing_time {
    int32_t mode[NXS_TF_ROWS];          /* NXS_TF_OFF / _LINEAR / _STEP */
    double fcoeff0[NXS_TF_ROWS];        /* |t - ftime_range[1]| / fdt of the row's dataset (LINEAR) */
    double fcoeff1[NXS_TF_ROWS];        /* |t - ftime_range[0]| / fdt */
    double factor[NXS_TF_ROWS];         /* M_factor */
    double bias[NXS_TF_ROWS];           /* M_bias_correction */
};
typedef struct nxs_dyn_forcing_grid {   /* the source grid of one dataset: the arguments of nxs_interp_grid_to_mesh */
    const double *x_in, *y_in;          /* pixel centres (x_rows == N, y_rows == M) or their contours (one more entry each) */
    int32_t x_rows, y_rows;
    int32_t M, N;                       /* rows (y) and columns (x) of data */
    int32_t interp;                     /* NXS_INTERP_TRIANGLE / _BILINEAR / _NEAREST (include/nxs_interp.h: 0 / 1 / 2) */
    int32_t row_major;                  /* 0: data [M][N][N_data]; else [N][M][N_data] */
    double default_value;               /* NaN and targets outside the grid */
} nxs_dyn_forcing_grid;

NXS_API int nxs_dyn_thermo_forcing_pair(nxs_dyn_handle *h, const nxs_dyn_thermo_forcing_rows *s0, const nxs_dyn_thermo_forcing_rows *s1 /* may be NULL */);
NXS_API int nxs_dyn_thermo_forcing_time(nxs_dyn_handle *h, const struct nxs_dyn_thermo_forcing_time *t);
NXS_API int nxs_dyn_thermo_forcing_targets(nxs_dyn_handle *h, int32_t set, const double *RX, const double *RY);
NXS_API int nxs_dyn_thermo_forcing_ingest(nxs_dyn_handle *h, int32_t set, const nxs_dyn_forcing_grid *g, const double *data, int32_t N_data, const int32_t *row,
                                          const int32_t *snapshot);
NXS_API int nxs_dyn_thermo_forcing_get(nxs_dyn_handle *h, int32_t which, const nxs_dyn_thermo_forcing_rows *out);

/* ---- The dynamics' nodal forcing on the device: both snapshots of M_wind, M_ocean and M_ssh made FROM THE SOURCE GRID without the host's transformData,
 * wrap and InterpFromGridToMeshx (ExternalData::loadDataset, model/externaldata.cpp:461-940), and a time blend with coefficients per dataset.  Everything here
 * is additive: a handle that never calls these entry points allocates and launches nothing new, and nxs_dyn_set_forcing / _pair / _time keep their bits.
 *
 * THE PROJECTION.  nxs_mapx_polar holds the derived constants forward_mapx reads for a north-aspect "Polar Stereographic Ellipsoid" map;
 * nxs_mapx_polar_north (host only) forms them from what an .mpp file holds -- init_polar_stereographic_ellipsoid (contrib/mapx/src/polar_stereographic.c:89-134)
 * and the tail of reinit_mapx (contrib/mapx/src/mapx.c:1011-1064: the rotation matrix, x0 / y0 from the centre, u0 / v0), operand for operand; lat1 == 999 means
 * lat0, as there; false easting / northing and maximum_error are 0, as new_mapx leaves them for such a file.  NXS_ERR_INVALID: out NULL, lat0 != 90.
 * nxs_mapx_forward runs forward_mapx on n points: device >= 0 on that device (one launch, arrays copied there and back), device < 0 the same source on the host.
 * NXS_ERR_INVALID: a NULL argument, n < 0.  nxs_mapx_constants is a TEST DOOR like nxs_dyn_physical_constants: mapx_Re_km and PI of contrib/mapx/include/mapx.h
 * as compiled into the kernels, in the order NXS_MAPX_CONST_*.
 *
 * THE INGEST.  nxs_dyn_forcing_targets gives the [Nn] node positions in the coordinates of dataset `set` (convertTargetXY's output: the projection of the targets
 * stays the host's); resident until the mesh changes.  nxs_dyn_forcing_ingest takes the data of one InterpFromGridToMeshx call, [M][N][N_data] (or [N][M][N_data]
 * with row_major), UNTRANSFORMED AND WITHOUT THE WRAP, uploads them and runs on the device, in the reference's order:
 *   transformData (externaldata.cpp:944-1288) for the column pairs `vectors` names: the east/north branch (:1155-1204) where east_west_oriented, the mean over the
 *     row beside a row at 90N (:1206-1243; y[0] == 90. or y[M-1] == 90. of the pixel centres, the last wins), the rotation by cos / sin(-rotation_angle) as the
 *     host computed them (:1246-1261) where `rotate`.  A pair is two COLUMNS of data (variable j of snapshot fstep is column fstep*nb_var + j in loadDataset's
 *     call), so two snapshots of one vector are two pairs.  vectors == NULL: no transform.
 *   interpolateDataset's wrap (:1315-1373): cyclic_x appends column N = column 0 and x[N-1] + (x[N-1] - x[N-2]) to the centres, cyclic_y the same with a row; the
 *     corner cell when both are set holds 0., as the reference's zero-initialised vector does.
 *   InterpFromGridToMeshx at the nodes (:1436): the arithmetic of nxs_interp_grid_to_mesh, the same bits.  Column j goes to snapshot snapshot[j] (0 or 1) of row
 *     row[j] (NXS_NF_*); row[j] = -1 skips the column.  The rows ARE the snapshots nxs_dyn_set_forcing_pair owns (V at offset Nn of the [2*Nn] vector), made here
 *     when the pair was never given; the two routes mix per half-row, and nxs_dyn_set_forcing_time / _time_rows see a pair once all ten half-rows have been given on
 *     this mesh by either route.
 *   The host arrays are free on return; the launches are asynchronous.  NXS_ERR_INVALID: a NULL argument (vectors may be NULL), a set out of range, M or N < 2,
 *   N_data outside 1 .. NXS_NF_MAX_COLUMNS, axes that are neither centres nor contours, an unknown interpolation, a row outside -1 .. NXS_NF_ROWS - 1, a snapshot
 *   other than 0 / 1, two columns for one snapshot of one row, contours or row_major data with a cyclic axis; with vectors: n_pairs outside 0 .. NXS_NF_MAX_VECTORS, a pair naming a
 *   column out of range, skipped or named twice, row_major != 0, lat / lon NULL while a pair is east_west_oriented, is_wav_dir (the wave-direction branch) or
 *   gridded_rotation_angle without `rotate` (the OASIS branch) -- neither is built.  NXS_ERR_STATE: before nxs_dyn_set_mesh, before nxs_dyn_forcing_targets of that
 *   set on this mesh.
 * nxs_dyn_set_forcing_time_rows is nxs_dyn_set_forcing_time with its own mode (NXS_TF_OFF / _LINEAR / _STEP), coefficients, M_factor and M_bias_correction per group
 * {wind, ocean, ssh} (the reference's atmosphere and ocean are different datasets with different ftime_ranges): LINEAR writes factor*(fcoeff0*d0 + fcoeff1*d1) + bias
 * -- nxs_dyn_set_forcing_time's expression, the same bits --, STEP factor*d0 + bias without reading d1, OFF leaves the vector alone.  One asynchronous launch.
 * NXS_ERR_INVALID: h or t NULL, an unknown mode.  NXS_ERR_STATE: before nxs_dyn_set_mesh, a LINEAR group without both snapshots, a STEP group without snapshot 0.
 * The step's forcing counts as given once wind, ocean and ssh have been written this way (or by the older calls) AND the element depth is there.
 * nxs_dyn_set_element_depth uploads the constant [Ne] row alone, so a host on this route never needs nxs_dyn_set_forcing_pair.
 * nxs_dyn_forcing_get (tests, a restart writer) returns the named half-rows of snapshot `which` (0 / 1), [Nn] each; NULL rows are skipped, a missing row that is
 * asked for is NXS_ERR_STATE.  nxs_dyn_debug_array "nf_grid" returns the last ingest's grid data after transform and wrap, [cM][cN][N_data].
 * MEMORY: the snapshots stay nxs_dyn_set_forcing_pair's (10 * 8 B * Nn); the targets (2 * 8 B * Nn per set) and the uploaded grid are a pool of their own that
 * goes with the mesh: nxs_dyn_set_mesh and nxs_dyn_regrid drop it. */
typedef struct nxs_mapx_polar {
    double lon0, Rg, m1, t1, eccentricity, scale, lat1;
    double T00, T01, T10, T11, u0, v0, false_easting, false_northing;
} nxs_mapx_polar;
enum { NXS_MAPX_CONST_RE_KM = 0, NXS_MAPX_CONST_PI, NXS_MAPX_CONST_COUNT };
NXS_API int nxs_mapx_constants(double *out, int32_t count);
NXS_API int nxs_mapx_polar_north(double lat0, double lon0, double lat1, double rotation, double scale, double center_lat, double center_lon, double equatorial_radius,
                                 double eccentricity, nxs_mapx_polar *out);
NXS_API int nxs_mapx_forward(const nxs_mapx_polar *map, int64_t n, const double *lat, const double *lon, double *x, double *y, int32_t device);

enum { NXS_NF_WIND_U = 0, NXS_NF_WIND_V, NXS_NF_OCEAN_U, NXS_NF_OCEAN_V, NXS_NF_SSH };
#define NXS_NF_ROWS 5
#define NXS_NF_SETS 4
#define NXS_NF_MAX_COLUMNS 32
#define NXS_NF_MAX_VECTORS 4
enum { NXS_NF_GROUP_WIND = 0, NXS_NF_GROUP_OCEAN, NXS_NF_GROUP_SSH };
#define NXS_NF_GROUPS 3
typedef struct nxs_dyn_forcing_vectors {   /* dataset->vectorial_variables and what transformData reads beside them */
    int32_t n_pairs;
    int32_t component0[NXS_NF_MAX_VECTORS], component1[NXS_NF_MAX_VECTORS];   /* the two columns of data of each pair */
    int32_t east_west_oriented[NXS_NF_MAX_VECTORS];
    int32_t is_wav_dir[NXS_NF_MAX_VECTORS];                                   /* wavDirOptions.isWavDir: not built */
    int32_t gridded_rotation_angle;                                           /* grid.gridded_rotation_angle (#ifdef OASIS): not built */
    int32_t latlon_per_point;              /* 0: lat[M], lon[N] (a regular lat-lon grid); else lat[M*N], lon[M*N] */
    int32_t rotate;                        /* dataset->rotation_angle != 0. */
    const double *lat, *lon;               /* degrees; may be NULL when no pair is east_west_oriented */
    nxs_mapx_polar map;                    /* the model's projection (Environment::nextsimMppfile) */
    double cos_m_diff_angle, sin_m_diff_angle;   /* std::cos(-rotation_angle), std::sin(-rotation_angle) */
} nxs_dyn_forcing_vectors;
typedef struct nxs_dyn_forcing_rows { double *row[NXS_NF_ROWS]; } nxs_dyn_forcing_rows;   /* [Nn] each, indexed by NXS_NF_* */
/* (a struct TAG only, as nxs_dyn_thermo_forcing_time) */
struct nxs_dyn_forcing_time_rows {
    int32_t mode[NXS_NF_GROUPS];           /* NXS_TF_OFF / _LINEAR / _STEP per NXS_NF_GROUP_* */
    double fcoeff0[NXS_NF_GROUPS];         /* |t - ftime_range[1]| / fdt of the group's dataset (LINEAR) */
    double fcoeff1[NXS_NF_GROUPS];         /* |t - ftime_range[0]| / fdt */
    double factor[NXS_NF_GROUPS];          /* M_factor */
    double bias[NXS_NF_GROUPS];            /* M_bias_correction */
};
NXS_API int nxs_dyn_forcing_targets(nxs_dyn_handle *h, int32_t set, const double *RX, const double *RY);
NXS_API int nxs_dyn_forcing_ingest(nxs_dyn_handle *h, int32_t set, const nxs_dyn_forcing_grid *g, int32_t cyclic_x, int32_t cyclic_y, const double *data, int32_t N_data,
                                   const int32_t *row, const int32_t *snapshot, const nxs_dyn_forcing_vectors *vectors /* may be NULL */);
NXS_API int nxs_dyn_set_forcing_time_rows(nxs_dyn_handle *h, const struct nxs_dyn_forcing_time_rows *t);
NXS_API int nxs_dyn_set_element_depth(nxs_dyn_handle *h, const double *depth);
NXS_API int nxs_dyn_forcing_get(nxs_dyn_handle *h, int32_t which, const nxs_dyn_forcing_rows *out);

/* ---- Nesting on the device: nestingIce() (FE.cpp:4878-4908) and nestingDynamics() (FE.cpp:4915-4958), the two statements FiniteElement::step() runs between
 * thermo() and the dynamics under nesting.use_nesting (FE.cpp:8172-8192).  Per entry x += (fNudge*(time_step/nudge_time)*(target - x)), with target =
 * ExternalData::get of the nesting dataset (externaldata.cpp:366-438, the semantics of nxs_dyn_thermo_forcing_time) evaluated in the same kernel from both resident
 * snapshots, and fNudge = 1. - std::min(1., dist/nudge_scale) (NXS_NUDGE_LINEAR) or std::exp(-dist/nudge_scale) (NXS_NUDGE_EXPONENTIAL).  All M_num_elements and
 * M_num_nodes are updated, ghosts included; nothing is exchanged, so both calls work on a handle with halo lists.  Nothing runs unless these entry points are
 * called: no allocation at nxs_dyn_set_mesh, no launch in nxs_dyn_step.
 * IN PLACE: between two steps M_sigma / M_damage are current either in their arrays or in the 4-double records the sub-step loop left behind;
 * nxs_dyn_nesting_dynamics nudges them where they are (no unpack now, no pack in the next step).  Under EVP / mEVP the records hold no damage: M_damage is nudged in
 * its array.  M_VT is nudged in the array nxs_dyn_get_state reads.
 *   nxs_nesting_config_check    what nxs_dyn_nesting_configure refuses, without a handle (the text: nxs_dyn_last_error(NULL)): nudge_function other than
 *                  NXS_NUDGE_LINEAR / _EXPONENTIAL (the reference throws, FE.cpp:4886-4888); nudge_timescale, nudge_scale not finite or <= 0; dtime_step not finite
 *   nxs_dyn_nesting_configure   the configuration is the handle's and survives nxs_dyn_set_mesh.  time_step is the model's int, dtime_step its double: the element
 *                  rows and all of nestingIce use (double)time_step / nudge_timescale, M_VT dtime_step / nudge_timescale (FE.cpp:4954-4955); both quotients are
 *                  formed once, here.  nudge_scale = M_nudge_lengthscale * M_res_root_mesh
 *   nxs_dyn_nesting_pair        host rows of snapshot 0 (s0) and 1 (s1, may be NULL) of a nesting interval: [Ne] element rows in the order of forcingNesting()
 *                  (FE.cpp:11062-11111), [Nn] nodal rows (FE.cpp:11113-11121).  A NULL row means "not given".  The rows go with the mesh: gone after
 *                  nxs_dyn_set_mesh and nxs_dyn_regrid.  NXS_ERR_STATE before nxs_dyn_set_mesh
 *   nxs_dyn_nesting_time        per DATASET (NXS_NEST_DS_*: the five of FE.cpp:822-827 without the ocean one) mode NXS_TF_LINEAR / NXS_TF_STEP (NXS_TF_OFF: a
 *                  dataset that is not read), fcoeff0, fcoeff1, M_factor, M_bias_correction.  The handle's; no launch.  NXS_ERR_INVALID: an unknown mode
 *   nxs_dyn_nesting_ice         one launch on the handle's stream: M_conc, M_thick, M_snow_thick, and M_conc_young, M_h_young, M_hs_young when the handle's
 *                  ice_cat_type is YOUNG_ICE (only then are the young-ice rows required).  NXS_ERR_STATE: no configuration, no time, no state, a dataset OFF that
 *                  is read, a required row (both snapshots under LINEAR, snapshot 0 under STEP) missing on this mesh -- the message names the row
 *   nxs_dyn_nesting_dynamics    one launch: M_sigma[0..2], M_damage, M_ridge_ratio per element, M_VT per node.  As above; NXS_ERR_STATE also when the configuration's
 *                  nest_dynamic_vars is 0
 *   nxs_dyn_nesting_get         which = 0 / 1: the snapshots back to the host (NULL rows are skipped; a missing row that is asked for is NXS_ERR_STATE).  The
 *                  tests' door */
enum { NXS_NEST_DIST = 0, NXS_NEST_THICK, NXS_NEST_CONC, NXS_NEST_SNOW_THICK, NXS_NEST_H_YOUNG, NXS_NEST_CONC_YOUNG, NXS_NEST_HS_YOUNG,
       NXS_NEST_SIGMA1, NXS_NEST_SIGMA2, NXS_NEST_SIGMA3, NXS_NEST_DAMAGE, NXS_NEST_RIDGE_RATIO };
#define NXS_NEST_ELEMENT_ROWS 12
enum { NXS_NEST_DIST_NODES = 0, NXS_NEST_VT1, NXS_NEST_VT2 };
#define NXS_NEST_NODE_ROWS 3
enum { NXS_NEST_DS_DISTANCE_ELEMENTS = 0, NXS_NEST_DS_ICE_ELEMENTS, NXS_NEST_DS_DYNAMICS_ELEMENTS, NXS_NEST_DS_DISTANCE_NODES, NXS_NEST_DS_NODES };
#define NXS_NEST_DATASETS 5
enum { NXS_NUDGE_LINEAR = 0, NXS_NUDGE_EXPONENTIAL = 1 };
typedef struct nxs_dyn_nesting_config {
    int32_t nudge_function;             /* NXS_NUDGE_LINEAR / NXS_NUDGE_EXPONENTIAL (nesting.nudge_function) */
    int32_t nest_dynamic_vars;          /* nesting.nest_dynamic_vars: nxs_dyn_nesting_dynamics may be called */
    int32_t time_step;                  /* the model's int time_step (s) */
    int32_t reserved0;
    double nudge_timescale;             /* M_nudge_timescale (s) */
    double nudge_scale;                 /* M_nudge_lengthscale * M_res_root_mesh (m) */
    double dtime_step;                  /* the model's double dtime_step (s) */
} nxs_dyn_nesting_config;
typedef struct nxs_dyn_nesting_rows {
    double *element[NXS_NEST_ELEMENT_ROWS];   /* [Ne] each, indexed by NXS_NEST_* (read by _pair, written by _get) */
    double *node[NXS_NEST_NODE_ROWS];         /* [Nn] each, indexed by NXS_NEST_DIST_NODES .. NXS_NEST_VT2 */
} nxs_dyn_nesting_rows;
/* (a struct TAG only, as nxs_dyn_thermo_forcing_time) */
struct nxs_dyn_nesting_time {
    int32_t mode[NXS_NEST_DATASETS];    /* NXS_TF_OFF / _LINEAR / _STEP per NXS_NEST_DS_* */
    int32_t reserved0;
    double fcoeff0[NXS_NEST_DATASETS];
    double fcoeff1[NXS_NEST_DATASETS];
    double factor[NXS_NEST_DATASETS];
    double bias[NXS_NEST_DATASETS];
};

NXS_API int nxs_nesting_config_check(const nxs_dyn_nesting_config *c);
NXS_API int nxs_dyn_nesting_configure(nxs_dyn_handle *h, const nxs_dyn_nesting_config *c);
NXS_API int nxs_dyn_nesting_pair(nxs_dyn_handle *h, const nxs_dyn_nesting_rows *s0, const nxs_dyn_nesting_rows *s1 /* may be NULL */);
NXS_API int nxs_dyn_nesting_time(nxs_dyn_handle *h, const struct nxs_dyn_nesting_time *t);
NXS_API int nxs_dyn_nesting_ice(nxs_dyn_handle *h);
NXS_API int nxs_dyn_nesting_dynamics(nxs_dyn_handle *h);
NXS_API int nxs_dyn_nesting_get(nxs_dyn_handle *h, int32_t which, const nxs_dyn_nesting_rows *out);

/* ---- Slab-ocean diffusion on the device: diffuse() (FE.cpp:2760-2815) for M_sst and M_sss, the first thing update() does whenever thermo.diffusivity_sst / _sss > 0
 * (FE.cpp:3938-3939).  One explicit Jacobi step over bamgmesh->ElementConnectivity: v[e] += f0 + f1 + f2 with fj = factor*(old[n_j] - old[e]), or 0. where the
 * element has no neighbour across edge j; every flux reads the OLD row.  An element without any neighbour still executes v += 0. + 0. + 0. (-0.0 becomes +0.0).
 * Neither explicitSolve() nor the element loop of update() reads or writes M_sst / M_sss, so nxs_dyn_diffuse right before nxs_dyn_step gives the reference's bits.
 *   nxs_dyn_diffusion_configure  factor = diffusivity * dtime_step / std::pow(dx, 2.) is formed here, on the host (FE.cpp:2775).  A diffusivity <= 0 switches that
 *                  field off (FE.cpp:2762).  The handle's; survives nxs_dyn_set_mesh.  NXS_ERR_INVALID: a non-finite argument, dx <= 0
 *   nxs_dyn_diffuse              works in place on the sst / sss rows of nxs_dyn_flux_state (their device addresses do not change): two launches -- {sst, sss}
 *                  packed into one [Ne] array of 16-byte pairs, then per element one index load and three gathers.  Both fields off: nothing is launched.  The
 *                  element-to-element table (ints [Ne][3], -1 on the boundary; debug array "diffuse_table", [3 Ne]) and the packed copy are made by the first call
 *                  after a mesh change and go with the mesh.  NXS_ERR_STATE: not configured, before nxs_dyn_set_mesh, sst or sss never put on this mesh, a
 *                  handle with halo lists (the reference diffuses on its root rank from gathered fields; no element-row exchange exists here)
 *   nxs_dyn_flux_device_rows     the DEVICE addresses of the eight rows of nxs_dyn_flux_state in its member order; NULL for a row never put on this mesh */
NXS_API int nxs_dyn_diffusion_configure(nxs_dyn_handle *h, double diffusivity_sst, double diffusivity_sss, double dx, double dtime_step);
NXS_API int nxs_dyn_diffuse(nxs_dyn_handle *h);
NXS_API int nxs_dyn_flux_device_rows(nxs_dyn_handle *h, const double **device_rows /* [8] */);

/* ---- A coupled ocean on the device: thermo() under OceanType::COUPLED (the reference's #ifdef OASIS, a neXtSIM-NEMO run).  The coupled ocean is ATTACHED to a
 * handle, the way the wave terms are; nxs_dyn_column_configure keeps refusing NXS_COL_OCEAN_COUPLED, and a handle that never calls these entry points allocates
 * nothing, launches nothing new and keeps its bits.  Each coupling step the reference runs ExternalData::check_and_reload for ocean_cpl_elements and
 * wave_cpl_elements (externaldata.cpp:163-236, 461-514, 1291-1493; dataset.cpp:2828-3031, 3219-3393): receiveCouplingData, ConservativeRemappingGridToMesh, get.
 * Here that is ONE launch (nxs_gridmap_receive_rows, include/nxs_interp.h) from the fields on the exchange grid to the [Ne] device rows thermo() reads -- no host
 * remap and no [Ne] upload.  The five rows:
 *   NXS_OC_OCEAN_TEMP, NXS_OC_OCEAN_SALT, NXS_OC_MLD   M_ocean_temp, M_ocean_salt, M_mld: the SAME device rows nxs_dyn_column_set_forcing and
 *                  nxs_dyn_thermo_forcing_time fill -- whichever came last wins, and the have-bits are set as after an upload
 *   NXS_OC_QSRML, NXS_OC_WLBK   M_qsrml (I_FrcQsr) and M_wlbk (I_wlbk): two rows of the attachment's own, in a pool that goes with the mesh
 * While a coupled ocean is attached with OCEAN_TEMP, OCEAN_SALT and QSRML configured, nxs_dyn_fluxes, nxs_dyn_column, nxs_dyn_slab and nxs_dyn_slab_coupled run
 * the reference's COUPLED statements (FE.cpp:5150-5157, 5348-5358, 5826-5841; see each of them above), nxs_dyn_column answers NXS_ERR_STATE unless
 * freezingpoint_type is UNESCO (FE.cpp:1244-1248: the reference overrides the option silently; a host that passes M_freezingpoint_type passes UNESCO), a needed
 * received row that is missing on this mesh is NXS_ERR_STATE naming the row, and nxs_dyn_diffuse answers NXS_ERR_STATE (FE.cpp:3934-3940).
 *   nxs_ocean_coupled_default_config   the reference's receive with coupler.rcv_first_layer_depth off and no wave model: I_SST, I_SSS, I_FrcQsr in that order,
 *                  a = 1, b = 0 (dataset.cpp), factor = 1, bias = 0.  (I_MLD: a = 1, b = 0; I_wlbk: a = 2, b = 0.)
 *   nxs_ocean_coupled_config_check     what the attach refuses in a configuration, without a handle: n_fields outside 1 .. NXS_OC_ROWS, an unknown row, a row twice
 *   nxs_dyn_ocean_coupled_attach   cfg names the rows that are received, in the order the fields arrive, with a, b, factor, bias per FIELD.  map is BORROWED (the
 *                  caller destroys it after the detach or the next nxs_dyn_set_mesh); NULL for a host that only uses _put_rows; otherwise its element count
 *                  must be the handle's (a partitioned run passes the nxs_gridmap_restrict-ed map): NXS_ERR_INVALID naming both sizes.  cfg == NULL DETACHES:
 *                  the two rows are freed and the handle is again the library without this section.  NXS_ERR_STATE before nxs_dyn_set_mesh.  nxs_dyn_set_mesh
 *                  and nxs_dyn_regrid DROP the attachment and the two rows: the map belonged to the old mesh, and the host builds new weights at rest as
 *                  FE.cpp:8037-8049 does.  nxs_dyn_regrid_carry_thermo still carries sst / sss as before
 *   nxs_dyn_ocean_coupled_receive  fields[k], k < n_fields: the [G] field of cfg.row[k] on the map's grid, host pointers or, with NXS_REGRID_IN_DEVICE, device
 *                  pointers.  One launch on the handle's stream: receive -> fluxes -> column needs no host synchronisation (host fields are uploaded on the
 *                  stream first and the call waits for those uploads).  A triangle no wet cell touches receives NaN, as in the reference.  NXS_ERR_STATE: not
 *                  attached, attached without a map
 *   nxs_dyn_ocean_coupled_put_rows the same five rows from host [Ne] arrays, a NULL row is skipped: the way in for a host that remapped itself.  NXS_ERR_INVALID
 *                  for a row the configuration does not name
 *   nxs_dyn_ocean_coupled_get      synchronised; [Ne] host rows, a NULL row is skipped, a row asked for that was never given on this mesh is NXS_ERR_STATE.
 *                  device_rows (may be NULL) [NXS_OC_ROWS]: the device addresses, NULL for a missing row -- device_rows[NXS_OC_WLBK] is what a host hands
 *                  nxs_dyn_fsd_breakup(..., NXS_FSD_WLBK_ON_DEVICE, ...)
 * The nodal half of the receive (I_Uocn, I_Vocn, I_SSH, I_tauwix / y: FromMeshToMeshQuick on a triangulated source, the gridTheta rotation of transformData) is
 * nxs_dyn_nodes_coupled_*, below.  OUT OF SCOPE: ocean_turning_angle = 0 (a parameter the host sets), the
 * reduction over ranks and the OASIS put of the outgoing side (its accumulators and grid: nxs_dyn_cpl_out_*), OASIS itself, reading and projecting the exchange
 * grid file, AEROBULK. */
enum { NXS_OC_OCEAN_TEMP = 0, NXS_OC_OCEAN_SALT = 1, NXS_OC_QSRML = 2, NXS_OC_MLD = 3, NXS_OC_WLBK = 4, NXS_OC_ROWS = 5 };
typedef struct nxs_dyn_ocean_coupled_config {
    int32_t n_fields;                  /* fields of one receive, 1 .. NXS_OC_ROWS */
    int32_t row[NXS_OC_ROWS];          /* row[k]: the NXS_OC_* row field k goes to; no row twice */
    double a[NXS_OC_ROWS], b[NXS_OC_ROWS];            /* receiveCouplingData: t = field; t *= a; t += b (per field k) */
    double factor[NXS_OC_ROWS], bias[NXS_OC_ROWS];    /* ExternalData::get: M_factor * x + M_bias_correction (per field k) */
} nxs_dyn_ocean_coupled_config;
typedef struct nxs_dyn_ocean_coupled_rows { double *row[NXS_OC_ROWS]; } nxs_dyn_ocean_coupled_rows;   /* [Ne] each, indexed by NXS_OC_* */
struct nxs_gridmap;   /* include/nxs_interp.h */
NXS_API int nxs_ocean_coupled_default_config(nxs_dyn_ocean_coupled_config *c);
NXS_API int nxs_ocean_coupled_config_check(const nxs_dyn_ocean_coupled_config *c);
NXS_API int nxs_dyn_ocean_coupled_attach(nxs_dyn_handle *h, struct nxs_gridmap *map /* may be NULL */, const nxs_dyn_ocean_coupled_config *c /* NULL: detach */);
NXS_API int nxs_dyn_ocean_coupled_receive(nxs_dyn_handle *h, const double *const *fields, int32_t flags);
NXS_API int nxs_dyn_ocean_coupled_put_rows(nxs_dyn_handle *h, const nxs_dyn_ocean_coupled_rows *rows);
NXS_API int nxs_dyn_ocean_coupled_get(nxs_dyn_handle *h, const nxs_dyn_ocean_coupled_rows *out /* may be NULL */, const double **device_rows /* [NXS_OC_ROWS], may be NULL */);

/* ---- The NODAL half of a coupled run's receive on the device: I_Uocn, I_Vocn, I_SSH of ocean_cpl_nodes and I_tauwix, I_tauwiy of wave_cpl_nodes through a node map
 * (nxs_nodemap_*, include/nxs_interp.h: InterpFromMeshToMesh2dx_weights once per mesh, _apply per coupling step; FE.cpp:7690-7697, 8041-8048, dataset.cpp:11157-11175,
 * externaldata.cpp:498-509, 944-1288, 1457-1463).  Everything here is additive: a handle that never attaches allocates nothing, launches nothing and keeps its bits.
 *   nxs_dyn_nodes_coupled_attach   which = NXS_NC_OCEAN or NXS_NC_WAVE: two datasets, two maps (their exchange grids may differ).  The map is BORROWED (the caller
 *                  keeps it alive and destroys it) and must have the handle's Nn targets, ghosts included, and a source (nxs_nodemap_set_source: reduced, the
 *                  rotation, lat / lon of an east/north pair).  c: a, b of receiveCouplingData and factor, bias of ExternalData::get per FIELD, in the order the
 *                  fields arrive; c == NULL detaches.  The attachment goes with the mesh: nxs_dyn_set_mesh and nxs_dyn_regrid drop it (the weights were the old
 *                  mesh's), attach the new map afterwards.
 *   nxs_dyn_nodes_coupled_receive  fields[k], k < n_fields: the [G] fields as OASIS delivers them, host pointers or, with NXS_REGRID_IN_DEVICE, device pointers.
 *                  Two launches on the handle's stream (k_nodemap_source, k_nodemap_gather), asynchronous; with device fields there is no host synchronisation.
 *                  NXS_NC_OCEAN: three fields, the vector (0, 1).  The interpolated values are stored RAW into snapshot 0 of the half-rows NXS_NF_OCEAN_U,
 *                  NXS_NF_OCEAN_V, NXS_NF_SSH -- the rows nxs_dyn_set_forcing_pair owns, marked as nxs_dyn_forcing_ingest marks them -- so that
 *                  nxs_dyn_set_forcing_time_rows with NXS_TF_STEP for the ocean and ssh groups IS ExternalData::get (factor and bias are that call's; the
 *                  attachment's are not read).  NXS_NC_WAVE: two fields, the vector (0, 1); factor*x + bias goes straight into the handle's M_tau_wi [u | v], which
 *                  is attached exactly as nxs_dyn_set_wave_stress(h, non-NULL) attaches it: the launch plan picks the wave-stress kernel builds as it does today.
 *                  (The receive that attaches it for the first time waits for the stream once, as that call does; every later one is asynchronous.)
 *   nxs_dyn_nodes_coupled_get      synchronised; out[k] (may be NULL, as may out) receives the [Nn] row of field k, device_rows[k] its device address.
 * NXS_ERR_STATE: before nxs_dyn_set_mesh, without an attachment of `which` on this mesh, a map without a source, a row asked for that was never received.
 * NXS_ERR_INVALID: h NULL, an unknown `which`, a map whose N is not Nn or that lives on another device than the handle, n_fields that is not the dataset's, a NULL field, a coefficient that is not finite. */
struct nxs_nodemap;   /* include/nxs_interp.h */
enum { NXS_NC_OCEAN = 0, NXS_NC_WAVE = 1 };
#define NXS_NC_DATASETS 2
#define NXS_NC_MAX_FIELDS 3
typedef struct nxs_dyn_nodes_coupled_config {
    double a[NXS_NC_MAX_FIELDS], b[NXS_NC_MAX_FIELDS];            /* receiveCouplingData: t *= a; t += b */
    double factor[NXS_NC_MAX_FIELDS], bias[NXS_NC_MAX_FIELDS];    /* ExternalData::get (NXS_NC_WAVE) */
} nxs_dyn_nodes_coupled_config;
NXS_API int nxs_nodes_coupled_default_config(nxs_dyn_nodes_coupled_config *c);   /* a = 1, b = 0, factor = 1, bias = 0 */
NXS_API int nxs_dyn_nodes_coupled_attach(nxs_dyn_handle *h, int32_t which, struct nxs_nodemap *map, const nxs_dyn_nodes_coupled_config *c /* NULL: detach */);
NXS_API int nxs_dyn_nodes_coupled_receive(nxs_dyn_handle *h, int32_t which, const double *const *fields, int32_t n_fields, int32_t flags);
NXS_API int nxs_dyn_nodes_coupled_get(nxs_dyn_handle *h, int32_t which, double *const *out /* may be NULL */, const double **device_rows /* may be NULL */);

/* ---- Forcing given on a TRIANGULATED source on the device: topaz4r_nodes (u, v, ssh at the nodes), topaz4r_elements (sst, sss, mld at the elements),
 * ocean_currents_nodes and their kin (grid.interpolation_method == FromMeshToMesh2dx, dataset.cpp:1777-2150, 10321-10690) through a node map
 * (nxs_nodemap_load_rows, include/nxs_interp.h: the tail of loadDataset, transformData and InterpFromMeshToMesh2dx, externaldata.cpp:886-931, 944-1288, 1334-1383,
 * 1442-1448).  The counterparts of nxs_dyn_forcing_ingest / nxs_dyn_thermo_forcing_ingest for a source that is a mesh.  Everything here is additive: a handle that
 * never attaches allocates nothing, launches nothing and keeps its bits; nxs_dyn_step's launch plan is untouched.
 *   nxs_dyn_forcing_attach_mesh         set 0 .. NXS_NF_SETS - 1: the map of that dataset, BORROWED (the caller keeps it alive and destroys it), with the handle's Nn
 *                  targets, ghosts included, on the handle's device, and a source (nxs_nodemap_set_source).  map == NULL detaches.  The attachment goes with the
 *                  mesh: nxs_dyn_set_mesh and nxs_dyn_regrid drop it (the weights were the old mesh's); attach the new map afterwards.
 *   nxs_dyn_forcing_ingest_mesh         one loadDataset: l as nxs_nodemap_load_rows takes it (fields host pointers or, with NXS_REGRID_IN_DEVICE, device pointers);
 *                  row [n_var]: variable j goes to the half-row row[j] (NXS_NF_*), -1 skips it.  Column (fstep, j) is stored to snapshot fstep of that half-row --
 *                  the rows nxs_dyn_set_forcing_pair owns, made here when never given, marked as nxs_dyn_forcing_ingest marks them (the routes mix per half-row;
 *                  the pair is complete once all ten are there).  n_step == 1 fills snapshot 0 only (a `constant` or `nearest_daily` dataset: NXS_TF_STEP).
 *                  Two launches on the handle's stream, asynchronous; with device fields there is no host synchronisation.  The time blend is
 *                  nxs_dyn_set_forcing_time_rows.
 *   nxs_dyn_thermo_forcing_attach_mesh  set 0 .. NXS_TF_SETS - 1: a map whose targets are the handle's Ne element barycentres.
 *   nxs_dyn_thermo_forcing_ingest_mesh  row [n_var]: NXS_TF_*, -1 skips.  Column (fstep, j) goes to snapshot fstep of row row[j] -- the rows
 *                  nxs_dyn_thermo_forcing_pair owns, made here when never given.  The time blend is nxs_dyn_thermo_forcing_time.
 * NXS_ERR_STATE: before nxs_dyn_set_mesh, without an attachment of `set` on this mesh, a map without a source.
 * NXS_ERR_INVALID: h, l or row NULL, a set out of range, a map on another device or with another target count, n_var or n_step out of range, a row out of range or
 * named twice, every variable skipped, flags other than NXS_REGRID_IN_DEVICE, and whatever nxs_nodemap_load_rows refuses (its message is passed on). */
struct nxs_nodemap_load;   /* include/nxs_interp.h */
NXS_API int nxs_dyn_forcing_attach_mesh(nxs_dyn_handle *h, int32_t set, struct nxs_nodemap *map /* NULL detaches */);
NXS_API int nxs_dyn_forcing_ingest_mesh(nxs_dyn_handle *h, int32_t set, const struct nxs_nodemap_load *l, const int32_t *row /* [n_var] NXS_NF_*, -1 skips */, int32_t flags);
NXS_API int nxs_dyn_thermo_forcing_attach_mesh(nxs_dyn_handle *h, int32_t set, struct nxs_nodemap *map /* NULL detaches */);
NXS_API int nxs_dyn_thermo_forcing_ingest_mesh(nxs_dyn_handle *h, int32_t set, const struct nxs_nodemap_load *l, const int32_t *row /* [n_var] NXS_TF_*, -1 skips */, int32_t flags);

/* ---- The rest of thermo()'s slab loop on the device: FE.cpp:5413-6133 as a default (non-OASIS) build compiles it -- the assimilation flux (FE.cpp:5415-5425),
 * section 6: new ice over open water and lateral melt (FE.cpp:5434-5646; newice_type 1 .. 4, type 3 with windSpeedElement, FE.cpp:6359-6370; melt_type 1, 2), the
 * freeze-days block (FE.cpp:5649-5682), the new concentration and thickness with Winton's (38), (39), (26) (FE.cpp:5685-5711), the limit block (FE.cpp:5714-5728),
 * section 7, section 8: the slab ocean with meltPonds (FE.cpp:5812-5846, 6538-6627), section 9: the temperature-dependent healing (FE.cpp:5854-5881), section 10: the
 * diagnostics (FE.cpp:5903-5976) and the age and type tracers (FE.cpp:5980-6132).  One launch, a thread per element, ghost elements included.  It reads the rows of
 * nxs_dyn_fluxes and of nxs_dyn_column -- both stay READ-ONLY: Qow, the reference's function-local vector, is a register copy, so nxs_dyn_fluxes_get answers the
 * same after the call -- M_precip and, under NXS_COL_MLD_ROW, M_mld (nxs_dyn_column_set_forcing), and under newice_type 3 M_wind at the element's three nodes.
 * The thermo type, the freezing point, freezingpoint_mu, snow_cond, the mixed-layer source and constant_mld are the column's configuration and ocean_albedo is the
 * fluxes': one copy of each.  UPDATED IN PLACE: in nxs_dyn_state conc, thick, snow_thick, ridge_ratio, conc_young, h_young, hs_young, conc_myi, thick_myi and (under
 * temp_dep_healing) time_relaxation_damage, so the next nxs_dyn_step reads them; in nxs_dyn_flux_state sst, sss and (under use_meltponds) pond_fraction,
 * lid_volume; tice0 and under WINTON the column's tice1 / tice2; nxs_dyn_slab_state except conc_upd.  It writes NXS_SLAB_ROWS rows, the D_* diagnostics of thermo().
 * The library knows no dates: the caller derives the five flags of nxs_dyn_slab_clock from M_current_time (FE.cpp:5653-5655, 5208, 5999, 6028, 6044).
 * NOT IN nxs_dyn_slab, all of it #ifdef OASIS in the reference: melt_type 3 (FE.cpp:5592-5640; refused by the configuration check), the FSD branches of the limit
 * block (FE.cpp:5729-5764), redistributeThermoFSD (FE.cpp:5768-5776), the in-loop weldingRoach (FE.cpp:5779-5797), the mechanical FSD healing of 9.b
 * (FE.cpp:5883-5898): these are nxs_dyn_slab_coupled's, below.  Because FE.cpp:5729-5764 would have to touch the bins, nxs_dyn_slab answers NXS_ERR_STATE while
 * floe-size bins are attached (nxs_dyn_put_coupled with num_fsd_bins > 0): such a host calls nxs_dyn_slab_coupled.  The throw of a wrong newice_type / melt_type is NXS_ERR_INVALID at
 * configuration.  By default nxs_dyn_regrid does NOT carry nxs_dyn_slab_state across a regrid: nxs_dyn_set_mesh and nxs_dyn_regrid make it missing again, like
 * tice1 / tice2.  A host that has called nxs_dyn_regrid_carry_thermo finds the rows it had put on the old mesh present on the new one, remapped as the reference
 * remaps M_prognostic_variables_elt; any other host fetches them before a regrid and puts them back after.  nxs_dyn_means_update accumulates the rows (NXS_MEANS_QA .. NXS_MEANS_SALTFLUX) where they lie.
 *   nxs_slab_default_config   model/options.cpp:329-331, 397-403, 428-449, 543-548
 *   nxs_slab_config_check     what nxs_dyn_slab_configure refuses, without a handle: newice_type outside 1 .. 4, melt_type outside 1 .. 2 (3 is the OASIS branch),
 *                  hnull, PhiF, h_young_min, meltpond_depth_to_fraction, time_relaxation_damage or deltaT_relaxation_damage <= 0 (or NaN), h_young_max <=
 *                  h_young_min; NXS_ERR_INVALID, the text in nxs_dyn_last_error(NULL)
 *   nxs_slab_constants        TEST DOOR like nxs_col_constants: the constants compiled into the kernel, in the order NXS_SLAB_CONST_* names them
 *   nxs_dyn_slab_configure    the configuration is the handle's and survives nxs_dyn_set_mesh
 *   nxs_dyn_slab_put / nxs_dyn_slab_get_state   [Ne] host rows, NULL members as in nxs_dyn_flux_put / _get.  Which rows the launch NEEDS follows from the
 *                  configuration: conc_upd only under use_assim_flux, pond_volume only under use_meltponds, the other eight always.  time_relaxation_damage is
 *                  ignored by _put (it is nxs_dyn_put_state's) and returned by _get_state, which nxs_dyn_get_state cannot do (the member is const there)
 *   nxs_dyn_slab              the launch, asynchronous on the handle's stream; dt is thermo()'s integer argument (ddt = dtime_step = double(dt): FE.cpp:1083-1084,
 *                  8140).  NXS_ERR_INVALID: dt <= 0, a NULL clock.  NXS_ERR_STATE: before nxs_dyn_slab_configure; before the first nxs_dyn_column since the last
 *                  nxs_dyn_set_mesh / nxs_dyn_regrid; while a needed row is missing; while floe-size bins are attached; newice_type 4 on a handle of the classic
 *                  category and another newice_type on one of the young-ice category (the category is the handle's); on a second nxs_dyn_slab without a new
 *                  nxs_dyn_column in between (the state has moved on and the column's rows are stale)
 *   nxs_dyn_slab_get          exactly like nxs_dyn_column_get.  NXS_ERR_STATE before the first nxs_dyn_slab
 * Debug array "slab_branches" [Ne] (nxs_dyn_debug_array): one word per element, a bit NXS_SLAB_BR_* per decision the element took; written by every launch. */
enum { NXS_SLAB_CONST_CMIN = 0, NXS_SLAB_CONST_HMIN, NXS_SLAB_CONST_RHOW, NXS_SLAB_CONST_CPW, NXS_SLAB_CONST_RHOI, NXS_SLAB_CONST_RHOS, NXS_SLAB_CONST_LF,
       NXS_SLAB_CONST_C, NXS_SLAB_CONST_KI, NXS_SLAB_CONST_SI, NXS_SLAB_CONST_DAYS_IN_SEC, NXS_SLAB_CONST_COUNT };
enum { NXS_SLAB_BR_SUPERCOOLED = 1,     /* tw_new < tfrw (FE.cpp:5438) */
       NXS_SLAB_BR_N2_HI_OLD = 2,       /* newice_type 2: hi_old > 0 */
       NXS_SLAB_BR_N2_NEWICE = 4,       /* newice_type 2: no old ice, newice > 0 */
       NXS_SLAB_BR_N3_H0 = 8,           /* newice_type 3: the wind's h0 is the larger */
       NXS_SLAB_BR_N4_YOUNG = 16,        /* newice_type 4: M_conc_young > 0 */
       NXS_SLAB_BR_N4_NOT_FILLED = 32,   /* ... the young ice does not fill its concentration (FE.cpp:5515) */
       NXS_SLAB_BR_N4_SHARP = 64,        /* ... thicker than h_young_max_sharp (FE.cpp:5523) */
       NXS_SLAB_BR_N4_NO_ROOM = 128,      /* ... no room for young ice (FE.cpp:5542) */
       NXS_SLAB_BR_MELT = 256,            /* del_hi < 0 */
       NXS_SLAB_BR_MELT_SIDE = 512,       /* melt_type 2: hi > 0; melt_type 1: M_conc < 1 */
       NXS_SLAB_BR_DAY_FREEZE = 1024,     /* last step of the day, M_del_vi_tend > 0 */
       NXS_SLAB_BR_DAY_MELT = 2048,       /* last step of the day, M_del_vi_tend < 0 */
       NXS_SLAB_BR_CONC_GE_CMIN = 4096,   /* FE.cpp:5689 */
       NXS_SLAB_BR_DEL_C_NEG = 8192,      /* FE.cpp:5692 */
       NXS_SLAB_BR_LIMIT = 16384,          /* the limit block, FE.cpp:5714 */
       NXS_SLAB_BR_RIDGE = 32768,          /* M_thick > old_vol (FE.cpp:5845) */
       NXS_SLAB_BR_HEAL_ICE = 65536,       /* temp_dep_healing with M_thick > 0 */
       NXS_SLAB_BR_POND_FLUSHED = 131072, NXS_SLAB_BR_LID_EXISTS = 262144, NXS_SLAB_BR_LID_FORMS = 524288, NXS_SLAB_BR_LID_REMOVED = 1048576,   /* meltPonds */
       NXS_SLAB_BR_NO_ICE_TRACERS = 2097152, /* FE.cpp:5984 */
       NXS_SLAB_BR_RESET = 4194304,          /* reset_myi */
       NXS_SLAB_BR_OLD_MELT = 8388608,       /* FE.cpp:6101 */
       NXS_SLAB_BR_ASSIM = 16777216,          /* the assimilation flux is taken (the pow) */
       NXS_SLAB_BR_DENOM_CLAMP = 33554432,    /* FE.cpp:5833 */
       NXS_SLAB_BR_SSS_BELOW_SI = 67108864,   /* si_eff = M_sss */
       NXS_SLAB_BR_FREEZE_DAYS_GE = 134217728  /* M_freeze_days >= reset_freeze_days */ };
typedef struct nxs_dyn_slab_config {
    int32_t newice_type;               /* thermo.newice_type, 1 .. 4 */
    int32_t melt_type;                 /* thermo.melt_type, 1 .. 2 */
    int32_t use_assim_flux;            /* thermo.use_assim_flux */
    int32_t temp_dep_healing;          /* dynamics.use_temperature_dependent_healing */
    int32_t use_meltponds;             /* thermo.use_meltponds */
    int32_t reset_by_date;             /* age.reset_by_date */
    int32_t include_young_ice;         /* age.include_young_ice (forced false when reset_by_date is false: FE.cpp:5649-5650) */
    int32_t equal_melting;             /* age.equal_melting */
    double hnull;                      /* thermo.hnull */
    double PhiF, PhiM;                 /* thermo.PhiF, thermo.PhiM */
    double h_young_min, h_young_max;   /* thermo.h_young_min, _max [m]; h_young_max_sharp = .5*(h_young_min + h_young_max), FE.cpp:1198 */
    double assim_flux_exponent;        /* thermo.assim_flux_exponent */
    double reset_freeze_days;          /* age.reset_freeze_days */
    double meltpond_runoff_fraction;   /* thermo.meltpond_runoff_fraction */
    double meltpond_depth_to_fraction; /* thermo.meltpond_depth_to_fraction */
    double time_relaxation_damage;     /* days_in_sec * dynamics.time_relaxation_damage [s] */
    double deltaT_relaxation_damage;   /* dynamics.deltaT_relaxation_damage */
} nxs_dyn_slab_config;
typedef struct nxs_dyn_slab_state {
    double *conc_upd;                  /* [Ne] M_conc_upd (read; needed under use_assim_flux) */
    double *pond_volume;               /* [Ne] M_pond_volume (needed under use_meltponds) */
    double *del_vi_tend, *freeze_days, *freeze_onset, *conc_summer, *thick_summer;   /* [Ne] M_del_vi_tend ... M_thick_summer */
    double *fyi_fraction, *age_det, *age;                                            /* [Ne] M_fyi_fraction, M_age_det, M_age */
    double *time_relaxation_damage;    /* [Ne] nxs_dyn_slab_get_state only: the device copy of nxs_dyn_state's row */
} nxs_dyn_slab_state;
typedef struct nxs_dyn_slab_clock {
    int32_t first_step_of_day;         /* step_in_day == 1 (FE.cpp:5656) */
    int32_t last_step_of_day;          /* step_in_day == num_steps_in_day (FE.cpp:5661) */
    int32_t fyi_reset_now;             /* "%m%d" == "0915" && fmod(M_current_time, 1) == 0 (FE.cpp:5999) */
    int32_t myi_reset_now;             /* "%m%d" == age.reset_date at midnight (FE.cpp:6028) */
    int32_t onset_reset_now;           /* "%m%d" == "0801" at midnight (FE.cpp:6044) */
} nxs_dyn_slab_clock;
enum { NXS_SLAB_QA = 0, NXS_SLAB_QSW, NXS_SLAB_QLW, NXS_SLAB_QSH, NXS_SLAB_QLH, NXS_SLAB_QO, NXS_SLAB_QNOSUN, NXS_SLAB_QSW_OCEAN, NXS_SLAB_QASSIM, NXS_SLAB_DELS,
       NXS_SLAB_FWFLUX_ICE, NXS_SLAB_FWFLUX, NXS_SLAB_BRINE, NXS_SLAB_EVAP, NXS_SLAB_RAIN,
       NXS_SLAB_VICE_MELT, NXS_SLAB_DEL_VI_YOUNG, NXS_SLAB_DEL_HI, NXS_SLAB_DEL_HI_YOUNG, NXS_SLAB_NEWICE, NXS_SLAB_MLT_TOP, NXS_SLAB_MLT_BOT, NXS_SLAB_SNOW2ICE,
       NXS_SLAB_ALBEDO, NXS_SLAB_SIALB,
       NXS_SLAB_DEL_CI_MLT_MYI, NXS_SLAB_DEL_VI_MLT_MYI, NXS_SLAB_DEL_CI_RPLNT_MYI, NXS_SLAB_DEL_VI_RPLNT_MYI };
#define NXS_SLAB_ROWS 29
typedef struct nxs_dyn_slab_rows { double *row[NXS_SLAB_ROWS]; } nxs_dyn_slab_rows;   /* [Ne] each, indexed by NXS_SLAB_* */

NXS_API int nxs_slab_default_config(nxs_dyn_slab_config *c);
NXS_API int nxs_slab_config_check(const nxs_dyn_slab_config *c);
NXS_API int nxs_slab_constants(double *out, int32_t count);
NXS_API int nxs_dyn_slab_configure(nxs_dyn_handle *h, const nxs_dyn_slab_config *c);
NXS_API int nxs_dyn_slab_put(nxs_dyn_handle *h, const nxs_dyn_slab_state *s);
NXS_API int nxs_dyn_slab_get_state(nxs_dyn_handle *h, nxs_dyn_slab_state *s);
NXS_API int nxs_dyn_slab(nxs_dyn_handle *h, int32_t dt, const nxs_dyn_slab_clock *clock);
NXS_API int nxs_dyn_slab_get(nxs_dyn_handle *h, const nxs_dyn_slab_rows *out /* may be NULL */, const double **device_rows /* [NXS_SLAB_ROWS], may be NULL */);

/* ---- thermo()'s slab loop with floe-size bins attached: the loop as an OASIS build compiles it, FE.cpp:5413-6133, on the bins of nxs_dyn_put_coupled and, while
 * attached, the M_conc_mech_fsd of nxs_dyn_fsd_put.  It is nxs_dyn_slab's loop (ONE source: the same device function) plus every line that touches the bins:
 *   FE.cpp:5592-5640        melt_type 3 (Roach et al. 2018): the unbroken test, melt_type 2's rule on ctot, else lat_melt_rate = -m1 * pow(tw_new - tfrw, m2) * 2
 *                           (m1 = 3.e-6, m2 = 1.36), cat0_del_c, the sum over the bins, Qow, del_c, M_conc_young; the early break at ctot < 1e-11
 *   FE.cpp:5729-5764        the FSD branches of the limit block AS WRITTEN: the else of 5754 belongs to if (M_distinguish_mech_fsd), so without the mechanical
 *                           bins every bin is zeroed even after the rescaling, and with them none is
 *   FE.cpp:5768-5776, 4487-4670   redistributeThermoFSD under melt_type 3 where the limit block was not taken; abs(lat_melt_rate) of 4519 is the floating-point
 *                           absolute value (as argued for 4831 under nxs_dyn_fsd_weld)
 *   FE.cpp:5779-5797, 4737-4870   the in-loop weldingRoach where del_hi > 0: nxs_dyn_fsd_weld's device code and its weld_crash rule
 *   FE.cpp:5883-5898        9.b, the mechanical healing, with the M_time_relaxation_damage section 9 has just written
 * Two launches on the handle's stream: the loop (the bins are read as a stream, four intermediates of thermo() are left as rows), then a thread per element with
 * its bins in registers (builds for 2 / 6 / 12 / 16 bins like nxs_dyn_fsd_*).  distinguish_mech_fsd, welding_type, welding_kappa, debug_fsd and the tables are
 * nxs_dyn_fsd_configure's: one copy of each.  nxs_dyn_slab and its refusals are unchanged.
 * While a coupled ocean is attached (nxs_dyn_ocean_coupled_attach, below) nxs_dyn_slab and nxs_dyn_slab_coupled -- one slab_element -- skip the two stores of
 * FE.cpp:5829 and 5841: M_sst and M_sss are NOT advanced, delsss still feeds D_delS, and section 9's Tbot = freezingPoint(M_sss) sees the received salinity.
 * The outgoing side of the coupling (M_cpl_out's accumulators and exchange grid) is nxs_dyn_cpl_out_*.  OUT OF SCOPE: the reduction over ranks, the OASIS put.
 *   nxs_slab_coupled_config_check   HOST ONLY: nxs_slab_config_check with the configuration's melt_type replaced by `melt_type` (1, 2, 3); 3 needs attached_bins >=
 *                  1 (the throw of FE.cpp:5595).  NXS_ERR_INVALID, the text in nxs_dyn_last_error(NULL)
 *   nxs_dyn_slab_coupled_configure  the melt type of nxs_dyn_slab_coupled, on top of nxs_dyn_slab_configure (NXS_ERR_STATE before it); nothing else is
 *                  overridden and nxs_dyn_slab keeps its own.  Survives nxs_dyn_set_mesh, which the bins do not: so 3 is accepted whether or not bins are
 *                  attached, and nxs_dyn_slab_coupled asks for them.  NXS_ERR_INVALID outside 1 .. 3.  Without it nxs_dyn_slab_coupled uses the slab's melt_type
 *   nxs_dyn_slab_coupled   NXS_ERR_STATE, naming what is missing: everything nxs_dyn_slab refuses except attached bins; no bins attached; before
 *                  nxs_dyn_fsd_configure; attached bins that differ from the configured number; distinguish_mech_fsd without M_conc_mech_fsd (so
 *                  melt_type 3 never runs without bins: the throw of FE.cpp:5595).  It spends the column's rows like nxs_dyn_slab; nxs_dyn_slab_get, nxs_dyn_slab_get_state and
 *                  "slab_branches" answer after it as after nxs_dyn_slab.  The welding's ndt_mrg loop is data-dependent and uncapped, as in nxs_dyn_fsd_weld
 *   nxs_dyn_slab_coupled_info   thermo_fsd_crash: any of the M_debug_fsd conditions of redistributeThermoFSD (FE.cpp:4531, 4568, 4617-4646) held on some element
 *                  since the last call (only under debug_fsd; the mechanical bins' sum of 4631 where distinguish_mech_fsd keeps them); reduced on the device, cleared by the call; the element is finished as the arithmetic says.  The
 *                  welding's conditions raise weld_crash (nxs_dyn_fsd_get)
 * Debug array "slab_fsd_branches" [Ne]: the NXS_SLAB_FSD_BR_* word of every element from the last nxs_dyn_slab_coupled. */
enum { NXS_SLAB_FSD_BR_MELT3 = 1,             /* melt_type 3 taken: del_hi < 0 and tw_new > tfrw (FE.cpp:5596) */
       NXS_SLAB_FSD_BR_UNBROKEN = 2,          /* ... abs(M_conc_fsd[nb-1] - ctot) < 1e-7: melt_type 2's rule (FE.cpp:5616) */
       NXS_SLAB_FSD_BR_CTOT_BREAK = 4,        /* ... ctot < 1e-11: the break (FE.cpp:5610) */
       NXS_SLAB_FSD_BR_LIMIT_RESCALED = 8,    /* the limit block rescaled the bins (FE.cpp:5739) */
       NXS_SLAB_FSD_BR_LIMIT_MECH_RESCALED = 16, /* ... the mechanical bins (FE.cpp:5748) */
       NXS_SLAB_FSD_BR_LIMIT_ZEROED = 32,     /* ... zeroed the bins (FE.cpp:5754) */
       NXS_SLAB_FSD_BR_LATERAL = 64,          /* redistributeThermoFSD: the Horvat & Tziperman branch (FE.cpp:4519) */
       NXS_SLAB_FSD_BR_LAT_MELTING = 128,     /* ... lat_melt_rate < 0 (FE.cpp:4550) */
       NXS_SLAB_FSD_BR_FILLS_LEAD = 256,      /* ... M_conc + M_conc_young == 1. (FE.cpp:4579) */
       NXS_SLAB_FSD_BR_DEL_C_FSD_GE0 = 512,   /* ... refreezing of the young-ice category with del_c_fsd >= 0 (FE.cpp:4585) */
       NXS_SLAB_FSD_BR_YOUNG_SHRINKS = 1024,  /* ... young_ice_growth < 0 (FE.cpp:4562) */
       NXS_SLAB_FSD_BR_WELDED = 2048,         /* weldingRoach merged floes (FE.cpp:4757) */
       NXS_SLAB_FSD_BR_HEALED = 4096          /* 9.b (FE.cpp:5888) */ };
struct nxs_dyn_slab_coupled_info {   /* (no typedef: the entry point has the name, the tag names the type) */
    int32_t thermo_fsd_crash;
};
NXS_API int nxs_slab_coupled_config_check(const nxs_dyn_slab_config *c, int32_t melt_type, int32_t attached_bins);
NXS_API int nxs_dyn_slab_coupled_configure(nxs_dyn_handle *h, int32_t melt_type);
NXS_API int nxs_dyn_slab_coupled(nxs_dyn_handle *h, int32_t dt, const nxs_dyn_slab_clock *clock);
NXS_API int nxs_dyn_slab_coupled_info(nxs_dyn_handle *h, struct nxs_dyn_slab_coupled_info *info);

/* One dynamics step on the device-resident state: FE.cpp:8197-8214.  Asynchronous on the
 * handle's stream; nxs_dyn_synchronize() waits for it. */
NXS_API int nxs_dyn_step(nxs_dyn_handle *h);
NXS_API int nxs_dyn_explicit_solve(nxs_dyn_handle *h);
NXS_API int nxs_dyn_update(nxs_dyn_handle *h);
NXS_API int nxs_dyn_synchronize(nxs_dyn_handle *h);
/* Literal drop-in for the three lines of step(): put_state + set_forcing + step + get_state. */
NXS_API int nxs_dyn_step_host(nxs_dyn_handle *h, nxs_dyn_state *s, const nxs_dyn_forcing *f);

/* checkRegridding(): local minimum angle [deg] and flip test; the cross-rank reduction
 * (FE.cpp:8306, 1812) is left to the caller's communicator.  The extrema are those of std::min_element / std::max_element
 * (FE.cpp:1806, 1835-1836): a NaN angle or Jacobian of element 0 IS the result (min_angle NaN, no flip, no regrid from the angle), a NaN of any
 * later element loses every comparison and is skipped. */
NXS_API int nxs_dyn_check_regridding(nxs_dyn_handle *h, double *min_angle, int32_t *flip, int32_t *regrid_local);
/* checkFieldsFast(): crash_local != 0 when a field is out of range / NaN (FE.cpp:14541-14629) -- with a wave stress attached also its NaN test (FE.cpp:14631-14643). */
NXS_API int nxs_dyn_check_fields_fast(nxs_dyn_handle *h, int32_t *crash_local);

NXS_API int nxs_dyn_get_timing(nxs_dyn_handle *h, nxs_dyn_timing *t);
/* Device time [ms] of every single nxs_dyn_step since the last "timing_reset" (HIP events on the handle's stream, steps stay asynchronous; at most 4096
 * are kept): ms[0 .. min(*count, capacity)) are filled, *count = steps recorded.  SURVEY 8d quotes the metric on the MEDIAN step. */
NXS_API int nxs_dyn_get_step_times(nxs_dyn_handle *h, double *ms, int32_t capacity, int32_t *count);

/* The bytes the kernels of the LAST step had to move, per launch, computed on the host from the tables the launches really walk (the patch
 * lists of nxs_dyn_set_mesh) -- the roofline model bench.py prices the event-timed launches with (SURVEY 8d asks for algorithmic bytes per
 * launch; with temporal blocking its per-sub-step figure is no longer a lower bound, this one is):
 *   *_scheme_bytes  every list a workgroup reads, once, plus what it writes, summed over the workgroups of one launch: the halo rings of the
 *                   blocking scheme count (several workgroups must read them), a workgroup's SECOND read of a record does not
 *   *_reread_bytes  those second reads (the caches may or may not serve them: the hardware counters say)
 *   *_unique_bytes  every array entry the launch touches, once: the floor of ANY kernel that advances this many sub-steps per launch
 * so unique <= scheme <= scheme + reread, and counted HBM traffic (rocprofv3 --pmc) lands between unique and scheme + reread (below scheme where the L2 serves
 * rings that neighbouring workgroups share). */
enum { NXS_KERNEL_NONE = 0, NXS_KERNEL_PER_LOOP = 1 /* k_sigma_* + k_solve_move */, NXS_KERNEL_FUSED = 2 /* k_substep_fused */,
       NXS_KERNEL_MULTI = 3 /* k_substep_multi */, NXS_KERNEL_PAIR = 4 /* k_substep_pair */, NXS_KERNEL_RESIDENT = 5 /* k_substep_resident */,
       NXS_KERNEL_RESIDENT_BIG = 6 /* k_substep_resident_big */, NXS_KERNEL_PAIR_FLOW = 7 /* k_substep_flow: k_substep_pair's patches, one data-flow launch per step */ };
enum { NXS_PREP_NONE = 0, NXS_PREP_FULL = 1 /* k_prep_elements + k_prep_nodes with the work arrays */, NXS_PREP_LEAN = 2 /* the same, records only */,
       NXS_PREP_FUSED = 3 /* k_prep_fused */ };
typedef struct nxs_dyn_traffic {
    int32_t substep_kernel;          /* NXS_KERNEL_*: the kernel the sub-step loop of the last step ran on */
    int32_t substeps_per_launch;     /* sub-steps one launch of it advances (the resident kernels: all of them) */
    int32_t halo_in_kernel;          /* != 0: the launch also performs updateGhosts through the device-direct mailboxes */
    int32_t prep_kernel;             /* NXS_PREP_* */
    double substep_scheme_bytes, substep_reread_bytes, substep_unique_bytes;   /* per launch of the sub-step kernel */
    double survey_model_bytes;       /* SURVEY 8d's 172 B per element + 217 B per node, x substeps_per_launch (the "algorithmic equivalent") */
    int32_t move_ring_slots;         /* velocity slots one k_move_ring launch applies (0: the mesh move is inside the sub-step kernel) */
    int32_t reserved0;
    double move_ring_bytes;          /* per k_move_ring launch */
    double prep_scheme_bytes, prep_unique_bytes;   /* per step: the prep kernel(s) */
    double update_bytes;             /* per step: k_update */
} nxs_dyn_traffic;
NXS_API int nxs_dyn_get_traffic_model(nxs_dyn_handle *h, nxs_dyn_traffic *t);
/* Options (none changes a bit of the results; the tests assert that):
 *   "prepare"      1 = build NOW what the first step would build lazily (tables of the exchange inside the kernels, of the resident loop): hosts that
 *                  run several ranks of one process on ONE device call it before their start barrier (building frees device memory, which waits for the
 *                  whole device -- including a neighbour rank's kernel that is already waiting for this rank); harmless anywhere else
 *   "graph"        1 = sub-step loop replayed from a hipGraph (default); 0 = plain launches
 *   "timing"       1 = record the per-phase events (default); "timing_reset": zero the averages
 *   "fused"        3 = automatic (default): on a single rank several sub-steps per launch -- four on meshes small enough for one patch per CU
 *                  (<= 256 nodes each, patches with that many rings of halo), two with the stresses in registers on larger ones (see
 *                  "pair_regs") --, one patch kernel per sub-step otherwise (several ranks, mEVP, a sub-step count the depth does not divide);
 *                  2 = several sub-steps per launch wherever possible (single rank, not mEVP, a depth that divides the
 *                  number of sub-steps); 1 = one patch kernel per sub-step; 0 = one kernel per reference loop;
 *                  4 = the whole sub-step loop in ONE resident launch whose workgroups wait for their neighbouring patches only
 *                  (one rank, or several with the device-direct mailboxes and "halo_fused" 1: the exchange between ranks then happens
 *                  inside that launch too; not mEVP; every workgroup resident at once -- checked, also against the other resident grids this
 *                  process runs on the device, else as 1): for a device the handle has to itself.  Partitions of up to ~200 k triangles run two
 *                  workgroups per CU with one element per thread (a rank of eight of a 1.5 M-triangle mesh: 0.85 instead of 1.3 ms per step),
 *                  partitions of 200 k - 400 k ONE workgroup per CU with four elements and two nodes per thread (a rank of four: 1.3 instead of
 *                  2.2 ms).  The option decides how the mesh is cut: setting or clearing it on a live mesh cuts the mesh again (same bits)
 *                  WITH cum_damage ATTACHED (nxs_dyn_put_coupled, BBM) the accumulation lives in the one-kernel-per-loop family, k_substep_fused and
 *                  k_substep_pair; where the settings would run k_substep_multi (several sub-steps per launch on small meshes), k_substep_flow ("pair_flow") or
 *                  the resident loop (4), the step runs k_substep_pair where it applies and one patch kernel per sub-step (as 1) otherwise -- the same bits;
 *                  nxs_dyn_get_traffic_model().substep_kernel names what ran.  No setting fails or skips the accumulation
 *   "resident_dryrun"  (an action, not a setting) builds the tables of the resident loop for the mesh and halo lists set so far -- no transport,
 *                  no neighbours needed -- and fails with NXS_ERR_INVALID when this partition cannot run it (a patch with more elements than
 *                  threads, more than one round of workgroups, LDS, > 24 neighbouring patches): a partition can be checked on its own
 *   "resident_wide"  with "fused" 4 on several ranks, a device that is this handle's alone and a partition that one workgroup per CU covers:
 *                  1 = the build of the resident kernel compiled for two waves per SIMD (no register limit to speak of: 15 % faster there);
 *                  default 0, because one such workgroup fills a CU and ranks sharing a device would no longer be resident side by side
 *   "resident_overlap"  with "fused" 4: 1 = the interior elements of every patch (no corner is a halo node) run one exchange ahead -- their next
 *                  update is computed while the exchange of the sub-step is awaited; 0 = never; -1 (default) = where it is known to pay: the
 *                  large patches of a 200 k - 400 k partition (one workgroup per CU, nothing else fills its wait: 4 % faster), not the
 *                  one-element-per-thread patches (inside one GPU the wait is filled by the other workgroup of the CU; between GPUs it is a
 *                  round trip over xGMI: bench.py times both and keeps one).  The same bits either way
 *   "band_patch_nodes"  several ranks with "fused" 4 (one element per thread): the nodes this rank sends -- its own nodes along the partition boundary --
 *                  are cut into small patches of their own: a boundary patch pays the exchange between ranks in every sub-step of the resident
 *                  loop, so it gets a shorter compute phase (two ranks of 87 k triangles rehearsed on one GPU: 0.985 -> 0.89-0.91 ms of
 *                  sub-steps).  16..512 nodes; 0 = off; -1 (default) = 48.  The cut does not change a bit of the results
 *   "prep_fused"   prep elements + prep nodes (FE.cpp:10235-10416) as ONE launch over the sub-step kernel's node patches, the elements'
 *                  values reaching their nodes through LDS (k_prep_fused: 2 km mesh 203 -> 113 us per step, the same bits); on a rank of several over the
 *                  patches of its own nodes, the ghost nodes' share of the nodal loops in a small pass of its own (k_prep_ghost_nodes): -1 (default) =
 *                  on meshes of 250 k triangles and more (a rank of several: 500 k), 0 = never, 1 = wherever its tables exist
 *   "smooth_depth" sweeps of the open-water smoother per launch on its own node-ring patches (single rank): 5, 10 or 25; 0 = automatic
 *                  (10 where ten rings of neighbours fit the LDS, else 5; sweep by sweep where neither fits)
 *   "substeps_per_launch"  depth of that temporal blocking, 2..8; 0 = automatic (4, lowered until it divides the count)
 *   "patch_nodes"  own nodes per patch of the fused kernel, 64..1024; 0 = automatic (whole rounds of resident workgroups)
 *   "pair_nodes"   the same for the several-sub-steps kernels, 16..1024; 0 = automatic
 *   "pair_regs"    not mEVP, an even number of sub-steps: TWO sub-steps per launch with the stresses between them in registers and two
 *                  workgroups per CU (k_substep_pair: stress, damage, element constants and nodal inputs cross HBM once per two sub-steps; 2 km
 *                  mesh 6.62 -> 5.5 ms per step, the same bits).  Several ranks (device-direct mailboxes, "halo_fused" 1): both updateGhosts of a launch
 *                  happen inside it -- the patches along the partition boundary store their first velocities into the neighbours' mailboxes, wait for
 *                  the neighbours' and go on, every other patch runs the single-rank body.  -1 (default) = on meshes / partitions of more than 65 k nodes
 *                  (smaller single-rank meshes run four sub-steps per launch, one patch per CU), 0 = never, 1 = wherever it can run
 *   "pair_hilbert" single rank: 1 = the two-ring patches are cut along a Hilbert curve even where the caller's numbering has locality (experiment: at 2 km the rings get
 *                  THICKER -- nodes x 1.27 / 1.54 instead of x 1.25 / 1.51 -- and the own nodes of a patch are no longer contiguous: 4.51-4.77 against 4.30-4.42 ms of
 *                  sub-steps); 0 (default) = only where the numbering has none
 *   "pair_move"    single rank, k_substep_pair with 512 threads, no "um_ring": the launch applies the mesh move of its two sub-steps (FE.cpp:10543-10550) to its
 *                  own nodes itself -- M_UM and M_UT read and written once per launch, the additions in the order the deferred flush makes them -- so the
 *                  step needs no ring of one velocity buffer per sub-step (120 x 11.7 MB at 2 km) and no k_move_ring: 2 km 5.27 -> 5.17 ms per step, the
 *                  same bits.  -1 (default) = wherever that kernel runs on one rank, 0 = never (one flush per step from the ring), 1 = as -1
 *   "pair_flow"    single rank, where k_substep_pair runs with 512 threads and the whole step fits the velocity ring: 1 = every pair of sub-steps of a step in ONE
 *                  data-flow launch (k_substep_flow) whose workgroups take (pair, patch) tasks from queues and wait for the patches around theirs only
 *                  (per-patch counters; what patches hand each other is stored write-through and read past the L1) -- no launch drains the device 60
 *                  times a step; the same bits.  MEASURED SLOWER at 2 km (7.5 against 5.05 ms of sub-steps: the write-through traffic and the
 *                  software hand-over between tasks cost more than the part-empty last round of a launch), so 0 / -1 (default) = one launch per pair
 *   "pair_threads" single rank: threads of a k_substep_pair workgroup, 512 (default: two workgroups per CU, patches of ~430 nodes at 2 km) or 256 (four per CU,
 *                  patches of ~180 nodes: measured slower, 5.67 against 5.30 ms of sub-steps at 2 km -- the thicker rings cost more than four independent
 *                  workgroups per CU hide); set before nxs_dyn_set_mesh or the next step cuts the mesh again
 *   "um_ring"      apply M_UM/M_UT += dt*M_VT every n sub-steps from a ring of velocity buffers, 1..128;
 *                  0 = automatic (once per step on meshes that stream from HBM, every sub-step on cache-resident ones)
 *   "nt_mask"      non-temporal access classes of the fused kernel (1 sigma/damage, 2 UM/UT, 4 element constants); -1 = automatic
 *                  (default): 3 from 1 M local triangles on, where a sub-step streams more than the Infinity Cache holds, 0 below
 *   "pin_host"     1 = page-lock the caller's state / forcing vectors the first time they are seen (hipHostRegister), so the
 *                  per-step copies of a host that keeps its thermodynamics on the CPU run at PCIe speed; registrations are
 *                  dropped at set_mesh / destroy / pin_host 0.  Default 0: the library does not touch the caller's pages.
 *   "shape_mem"    the several-sub-steps kernel reads M_shape_coeff from a per-step 48-byte record (1, and -1 = automatic, the default)
 *                  or rebuilds it from the staged frozen coordinates every sub-step as the one-sub-step kernel always does (0)
 *   "trace_branches"  see nxs_dyn_get_branch_trace
 *   "work_arrays"  1 = the prep kernels also fill the one-array-per-quantity work vectors (M_shape_coeff, element mass, the per-step
 *                  element constants, rlmass, C_bu, grad_ssh, fcor) that only the fused = 0 kernels and nxs_dyn_debug_array read;
 *                  default 0: with fused != 0 the step writes its records only
 *   "halo_fused"   device-direct transport only: 1 = updateGhosts inside the fused sub-step kernel (default),
 *                  0 = separate push / pull kernels
 *   "resident_release"  "fused" 4 on several ranks: 1 (default) = a system-scope release fence in front of every sub-step's flags; 0 = none -- the flags publish
 *                  mailbox stores of other workgroups that were written through and drained before those workgroups took their tickets, which the publishing lane's
 *                  fence does not reach: 0.65 us per sub-step (a rank of eight of the 2 km mesh, looped back: 1.03 -> 0.95 ms of sub-steps).  The same bits on one
 *                  device; no run on several devices has told the two apart yet, hence the default; bench.py tries both and keeps 0 only if bit-identical
 *   "smooth_persist"  several ranks, device-direct mailboxes with the exchange inside the kernels: the 50 sweeps of the open-water smoother (FE.cpp:10578-10611) as ONE launch
 *                  of at most 128 persistent workgroups that meet at a barrier of their own between the sweeps (k_smooth_persist) instead of 50 launches of one sweep each
 *                  (0.12-0.16 ms per step saved on a rank of eight; a rank without ice-free own nodes whose exchanged nodes cannot change is done after one sweep); the same
 *                  bits.  -1 (default) / 1 = on, 0 = one launch per sweep
 *   "ipc_pad"      before nxs_dyn_ipc_export: the mailbox gets room for at least this many received nodes (profiling aid: a rank whose mailbox is connected
 *                  to itself stores its own, possibly longer, send segments into it)
 *   "means_stage"  the read-modify-write of the Moorings accumulators (nxs_dyn_means_update): 1 (default) = a workgroup's rows staged through LDS and
 *                  added as one contiguous stream of 16-byte accesses; 0 = every thread walks its own row in 16-byte accesses (rows of an even number of
 *                  variables; 8-byte otherwise).  The same bits; scripts/time_means.py times both
 *   "regrid_tile"  nxs_dyn_regrid with more than 31 element columns (a thermodynamic run with the coupled build's columns attached): 1 (default) = a workgroup's
 *                  rows pass through LDS in tiles of up to 31 columns; 0 = every thread walks its own row in global memory.  The same bits;
 *                  scripts/time_regrid_thermo.py times both
 *   "means_timing" 1 = nxs_dyn_means_update records events around its two launches; nxs_dyn_debug_array "means_update_ms" returns their device times
 *                  [elemental, nodal] in ms.  Default 0
 *   "slab_coupled_timing" 1 = nxs_dyn_slab_coupled records events around its two launches; nxs_dyn_debug_array "slab_coupled_ms" returns their device times
 *                  [k_coupled_thermo, k_coupled_bins] in ms.  Default 0
 *   "drifters_timing" 1 = the nxs_dyn_drifters_* calls record events around their launches and wait for them; nxs_dyn_debug_array "drifters_ms" returns the device
 *                  times [locator build, move kernels, conc kernel, mask kernels] of the last of each in ms.  nxs_dyn_means_points_update is timed by the
 *                  same option: "means_points_ms" returns [its locator build (0: the locator was current), its kernel].  Default 0
 *   "ipc_delay", "halo_one_directional"   test doors of the exchange protocols, see NXS_DELAY_* above */
NXS_API int nxs_dyn_set_option(nxs_dyn_handle *h, const char *key, int64_t value);

/* Test door: copies a named internal work array (rlmass, node_mass, C_bu, grad_ssh, fcor, VTM, shape,
 * emass, ecbu, force, volume, expC; drag_ui, drag_ui_young: the two inputs of nxs_dyn_state that nxs_dyn_fluxes updates in place) to the host so that
 * parity tests can localise a difference.  "guard_launch" [2]: the launch shape of the guards -- threads per block of k_check_fields and
 * k_regrid_partials, blocks of k_regrid_partials (beyond blocks x threads elements its grid-stride loop takes another trip).  "update_launch" [3]: the
 * instantiation of k_update the last update() launched -- REC (M_sigma was in the sub-step loop's records), FSD (the bins were attached) -- and its threads per
 * block; NXS_ERR_STATE before the first update(). */
NXS_API int nxs_dyn_debug_array(nxs_dyn_handle *h, const char *name, double *out, int64_t n);

/* Test door: option "trace_branches" = 1 zeroes a per-element record and makes every following step run the one-kernel-per-loop
 * family with the record kept: 4 words per element -- a hash of the branch updateSigmaDamage took at every sub-step (damage
 * increment yes / no, FE.cpp:4229; skipped, conc <= 0.1, FE.cpp:4151), the number of damaging sub-steps, flag bits (|dcrit - 1| <
 * 1e-9 seen, |conc - 0.1| < 1e-12 seen, skipped) and the sub-steps seen.  The oracle keeps the same record (oracle/dyn_ref.h), so a
 * test can name the elements where the two implementations ever took different branches.  Results are unchanged by the option. */
NXS_API int nxs_dyn_get_branch_trace(nxs_dyn_handle *h, uint64_t *out, int64_t num_words);

/* Connectivity tables with the exact content and ordering of BamgConvertMeshx -> Mesh::WriteMesh
 * (contrib/bamg/src/Mesh.cpp:514-543, 798-865) for a mesh given as 1-based triangles.
 * Pass NULL outputs to query the widths first. Tables are doubles (NaN / 0 padded) like bamg's. */
NXS_API int nxs_mesh_connectivity(const int32_t *indices, int32_t num_nodes, int32_t num_elements,
                          int32_t *nec_width, double *nodal_element_connectivity,
                          int32_t *nc_width, double *nodal_connectivity);

/* bamgmesh->ElementConnectivity (contrib/bamg/src/Mesh.cpp:777-796): ec[3*e+j] = 1-based number of the triangle
 * across local edge j (vertices (j+1)%3,(j+2)%3) of triangle e, NaN on the boundary.  Host only. */
/* M_Cohesion of calcCohesion() (FE.cpp:3909-3914) from initIce's random field (FE.cpp:11459-11475): C_fix + C_alea * r(id),
 * r = boost::uniform_01<boost::minstd_rand>, one draw per global element in id order.  global_element_id: 1-based
 * (M_mesh.trianglesIdWithGhost()).  Host only. */
NXS_API int nxs_calc_cohesion(double C_fix, double C_alea, const int32_t *global_element_id, int64_t num_elements,
                              int64_t num_global_elements, double *cohesion);

NXS_API int nxs_mesh_element_connectivity(const int32_t *indices, int32_t num_nodes, int32_t num_elements,
                                  double *element_connectivity);

#ifdef __cplusplus
}
#endif
#endif /* NXS_DYN_H */
