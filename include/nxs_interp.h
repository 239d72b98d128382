/*
 * nxs_interp.h -- C ABI of the mesh-to-mesh interpolation used at regrid (SURVEY.md section 8f, row N1;
 * BASELINE config 5).  Replaces the root-serial call
 *
 *   InterpFromMeshToMesh2dx(&interp_out, &mesh_prev.indexTr()[0], &coordX[0], &coordY[0], numNodes, numTriangles,
 *                           &interp_in[0], numNodes, nb_var, &new_coordX[0], &new_coordY[0], new_numNodes, false);
 *
 * of FiniteElement::interpFields (FE.cpp:3131-3139; contrib/bamg/src/InterpFromMeshToMesh2dx.cpp:17-179)
 * with a HIP gather kernel: exact integer point location (bamg's own integer coordinates and
 * determinants, contrib/bamg/src/Mesh.cpp:3441-3468, 3688-3690, include/det.h:8-12) through a uniform
 * bucket grid, then the barycentric (nodal data) or piecewise-constant (element data) gather.
 *
 * Semantics, relative to the reference:
 *   - a target point inside a triangle of the data mesh gets exactly the reference's value: area
 *     coordinates are ratios of the same 64-bit integer determinants, combined in the same order;
 *   - isdefault != 0: points outside the data mesh get defaultvalue (as the reference);
 *   - isdefault == 0 (the regrid call): the reference locates its points in bamg's RECONSTRUCTED mesh -- the data mesh plus
 *     triangles that fill its holes and the concave parts of its boundary up to the convex hull (Mesh.cpp:3135-3440) -- and
 *     projects points beyond the hull on a hull edge (CloseBoundaryEdge, Mesh.cpp:4590-4627).  The same here: the fill
 *     triangles are rebuilt on the host (constrained Delaunay triangulation of every pocket and hole with exact integer
 *     predicates, csrc/nxs_hull.inl: the same triangles as bamg's, checked against the real bamg), numbered behind the
 *     mesh's, and the hull projection is CloseBoundaryEdge's.  A point beyond the hull whose hull edge belongs to a mesh
 *     triangle gets the reference's bits; inside a fill triangle the three products of the P1 sum are the reference's but may
 *     be added in a rotated order (bamg's vertex order inside a fill triangle depends on its insertion history): <= 1 ulp.
 *     Element data outside the mesh (where the reference stops with an error) and meshes the completion does not cover
 *     (several components, pinched boundaries) take the nearest boundary edge instead; nxs_interp_last_info says how many
 *     points went which way.
 */
#ifndef NXS_INTERP_H
#define NXS_INTERP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define NXS_INTERP_API __attribute__((visibility("default")))
#else
#define NXS_INTERP_API
#endif

/* Same argument meaning and layout as InterpFromMeshToMesh2dx: index_data 1-based [3*nels_data];
 * data [M_data][N_data] row-major with M_data == nods_data (P1) or nels_data (P0);
 * data_interp [N_interp][N_data] is CALLER-allocated here (the reference allocates it).
 * Returns 0, or a negative NXS_ERR_* code of nxs_dyn.h (no HIP device: -2, never a CPU fallback).
 * kernel_ms (may be NULL) receives the device time of the gather kernel alone. */
NXS_INTERP_API int nxs_interp_mesh_to_mesh_2d(double *data_interp, const int32_t *index_data, const double *x_data,
                                              const double *y_data, int32_t nods_data, int32_t nels_data, const double *data,
                                              int32_t M_data, int32_t N_data, const double *x_interp, const double *y_interp,
                                              int32_t N_interp, int32_t isdefault, double defaultvalue, int32_t device,
                                              int32_t *num_exterior, double *kernel_ms);

/* Mesh -> regular grid sampling of the Moorings output (model/gridoutput.cpp:467-500 calls
 * InterpFromMeshToGridx, contrib/bamg/src/InterpFromMeshToGridx.cpp:11-193).  Same arguments: grid point
 * (i,j), i < nrows along x, j < ncols along y (x_i = xmin + i*xposting, y_j descending from ymax when
 * yposting > 0), griddata[N_data*(i*ncols+j)+k] CALLER-allocated.  A grid point takes the value of the LAST
 * element (highest number) whose area coordinates are all > -1e-11, exactly as the reference's element loop
 * overwrites; points in no element keep default_value; NaN results become default_value.  The area
 * coordinates are the reference's double expressions, so the values are bit-identical. */
NXS_INTERP_API int nxs_interp_mesh_to_grid(double *griddata, const int32_t *index_mesh, const double *x_mesh, const double *y_mesh,
                                           int32_t nods, int32_t nels, const double *data_mesh, int32_t data_length, int32_t N_data,
                                           double xmin, double ymax, double xposting, double yposting, int32_t nrows,
                                           int32_t ncols, double default_value, int32_t device, double *kernel_ms);
/* The same with the mesh data already on `device` (a device pointer to [data_length][N_data] rows, e.g. what nxs_dyn_ice_diagnostics returns):
 * a Moorings record without a round trip of the element state through the host. */
NXS_INTERP_API int nxs_interp_mesh_to_grid_device(double *griddata, const int32_t *index_mesh, const double *x_mesh, const double *y_mesh,
                                           int32_t nods, int32_t nels, const double *data_mesh_device, int32_t data_length, int32_t N_data,
                                           double xmin, double ymax, double xposting, double yposting, int32_t nrows,
                                           int32_t ncols, double default_value, int32_t device, double *kernel_ms);

/* Conservative remapping of the element variables at regrid: replaces the root-serial
 *
 *   ConservativeRemappingMeshToMesh(interp_elt_out, interp_in_elements, nb_var_element, bamgmesh_previous, bamgmesh_root);
 *
 * of FiniteElement::interpFields (FE.cpp:3108; contrib/bamg/src/ConservativeRemapping.cpp:176-328).  One thread per
 * triangle of the new mesh: the old triangle holding its barycentre (the reference finds it with
 * InterpFromMeshToMesh2dx, :243-249), the "same three vertices" shortcut through PreviousNumbering (:263-289),
 * otherwise the walk over the overlapping old triangles (checkTriangle, :330-449) with the polygon-clipping
 * weights, then out = (sum_k in[tri_k]*w_k) * (1/area(new triangle)) in the reference's visiting order
 * (ConservativeRemappingMeshToGrid, :97-131).  Same predicates, tolerances, sort and operand order as the
 * reference, so the result is bit-identical (tests/test_remap.py).
 *
 *   interp_in  [nels_old][nb_var], interp_out [nels_new][nb_var] (caller-allocated; the reference allocates it)
 *   index_     1-based triangles (bamgmesh->Triangles without the 4th column), x_, y_ = bamgmesh->Vertices
 *   nec_old / nec_width / ec_old   bamgmesh_previous->NodalElementConnectivity (+Size[1]) and ->ElementConnectivity
 *              as bamg leaves them (doubles, NaN padding); NULL = built here with nxs_mesh_connectivity /
 *              nxs_mesh_element_connectivity, which reproduce bamg's tables
 *   previous_numbering  bamgmesh_root->PreviousNumbering (1-based old number of every new vertex, 0 = new), may be NULL
 *   n_geom_vertices     bamgmesh_root->VerticesOnGeomVertexSize[0]
 *   num_failed (may be NULL)  new triangles whose barycentre is in no old triangle (the reference asserts) or that overlap
 *              more than 4096 old triangles (up to 96: lists in registers/scratch; beyond: a second pass with lists in
 *              global memory); their rows are NaN
 *   visits (may be NULL) [nels_new]  number of old triangles that contributed (1 = unchanged triangle)
 */
NXS_INTERP_API int nxs_interp_conservative_remap(double *interp_out, const double *interp_in, int32_t nb_var, const int32_t *index_old,
                                                 const double *x_old, const double *y_old, int32_t nods_old, int32_t nels_old,
                                                 const double *nec_old, int32_t nec_width, const double *ec_old,
                                                 const int32_t *index_new, const double *x_new, const double *y_new, int32_t nods_new,
                                                 int32_t nels_new, const double *previous_numbering, int32_t n_geom_vertices,
                                                 int32_t device, int32_t *num_failed, int32_t *visits, double *kernel_ms);

/* Structured grid -> mesh: the forcing ingest.  Replaces
 *
 *   InterpFromGridToMeshx(data_out, &gridX[0], gridX.size(), &gridY[0], gridY.size(), &data_in[0], gridY.size(), gridX.size(),
 *                         nb_var*nb_forcing_step, &RX[0], &RY[0], M_target_size, 100000000., interp_type);
 *
 * of ExternalData::loadDataset (model/externaldata.cpp:1436; contrib/bamg/src/InterpFromGridToMeshx.cpp:14-485), which
 * fills M_wind / M_ocean / M_ssh, the forcing inputs of the dynamics.  Same arguments: x_in / y_in are the pixel centres
 * (x_rows == N, y_rows == M) or their contours (one more entry each: centres are taken); data [M][N][N_data]
 * (row_major == 0, the call above) or [N][M][N_data]; data_mesh [nods][N_data] CALLER-allocated.  A node takes the
 * first grid interval that brackets it in x and in y (either orientation of the axes; the last coordinate belongs to the
 * last interval), then the triangle / bilinear / nearest formula with the reference's operand order -- including its
 * nearest-neighbour rule, which compares the node with the HALF EXTENT of the cell rather than its centre; NaN and
 * nodes outside the grid get default_value.  Bit-identical to the reference (tests/test_grid_to_mesh.py). */
enum { NXS_INTERP_TRIANGLE = 0, NXS_INTERP_BILINEAR = 1, NXS_INTERP_NEAREST = 2 };
NXS_INTERP_API int nxs_interp_grid_to_mesh(double *data_mesh, const double *x_in, int32_t x_rows, const double *y_in, int32_t y_rows,
                                           const double *data, int32_t M, int32_t N, int32_t N_data, const double *x_mesh,
                                           const double *y_mesh, int32_t nods, double default_value, int32_t interp, int32_t row_major,
                                           int32_t device, double *kernel_ms);

/* Of this thread's last nxs_interp_mesh_to_mesh_2d call: size of the completion, and how many target points were in no
 * triangle of the data mesh / of those, inside a fill triangle / projected on the hull / handled by the nearest-boundary-edge
 * stand-in; *completion_refused = why no completion was built (NULL when one was, or when isdefault != 0).  Any pointer may be NULL. */
NXS_INTERP_API int nxs_interp_last_info(int32_t *num_fill_triangles, int32_t *num_hull_edges, int32_t *num_exterior, int32_t *num_in_fill,
                                        int32_t *num_on_hull, int32_t *num_stand_in, const char **completion_refused);

/* Host only: bamg's convex completion of a mesh (index 1-based): the triangles ReconstructExistingMesh adds between the
 * boundary and the convex hull and inside the holes (fill_tri: 1-based, counter-clockwise, [3*cap_fill]) and the hull edges
 * counter-clockwise (hull_edges: 1-based vertex pairs, [2*cap_hull]).  Output arrays may be NULL to query the counts. */
NXS_INTERP_API int nxs_mesh_convex_completion(const int32_t *index, const double *x, const double *y, int32_t nods, int32_t nels,
                                              int32_t *num_fill, int32_t *fill_tri, int32_t cap_fill, int32_t *num_hull,
                                              int32_t *hull_edges, int32_t cap_hull);
/* mode: 0 = as above (the pocket construction; where it does not apply -- several components, a boundary that pinches -- the general one: the
 * constrained Delaunay triangulation of the boundary vertices minus the domain), 1 = the general construction, 2 = the pocket construction only */
NXS_INTERP_API int nxs_mesh_convex_completion_mode(const int32_t *index, const double *x, const double *y, int32_t nods, int32_t nels,
                                              int32_t *num_fill, int32_t *fill_tri, int32_t cap_fill, int32_t *num_hull,
                                              int32_t *hull_edges, int32_t cap_hull, int32_t mode);

NXS_INTERP_API const char *nxs_interp_last_error(void);

/* ---- a regrid's context: the old mesh's search tables built once (on the device) and shared by the two interpolation calls of
 * FiniteElement::interpFields (FE.cpp:3071-3154) and by any later call on the same mesh.  The one-shot functions above make one per call. */
typedef struct nxs_regrid nxs_regrid;
#define NXS_REGRID_IN_DEVICE 1   /* flags: the input data is a device pointer on the context's device */
#define NXS_REGRID_OUT_DEVICE 2  /*        the output array is */
NXS_INTERP_API int nxs_regrid_create(const int32_t *index_old, const double *x_old, const double *y_old, int32_t nods_old, int32_t nels_old, int32_t device,
                                     nxs_regrid **out);
NXS_INTERP_API int nxs_regrid_destroy(nxs_regrid *r);
/* InterpFromMeshToMesh2dx (arguments as nxs_interp_mesh_to_mesh_2d) */
NXS_INTERP_API int nxs_regrid_interp_nodes(nxs_regrid *r, double *data_interp, const double *data, int32_t M_data, int32_t N_data, const double *x_interp,
                                           const double *y_interp, int32_t N_interp, int32_t isdefault, double defaultvalue, int32_t flags,
                                           int32_t *num_exterior, double *kernel_ms);
/* ConservativeRemappingMeshToMesh (arguments as nxs_interp_conservative_remap) */
NXS_INTERP_API int nxs_regrid_remap_elements(nxs_regrid *r, double *interp_out, const double *interp_in, int32_t nb_var, const double *nec_old, int32_t nec_width,
                                             const double *ec_old, const int32_t *index_new, const double *x_new, const double *y_new, int32_t nods_new,
                                             int32_t nels_new, const double *previous_numbering, int32_t n_geom_vertices, int32_t flags,
                                             int32_t *num_failed, int32_t *visits, double *kernel_ms);
/* where the last regrid call of this thread spent its time, ms: [0] connectivity tables, [1] integer plane + bucket grid, [2] convex completion,
 * [3] host -> device copies, [4] kernels, [5] device -> host copies, [6] the whole call */
NXS_INTERP_API int nxs_interp_last_timing(double *ms8);
/* test door: the device-built tables (which = 0 bucket grid offsets, 1 its lists, 2 NodalElementConnectivity, 3 ElementConnectivity; ints, -1 = NaN) */
NXS_INTERP_API int nxs_regrid_debug_tables(nxs_regrid *r, int32_t which, int32_t *out, int64_t cap, int64_t *count);

/* ---- conservative remapping between the mesh and a grid of quadrilateral cells (a coupler's grid, or a loaded Moorings grid with
 * moorings.use_conservative_remapping), the weights resident on the device as lists.  Replaces, in a coupled run's step,
 *
 *   ConservativeRemappingWeights(bamgmesh_root, gridX, gridY, gridCornerX, gridCornerY, gridP, triangles, weights);     gridoutput.cpp:699
 *   ConservativeRemappingMeshToGrid(interp_out, interp_in, nb_var, grid_size, miss_val, gridP, cornerX, cornerY, triangles, weights);  :473
 *   ConservativeRemappingGridToMesh(interp_out, interp_in, nb_var, numElements, gridP, triangles, weights);             dataset.cpp
 *
 * (contrib/bamg/src/ConservativeRemapping.cpp:15-171).  nxs_gridmap_create is the first on the mesh of a regrid context AT REST (the reference
 * builds the weights on bamgmesh_root after a regrid, where M_UM = 0): the seed of a cell is the element holding its P-point (gridX, gridY) -- the
 * context's exact locator with default -1, as InterpFromMeshToMesh2dx(..., true, -1) at :55-61 -- and a cell whose P-point is in no element is land
 * and gets no row, even if it overlaps the mesh; a wet cell's row is checkTriangle's walk (the code of nxs_interp_conservative_remap with four
 * corners), its (triangle, weight) entries in the reference's push order, which is the order of every floating-point sum below.  Same predicates,
 * tolerances, sort and operand order as the reference: lists, weights and both applications are bit-identical (tests/golden/bamg_grid_remap.npz).
 *
 * The stored form is the COMPACT one GridOutput keeps after gridoutput.cpp:706-735: wet rows only, gridP ascending.  (The raw output of
 * ConservativeRemappingWeights keeps a row for every cell with gridP[land] = 0 and no entry, which makes ConservativeRemappingMeshToGrid overwrite
 * cell 0 with 0 * (1 / area); that quirk never reaches GridOutput, which drops the empty rows, and is not reproduced.)
 *
 *   cornerX, cornerY [4*G]  the corners of cell c at 4*c .. 4*c+3, in order around the cell (gridCornerX / gridCornerY)
 *   A cell is FAILED when it overlaps more than 4096 triangles or one of its polygons has more than 16 points (a cell that is not convex;
 *   a triangle against a convex quadrilateral gives at most 13): it gets no row and is counted in nxs_gridmap_info, never truncated.
 *   Cells are walked in chunks so that the arena of 4096-entry lists stays under 2 GiB.
 * There is no CPU path: NXS_ERR_NO_DEVICE without a device. */
typedef struct nxs_gridmap nxs_gridmap;
NXS_INTERP_API int nxs_gridmap_create(nxs_regrid *r, const double *gridX, const double *gridY, const double *cornerX, const double *cornerY, int32_t G,
                                      nxs_gridmap **out);
NXS_INTERP_API int nxs_gridmap_destroy(nxs_gridmap *map);
/* wet cells (rows), entries, the longest row, failed cells, the element count of the mesh and the size of the grid; any pointer may be NULL */
NXS_INTERP_API int nxs_gridmap_info(const nxs_gridmap *map, int32_t *wet_cells, int64_t *entries, int32_t *longest_row, int32_t *failed_cells, int32_t *nels,
                                    int32_t *grid_size);
/* ConservativeRemappingMeshToGrid (:103-135): out [G][nb_var], in [nels][nb_var].  Every cell gets miss_val; a wet cell gets
 * (sum_k in[tri_k] * w_k) * (1 / area(cell)), summed from 0 in list order.  flags: NXS_REGRID_IN_DEVICE / NXS_REGRID_OUT_DEVICE. */
NXS_INTERP_API int nxs_gridmap_mesh_to_grid(nxs_gridmap *map, double *out, const double *in, int32_t nb_var, double miss_val, int32_t flags);
/* ConservativeRemappingGridToMesh (:138-171): out [nels][nb_var], in [G][nb_var]; a gather over the transposed lists, whose rows are in the order
 * the reference's scatter over (cell, position) reaches each triangle -- the same sums, triangle_area included.  A triangle no wet cell touches
 * gets 0 * (1 / 0.), a NaN, as in the reference. */
NXS_INTERP_API int nxs_gridmap_grid_to_mesh(nxs_gridmap *map, double *out, const double *in, int32_t nb_var, int32_t flags);
/* The coupler's receive of element variables (ExternalData::check_and_reload of ocean_cpl_elements / wave_cpl_elements, externaldata.cpp:163-236, 461-514,
 * 1291-1493; dataset.cpp:2828-3031, 3219-3393) in ONE launch: per variable v < n_var (1 .. NXS_GRIDMAP_MAX_RECEIVE)
 *   receiveCouplingData      t = fields[v][c]; t *= a[v]; t += b[v]           (two roundings; a = 1, b = 0 for I_SST, I_SSS, I_FrcQsr, I_MLD, a = 2 for I_wlbk)
 *   interpolateDataset       ConservativeRemappingGridToMesh of the transformed fields, as nxs_gridmap_grid_to_mesh: from 0, in the scatter's (cell, position)
 *                            order, triangle_area summed alongside, times 1. / triangle_area; a triangle no wet cell touches gets 0 * (1 / 0.), a NaN
 *   ExternalData::get        out_rows[v][t] = factor[v] * x + bias[v]         (the "coupled" step branch, externaldata.cpp:434, 438: always evaluated, so a -0.
 *                            becomes +0. under factor 1 and bias 0)
 * fields[v] is an [G] array of its own, as OASIS delivers one 2-D field per get_2d; out_rows[v] an [nels] row of its own.  One thread per triangle walks the
 * triangle's transposed list once for all variables: the bits are those of nxs_gridmap_grid_to_mesh on the interleaved, transformed input followed by
 * factor * x + bias.  reduced_nodes_ind is empty for this interpolation method (DataSet::loadGrid builds it only in its FromMeshToMesh2dx / FromMeshToMeshQuick branch,
 * dataset.cpp:10321-10690; the ConservativeRemapping branch from :10692 leaves it empty), so every
 * cell of the field is read as delivered; nb_forcing_step = 1; there is no cyclic axis.
 * flags: NXS_REGRID_IN_DEVICE = fields[] are device pointers, NXS_REGRID_OUT_DEVICE = out_rows[] are (the arrays `fields` and `out_rows` themselves are host
 * arrays of pointers).  stream: a hipStream_t of the map's device, or NULL for the library's own.  With a stream and device rows out the call is ASYNCHRONOUS on
 * that stream (host fields are uploaded on it first, and the call waits for the uploads only); otherwise it returns when the rows are written.  The map's
 * lists are complete when nxs_gridmap_create / _import / _restrict return (they synchronise): a launch on any stream may follow without a fence. */
#define NXS_GRIDMAP_MAX_RECEIVE 5
NXS_INTERP_API int nxs_gridmap_receive_rows(nxs_gridmap *map, int32_t n_var, const double *const *fields, const double *a, const double *b, const double *factor,
                                            const double *bias, double *const *out_rows, int32_t flags, void *stream);
/* The coupler's put of element variables: GridOutput::updateGridMean's conservative elemental leg (gridoutput.cpp:473, 545) with the grid accumulators left
 * where they are.  in [nels][n_var] (the interleaved mesh accumulators), data_grid [n_var][G] (one [G] row per variable, as OASIS takes one 2-D field per put_2d):
 * per cell and variable  v = 0; v += in[tri*n_var+var]*w in list order; v *= 1 / area(cell); data_grid[var][c] += v  (ConservativeRemapping.cpp:128-132), and a
 * cell without a row adds 0. -- the reference passes 0., not its missing value, there; the += is kept on such a cell too (a -0. becomes +0.).  One thread per
 * cell walks the cell's list once for all variables (lists longer than 12 variables in column tiles of 12): the bits are those of nxs_gridmap_mesh_to_grid with
 * miss_val 0., transposed and added.  No transposition on the host, no atomics.  A restricted map (nxs_gridmap_restrict) gives this rank's partial sums.
 * flags: NXS_REGRID_IN_DEVICE = `in` is a device pointer, NXS_REGRID_OUT_DEVICE = `data_grid` is (a host data_grid is uploaded, added to and copied back).
 * stream as for nxs_gridmap_receive_rows: with a stream and both arrays on the device the call is ASYNCHRONOUS on it. */
NXS_INTERP_API int nxs_gridmap_send_rows(nxs_gridmap *map, int32_t n_var, const double *in, double *data_grid, int32_t flags, void *stream);
/* test door: how nxs_gridmap_receive_rows reads the cell and weight of an entry -- 1 (the default: the faster of the two on the 2 km mesh) through
 * copies of both in transposed order, so that a triangle's walk is contiguous (12 bytes per entry more, made by the first receive on a map, which waits for
 * them once), 0 through the index list of the transposed lists, as nxs_gridmap_grid_to_mesh does.  The same bits.  *previous (may be NULL) = the mode before */
NXS_INTERP_API int nxs_gridmap_debug_receive_lists(int32_t mode, int32_t *previous);
/* Partitioned runs (gridoutput.cpp:691-735: the root computes, everybody filters).  export: the host lists for the caller's broadcast --
 * gridP [rows], off [rows + 1], tris, w [entries], cornerX, cornerY [4*G], sizes from nxs_gridmap_info, any pointer may be NULL; import: a map out of
 * such lists on `device`; restrict: the entries of local triangles (local_of_root [nels of the map], -1 = not here), renumbered, rows left empty
 * dropped -- a new map on a mesh of nels_local elements. */
NXS_INTERP_API int nxs_gridmap_export(nxs_gridmap *map, int32_t *gridP, int32_t *off, int32_t *tris, double *w, double *cornerX, double *cornerY);
NXS_INTERP_API int nxs_gridmap_import(int32_t device, int32_t nels, int32_t G, int32_t rows, const int32_t *gridP, const int32_t *off, const int32_t *tris,
                                      const double *w, const double *cornerX, const double *cornerY, nxs_gridmap **out);
NXS_INTERP_API int nxs_gridmap_restrict(nxs_gridmap *map, const int32_t *local_of_root, int32_t nels_local, nxs_gridmap **out);
/* test door: build the weights in chunks of `cells` cells (0 = as many as the arena allows); *last_chunks (may be NULL) = the chunks the last build took */
NXS_INTERP_API int nxs_gridmap_debug_chunk(int32_t cells, int32_t *last_chunks);

/* ---- the coupler's receive of NODAL fields (I_Uocn, I_Vocn, I_SSH of ocean_cpl_nodes; I_tauwix, I_tauwiy of wave_cpl_nodes): the location of every node in the
 * triangulated exchange grid computed ONCE per mesh, three weights applied per coupling step.  Replaces, under #ifdef OASIS,
 *
 *   InterpFromMeshToMesh2dx_weights(M_areacoord, M_vertex, M_it, pfindex, gridX, gridY, ...)    DataSet::setNodalWeights, dataset.cpp:11157-11175
 *   receiveCouplingData -> transformData -> InterpFromMeshToMesh2dx_apply -> ExternalData::get   externaldata.cpp:498-509, 944-1288, 1457-1463, 434-438
 *
 * nxs_nodemap_create runs contrib/bamg/src/InterpFromMeshToMesh2dx_weights.cpp:59-120 for nodal data on a regrid context made of the SOURCE triangulation
 * (grid.pfindex, grid.gridX, grid.gridY of the reduced exchange-grid nodes; triangulating them stays the host's, as in DataSet::loadGrid).  x, y [N] are the targets
 * in the dataset's coordinates (convertTargetXY's output, the host's job).  The integers, the division (double)dete[k]/tb.det and the hull projection
 * (CloseBoundaryEdge, both outcomes) are those of nxs_regrid_interp_nodes with isdefault == 0; the map keeps the three 0-based source vertices and the three area
 * coordinates of every target as six rows.  At the VERTEX outcome of CloseBoundaryEdge the weights are 1, 0, 0 in the triangle behind one of the two hull edges
 * that end at the vertex; which of the two the reference takes depends on its walk, and the value differs only where a zero-weight vertex holds NaN or Inf.
 *   NXS_ERR_INVALID: a NULL argument, N < 1, flags other than 0 (none is defined yet); a target inside the convex hull but in a triangle of the completion (the reference throws,
 *   _weights.cpp:72-73): the message names their count and the first one, no map is made; a source the convex completion does not cover (the message carries the
 *   context's own reason): a map never holds stand-in weights.
 * nxs_nodemap_info: targets, source nodes, targets beyond the hull (-1 for an imported map; any pointer may be NULL).  nxs_nodemap_device: the device the map's rows live on (the context's, or nxs_nodemap_import's argument).  nxs_nodemap_export hands out the six rows (M_vertex / M_areacoord
 * transposed; any pointer may be NULL), nxs_nodemap_import makes a map of such rows (vertices in 0 .. nods_src - 1, else NXS_ERR_INVALID).
 *
 * nxs_nodemap_set_source gives the source side of the dataset; everything is copied.
 *   G        MN_full, the length of a field as OASIS3::get_2d delivers it
 *   R        the reduced nodes: the map's source nodes (else NXS_ERR_INVALID); reduced [R] = grid.reduced_nodes_ind (0 .. G - 1), NULL = the identity and R == G
 *   rotation_mode  what transformData does to a vector pair after the east/north branch: NXS_NODEMAP_ROTATE_NONE; _UNIFORM (dataset->rotation_angle != 0.,
 *            externaldata.cpp:1246-1261) with cos_m_diff_angle, sin_m_diff_angle as the host computed them; _GRID_THETA (grid.gridded_rotation_angle, :1263-1281)
 *            with rotation = mapNextsim->rotation*PI/180. and theta [R] = grid.gridTheta: std::cos(rotation - theta[i]) and std::sin(rotation - theta[i]) are
 *            evaluated here, once, ON THE HOST (the function nxs_dyn_means_points_set uses), and both rows stay resident: the device only multiplies and adds
 *   east_west_oriented  the pairs are east / north components (wave_cpl_nodes, dataset.cpp:3202-3207): lat, lon [R] in degrees, map = the model's projection
 *            (nxs_mapx_polar of nxs_dyn.h), delta_t = 1., the reference's constant (externaldata.cpp:956; anything else is NXS_ERR_INVALID)
 * The wave-direction branch of transformData is not built.
 *
 * nxs_nodemap_receive_rows, per coupling step, 1 <= n_var <= NXS_NODEMAP_MAX_RECEIVE: two launches on `stream`.
 *   k_nodemap_source    per reduced point and variable  t = fields[v][reduced[i]]; t *= a[v]; t += b[v]  (receiveCouplingData), then per pair the east/north
 *                       branch and the rotation, new0 = c*t0 + s*t1, new1 = -s*t0 + c*t1: loaded_data, [n_var][R] rows of the map
 *   k_nodemap_gather    per target and variable  a0*d[v0] + a1*d[v1] + a2*d[v2], left to right (_apply.cpp:57-59); with NXS_NODEMAP_GET the value stored is
 *                       factor[v]*x + bias[v] (ExternalData::get, always evaluated), else x
 *   pairs    [n_var] or NULL: pairs[v] = w >= 0 names the vector (v, w), component 0 first; -1 elsewhere.  At most two pairs, no variable in two of them.
 *   flags    NXS_REGRID_IN_DEVICE = fields[] are device pointers, NXS_REGRID_OUT_DEVICE = out_rows[] are ([N] each), NXS_NODEMAP_GET.  stream as for
 *            nxs_gridmap_receive_rows: with a stream and device rows out the call is ASYNCHRONOUS on it (host fields are uploaded on it first, and the call waits
 *            for the uploads only); with device fields too there is no host synchronisation at all.
 *   NXS_ERR_STATE before nxs_nodemap_set_source.  NXS_ERR_INVALID: a NULL argument or field, n_var out of range, a pair that is out of range or names a variable twice.
 *   ONE STREAM AT A TIME: the rows of loaded_data and the buffer host fields are uploaded to are the MAP's, one of each.  Two receives on one map are ordered only
 *            when they are enqueued on the same stream (as a handle's are); on two streams the caller orders them.
 * nxs_nodemap_debug_source (test door): the first n_var rows of the last receive's loaded_data, [n_var][R].
 * There is no CPU path: NXS_ERR_NO_DEVICE without a device. */
typedef struct nxs_nodemap nxs_nodemap;
struct nxs_mapx_polar;
#define NXS_NODEMAP_MAX_RECEIVE 4
#define NXS_NODEMAP_GET 4   /* flags of nxs_nodemap_receive_rows, beside NXS_REGRID_IN_DEVICE / NXS_REGRID_OUT_DEVICE */
enum { NXS_NODEMAP_ROTATE_NONE = 0, NXS_NODEMAP_ROTATE_UNIFORM = 1, NXS_NODEMAP_ROTATE_GRID_THETA = 2 };
typedef struct nxs_nodemap_source {
    int32_t G, R;
    const int32_t *reduced;
    int32_t rotation_mode;
    int32_t east_west_oriented;
    double cos_m_diff_angle, sin_m_diff_angle;
    double rotation;
    const double *theta;
    const double *lat, *lon;
    const struct nxs_mapx_polar *map;
    double delta_t;
} nxs_nodemap_source;
NXS_INTERP_API int nxs_nodemap_create(nxs_regrid *src, const double *x, const double *y, int32_t N, int32_t flags, nxs_nodemap **out);
NXS_INTERP_API int nxs_nodemap_destroy(nxs_nodemap *map);
NXS_INTERP_API int nxs_nodemap_info(const nxs_nodemap *map, int32_t *N, int32_t *nods_src, int32_t *beyond_hull);
NXS_INTERP_API int nxs_nodemap_device(const nxs_nodemap *map, int32_t *device);
NXS_INTERP_API int nxs_nodemap_export(nxs_nodemap *map, int32_t *v0, int32_t *v1, int32_t *v2, double *a0, double *a1, double *a2);
NXS_INTERP_API int nxs_nodemap_import(int32_t device, int32_t N, int32_t nods_src, const int32_t *v0, const int32_t *v1, const int32_t *v2, const double *a0,
                                      const double *a1, const double *a2, nxs_nodemap **out);
NXS_INTERP_API int nxs_nodemap_set_source(nxs_nodemap *map, const nxs_nodemap_source *s);
NXS_INTERP_API int nxs_nodemap_receive_rows(nxs_nodemap *map, int32_t n_var, const double *const *fields, const double *a, const double *b, const int32_t *pairs,
                                            const double *factor, const double *bias, double *const *out_rows, int32_t flags, void *stream);
NXS_INTERP_API int nxs_nodemap_debug_source(nxs_nodemap *map, double *out, int32_t n_var);

/* ---- forcing given on a TRIANGULATED source (topaz4r_nodes, topaz4r_elements, ocean_currents_nodes, the nesting_* datasets: grid.interpolation_method ==
 * FromMeshToMesh2dx, dataset.cpp:1777-2150, 10321-10690) through the weights of a node map.  nxs_nodemap_load_rows is ONE loadDataset on a map that has its source
 * (nxs_nodemap_set_source: reduced, the rotation, lat / lon of an east/north pair); it replaces
 *
 *   the tail of loadDataset        externaldata.cpp:886-931     d = (d*scale_factor + add_offset)*a + b on data_in_tmp, NaN -> 0., loaded_data[fstep][i] = d[reduced[i]]
 *   transformData                  externaldata.cpp:944-1288    per forcing step and vector pair: the east/north branch, then the uniform or the gridTheta rotation
 *   interpolateDataset             externaldata.cpp:1334-1383, 1442-1448   data_in in the order fstep*n_var + j, InterpFromMeshToMesh2dx(..., isdefault = false)
 *
 * The map's targets are any points: the nodes for a nodal dataset, the element barycentres for an elemental one (nxs_nodemap_create takes both).  The source has
 * not moved since the map was made, so nothing is located again: InterpFromMeshToMesh2dx with isdefault == false is statement for statement _weights followed by
 * _apply, and the weights are the map's.  Two launches on `stream`:
 *   k_nodemap_load          one thread per reduced point.  Per column c = fstep*n_var + j: d = fields[c][reduced[i]]; d = (d*scale_factor[c] + add_offset[c])*a[c] + b[c]
 *                           as FOUR separately rounded operations in that order; NaN becomes 0. (the wave-direction exception is not built).  Then per forcing step and
 *                           pair the east/north branch and the rotation of nxs_nodemap_receive_rows, on the point's own two entries.  loaded_data, [n_step*n_var][R]
 *                           rows of a staging buffer the map makes at its first load (a map that never loads allocates nothing for it).
 *   k_nodemap_cols_gather   one thread per target: three vertices and three weights loaded once, per KEPT column a0*d[v0] + a1*d[v1] + a2*d[v2], left to right
 *                           (InterpFromMeshToMesh2dx.cpp:157-159), stored to out_rows[c].  No factor / bias: ExternalData::get is the time blend's
 *                           (nxs_dyn_set_forcing_time_rows, nxs_dyn_thermo_forcing_time).
 *   n_var    dataset->variables.size(), 1 .. 4;  n_step  dataset->nb_forcing_step, 1 or 2
 *   fields   [n_step*n_var] host array of pointers; entry fstep*n_var + j is data_in_tmp of variable j of forcing step fstep, [G], as read from the file
 *   scale_factor, add_offset   the file's attributes per COLUMN (the two forcing steps may come from two files); a, b  Variable::a, ::b per column
 *   pairs    as nxs_nodemap_receive_rows: pairs[j] = w >= 0 names the vector (j, w) of VARIABLES, -1 elsewhere; the pair is transformed in EVERY forcing step
 *   out_rows [n_step*n_var] host array of pointers to [N] rows; a NULL entry skips that column (it is still loaded: a pair may need it)
 *   flags    NXS_REGRID_IN_DEVICE = fields[] are device pointers, NXS_REGRID_OUT_DEVICE = out_rows[] are.  stream as for nxs_nodemap_receive_rows: with a stream and
 *            device rows out the call is ASYNCHRONOUS on it (host fields are uploaded on it first, and the call waits for the uploads only); with device fields too
 *            there is no host synchronisation at all (the first load on a map, and the first with more columns, allocates the staging buffer behind one).
 *   NXS_ERR_STATE before nxs_nodemap_set_source.  NXS_ERR_INVALID: a NULL argument or field, n_var or n_step out of range, a pair that is out of range or names a
 *   variable twice, a scale_factor, add_offset, a or b that is not finite, every column skipped, an unknown flag.  NXS_ERR_NO_DEVICE without a device: no CPU path.
 *   ONE STREAM AT A TIME, as for nxs_nodemap_receive_rows: the staging rows and the upload buffer are the MAP's; a load and a receive on one map are ordered when
 *   they are enqueued on the same stream.
 * nxs_nodemap_debug_load (test door): the first n_cols rows of the last load's loaded_data, [n_cols][R].
 * NOT BUILT: reading the files, the two time indices, the mask and reduced_nodes_ind, BamgTriangulatex of the source, convertTargetXY, the wave-direction branch and
 * the North-Pole mean of transformData (:1206-1243 compares gridY with 90., which a projected source never holds). */
#define NXS_NODEMAP_MAX_LOAD 8          /* columns: up to 4 variables x nb_forcing_step (1 or 2) */
typedef struct nxs_nodemap_load {
    int32_t n_var, n_step;
    const double *const *fields;
    double scale_factor[NXS_NODEMAP_MAX_LOAD], add_offset[NXS_NODEMAP_MAX_LOAD];
    double a[NXS_NODEMAP_MAX_LOAD], b[NXS_NODEMAP_MAX_LOAD];
    int32_t pairs[4];
} nxs_nodemap_load;
NXS_INTERP_API int nxs_nodemap_load_rows(nxs_nodemap *map, const nxs_nodemap_load *l, double *const *out_rows, int32_t flags, void *stream);
NXS_INTERP_API int nxs_nodemap_debug_load(nxs_nodemap *map, double *out, int32_t n_cols);


#ifdef __cplusplus
}
#endif
#endif
