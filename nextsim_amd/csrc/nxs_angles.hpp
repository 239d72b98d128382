// nxs_angles.hpp -- the cos / sin rows of a rotation that differs per point, formed ON THE HOST with the reference's own expressions
//   std::cos(rotation_angle - angle), std::sin(rotation_angle - angle)      gridoutput.cpp:602-614, externaldata.cpp:1272-1273
// so that a kernel that rotates with them does + - * only and keeps the reference's bits.  The ONE copy: nxs_dyn_means_points_set / nxs_dyn_cpl_out_attach_grid
// (nxs_means_points.inl) and nxs_nodemap_set_source (nxs_interp.hip) go through it.
#ifndef NXS_ANGLES_HPP
#define NXS_ANGLES_HPP
#include <cmath>

inline void nxs_cos_sin_of_difference(double rotation_angle, double angle, double *c, double *s) {
    *c = std::cos(rotation_angle - angle);
    *s = std::sin(rotation_angle - angle);
}
#endif
