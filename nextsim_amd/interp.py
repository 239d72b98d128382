"""Mesh-to-mesh interpolation at regrid over the C ABI of include/nxs_interp.h.

`InterpFromMeshToMesh2dx` keeps the name and argument meaning of the reference routine
(contrib/bamg/src/InterpFromMeshToMesh2dx.cpp:17-24, called at FE.cpp:3131-3139); the work is done by the
HIP kernel in libnxsdyn.so -- no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from .dynamics import NxsError, load_library

_declared = False


def _lib():
    global _declared
    L = load_library()
    if not _declared:
        L.nxs_interp_mesh_to_mesh_2d.argtypes = [_abi.c_double_p, _abi.c_int32_p, _abi.c_double_p, _abi.c_double_p, C.c_int32,
                                                 C.c_int32, _abi.c_double_p, C.c_int32, C.c_int32, _abi.c_double_p, _abi.c_double_p,
                                                 C.c_int32, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_double)]
        L.nxs_interp_mesh_to_mesh_2d.restype = C.c_int
        L.nxs_interp_last_error.restype = C.c_char_p
        I = C.POINTER(C.c_int32)
        L.nxs_interp_last_info.argtypes = [I, I, I, I, I, I, C.POINTER(C.c_char_p)]
        L.nxs_mesh_convex_completion_mode.argtypes = [_abi.c_int32_p, _abi.c_double_p, _abi.c_double_p, C.c_int32, C.c_int32, I, _abi.c_int32_p,
                                                      C.c_int32, I, _abi.c_int32_p, C.c_int32, C.c_int32]
        _declared = True
    return L


def last_info() -> dict:
    """Of this thread's last InterpFromMeshToMesh2dx call: the completion's size and which way the exterior points went."""
    L = _lib()
    v = [C.c_int32(0) for _ in range(6)]
    why = C.c_char_p()
    L.nxs_interp_last_info(*[C.byref(q) for q in v], C.byref(why))
    keys = ("num_fill_triangles", "num_hull_edges", "num_exterior", "num_in_fill", "num_on_hull", "num_stand_in")
    out = {k: q.value for k, q in zip(keys, v)}
    out["completion_refused"] = why.value.decode() if why.value else None
    return out


def convex_completion(index, x, y, mode=0):
    """bamg's convex completion of a mesh (index 1-based): (fill triangles [n, 3], hull edges [m, 2]), 1-based, counter-clockwise.
    Host code of the product library (csrc/nxs_hull.inl).  mode 0: automatic, 1: the general construction (constrained Delaunay of the boundary
    vertices), 2: the pocket construction only."""
    L = _lib()
    index = np.ascontiguousarray(index, np.int32).ravel()
    x = np.ascontiguousarray(x, np.float64); y = np.ascontiguousarray(y, np.float64)
    nf, nh = C.c_int32(0), C.c_int32(0)
    rc = L.nxs_mesh_convex_completion_mode(_abi.iptr(index), _abi.dptr(x), _abi.dptr(y), x.size, index.size // 3, C.byref(nf), None, 0, C.byref(nh), None, 0, mode)
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    fill = np.zeros((max(nf.value, 1), 3), np.int32); hull = np.zeros((max(nh.value, 1), 2), np.int32)
    rc = L.nxs_mesh_convex_completion_mode(_abi.iptr(index), _abi.dptr(x), _abi.dptr(y), x.size, index.size // 3, C.byref(nf), _abi.iptr(fill), nf.value,
                                           C.byref(nh), _abi.iptr(hull), nh.value, mode)
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    return fill[:nf.value], hull[:nh.value]


def InterpFromMeshToMesh2dx(index_data, x_data, y_data, data, x_interp, y_interp, isdefault=False, defaultvalue=1e-24,
                            device=0, return_info=False):
    """index_data: 1-based [3*nels]; data: [M_data, N_data] with M_data == nods (P1) or nels (P0).
    Returns data_interp [N_interp, N_data] (and {'num_exterior', 'kernel_ms'} when return_info)."""
    L = _lib()
    index_data = np.ascontiguousarray(index_data, np.int32).ravel()
    x_data = np.ascontiguousarray(x_data, np.float64); y_data = np.ascontiguousarray(y_data, np.float64)
    data = np.ascontiguousarray(data, np.float64)
    if data.ndim == 1:
        data = data[:, None]
    x_interp = np.ascontiguousarray(x_interp, np.float64); y_interp = np.ascontiguousarray(y_interp, np.float64)
    out = np.empty((x_interp.size, data.shape[1]))
    next_, ms = C.c_int32(0), C.c_double(0.0)
    rc = L.nxs_interp_mesh_to_mesh_2d(_abi.dptr(out), _abi.iptr(index_data), _abi.dptr(x_data), _abi.dptr(y_data), x_data.size,
                                      index_data.size // 3, _abi.dptr(data), data.shape[0], data.shape[1], _abi.dptr(x_interp),
                                      _abi.dptr(y_interp), x_interp.size, int(bool(isdefault)), float(defaultvalue), device,
                                      C.byref(next_), C.byref(ms))
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    if return_info:
        return out, dict(last_info(), num_exterior=next_.value, kernel_ms=ms.value)
    return out


def InterpFromMeshToGridx(index_mesh, x_mesh, y_mesh, data, xmin, ymax, xposting, yposting, nrows, ncols, default_value,
                          device=0, return_info=False):
    """Mesh -> regular grid (Moorings) sampling, argument meaning of contrib/bamg's InterpFromMeshToGridx
    (model/gridoutput.cpp:496-505).  Returns griddata [nrows, ncols, N_data]."""
    L = _lib()
    if not hasattr(L, "_grid_declared"):
        L.nxs_interp_mesh_to_grid.argtypes = [_abi.c_double_p, _abi.c_int32_p, _abi.c_double_p, _abi.c_double_p, C.c_int32, C.c_int32,
                                              _abi.c_double_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                              C.c_int32, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_double)]
        L.nxs_interp_mesh_to_grid.restype = C.c_int
        L._grid_declared = True
    index_mesh = np.ascontiguousarray(index_mesh, np.int32).ravel()
    x_mesh = np.ascontiguousarray(x_mesh, np.float64); y_mesh = np.ascontiguousarray(y_mesh, np.float64)
    data = np.ascontiguousarray(data, np.float64)
    if data.ndim == 1:
        data = data[:, None]
    out = np.empty((nrows, ncols, data.shape[1]))
    ms = C.c_double(0.0)
    rc = L.nxs_interp_mesh_to_grid(_abi.dptr(out), _abi.iptr(index_mesh), _abi.dptr(x_mesh), _abi.dptr(y_mesh), x_mesh.size,
                                   index_mesh.size // 3, _abi.dptr(data), data.shape[0], data.shape[1], float(xmin), float(ymax),
                                   float(xposting), float(yposting), int(nrows), int(ncols), float(default_value), device, C.byref(ms))
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    return (out, {"kernel_ms": ms.value}) if return_info else out


def InterpFromMeshToGridx_device(index_mesh, x_mesh, y_mesh, data_device_ptr, data_length, N_data, xmin, ymax, xposting, yposting, nrows, ncols,
                                 default_value, device=0):
    """InterpFromMeshToGridx with the mesh data already on the device: `data_device_ptr` is a device address of [data_length][N_data]
    rows (e.g. the second value of FiniteElementDynamics.updateIceDiagnostics)."""
    L = _lib()
    if not hasattr(L, "_grid_dev_declared"):
        L.nxs_interp_mesh_to_grid_device.argtypes = [_abi.c_double_p, _abi.c_int32_p, _abi.c_double_p, _abi.c_double_p, C.c_int32, C.c_int32,
                                                     C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double,
                                                     C.c_int32, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_double)]
        L.nxs_interp_mesh_to_grid_device.restype = C.c_int
        L._grid_dev_declared = True
    index_mesh = np.ascontiguousarray(index_mesh, np.int32).ravel()
    x_mesh = np.ascontiguousarray(x_mesh, np.float64); y_mesh = np.ascontiguousarray(y_mesh, np.float64)
    out = np.empty((nrows, ncols, N_data))
    ms = C.c_double(0.0)
    rc = L.nxs_interp_mesh_to_grid_device(_abi.dptr(out), _abi.iptr(index_mesh), _abi.dptr(x_mesh), _abi.dptr(y_mesh), x_mesh.size,
                                          index_mesh.size // 3, C.c_void_p(data_device_ptr), int(data_length), int(N_data), float(xmin), float(ymax),
                                          float(xposting), float(yposting), int(nrows), int(ncols), float(default_value), device, C.byref(ms))
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    return out


def ConservativeRemappingMeshToMesh(interp_in, index_old, x_old, y_old, index_new, x_new, y_new, previous_numbering=None,
                                    n_geom_vertices=0, nec_old=None, ec_old=None, device=0, return_info=False):
    """Element variables old mesh -> new mesh, argument meaning of contrib/bamg's ConservativeRemappingMeshToMesh
    (FE.cpp:3108) with the BamgMesh members spelled out: index_* 1-based [3*nels], previous_numbering 1-based
    (0 = vertex created by the remesher).  interp_in [nels_old, nb_var] -> [nels_new, nb_var]."""
    L = _lib()
    if not hasattr(L, "_remap_declared"):
        D, I = _abi.c_double_p, _abi.c_int32_p
        L.nxs_interp_conservative_remap.argtypes = [D, D, C.c_int32, I, D, D, C.c_int32, C.c_int32, D, C.c_int32, D, I, D, D, C.c_int32,
                                                    C.c_int32, D, C.c_int32, C.c_int32, C.POINTER(C.c_int32), I, C.POINTER(C.c_double)]
        L.nxs_interp_conservative_remap.restype = C.c_int
        L._remap_declared = True
    f64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    index_old = np.ascontiguousarray(index_old, np.int32).ravel(); index_new = np.ascontiguousarray(index_new, np.int32).ravel()
    x_old, y_old, x_new, y_new = f64(x_old), f64(y_old), f64(x_new), f64(y_new)
    interp_in = f64(interp_in)
    if interp_in.ndim == 1:
        interp_in = interp_in[:, None]
    ne_new = index_new.size // 3
    out = np.empty((ne_new, interp_in.shape[1]))
    visits = np.zeros(ne_new, np.int32)
    prev = None if previous_numbering is None else f64(previous_numbering)
    nec = None if nec_old is None else f64(nec_old)
    ec = None if ec_old is None else f64(ec_old)
    nfail, ms = C.c_int32(0), C.c_double(0.0)
    rc = L.nxs_interp_conservative_remap(_abi.dptr(out), _abi.dptr(interp_in), interp_in.shape[1], _abi.iptr(index_old), _abi.dptr(x_old),
                                         _abi.dptr(y_old), x_old.size, index_old.size // 3, None if nec is None else _abi.dptr(nec),
                                         0 if nec is None else nec.shape[1], None if ec is None else _abi.dptr(ec), _abi.iptr(index_new),
                                         _abi.dptr(x_new), _abi.dptr(y_new), x_new.size, ne_new, None if prev is None else _abi.dptr(prev),
                                         int(n_geom_vertices), device, C.byref(nfail), _abi.iptr(visits), C.byref(ms))
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    if return_info:
        return out, {"num_failed": nfail.value, "visits": visits, "kernel_ms": ms.value}
    return out


def last_timing() -> dict:
    """Where this thread's last regrid call spent its time (ms)."""
    L = _lib()
    v = (C.c_double * 8)()
    L.nxs_interp_last_timing.argtypes = [C.POINTER(C.c_double)]
    L.nxs_interp_last_timing(v)
    keys = ("connectivity_ms", "plane_and_grid_ms", "completion_ms", "h2d_ms", "kernel_ms", "d2h_ms", "call_ms")
    return {k: float(v[i]) for i, k in enumerate(keys)}


def _result_array(out, shape):
    """A caller-supplied result array (C-contiguous float64 of exactly `shape`) or a fresh one."""
    if out is None:
        return np.empty(shape)
    if not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable and out.shape == tuple(shape)):
        raise ValueError(f"out must be a writeable C-contiguous float64 array of shape {tuple(shape)}")
    return out


class Regrid:
    """A regrid's context (include/nxs_interp.h, nxs_regrid_*): the OLD mesh's search tables -- integer plane, bucket grid, convex completion,
    the two connectivity tables -- built once, on the device, and shared by interpFields' two interpolation calls (FE.cpp:3071-3154)."""

    IN_DEVICE, OUT_DEVICE = 1, 2

    def __init__(self, index_old, x_old, y_old, device=0):
        L = self.L = _lib()
        if not hasattr(L, "_regrid_declared"):
            D, I, V = _abi.c_double_p, _abi.c_int32_p, C.c_void_p
            L.nxs_regrid_create.argtypes = [I, D, D, C.c_int32, C.c_int32, C.c_int32, C.POINTER(V)]
            L.nxs_regrid_destroy.argtypes = [V]
            L.nxs_regrid_interp_nodes.argtypes = [V, V, V, C.c_int32, C.c_int32, D, D, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double)]
            L.nxs_regrid_remap_elements.argtypes = [V, V, V, C.c_int32, D, C.c_int32, D, I, D, D, C.c_int32, C.c_int32, D, C.c_int32, C.c_int32,
                                                    C.POINTER(C.c_int32), I, C.POINTER(C.c_double)]
            L.nxs_regrid_debug_tables.argtypes = [V, C.c_int32, I, C.c_int64, C.POINTER(C.c_int64)]
            for n in ("nxs_regrid_create", "nxs_regrid_destroy", "nxs_regrid_interp_nodes", "nxs_regrid_remap_elements", "nxs_regrid_debug_tables"):
                getattr(L, n).restype = C.c_int
            L._regrid_declared = True
        self.index = np.ascontiguousarray(index_old, np.int32).ravel()
        self.x = np.ascontiguousarray(x_old, np.float64); self.y = np.ascontiguousarray(y_old, np.float64)
        self.h = C.c_void_p()
        rc = L.nxs_regrid_create(_abi.iptr(self.index), _abi.dptr(self.x), _abi.dptr(self.y), self.x.size, self.index.size // 3, device, C.byref(self.h))
        if rc:
            raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.nxs_regrid_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise NxsError(rc, (self.L.nxs_interp_last_error() or b"").decode())

    def interp_nodes(self, data, x_interp, y_interp, isdefault=False, defaultvalue=1e-24, data_device=None, out_device=None, return_info=False, out=None):
        """InterpFromMeshToMesh2dx.  data_device = (device pointer, M_data, N_data) instead of `data`; out_device = a device pointer for the result."""
        x_interp = np.ascontiguousarray(x_interp, np.float64); y_interp = np.ascontiguousarray(y_interp, np.float64)
        flags = 0
        if data_device is not None:
            dptr, M, N = data_device
            src = C.c_void_p(dptr); flags |= self.IN_DEVICE
        else:
            data = np.ascontiguousarray(data, np.float64)
            if data.ndim == 1:
                data = data[:, None]
            M, N = data.shape
            src = C.c_void_p(data.ctypes.data)
        if out_device is not None:
            out = None
            dst = C.c_void_p(out_device); flags |= self.OUT_DEVICE
        else:
            out = _result_array(out, (x_interp.size, N))
            dst = C.c_void_p(out.ctypes.data)
        next_, ms = C.c_int32(0), C.c_double(0.0)
        self._chk(self.L.nxs_regrid_interp_nodes(self.h, dst, src, M, N, _abi.dptr(x_interp), _abi.dptr(y_interp), x_interp.size, int(bool(isdefault)),
                                                 float(defaultvalue), flags, C.byref(next_), C.byref(ms)))
        if return_info:
            return out, dict(last_info(), num_exterior=next_.value, kernel_ms=ms.value, timing=last_timing())
        return out

    def remap_elements(self, interp_in, index_new, x_new, y_new, previous_numbering=None, n_geom_vertices=0, nec_old=None, ec_old=None,
                       in_device=None, out_device=None, return_info=False, out=None):
        """ConservativeRemappingMeshToMesh.  out = an array of the result's shape to fill (a caller that regrids repeatedly keeps it: a fresh
        370 MB array costs its page faults inside the copy back).  in_device = (device pointer, nb_var) instead of `interp_in`; out_device = a device pointer for the result."""
        f64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
        index_new = np.ascontiguousarray(index_new, np.int32).ravel()
        x_new, y_new = f64(x_new), f64(y_new)
        flags = 0
        if in_device is not None:
            dptr, nv = in_device
            src = C.c_void_p(dptr); flags |= self.IN_DEVICE
        else:
            interp_in = f64(interp_in)
            if interp_in.ndim == 1:
                interp_in = interp_in[:, None]
            nv = interp_in.shape[1]
            src = C.c_void_p(interp_in.ctypes.data)
        ne_new = index_new.size // 3
        if out_device is not None:
            out = None
            dst = C.c_void_p(out_device); flags |= self.OUT_DEVICE
        else:
            out = _result_array(out, (ne_new, nv))
            dst = C.c_void_p(out.ctypes.data)
        visits = np.zeros(ne_new, np.int32)
        prev = None if previous_numbering is None else f64(previous_numbering)
        nec = None if nec_old is None else f64(nec_old)
        ec = None if ec_old is None else f64(ec_old)
        nfail, ms = C.c_int32(0), C.c_double(0.0)
        self._chk(self.L.nxs_regrid_remap_elements(self.h, dst, src, nv, None if nec is None else _abi.dptr(nec), 0 if nec is None else nec.shape[1],
                                                   None if ec is None else _abi.dptr(ec), _abi.iptr(index_new), _abi.dptr(x_new), _abi.dptr(y_new), x_new.size, ne_new,
                                                   None if prev is None else _abi.dptr(prev), int(n_geom_vertices), flags, C.byref(nfail), _abi.iptr(visits), C.byref(ms)))
        if return_info:
            return out, {"num_failed": nfail.value, "visits": visits, "kernel_ms": ms.value, "timing": last_timing()}
        return out

    def debug_table(self, which: int) -> np.ndarray:
        """0 bucket-grid offsets, 1 its lists, 2 NodalElementConnectivity, 3 ElementConnectivity -- as the device built them (ints, -1 = NaN)."""
        n = C.c_int64(0)
        self._chk(self.L.nxs_regrid_debug_tables(self.h, which, None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), np.int32)
        self._chk(self.L.nxs_regrid_debug_tables(self.h, which, _abi.iptr(out), out.size, C.byref(n)))
        return out[:n.value]


class GridMap:
    """Conservative remapping between a mesh and a grid of quadrilateral cells with the weights resident on the device (include/nxs_interp.h,
    nxs_gridmap_*): ConservativeRemappingWeights / MeshToGrid / GridToMesh of contrib/bamg.  Made by weights() from a Regrid context of the mesh at
    rest, by import_() from exported lists, or by restrict() from another map."""

    IN_DEVICE, OUT_DEVICE = 1, 2

    def __init__(self, handle):
        self.L = _declare_gridmap()
        self.h = handle

    @classmethod
    def weights(cls, regrid, gridX, gridY, cornerX, cornerY):
        """ConservativeRemappingWeights: gridX, gridY [G] the P-points, cornerX, cornerY [G, 4] the corners in order around each cell."""
        L = _declare_gridmap()
        f64 = lambda a: np.ascontiguousarray(a, np.float64).ravel()  # noqa: E731
        gx, gy, cx, cy = f64(gridX), f64(gridY), f64(cornerX), f64(cornerY)
        if gy.size != gx.size or cx.size != 4 * gx.size or cy.size != 4 * gx.size:
            raise ValueError("gridX, gridY [G] and cornerX, cornerY [G, 4] expected")
        h = C.c_void_p()
        rc = L.nxs_gridmap_create(regrid.h, _abi.dptr(gx), _abi.dptr(gy), _abi.dptr(cx), _abi.dptr(cy), gx.size, C.byref(h))
        if rc:
            raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
        return cls(h)

    @classmethod
    def import_(cls, lists, device=0):
        """A map out of what export() returned (after the caller's broadcast)."""
        L = _declare_gridmap()
        i32 = lambda a: np.ascontiguousarray(a, np.int32).ravel()  # noqa: E731
        f64 = lambda a: np.ascontiguousarray(a, np.float64).ravel()  # noqa: E731
        gp, off, tr, w, cx, cy = i32(lists["gridP"]), i32(lists["off"]), i32(lists["tris"]), f64(lists["w"]), f64(lists["cornerX"]), f64(lists["cornerY"])
        if off.size != gp.size + 1 or tr.size != w.size or (off.size and off[-1] != tr.size) or cx.size != 4 * int(lists["grid_size"]) or cy.size != cx.size:
            raise ValueError("inconsistent lists")
        h = C.c_void_p()
        rc = L.nxs_gridmap_import(device, int(lists["nels"]), int(lists["grid_size"]), gp.size, _abi.iptr(gp), _abi.iptr(off), _abi.iptr(tr), _abi.dptr(w),
                                  _abi.dptr(cx), _abi.dptr(cy), C.byref(h))
        if rc:
            raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
        return cls(h)

    def _chk(self, rc):
        if rc:
            raise NxsError(rc, (self.L.nxs_interp_last_error() or b"").decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.nxs_gridmap_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        wet, lng, failed, nels, G = (C.c_int32() for _ in range(5))
        n = C.c_int64()
        self._chk(self.L.nxs_gridmap_info(self.h, C.byref(wet), C.byref(n), C.byref(lng), C.byref(failed), C.byref(nels), C.byref(G)))
        return {"wet": wet.value, "entries": n.value, "longest": lng.value, "failed": failed.value, "nels": nels.value, "grid_size": G.value}

    def export(self):
        """The host lists: gridP [rows], off [rows + 1], tris, w [entries], cornerX, cornerY [G, 4], with nels and grid_size."""
        i = self.info()
        gp, off, tr = np.empty(i["wet"], np.int32), np.empty(i["wet"] + 1, np.int32), np.empty(i["entries"], np.int32)
        w, cx, cy = np.empty(i["entries"]), np.empty((i["grid_size"], 4)), np.empty((i["grid_size"], 4))
        self._chk(self.L.nxs_gridmap_export(self.h, _abi.iptr(gp), _abi.iptr(off), _abi.iptr(tr), _abi.dptr(w), _abi.dptr(cx), _abi.dptr(cy)))
        return {"gridP": gp, "off": off, "tris": tr, "w": w, "cornerX": cx, "cornerY": cy, "nels": i["nels"], "grid_size": i["grid_size"]}

    def restrict(self, local_of_root, nels_local):
        """The map of a partition: local_of_root [nels] = the local number of every triangle, -1 = not here (gridoutput.cpp:706-735)."""
        lor = np.ascontiguousarray(local_of_root, np.int32).ravel()
        if lor.size != self.info()["nels"]:
            raise ValueError("local_of_root has one entry per triangle of the map's mesh")
        h = C.c_void_p()
        self._chk(self.L.nxs_gridmap_restrict(self.h, _abi.iptr(lor), int(nels_local), C.byref(h)))
        return GridMap(h)

    def _apply(self, fn, rows_in, rows_out, data, in_device, out_device, out, extra):
        flags = 0
        if in_device is not None:
            dptr, nv = in_device
            src = C.c_void_p(dptr); flags |= self.IN_DEVICE
        else:
            data = np.ascontiguousarray(data, np.float64)
            if data.ndim == 1:
                data = data[:, None]
            if data.shape[0] != rows_in:
                raise ValueError(f"data has {data.shape[0]} rows, expected {rows_in}")
            nv = data.shape[1]
            src = C.c_void_p(data.ctypes.data)
        if out_device is not None:
            out = None
            dst = C.c_void_p(out_device); flags |= self.OUT_DEVICE
        else:
            out = _result_array(out, (rows_out, nv))
            dst = C.c_void_p(out.ctypes.data)
        self._chk(fn(self.h, dst, src, nv, *extra, flags))
        return out

    def mesh_to_grid(self, data, miss_val=0., in_device=None, out_device=None, out=None):
        """ConservativeRemappingMeshToGrid: data [nels, nb_var] -> [G, nb_var].  in_device = (device pointer, nb_var) instead of `data`; out_device = a device pointer."""
        i = self.info()
        return self._apply(self.L.nxs_gridmap_mesh_to_grid, i["nels"], i["grid_size"], data, in_device, out_device, out, (float(miss_val),))

    def grid_to_mesh(self, data, in_device=None, out_device=None, out=None):
        """ConservativeRemappingGridToMesh: data [G, nb_var] -> [nels, nb_var]."""
        i = self.info()
        return self._apply(self.L.nxs_gridmap_grid_to_mesh, i["grid_size"], i["nels"], data, in_device, out_device, out, ())


    def receive_rows(self, fields, a=1., b=0., factor=1., bias=0., in_device=False, out_device=None, stream=None):
        """nxs_gridmap_receive_rows: the coupler's receive of up to five element variables in one launch.  fields: one [G] array per variable (in_device: one
        device address each); a, b, factor, bias: per variable (scalars are broadcast).  Returns [n_var, nels] rows -- or, with out_device (one device address
        of an [nels] row per variable), None.  stream: a hipStream_t as an int (asynchronous when the rows stay on the device), None for the library's own."""
        i = self.info()
        n = len(fields)
        co = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (n,))) for v in (a, b, factor, bias)]
        src, dst, keep, flags = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))(), [], 0
        for k, f in enumerate(fields):
            if in_device:
                src[k] = int(f)
            else:
                arr = np.ascontiguousarray(f, np.float64).ravel()
                if arr.size != i["grid_size"]:
                    raise ValueError(f"field {k} has {arr.size} cells, expected {i['grid_size']}")
                keep.append(arr)
                src[k] = arr.ctypes.data
        flags |= self.IN_DEVICE if in_device else 0
        out = None
        if out_device is not None:
            if len(out_device) != n:
                raise ValueError("one output row per field expected")
            for k, p in enumerate(out_device):
                dst[k] = int(p)
            flags |= self.OUT_DEVICE
        else:
            out = np.empty((n, i["nels"]))
            for k in range(n):
                dst[k] = out[k].ctypes.data
        self._chk(self.L.nxs_gridmap_receive_rows(self.h, n, src, _abi.dptr(co[0]), _abi.dptr(co[1]), _abi.dptr(co[2]), _abi.dptr(co[3]), dst, flags,
                                                  C.c_void_p(int(stream)) if stream else None))
        del keep
        return out


    def send_rows(self, data=None, data_grid=None, in_device=None, out_device=None, stream=None):
        """nxs_gridmap_send_rows: the coupler's put of element variables, ADDED to data_grid [n_var, G] (made of zeros when None) in one launch per twelve
        variables.  data [nels, n_var], or in_device = (device pointer, n_var); out_device = the device address of the [n_var, G] rows (then None is returned).
        stream: a hipStream_t as an int (asynchronous when both sides are on the device), None for the library's own."""
        i = self.info()
        flags, keep = 0, None
        if in_device is not None:
            dptr, nv = in_device
            src = C.c_void_p(int(dptr)); flags |= self.IN_DEVICE
        else:
            keep = np.ascontiguousarray(data, np.float64)
            if keep.ndim == 1:
                keep = keep[:, None]
            if keep.shape[0] != i["nels"]:
                raise ValueError(f"data has {keep.shape[0]} rows, expected {i['nels']}")
            nv = keep.shape[1]
            src = C.c_void_p(keep.ctypes.data)
        if out_device is not None:
            data_grid = None
            dst = C.c_void_p(int(out_device)); flags |= self.OUT_DEVICE
        else:
            if data_grid is None:
                data_grid = np.zeros((nv, i["grid_size"]))
            if data_grid.shape != (nv, i["grid_size"]) or data_grid.dtype != np.float64 or not data_grid.flags.c_contiguous:
                raise ValueError(f"data_grid has shape {data_grid.shape}, expected a C-contiguous float64 ({nv}, {i['grid_size']})")
            dst = C.c_void_p(data_grid.ctypes.data)
        self._chk(self.L.nxs_gridmap_send_rows(self.h, int(nv), src, dst, flags, C.c_void_p(int(stream)) if stream else None))
        del keep
        return data_grid


class NodeMap:
    """The coupler's receive of nodal fields with the weights resident on the device (include/nxs_interp.h, nxs_nodemap_*): InterpFromMeshToMesh2dx_weights once per
    mesh, receiveCouplingData -> transformData -> InterpFromMeshToMesh2dx_apply -> ExternalData::get per coupling step.  Made by weights() from a Regrid context of
    the SOURCE triangulation and the targets, or by import_() from exported rows."""

    IN_DEVICE, OUT_DEVICE, GET = 1, 2, _abi.NXS_NODEMAP_GET

    def __init__(self, handle):
        self.L = _declare_nodemap()
        self.h = handle
        self._keep = None

    @classmethod
    def weights(cls, regrid, x, y):
        """nxs_nodemap_create: x, y [N] the targets in the dataset's coordinates."""
        L = _declare_nodemap()
        x, y = np.ascontiguousarray(x, np.float64).ravel(), np.ascontiguousarray(y, np.float64).ravel()
        if x.size != y.size:
            raise ValueError("x and y [N] expected")
        h = C.c_void_p()
        rc = L.nxs_nodemap_create(regrid.h, _abi.dptr(x), _abi.dptr(y), x.size, 0, C.byref(h))
        if rc:
            raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
        return cls(h)

    @classmethod
    def import_(cls, rows, device=0):
        """A map out of what export() returned: v [N, 3] the 0-based source vertices, a [N, 3] their area coordinates, nods_src."""
        L = _declare_nodemap()
        v, a = np.asarray(rows["v"], np.int32), np.asarray(rows["a"], np.float64)
        if v.ndim != 2 or v.shape[1] != 3 or a.shape != v.shape:
            raise ValueError("v and a [N, 3] expected")
        vc = [np.ascontiguousarray(v[:, k]) for k in range(3)]
        ac = [np.ascontiguousarray(a[:, k]) for k in range(3)]
        h = C.c_void_p()
        rc = L.nxs_nodemap_import(device, v.shape[0], int(rows["nods_src"]), *(_abi.iptr(q) for q in vc), *(_abi.dptr(q) for q in ac), C.byref(h))
        if rc:
            raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
        return cls(h)

    def _chk(self, rc):
        if rc:
            raise NxsError(rc, (self.L.nxs_interp_last_error() or b"").decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.nxs_nodemap_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        N, nods, beyond = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self.L.nxs_nodemap_info(self.h, C.byref(N), C.byref(nods), C.byref(beyond)))
        dev = C.c_int32(-1)
        self._chk(self.L.nxs_nodemap_device(self.h, C.byref(dev)))
        return {"N": N.value, "nods_src": nods.value, "beyond_hull": beyond.value, "device": dev.value}

    def export(self):
        """v [N, 3] int32, a [N, 3] (M_vertex, M_areacoord) and nods_src."""
        i = self.info()
        vc, ac = [np.empty(i["N"], np.int32) for _ in range(3)], [np.empty(i["N"]) for _ in range(3)]
        self._chk(self.L.nxs_nodemap_export(self.h, *(_abi.iptr(q) for q in vc), *(_abi.dptr(q) for q in ac)))
        return {"v": np.stack(vc, axis=1), "a": np.stack(ac, axis=1), "nods_src": i["nods_src"]}

    def set_source(self, G, reduced=None, rotation="none", cos_m_diff_angle=1., sin_m_diff_angle=0., map_rotation=0., theta=None, east_west=False, lat=None, lon=None,
                   mapx=None, delta_t=1.):
        """nxs_nodemap_set_source.  G: the length of a delivered field; reduced [R]: grid.reduced_nodes_ind (None: the identity); rotation: "none", "uniform"
        (cos_m_diff_angle, sin_m_diff_angle) or "grid_theta" (map_rotation = mapNextsim->rotation*PI/180., theta [R]); east_west: the pairs are east / north components
        (lat, lon [R] degrees, mapx = dynamics.mapx_polar_north(...))."""
        s = _abi.NodemapSource()
        keep = []

        def arr(a, dt):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt).ravel()
            keep.append(a)
            return _abi.iptr(a) if dt == np.int32 else _abi.dptr(a)
        R = self.info()["nods_src"] if reduced is None else np.asarray(reduced).size
        s.G, s.R, s.reduced = int(G), int(R), arr(reduced, np.int32)
        s.rotation_mode = _abi.NODEMAP_ROTATE[rotation] if isinstance(rotation, str) else int(rotation)
        s.east_west_oriented = int(bool(east_west))
        s.cos_m_diff_angle, s.sin_m_diff_angle, s.rotation = float(cos_m_diff_angle), float(sin_m_diff_angle), float(map_rotation)
        s.theta, s.lat, s.lon = arr(theta, np.float64), arr(lat, np.float64), arr(lon, np.float64)
        for name, a in (("theta", theta), ("lat", lat), ("lon", lon)):
            if a is not None and np.asarray(a).size != R:
                raise ValueError(f"{name} has {np.asarray(a).size} entries, expected R = {R}")
        if mapx is not None:
            keep.append(mapx)
            s.map = C.pointer(mapx)
        s.delta_t = float(delta_t)
        self._chk(self.L.nxs_nodemap_set_source(self.h, C.byref(s)))
        self._G = int(G)
        del keep

    def receive_rows(self, fields, a=1., b=0., pairs=(), factor=1., bias=0., get=False, in_device=False, out_device=None, stream=None):
        """nxs_nodemap_receive_rows: up to four nodal variables in two launches.  fields: one [G] array per variable (in_device: one device address each); pairs:
        [(j0, j1)] the vector pairs, component 0 first; a, b, factor, bias per variable (scalars are broadcast); get: store factor*x + bias, else x.  Returns
        [n_var, N] rows -- or, with out_device (one device address of an [N] row per variable), None.  stream: a hipStream_t as an int, None for the library's own."""
        i = self.info()
        n = len(fields)
        co = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (max(n, 1),))) for v in (a, b, factor, bias)]
        pr = np.full(max(n, 1), -1, np.int32)
        for j0, j1 in pairs:
            pr[j0] = j1
        src, dst, keep, flags = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))(), [], 0
        for k, f in enumerate(fields):
            if in_device:
                src[k] = int(f)
            else:
                arr = np.ascontiguousarray(f, np.float64).ravel()
                if arr.size != getattr(self, "_G", arr.size):
                    raise ValueError(f"field {k} has {arr.size} points, expected {self._G}")
                keep.append(arr)
                src[k] = arr.ctypes.data
        flags |= self.IN_DEVICE if in_device else 0
        flags |= self.GET if get else 0
        out = None
        if out_device is not None:
            if len(out_device) != n:
                raise ValueError("one output row per field expected")
            for k, p in enumerate(out_device):
                dst[k] = int(p)
            flags |= self.OUT_DEVICE
        else:
            out = np.empty((n, i["N"]))
            for k in range(n):
                dst[k] = out[k].ctypes.data
        self._chk(self.L.nxs_nodemap_receive_rows(self.h, n, src, _abi.dptr(co[0]), _abi.dptr(co[1]), _abi.iptr(pr) if len(pairs) else None, _abi.dptr(co[2]),
                                                  _abi.dptr(co[3]), dst, flags, C.c_void_p(int(stream)) if stream else None))
        del keep
        return out

    def debug_source(self, n_var):
        """Test door: loaded_data of the last receive, [n_var, R]."""
        out = np.empty((int(n_var), self.info()["nods_src"]))
        self._chk(self.L.nxs_nodemap_debug_source(self.h, _abi.dptr(out), int(n_var)))
        return out

    def _load_struct(self, fields, n_step, scale_factor=1., add_offset=0., a=1., b=0., pairs=(), in_device=False):
        """(nxs_nodemap_load, what it points to) of n_step*n_var fields in loadDataset's order fstep*n_var + j; the coefficients per column (scalars are broadcast)."""
        n_cols, n_step = len(fields), int(n_step)
        if not 1 <= n_cols <= _abi.NXS_NODEMAP_MAX_LOAD or n_step not in (1, 2) or n_cols % n_step:
            raise ValueError(f"{n_cols} fields for n_step = {n_step}: n_step*n_var fields (n_var 1 .. 4, n_step 1 or 2) expected")
        l, keep = _abi.NodemapLoad(), []
        l.n_step, l.n_var = n_step, n_cols // n_step
        src = (C.c_void_p * _abi.NXS_NODEMAP_MAX_LOAD)()
        for k, f in enumerate(fields):
            if in_device:
                src[k] = int(f) if f is not None else None
            elif f is not None:
                arr = np.ascontiguousarray(f, np.float64).ravel()
                if arr.size != getattr(self, "_G", arr.size):
                    raise ValueError(f"field {k} has {arr.size} points, expected {self._G}")
                keep.append(arr)
                src[k] = arr.ctypes.data
        keep.append(src)
        l.fields = C.cast(src, C.POINTER(C.c_void_p))
        for name, v in (("scale_factor", scale_factor), ("add_offset", add_offset), ("a", a), ("b", b)):
            co = np.broadcast_to(np.asarray(v, np.float64), (n_cols,))
            for k in range(n_cols):
                getattr(l, name)[k] = co[k]
        for j in range(4):
            l.pairs[j] = -1
        for j0, j1 in pairs:
            l.pairs[j0] = j1
        return l, keep

    def load_rows(self, fields, n_step=2, scale_factor=1., add_offset=0., a=1., b=0., pairs=(), skip=(), in_device=False, out_device=None, stream=None):
        """nxs_nodemap_load_rows: one loadDataset of a dataset on a triangulated source in two launches.  fields: n_step*n_var [G] arrays in the order fstep*n_var + j
        (in_device: one device address each); scale_factor, add_offset, a, b per COLUMN (scalars are broadcast); pairs: [(j0, j1)] the vector pairs of VARIABLES,
        transformed in every forcing step; skip: columns that are loaded but not gathered.  Returns [n_cols, N] rows (a skipped column's row is NaN) -- or, with
        out_device (one device address of an [N] row per column, None / 0 skips), None.  stream: a hipStream_t as an int, None for the library's own."""
        i = self.info()
        l, keep = self._load_struct(fields, n_step, scale_factor, add_offset, a, b, pairs, in_device)
        n_cols = len(fields)
        dst, flags, out = (C.c_void_p * _abi.NXS_NODEMAP_MAX_LOAD)(), (self.IN_DEVICE if in_device else 0), None
        if out_device is not None:
            if len(out_device) != n_cols:
                raise ValueError("one output row per column expected")
            for k, p in enumerate(out_device):
                dst[k] = int(p) if p else None
            flags |= self.OUT_DEVICE
        else:
            out = np.full((n_cols, i["N"]), np.nan)
            for k in range(n_cols):
                dst[k] = None if k in skip else out[k].ctypes.data
        self._chk(self.L.nxs_nodemap_load_rows(self.h, C.byref(l), dst, flags, C.c_void_p(int(stream)) if stream else None))
        del keep
        return out

    def debug_load(self, n_cols):
        """Test door: loaded_data of the last load, [n_cols, R]."""
        out = np.empty((int(n_cols), self.info()["nods_src"]))
        self._chk(self.L.nxs_nodemap_debug_load(self.h, _abi.dptr(out), int(n_cols)))
        return out


def _declare_nodemap():
    L = _lib()
    if not hasattr(L, "_nodemap_declared"):
        D, I, V = _abi.c_double_p, _abi.c_int32_p, C.c_void_p
        P32 = C.POINTER(C.c_int32)
        L.nxs_nodemap_create.argtypes = [V, D, D, C.c_int32, C.c_int32, C.POINTER(V)]
        L.nxs_nodemap_destroy.argtypes = [V]
        L.nxs_nodemap_info.argtypes = [V, P32, P32, P32]
        L.nxs_nodemap_device.argtypes = [V, P32]
        L.nxs_nodemap_export.argtypes = [V, I, I, I, D, D, D]
        L.nxs_nodemap_import.argtypes = [C.c_int32, C.c_int32, C.c_int32, I, I, I, D, D, D, C.POINTER(V)]
        L.nxs_nodemap_set_source.argtypes = [V, C.POINTER(_abi.NodemapSource)]
        L.nxs_nodemap_receive_rows.argtypes = [V, C.c_int32, C.POINTER(V), D, D, I, D, D, C.POINTER(V), C.c_int32, V]
        L.nxs_nodemap_debug_source.argtypes = [V, D, C.c_int32]
        L.nxs_nodemap_load_rows.argtypes = [V, C.POINTER(_abi.NodemapLoad), C.POINTER(V), C.c_int32, V]
        L.nxs_nodemap_debug_load.argtypes = [V, D, C.c_int32]
        for n in ("create", "destroy", "info", "device", "export", "import", "set_source", "receive_rows", "debug_source", "load_rows", "debug_load"):
            getattr(L, "nxs_nodemap_" + n).restype = C.c_int
        L._nodemap_declared = True
    return L


def gridmap_debug_receive_lists(mode: int) -> int:
    """Test door: 0 = receive_rows reads cell and weight through the index list, 1 = through copies in transposed order.  Returns the mode before."""
    L = _declare_gridmap()
    prev = C.c_int32(0)
    rc = L.nxs_gridmap_debug_receive_lists(int(mode), C.byref(prev))
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    return prev.value


def _declare_gridmap():
    L = _lib()
    if not hasattr(L, "_gridmap_declared"):
        D, I, V = _abi.c_double_p, _abi.c_int32_p, C.c_void_p
        P32, P64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        L.nxs_gridmap_create.argtypes = [V, D, D, D, D, C.c_int32, C.POINTER(V)]
        L.nxs_gridmap_destroy.argtypes = [V]
        L.nxs_gridmap_info.argtypes = [V, P32, P64, P32, P32, P32, P32]
        L.nxs_gridmap_mesh_to_grid.argtypes = [V, V, V, C.c_int32, C.c_double, C.c_int32]
        L.nxs_gridmap_grid_to_mesh.argtypes = [V, V, V, C.c_int32, C.c_int32]
        L.nxs_gridmap_export.argtypes = [V, I, I, I, D, D, D]
        L.nxs_gridmap_import.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, I, I, I, D, D, D, C.POINTER(V)]
        L.nxs_gridmap_restrict.argtypes = [V, I, C.c_int32, C.POINTER(V)]
        L.nxs_gridmap_debug_chunk.argtypes = [C.c_int32, P32]
        L.nxs_gridmap_receive_rows.argtypes = [V, C.c_int32, C.POINTER(V), D, D, D, D, C.POINTER(V), C.c_int32, V]
        L.nxs_gridmap_debug_receive_lists.argtypes = [C.c_int32, P32]
        L.nxs_gridmap_send_rows.argtypes = [V, C.c_int32, V, V, C.c_int32, V]
        for n in ("create", "destroy", "info", "mesh_to_grid", "grid_to_mesh", "export", "import", "restrict", "debug_chunk", "receive_rows", "debug_receive_lists", "send_rows"):
            getattr(L, "nxs_gridmap_" + n).restype = C.c_int
        L._gridmap_declared = True
    return L


def gridmap_debug_chunk(cells=0):
    """Test door: build the weights in chunks of `cells` cells (0 = the default); returns the chunks the last build took."""
    L = _declare_gridmap()
    last = C.c_int32(0)
    rc = L.nxs_gridmap_debug_chunk(int(cells), C.byref(last))
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    return last.value


TRIANGLE, BILINEAR, NEAREST = 0, 1, 2


def InterpFromGridToMeshx(x_in, y_in, data, x_mesh, y_mesh, default_value=1e8, interp=BILINEAR, row_major=False, device=0, return_info=False):
    """Structured grid -> mesh nodes (forcing ingest), argument meaning of contrib/bamg's InterpFromGridToMeshx
    (model/externaldata.cpp:1436): data [M, N, N_data] ([N, M, N_data] when row_major), x_in / y_in centres or contours."""
    L = _lib()
    if not hasattr(L, "_g2m_declared"):
        D = _abi.c_double_p
        L.nxs_interp_grid_to_mesh.argtypes = [D, D, C.c_int32, D, C.c_int32, D, C.c_int32, C.c_int32, C.c_int32, D, D, C.c_int32, C.c_double, C.c_int32,
                                              C.c_int32, C.c_int32, C.POINTER(C.c_double)]
        L.nxs_interp_grid_to_mesh.restype = C.c_int
        L._g2m_declared = True
    f64 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    x_in, y_in, data, xm, ym = f64(x_in), f64(y_in), f64(data), f64(x_mesh), f64(y_mesh)
    if data.ndim == 2:
        data = data[:, :, None]
    M, N = (data.shape[1], data.shape[0]) if row_major else (data.shape[0], data.shape[1])
    out = np.empty((xm.size, data.shape[2]))
    ms = C.c_double(0.0)
    rc = L.nxs_interp_grid_to_mesh(_abi.dptr(out), _abi.dptr(x_in), x_in.size, _abi.dptr(y_in), y_in.size, _abi.dptr(data), M, N, data.shape[2],
                                   _abi.dptr(xm), _abi.dptr(ym), xm.size, float(default_value), int(interp), int(bool(row_major)), device, C.byref(ms))
    if rc:
        raise NxsError(rc, (L.nxs_interp_last_error() or b"").decode())
    return (out, {"kernel_ms": ms.value}) if return_info else out
