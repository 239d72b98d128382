"""Shared by the grid-remapping tests: the committed golden cases (tests/golden/bamg_grid_remap.npz, the real bamg's output) and a driver of
tests/native/gridmap_host.cpp, the host build of the code nxs_gridmap_create / _mesh_to_grid / _grid_to_mesh run on the device."""
import os
import struct
import subprocess
import time

import numpy as np

from nextsim_amd import dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bamg_grid_remap.npz")
CASES = ("coarse", "long_rows", "fine", "aligned", "all_land", "one_cell", "inside")
MISS = 1e14          # the miss_val the golden outputs were made with
CAP = 4096           # kMaxVisitBig
# wet cells, entries, longest row as the real routine gave them (printed by tests/golden/make_grid_remap_golden.py)
COUNTS = {"coarse": (10, 335, 49), "long_rows": (6, 1968, 373), "fine": (97, 411, 7), "aligned": (12, 341, 38), "all_land": (0, 0, 0), "one_cell": (1, 52, 52),
          "inside": (144, 315, 6)}

_gold = None


def case(name):
    global _gold
    if _gold is None:
        z = np.load(GOLD)
        _gold = {k: z[k] for k in z.files}
    return {k[len(name) + 1:]: v for k, v in _gold.items() if k.startswith(name + "_")}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(got, want):
    """uint64 equality; NaNs by position only (the sign of a generated NaN differs between x86 and gfx950)."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn]))


def seeds(x, y, tri, px, py):
    """The element holding each P-point by brute force, -1 = in none (counter-clockwise triangles; no P-point of the cases lies on an edge)."""
    out = np.full(px.size, -1, np.int32)
    x0, y0, x1, y1, x2, y2 = x[tri[:, 0]], y[tri[:, 0]], x[tri[:, 1]], y[tri[:, 1]], x[tri[:, 2]], y[tri[:, 2]]
    for i, (qx, qy) in enumerate(zip(px, py)):
        a = (x1 - x0) * (qy - y0) - (y1 - y0) * (qx - x0)
        b = (x2 - x1) * (qy - y1) - (y2 - y1) * (qx - x1)
        c = (x0 - x2) * (qy - y2) - (y0 - y2) * (qx - x2)
        hit = np.flatnonzero((a >= 0) & (b >= 0) & (c >= 0))
        if hit.size:
            out[i] = hit[0]
    return out


def build_host(dst, sanitize=False):
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "nextsim_amd", "csrc")]
    if sanitize:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd + [os.path.join(ROOT, "tests", "native", "gridmap_host.cpp"), "-o", dst])
    return dst


def run_host(binary, tmp, x, y, tri, gridX, gridY, cornerX, cornerY, m2g_in, g2m_in, miss=MISS, local=None, cap=CAP, seed=None):
    """-> dict(program_ms, gridP, off, tris, w, failed, longest, r_gridP, r_off, r_tris, r_w, m2g_out, g2m_out); seed: the element of every P-point when the
    caller knows it (brute force otherwise)"""
    tri = np.ascontiguousarray(tri, np.int32)
    nods, nels, G = x.size, tri.shape[0], gridX.size
    idx = np.ascontiguousarray((tri + 1).ravel(), np.int32)
    nec, _ = dynamics.mesh_connectivity(idx, nods)
    ec = dynamics.mesh_element_connectivity(idx, nods)
    neci = np.ascontiguousarray(np.where(np.isnan(nec), 0, nec).astype(np.int32) - 1)
    eci = np.ascontiguousarray(np.where(np.isnan(ec), 0, ec).astype(np.int32) - 1)
    m2g_in = np.ascontiguousarray(m2g_in, np.float64).reshape(nels, -1)
    nv = m2g_in.shape[1]
    g2m_in = np.ascontiguousarray(g2m_in, np.float64).reshape(G, nv)
    sd = seeds(x, y, tri, gridX, gridY) if seed is None else np.ascontiguousarray(seed, np.int32)
    fin, fout = os.path.join(str(tmp), "gm_in.bin"), os.path.join(str(tmp), "gm_out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", nods, nels, neci.shape[1], G, nv, int(local is not None), cap, 0))
        for a in (tri, neci, eci, sd) + (() if local is None else (np.ascontiguousarray(local, np.int32),)):
            f.write(a.tobytes())
        for a in (x, y, cornerX, cornerY, m2g_in, g2m_in):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
        f.write(struct.pack("d", miss))
    t0 = time.perf_counter()
    subprocess.check_call([binary, fin, fout])
    program_ms = (time.perf_counter() - t0) * 1e3
    raw = open(fout, "rb").read()
    pos = [0]

    def take(dtype, n):
        a = np.frombuffer(raw, dtype, n, pos[0]).copy()
        pos[0] += a.nbytes
        return a
    rows, n, failed, longest = take(np.int32, 4)
    out = dict(program_ms=program_ms, failed=int(failed), longest=int(longest), gridP=take(np.int32, rows), off=take(np.int32, rows + 1), tris=take(np.int32, n), w=take(np.float64, n))
    r_rows, r_n = take(np.int32, 2)
    out.update(r_gridP=take(np.int32, r_rows), r_off=take(np.int32, r_rows + 1), r_tris=take(np.int32, r_n), r_w=take(np.float64, r_n))
    out.update(m2g_out=take(np.float64, G * nv).reshape(G, nv), g2m_out=take(np.float64, nels * nv).reshape(nels, nv))
    assert pos[0] == len(raw)
    return out
