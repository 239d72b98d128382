"""Generates tests/golden/mesh_forcing.npz with the REAL contrib/bamg (oracle/_ref, built by `python __graft_entry__.py` where the reference is present):
    python tests/golden/make_mesh_forcing_golden.py

One loadDataset of a dataset on a triangulated source (externaldata.cpp:886-931, 944-1288, 1334-1383, 1442-1448): the restated load of seeded raw fields
(tests/mesh_forcing_ref.fixture_load: three variables, two forcing steps, scale_factor / add_offset and a / b off their defaults, the (0, 1) pair under the uniform
rotation, NaN at several wet points) interpolated by InterpFromMeshToMesh2dx with isdefault = 0 -- O.bamg_interp_mesh_to_mesh(..., False, 0.) -- from the sources
nodal_receive_ref.source("full") and ("strip") to
  nodes      the node targets already in tests/golden/nodal_receive.npz
  elements   the barycentres of the same scaled cases.mesh_with_holes("small"), reaching 10 % beyond the source's box
  Y_<kind>_<source>   [N, 6]  data_out in loadDataset's order, index fstep*n_var + j
  Wb_<source>         [Ne, R] the interpolation of the IDENTITY matrix at the barycentres: the real library's area coordinates at its vertices (the nodes' are
                              W_<source> of nodal_receive.npz)
  bx_, by_<source>    the barycentres
main() asserts before it writes: ZERO ties among the barycentres and the nodes (a zero integer area coordinate: the reference's answer depends on its walk), zero
targets in a fill triangle, targets inside, beyond a hull edge and in a hull vertex's cone all present in every case, no Inf in the data, and that the restated
gather on the weights read out of W gives the real library's bits.  If a tie turns up change mesh_forcing_ref.BARY_SCALE, not the count of targets."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mesh_forcing_ref as MF  # noqa: E402
import nodal_receive_ref as R  # noqa: E402

OUT = os.path.join(HERE, "mesh_forcing.npz")


def real_bamg(src, data, px, py):
    from oracle import pyoracle as O
    return O.bamg_interp_mesh_to_mesh((src["tri"] + 1).astype(np.int32).ravel(), src["x"], src["y"], data, px, py, False, 0.)


def main():
    out = {}
    nodal = np.load(R.GOLD)
    for name in MF.SOURCES:
        src = R.source(name)
        n = src["reduced"].size
        loaded = MF.fixture_load(name)
        d = MF.data_in(loaded, MF.N_VAR, MF.N_STEP)
        assert d.shape == (n, 6) and np.isfinite(d).all() and np.abs(d).max() < 1e6      # no Inf, no NaN (zeroed), no land value
        for kind in MF.KINDS:
            px, py = MF.targets(src, kind)
            if kind == "nodes":
                assert np.array_equal(px, nodal["px_" + name]) and np.array_equal(py, nodal["py_" + name])
                W = nodal["W_" + name]
            else:
                W = real_bamg(src, np.eye(n), px, py)
                out["bx_" + name], out["by_" + name], out["Wb_" + name] = px, py, W
            assert R.ties(src, px, py) == 0, (name, kind, R.ties(src, px, py))      # change BARY_SCALE rather than leave a target out
            assert R.in_fill(src, px, py).size == 0, (name, kind)
            nnz = (W != 0).sum(1)
            assert (nnz >= 1).all() and (nnz <= 3).all()
            it, _ = R.D.locate(src["x"], src["y"], src["tri"], px, py)
            assert (it >= 0).any() and ((it < 0) & (nnz == 1)).any() and ((it < 0) & (nnz >= 2)).any(), "targets inside, at a hull vertex and on a hull edge are all needed"
            Y = real_bamg(src, d, px, py)
            v, a = R.weights_from_dense(W, src["tri"])
            assert np.array_equal(R.dense(v, a, n), W)
            for c in range(6):      # the restated gather on the weights read out of W gives the real library's bits
                assert R.equal(R.apply(v, a, d[:, c]), Y[:, c]), (name, kind, c)
            assert np.isfinite(Y).all()
            out[f"Y_{kind}_{name}"] = Y
            print(name, kind, "targets", px.size, "inside", int((it >= 0).sum()), "hull edge", int(((it < 0) & (nnz >= 2)).sum()), "hull vertex", int(((it < 0) & (nnz == 1)).sum()))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
