"""Generates tests/golden/nodal_receive.npz with the REAL contrib/bamg (oracle/_ref, built by `python __graft_entry__.py` where the reference is present):
    python tests/golden/make_nodal_receive_golden.py

InterpFromMeshToMesh2dx with isdefault = 0 -- statement for statement InterpFromMeshToMesh2dx_weights followed by InterpFromMeshToMesh2dx_apply -- from small
triangulated exchange grids (tests/nodal_receive_ref.source: 7 x 9 curvilinear points; no mask / a masked strip / a notched wet set) to the nodes of
cases.mesh_with_holes("small") scaled to reach 10 % beyond the source's box (targets inside, beyond a hull edge, in the cone of a hull vertex).
  W_<case>   [N, R]  the interpolation of the IDENTITY matrix (N_data = R columns): a*1 + b*0 + c*0 returns each weight exactly, so W holds the real library's
                     area coordinates at the real library's vertices                                                         (full, strip)
  Y_<case>   [N, 2]  the interpolation of nodal_receive_ref.awkward_data: negative values, a row of zeros, one NaN source node (full, strip)
  px_, py_<case>     the targets;  fill_notch: the targets of the notched case that lie in a triangle of the completion, where _weights throws
NO TIES: the inputs are seeded (nodal_receive_ref.SEED) so that no target inside a source has a zero integer area coordinate -- the reference's answer there depends
on its triangle walk; main() asserts that ZERO targets are left out before it writes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nodal_receive_ref as R  # noqa: E402

OUT = os.path.join(HERE, "nodal_receive.npz")


def real_bamg(src, data, px, py):
    from oracle import pyoracle as O
    return O.bamg_interp_mesh_to_mesh((src["tri"] + 1).astype(np.int32).ravel(), src["x"], src["y"], data, px, py, False, 0.)


def main():
    out = {}
    for name in R.CASES:
        src = R.source(name)
        px, py = R.targets(src)
        assert R.ties(src, px, py) == 0, (name, R.ties(src, px, py))      # pick another SEED rather than leave a target out
        out["px_" + name], out["py_" + name] = px, py
        fill = R.in_fill(src, px, py)
        if name == "notch":
            assert fill.size > 0
            out["fill_notch"] = fill.astype(np.int32)
            continue
        assert fill.size == 0, (name, fill)
        n = src["reduced"].size
        W = real_bamg(src, np.eye(n), px, py)
        assert ((W != 0).sum(1) >= 1).all() and ((W != 0).sum(1) <= 3).all()
        nnz = (W != 0).sum(1)
        it, _ = R.D.locate(src["x"], src["y"], src["tri"], px, py)
        assert (it >= 0).any() and ((it < 0) & (nnz == 1)).any() and ((it < 0) & (nnz >= 2)).any(), "targets inside, at a hull vertex and on a hull edge are all needed"
        d = R.awkward_data(src)
        Y = real_bamg(src, d, px, py)
        v, a = R.weights_from_dense(W, src["tri"])
        assert np.array_equal(R.dense(v, a, n), W)
        for k in range(2):      # the restated apply on the weights read out of W gives the real library's bits: the order of the three products is pinned
            assert R.equal(R.apply(v, a, d[:, k]), Y[:, k]), (name, k)
        assert np.isnan(Y).any() and not np.isnan(Y).all(0).any()
        out["W_" + name], out["Y_" + name] = W, Y
        print(name, "targets", px.size, "inside", int((it >= 0).sum()), "hull edge", int(((it < 0) & (nnz >= 2)).sum()), "hull vertex", int(((it < 0) & (nnz == 1)).sum()),
              "NaN", int(np.isnan(Y).sum()))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes; in the notch:", out["fill_notch"].size)


if __name__ == "__main__":
    main()
