"""One loadDataset of a dataset interpolated with InterpFromMeshToMesh2dx, restated line by line (numpy; no device, no library):

    the tail of loadDataset   model/externaldata.cpp:886-931     d = (d*scale_factor + add_offset)*a + b on data_in_tmp (four roundings), NaN -> 0.,
                                                                 loaded_data[fstep][i] = d[reduced[i]]
    transformData             externaldata.cpp:944-1288          per forcing step and pair: the east/north branch (tests/nodal_forcing_ref.transform), then
                                                                 rotation_angle != 0. (:1246-1261) else gridded_rotation_angle (:1263-1281)
    interpolateDataset        externaldata.cpp:1334-1383         data_in[n_cols*i + fstep*n_var + j] = loaded_data of variable j, step fstep
                              :1442-1448                         InterpFromMeshToMesh2dx(..., isdefault = false): a0*d[v0] + a1*d[v1] + a2*d[v2], left to right
                                                                 (contrib/bamg/src/InterpFromMeshToMesh2dx.cpp:157-159)

and the seeded inputs of tests/golden/mesh_forcing.npz (made by tests/golden/make_mesh_forcing_golden.py with the REAL bamg).  Columns are in loadDataset's order
c = fstep*n_var + j throughout.  `mistake` plants one wrong statement at a time (tests/test_mesh_forcing_ref.py: each changes a bit)."""
import os

import numpy as np

import cases
import nodal_forcing_ref as NF
import nodal_receive_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "mesh_forcing.npz")
SEED = 23
N_VAR, N_STEP = 3, 2
SOURCES = ("full", "strip")
KINDS = ("nodes", "elements")
MISTAKES = ("nan_after_rotation", "ab_before_scale", "snapshots_swapped", "column_index", "rotation_first_step_only", "reduced_ignored")
BARY_SCALE = 1.1      # the barycentres' mesh reaches 10 % beyond the source's box, as the node targets do (a tie: change this, not the count of targets)

# per COLUMN (two forcing steps may be two files): scale_factor != 1 and add_offset != 0 on the third variable, a != 1 and b != 0 on the second; the third variable
# of the second step carries both, so that the ORDER of the two affine maps shows
COEF = dict(scale_factor=[1., 1., 0.01, 1., 1., 0.02], add_offset=[0., 0., 1.5, 0., 0., 1.25], a=[1., -0.5, 1., 1., -0.5, 1.5], b=[0., 0.25, 0., 0., 0.25, -0.125])
PAIRS = [(0, 1)]


def coef(n_var=N_VAR, n_step=N_STEP):
    """the coefficients of the first n_var variables of the first n_step forcing steps, per column"""
    cols = [s * N_VAR + j for s in range(n_step) for j in range(n_var)]
    return {k: np.array([v[c] for c in cols]) for k, v in COEF.items()}


def coef8():
    """four variables, two steps: the fixture's six columns and a fourth variable with all four coefficients off their defaults"""
    out = {}
    extra = dict(scale_factor=[0.5, 0.25], add_offset=[-1., 2.], a=[3., -1.5], b=[0.125, -0.75])
    for k, v in COEF.items():
        out[k] = np.array(v[:3] + [extra[k][0]] + v[3:] + [extra[k][1]])
    return out


def raw_fields(G, reduced=None, n_cols=N_VAR * N_STEP, seed=SEED):
    """Seeded [n_cols, G] fields as read from the file (data_in_tmp): every point that is not in `reduced` (the land column of the strip case) holds the fill value the reduced index must
    skip, NaN at several WET points -- in both components of the pair (at different points) and in the scalar, in both forcing steps -- two rows inside
    the wet set, so that no triangle behind a hull edge holds them (nodal_receive_ref.awkward_data).  No Inf."""
    rng = np.random.default_rng(seed + n_cols)
    f = rng.normal(0.1, 0.5, (n_cols, G))
    if reduced is not None:
        land = np.ones(G, bool)
        land[reduced] = False
        f[:, land] = 1e20
    wet_inside = [2 * R.NV + 3, 3 * R.NV + 4, 4 * R.NV + 5, 3 * R.NV + 6, 2 * R.NV + 5, 4 * R.NV + 2, 3 * R.NV + 2, 4 * R.NV + 4]
    for c in range(n_cols):
        f[c, wet_inside[c % len(wet_inside)]] = np.nan
    f[0, wet_inside[5]] = np.nan      # a second NaN in the first component
    return f


def load_value(d, scale_factor, add_offset, a, b, mistake=None):
    """externaldata.cpp:908 on an array: four separately rounded operations"""
    with np.errstate(invalid="ignore", over="ignore"):
        if mistake == "ab_before_scale":
            return (d * a + b) * scale_factor + add_offset
        t = d * scale_factor
        t = t + add_offset
        t = t * a
        t = t + b
    return t


def loaded_data(fields, reduced, n_var, n_step, scale_factor=1., add_offset=0., a=1., b=0., pairs=(), rotate=None, east_west=None, details=None, mistake=None):
    """The tail of loadDataset + transformData: [n_step*n_var, R], row fstep*n_var + j.  fields [n_step*n_var, G] in the same order; the coefficients per column
    (scalars are broadcast); pairs = [(j0, j1)] of VARIABLES; rotate = None or (c, s), scalars or [R] rows; east_west = None or dict(lat, lon [R], forward)."""
    fields = np.asarray(fields, np.float64)
    n_cols = n_var * n_step
    assert fields.shape[0] == n_cols
    co = [np.broadcast_to(np.asarray(v, np.float64), (n_cols,)) for v in (scale_factor, add_offset, a, b)]
    idx = np.arange(reduced.size) if mistake == "reduced_ignored" else reduced
    out = np.empty((n_cols, reduced.size))
    for c in range(n_cols):
        t = load_value(fields[c], co[0][c], co[1][c], co[2][c], co[3][c], mistake)      # on data_in_tmp, every point of the file
        t = t[idx].copy()
        if mistake != "nan_after_rotation":
            t[np.isnan(t)] = 0.                                                          # :923-927
        out[c] = t
    for fstep in range(n_step):
        if mistake == "rotation_first_step_only" and fstep > 0:
            break
        for k, (j0, j1) in enumerate(pairs):
            c0, c1 = fstep * n_var + j0, fstep * n_var + j1
            if east_west is not None:
                cell = np.stack([out[c0], out[c1]], axis=1)[None]
                det = {} if details is not None else None
                cell = NF.transform(cell, east_west["lat"], east_west["lon"], [0.], [(0, 1, True)], east_west["forward"], per_point=True, details=det)
                out[c0], out[c1] = cell[0, :, 0], cell[0, :, 1]
                if details is not None:
                    details[(fstep, k)] = det[0]
            if rotate is not None:
                out[c0], out[c1] = R.rotated(out[c0], out[c1], *rotate)
    if mistake == "nan_after_rotation":
        out[np.isnan(out)] = 0.
    return out


def data_in(loaded, n_var, n_step, mistake=None):
    """externaldata.cpp:1376-1380: [R, n_cols], entry fstep*n_var + j of a point"""
    n_cols = n_var * n_step
    out = np.empty((loaded.shape[1], n_cols))
    for fstep in range(n_step):
        for j in range(n_var):
            src = loaded[((n_step - 1 - fstep) if mistake == "snapshots_swapped" else fstep) * n_var + j]
            out[:, (j * n_step + fstep) if mistake == "column_index" else (fstep * n_var + j)] = src
    return out


def ingest(fields, reduced, n_var, n_step, v, w, mistake=None, **kw):
    """The whole chain: [n_cols, N] rows, row fstep*n_var + j (the transposed data_out of InterpFromMeshToMesh2dx)."""
    d = data_in(loaded_data(fields, reduced, n_var, n_step, mistake=mistake, **kw), n_var, n_step, mistake)
    return np.stack([R.apply(v, w, d[:, c]) for c in range(d.shape[1])])


def fixture_load(name, mistake=None):
    """loaded_data of the fixture's case: three variables, two steps, the (0, 1) pair under the uniform rotation: [6, R]"""
    src = R.source(name)
    return loaded_data(raw_fields(src["G"], src["reduced"]), src["reduced"], N_VAR, N_STEP, pairs=PAIRS, rotate=R.uniform_rotation(), mistake=mistake, **coef())


def scaled_to(src, tx, ty, scale=1.1):
    """points scaled to reach `scale` times the box of the source, about its centre (nodal_receive_ref.targets' statement)"""
    cx, cy = 0.5 * (src["x"].min() + src["x"].max()), 0.5 * (src["y"].min() + src["y"].max())
    px = cx + scale * np.ptp(src["x"]) * (tx - 0.5 * (tx.min() + tx.max())) / np.ptp(tx)
    py = cy + scale * np.ptp(src["y"]) * (ty - 0.5 * (ty.min() + ty.max())) / np.ptp(ty)
    return np.ascontiguousarray(px), np.ascontiguousarray(py)


def targets(src, kind):
    """nodes: nodal_receive_ref.targets; elements: the barycentres of the same mesh (cases.mesh_with_holes("small")), whose NODES are scaled to reach 10 % beyond
    the source's box -- (x0 + x1 + x2) / 3., mesh.bCoordX's statement"""
    if kind == "nodes":
        return R.targets(src)
    tx, ty, tri = cases.mesh_with_holes("small")
    px, py = scaled_to(src, tx, ty, BARY_SCALE)
    bx = (px[tri[:, 0]] + px[tri[:, 1]] + px[tri[:, 2]]) / 3.
    by = (py[tri[:, 0]] + py[tri[:, 1]] + py[tri[:, 2]]) / 3.
    return np.ascontiguousarray(bx), np.ascontiguousarray(by)


def weights(name, kind):
    """(v [N, 3], a [N, 3]) of a fixture case, read out of the real library's interpolation of the identity matrix: the node targets' in
    tests/golden/nodal_receive.npz, the barycentres' in tests/golden/mesh_forcing.npz"""
    W = np.load(R.GOLD)["W_" + name] if kind == "nodes" else np.load(GOLD)["Wb_" + name]
    return R.weights_from_dense(W, R.source(name)["tri"])


def synthetic_case(R_, N, n_cols, seed=SEED):
    """nodal_receive_ref.synthetic_case with n_cols fields that hold NaN now and then"""
    c = R.synthetic_case(R_, N, 1, seed)
    rng = np.random.default_rng(seed + 7 * R_ + N)
    f = rng.normal(0.1, 0.5, (n_cols, c["G"]))
    f[rng.uniform(size=f.shape) < 0.05] = np.nan
    c["fields"] = f
    return c


equal = R.equal
