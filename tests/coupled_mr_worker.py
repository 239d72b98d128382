"""Worker of tests/test_gpu_coupled_multirank.py: one rank (one process) of a several-rank run on one device with the coupled build's terms attached --
device-direct mailboxes, the exchange inside the sub-step kernels.  Three collective runs from the same start:
  A  wave stress, cum_damage and three floe-size bins attached; explicitSolve, update: against the composed multi-rank oracle, the bins' identity
  B  the same with garbage in tau_wi on this rank's GHOST nodes: every array must keep the bits of A
  C  healing off, cum_damage from a non-zero field, explicitSolve: the damage identity over the S sub-steps
Writes report<rank>.json; the parent asserts."""
import json, os, sys, traceback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch, torch.distributed as dist   # torch first: its bundled HIP runtime is the process's runtime
import cases
from nextsim_amd import dynamics
from test_coupled_abi import composed_explicit_solve, wave_stress_at

rank = int(os.environ["RANK"]); world = int(os.environ["WORLD_SIZE"])
out = sys.argv[1]; kind = sys.argv[2]; over = json.loads(sys.argv[3]); options = over.pop("options", {})
dist.init_process_group("gloo", rank=rank, world_size=world)
STATE_KEYS = ("VT", "UM", "UT", "sigma0", "sigma1", "sigma2", "damage", "conc", "thick", "snow_thick",
              "ridge_ratio", "conc_young", "h_young", "hs_young", "conc_myi", "thick_myi")
NBINS = 3
report = dict(rank=rank, ok=False)


def all_gather(obj):
    res = [None] * world
    dist.all_gather_object(res, obj)
    return res


def main():
    from oracle import pyoracle as O
    gm, p, g, lms, fields = cases.make_case(kind, nparts=world, **over)
    lm, f = lms[rank], fields[rank]
    Ne, Nn, No = lm.num_elements, lm.num_nodes, lm.local_ndof
    L = max(np.ptp(gm.x), np.ptp(gm.y))
    taus = [wave_stress_at(m.coord_x, m.coord_y, L) for m in lms]
    rng = np.random.default_rng(100 + rank)
    cum0 = rng.uniform(0.5, 3., Ne)
    fsd0 = rng.uniform(0.01, 0.9, (NBINS, Ne))
    fe = dynamics.FiniteElementDynamics(p, device=int(os.environ.get("NXS_TEST_DEVICE", "0")))
    fe.set_mesh(lm)
    for k, v in options.items():
        fe.set_option(k, v)
    if not fe.ipc_setup(all_gather):
        raise RuntimeError("ipc self-test failed: " + getattr(fe, "_ipc_error", ""))

    def run(state, tau, cum, fsd, update):
        fe.put_state(state); fe.set_forcing(state)
        fe.set_wave_stress(tau); fe.put_coupled(cum_damage=cum, conc_fsd=fsd)
        fe.set_option("prepare", 1)
        all_gather(0)                       # nobody steps before every rank's state is resident
        fe.explicitSolve(); fe.synchronize()
        res = dict(surface_old=fe.get_diag()["surface"])
        if update:
            fe.update(); fe.synchronize()
        res["surface_new"] = fe.get_diag()["surface"]
        res["D_tau_a"] = fe.get_diag()["D_tau_a"]
        res.update(fe.get_state())
        res.update(fe.get_coupled(num_fsd_bins=NBINS if fsd is not None else 0))
        res["traffic"] = fe.traffic_model()
        res["nrec"] = fe.debug_array("nrec").reshape(Nn, 10)
        all_gather(0)
        return res

    # ---- A
    a = run(f, taus[rank], cum0, fsd0, True)
    report["substep_kernel"] = a["traffic"]["substep_kernel_name"]; report["halo_in_kernel"] = a["traffic"]["halo_in_kernel"]
    report["prep_kernel"] = a["traffic"]["prep_kernel_name"]
    report["crash"] = fe.checkFieldsFast()
    # the nodal records of EVERY node, ghosts included, carry D_tau_a + tau_wi in slots 6, 7 (one IEEE addition: the same bits from numpy): no prep kernel skips a ghost
    want_rec = a["D_tau_a"] + taus[rank]
    rec_ok = (a["nrec"][:, 6].view(np.uint64) == want_rec[:Nn].view(np.uint64)) & (a["nrec"][:, 7].view(np.uint64) == want_rec[Nn:].view(np.uint64))
    report["records_wrong_own"] = int((~rec_ok[:No]).sum()); report["records_wrong_ghost"] = int((~rec_ok[No:]).sum())
    ranks = [O.OracleRank(m, p, ff) for m, ff in zip(lms, fields)]
    composed_explicit_solve(ranks, taus)
    for r in ranks:
        r.update()
    plain = [O.OracleRank(m, p, ff) for m, ff in zip(lms, fields)]
    O.multirank_step(plain)
    report["errs"] = {k: cases.rel_err(a[k], ranks[rank].arr[k]) for k in STATE_KEYS}
    report["term_size"] = cases.rel_err(ranks[rank].arr["VT"], plain[rank].arr["VT"])      # what the term changes: far above the tolerance
    report["D_tau_a_err"] = cases.rel_err(a["D_tau_a"], plain[rank].work_array("D_tau_a", 2 * Nn))
    on_neumann = np.isin(lm.indices.reshape(-1, 3) - 1, lm.neumann_flags).any(1)
    scaled = (f["conc"] > 0.) & ~on_neumann
    want = np.where(scaled, fsd0 * (a["surface_old"] / a["surface_new"]), fsd0)
    report["fsd_exact"] = bool(np.array_equal(a["conc_fsd"].view(np.uint64), want.view(np.uint64)))
    report["fsd_scaled"] = int(scaled.sum()); report["fsd_changed"] = int((a["conc_fsd"][0] != fsd0[0]).sum())
    # healing on: the oracle's branch trace says which elements cannot / must have accumulated
    tr_ranks = [O.OracleRank(m, p, ff) for m, ff in zip(lms, fields)]
    for r in tr_ranks:
        r.enable_branch_trace()
    composed_explicit_solve(tr_ranks, taus)
    tr = tr_ranks[rank].branch_trace()
    never = tr["damage_substeps"] == 0
    sure = (tr["damage_substeps"] > 0) & ((tr["flags"] & 1) == 0)
    bbm = p.dynamics_type == 0
    report["cum_never_kept"] = bool(np.array_equal(a["cum_damage"][never].view(np.uint64), cum0[never].view(np.uint64)))
    report["cum_sure_grew"] = bool(np.all(a["cum_damage"][sure] > cum0[sure])) if bbm else True
    report["n_never"] = int(never.sum()); report["n_sure"] = int(sure.sum())
    # ---- B: garbage on the ghost nodes
    tau_b = taus[rank].copy()
    tau_b[No:Nn] = 1e3 * rng.normal(size=Nn - No); tau_b[Nn + No:] = -1e3 * rng.normal(size=Nn - No)
    b = run(f, tau_b, cum0, fsd0, True)
    report["ghosts"] = int(Nn - No)
    want_rec = b["D_tau_a"] + tau_b                      # ... and the garbage does arrive in the ghosts' records: they are written, just never solved from
    report["garbage_records_wrong_ghost"] = int(((b["nrec"][No:, 6].view(np.uint64) != want_rec[No:Nn].view(np.uint64)) | (b["nrec"][No:, 7].view(np.uint64) != want_rec[Nn + No:].view(np.uint64))).sum())
    report["ghost_tau_differs"] = [k for k in STATE_KEYS + ("cum_damage", "conc_fsd", "D_tau_a", "surface_new") if not np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64))]
    # ---- C: the damage identity, healing off
    fc = dict(f); fc["time_relaxation_damage"] = np.full(Ne, 1e300)
    c = run(fc, taus[rank], cum0, None, False)
    S = p.substeps
    keep = (fc["conc"] > 0.1) & (c["conc"] > 0.1)
    lhs = np.abs((c["cum_damage"] - cum0) - (c["damage"] - fc["damage"]))[keep]
    bound = (S * 2.**-52 * np.maximum(1., c["cum_damage"]))[keep]
    report["identity4_worst"] = float((lhs / bound).max()) if lhs.size else 0.
    report["identity4_damaged"] = int((c["cum_damage"] != cum0).sum())
    report["ok"] = True
    all_gather(0)                           # keep every mailbox alive until all ranks are done
    fe.close()


try:
    main()
except Exception as e:  # noqa: BLE001
    report["error"] = repr(e) + "\n" + traceback.format_exc()
json.dump(report, open(os.path.join(out, f"report{rank}.json"), "w"))
try:
    dist.barrier(); dist.destroy_process_group()
except Exception:
    pass
