"""The coupled build's terms on several ranks of one device: device-direct mailboxes with the exchange inside the sub-step kernels
(k_substep_pair<HALO, CUM> with option pair_regs = 1, k_substep_fused<HALO, CUM> without), regular and ragged partitions.  Per rank
(tests/coupled_mr_worker.py): the step with a wave stress against the composed MULTI-RANK oracle (<= 1e-10, the tolerance of tests/test_gpu_multirank.py for
the same comparison), the exact identities of the cumulated damage and of the floe-size bins, and values of tau_wi on a rank's GHOST nodes changing no bit of
any array (only owned nodes are solved, FE.cpp:10472) while the prep kernels still write those nodes' records."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run(world, kind, over, tmp_path, timeout=300):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "coupled_mr_worker.py"), str(tmp_path), kind, json.dumps(over)], env=env))
    for p in procs:
        try:
            p.wait(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("multi-rank workers hung")
    return [json.load(open(tmp_path / f"report{r}.json")) for r in range(world)]


# (option prep_fused 1 forces k_prep_fused<WAVE> + k_prep_ghost_nodes<WAVE> on these small partitions -- automatic from 500 k triangles per rank --, else the two
#  separate prep kernels do the ghost nodes)
@pytest.mark.parametrize("world,over,options,kernel", [(2, {}, {"pair_regs": 1}, "k_substep_pair"), (3, {"ragged_seed": 1}, {"pair_regs": 1}, "k_substep_pair"),
                                                       (2, {}, {}, "k_substep_fused"), (3, {"ragged_seed": 1}, {}, "k_substep_fused"),
                                                       (2, {"dynamics_type": 3}, {"pair_regs": 1}, "k_substep_pair"),
                                                       (2, {}, {"pair_regs": 1, "prep_fused": 1}, "k_substep_pair"), (3, {"ragged_seed": 1}, {"pair_regs": 1, "prep_fused": 1}, "k_substep_pair"),
                                                       (3, {"ragged_seed": 1}, {"prep_fused": 1}, "k_substep_fused"), (2, {"dynamics_type": 3}, {"prep_fused": 1}, "k_substep_fused")])
def test_coupled_terms_on_several_ranks(world, over, options, kernel, tmp_path):
    reps = _run(world, "small", dict(over, options=options), tmp_path)
    evp = bool(over.get("dynamics_type"))
    for r in reps:
        print({k: v for k, v in r.items() if k != "error"})
    for r in reps:
        assert r["ok"], r.get("error", r)
        assert r["substep_kernel"] == kernel and r["halo_in_kernel"] == 1, r
        assert r["crash"] == 0
        if options.get("prep_fused") == 1:
            assert r["prep_kernel"] == "k_prep_fused", r
        else:
            assert r["prep_kernel"].startswith("k_prep_elements"), r
        assert r["records_wrong_own"] == 0 and r["records_wrong_ghost"] == 0 and r["garbage_records_wrong_ghost"] == 0, r     # no prep kernel skips a ghost node
        for k, e in r["errs"].items():                      # 1. against the composed multi-rank oracle
            assert e <= 1e-10, (r["rank"], k, e)
        assert r["term_size"] > 1e-7, r                      # (the term is far above the tolerance: the check cannot pass without it)
        assert r["D_tau_a_err"] <= 1e-15, r                  # the diagnostic stays drag * wind
        assert r["fsd_exact"] and r["fsd_scaled"] > 10 and r["fsd_changed"] > 10, r            # 6.
        assert r["cum_never_kept"] and r["cum_sure_grew"], r
        if evp:
            assert r["identity4_damaged"] == 0, r            # (EVP leaves cum_damage alone)
        else:
            assert r["n_sure"] > 10 and r["identity4_damaged"] > 10, r
            assert r["identity4_worst"] <= 1., r             # 4. |d cum - d damage| <= S 2^-52 max(1, cum_end)
        assert r["ghosts"] > 0 and r["ghost_tau_differs"] == [], r                             # ghost-node values of tau_wi count for nothing
