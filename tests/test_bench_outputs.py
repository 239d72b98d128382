"""bench.py --dump-outputs: the state the last timed step left, as whole-mesh float64 arrays (gathered from the entries every rank owns), sampled with a fixed
seed where it would exceed 64 MiB; and a plain run (no --full) that times exactly --steps steps and runs none of the secondary legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import cases
from nextsim_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _local_states(gm, lms, seed=3):
    """Whole-mesh arrays with distinct values everywhere, and what each rank's get_state() would hold of them (owned entries, then ghosts)."""
    rng = np.random.default_rng(seed)
    Nn, Ne = gm.num_nodes, gm.num_elements
    want = {k: rng.standard_normal(2 * Nn) for k in _abi.STATE_NODAL}
    want.update({k: rng.standard_normal(Ne) for k in _abi.STATE_ELEMENT})
    local = []
    for lm in lms:
        st = {k: np.concatenate([want[k][lm.node_gid], want[k][Nn + lm.node_gid]]) for k in _abi.STATE_NODAL}
        st.update({k: want[k][lm.elem_gid] for k in _abi.STATE_ELEMENT})
        local.append(st)
    return want, local


class _Gather:
    """torch.distributed's gather_object for ranks that run one after the other in this process: ranks 1.. leave their object, rank 0 receives all."""
    def __init__(self):
        self.sent = {}

    def gather_object(self, obj, object_gather_list=None, dst=0):
        if object_gather_list is None:
            self.sent[len(self.sent) + 1] = obj
        else:
            object_gather_list[:] = [obj] + [self.sent[r] for r in sorted(self.sent)]


@pytest.mark.parametrize("nparts", [1, 3])
def test_global_state_puts_every_rank_s_owned_entries_where_they_belong(nparts):
    gm, p, g, lms, fields = cases.make_case("small", nparts=nparts, ragged_seed=5 if nparts > 1 else None)
    want, local = _local_states(gm, lms)
    d = _Gather()
    for r in range(nparts - 1, 0, -1):   # (ranks 1.. first: rank 0 is the one that receives)
        assert bench.global_state(local[r], lms[r], gm, r, nparts, d) is None
    got = bench.global_state(local[0], lms[0], gm, 0, nparts, d)
    assert sorted(got) == sorted(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k


def test_dump_is_whole_below_the_limit_and_a_fixed_sample_above_it(tmp_path, monkeypatch):
    gm, p, g, lms, fields = cases.make_case("small")
    want, local = _local_states(gm, lms)
    info = bench.dump_outputs(str(tmp_path / "whole"), want, gm.num_nodes, gm.num_elements)
    assert info["sample"] is None and sorted(info["arrays"]) == sorted(want)
    for k in want:
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, want[k]), k
    limit = sum(a.nbytes for a in want.values()) // 5
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    infos = [bench.dump_outputs(str(tmp_path / f"s{i}"), want, gm.num_nodes, gm.num_elements) for i in range(2)]
    s = infos[0]["sample"]
    assert s is not None and 0 < s["nodes"] < gm.num_nodes and 0 < s["elements"] < gm.num_elements
    assert infos[0]["bytes"] <= limit and sum(os.path.getsize(tmp_path / "s0" / f"{k}.npy") for k in want) == infos[0]["bytes"]
    rng = np.random.default_rng(s["seed"])
    nodes = np.sort(rng.choice(gm.num_nodes, s["nodes"], replace=False))
    elems = np.sort(rng.choice(gm.num_elements, s["elements"], replace=False))
    for k in want:
        a, b = np.load(tmp_path / "s0" / f"{k}.npy"), np.load(tmp_path / "s1" / f"{k}.npy")
        assert np.array_equal(a, b), k                                         # the same sample every time
        if k in _abi.STATE_NODAL:
            assert np.array_equal(a, want[k].reshape(2, -1)[:, nodes].ravel()), k
        else:
            assert np.array_equal(a, want[k][elems]), k


@pytest.mark.gpu
def test_a_plain_bench_run_times_its_steps_runs_no_secondary_leg_and_dumps_the_state_of_its_last_step(tmp_path):
    steps, warmup = 3, 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--mesh", "40km",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0 and d["fields_ok"] is True and d["full"] is False
    assert d["step_times_ms"]["n"] == steps
    assert not any(k == "cpu_baseline" or k.startswith("aux_") for k in d), sorted(d)
    assert d["roofline"]["traffic_measured_in_this_run"] is False
    assert d["outputs"]["sample"] is None and d["outputs"]["bytes"] <= 64 << 20

    from nextsim_amd import dynamics
    gm, p, lm, f = bench.build_case("40km", 1, 0)
    fe = dynamics.FiniteElementDynamics(p, device=0)
    try:
        fe.set_mesh(lm)
        fe.put_state(f)
        fe.set_forcing(f)
        fe.set_option("prepare", 1)
        for _ in range(warmup + steps):
            fe.step()
        fe.synchronize()
        want = fe.get_state()
    finally:
        fe.close()
    assert sorted(d["outputs"]["arrays"]) == sorted(want)
    for k, v in want.items():
        assert np.array_equal(np.load(tmp_path / "out" / f"{k}.npy"), v), k
