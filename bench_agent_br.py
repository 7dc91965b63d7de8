"""
bench_agent_br.py -- exact best response of a NEURAL agent (TorchPolicyAgent, GRU over the observation history: HistoryEnvBuilder) through
LocalBRMaster on the Flop5Holdem public tree (secondary to bench.py). One line of JSON.

    python bench_agent_br.py [--gpus 1] [--boards 65536] [--host-boards 4096] [--steps K] [--warmup W] [--no-host]

Per configuration, seconds of: the tree build (LocalBRMaster's constructor: tree + solver), the agent fill (PublicTree.fill_with_agent_policy)
split into the node observations (PublicTree.node_observations; its kernels timed with HIP events on the tree's stream, prl_tree_obs_stats),
the network forwards and the scatter into the solver (prl_solver_set_strategy_device), then compute_ev, and the whole evaluate.
  device_<B>:  the device path (the library's observation kernels) at --host-boards and --boards boards
  host_<B>:    the host walk (wrappers.history_of_nodes, one Python replay per decision node) at --host-boards boards
Observation kernels' bandwidth: the bytes they write (rows x row_dim x 4 + legal masks) over their kernel time, as a fraction of HBM peak.
--steps evaluations per configuration after --warmup (the first builds the tree's env-state cache, timed separately as obs_states_ms).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def t_prof(path):
    from pokerrl_amd.game.games import Flop5Holdem
    from pokerrl_amd.game.wrappers import HistoryEnvBuilder
    from pokerrl_amd.rl.base_cls.TrainingProfileBase import TrainingProfileBase
    return TrainingProfileBase(
        name="agent_br", log_verbose=False, log_export_freq=1, checkpoint_freq=10 ** 9, eval_agent_export_freq=10 ** 9, game_cls=Flop5Holdem,
        env_bldr_cls=HistoryEnvBuilder, start_chips=None, eval_modes_of_algo=("POLICY",), eval_stack_sizes=None,
        module_args={"env": Flop5Holdem.ARGS_CLS(n_seats=2)}, path_data=path, device_inference="cuda")


def run(n_boards, device_path, steps, warmup):
    import torch
    from pokerrl_amd.eval.br.LocalBRMaster import LocalBRMaster
    from pokerrl_amd.rl.base_cls.workers.ChiefBase import ChiefBase
    from pokerrl_amd.rl.neural import TorchPolicyAgent

    class Chief(ChiefBase):
        def pull_current_eval_strategy(self, last):
            return None, last

    class Agent(TorchPolicyAgent):
        DEVICE_RESIDENT_FILL = device_path

    phase = {}

    def timed(name, fn):
        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            phase[name] = phase.get(name, 0.0) + time.perf_counter() - t0
            return r
        return wrapper

    tp = t_prof(tempfile.mkdtemp())
    t0 = time.perf_counter()
    br = LocalBRMaster(t_prof=tp, chief_handle=Chief(tp), eval_agent_cls=Agent, boards=bench.seeded_boards(n_boards, 0), engine="fused")
    br.update_weights()
    build_s = time.perf_counter() - t0
    tree = br._game_trees[0]
    # phase timers on this tree only (instance attributes)
    tree.node_observations = timed("obs", tree.node_observations)
    tree.fill_with_agent_policy = timed("fill", tree.fill_with_agent_policy)
    tree.compute_ev = timed("compute_ev", tree.compute_ev)
    tree.solver.set_strategy_device = timed("scatter", tree.solver.set_strategy_device)
    rows, totals, obs_ms, obs_bytes, states_ms, first_s = [], [], [], [], None, None
    for it in range(warmup + steps):
        phase.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        br.evaluate(iter_nr=it)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        st = tree.native_tree.obs_stats() if device_path else None
        if it == 0:
            first_s = total  # includes the one-time env-state cache of the tree
            states_ms = st["states_ms"] if st is not None else None
        if it >= warmup:
            totals.append(total)
            rows.append(dict(phase))
            if st is not None:
                obs_ms.append(st["obs_ms"])
                obs_bytes.append(st["obs_bytes"])
    expl = [float(x) for x in np.atleast_1d(tree.root.exploitability)]
    med = lambda xs: float(np.median(xs)) if xs else None  # noqa: E731
    fill, obs, scatter, ev = (med([r.get(k, 0.0) for r in rows]) for k in ("fill", "obs", "scatter", "compute_ev"))
    out = dict(boards=n_boards, decision_nodes=int(np.sum(tree._kind == 0)), tree_build_s=round(build_s, 3), evaluate_s=round(med(totals), 4),
               end_to_end_s=round(build_s + first_s, 3), first_evaluate_s=round(first_s, 4), fill_s=round(fill, 4), compute_ev_s=round(ev, 4), scatter_s=round(scatter, 4), exploitability=expl)
    if device_path:
        kms = med(obs_ms)
        out.update(obs_s=round(obs, 4), obs_kernels_ms=round(kms, 3), obs_states_ms=round(states_ms, 3), obs_bytes=int(med(obs_bytes)),
                   obs_state_cache_bytes=int(tree.native_tree.obs_stats()["state_bytes"]), forward_s=round(fill - obs - scatter, 4),
                   obs_kernels_share_of_fill=round(kms / 1e3 / fill, 4),
                   obs_kernels_gbps=round(med(obs_bytes) / (kms / 1e3) / 1e9, 1) if kms else None)
        out["obs_kernels_hbm_fraction"] = round(out["obs_kernels_gbps"] / HBM_PEAK_GBPS, 4) if out["obs_kernels_gbps"] else None
    else:
        out["forward_and_host_walk_s"] = round(fill - scatter, 4)
    del br, tree
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--host-boards", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    assert a.gpus == 1, "one GPU: the agent's tree is not sharded here"
    from pokerrl_amd import _native
    _native.require_device()
    res = {"bench": "agent_br", "game": "Flop5Holdem", "builder": "HistoryEnvBuilder", "agent": "TorchPolicyAgent (GRU)", "steps": a.steps,
           "warmup": a.warmup}
    res["device_%d" % a.host_boards] = run(a.host_boards, True, a.steps, a.warmup)
    if not a.no_host:
        res["host_%d" % a.host_boards] = run(a.host_boards, False, 1, 0)
    res["device_%d" % a.boards] = run(a.boards, True, a.steps, a.warmup)
    big = res["device_%d" % a.boards]
    res["end_to_end_s"] = big["end_to_end_s"]
    if not a.no_host:
        res["host_path_evaluate_s_at_%d" % a.host_boards] = res["host_%d" % a.host_boards]["evaluate_s"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
