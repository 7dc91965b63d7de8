"""Public-tree node observations from the library's kernels (prl_tree_observations_device, PublicTree.node_observations): bit for bit what
`wrapper.set_to_public_tree_node_state(node); wrapper.get_current_obs()` returns (wrappers.history_of_nodes), the legal masks and history
lengths, the argument checks, and TorchPolicyAgent's fill through them without per-node Python."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from pokerrl_amd import _native  # noqa: E402
from pokerrl_amd.game import bet_sets  # noqa: E402
from pokerrl_amd.game import wrappers as W  # noqa: E402
from pokerrl_amd.game.games import DiscretizedNLHoldem, DiscretizedNLLeduc, Flop5Holdem, LimitHoldem, StandardLeduc  # noqa: E402


@pytest.fixture()
def emu_lib(monkeypatch):
    sys.path.insert(0, os.path.join(HERE, "emu"))
    import build_emu
    L = _native.bind(build_emu.build())
    monkeypatch.setattr(_native, "lib", lambda: L)
    monkeypatch.setattr(_native, "require_device", lambda: None)
    return L


def seeded_boards(n):
    sys.path.insert(0, os.path.dirname(HERE))
    import bench
    return bench.seeded_boards(n, 0)


def build(game_cls, bldr_cls, bets=None, stack=None, boards=None, engine="auto", invert=False):
    from pokerrl_amd.game.PublicTree import PublicTree
    kw = {} if bets is None else {"bet_sizes_list_as_frac_of_pot": bets}
    args = game_cls.ARGS_CLS(n_seats=2, **kw)
    if stack is not None:
        args.starting_stack_sizes_list = [stack, stack]
    bldr = W.HistoryEnvBuilder(game_cls, args, invert_history_order=True) if invert else bldr_cls(game_cls, args)
    tree = PublicTree(env_bldr=bldr, stack_size=list(args.starting_stack_sizes_list), stop_at_street=None, boards=boards, engine=engine)
    tree.build_tree()
    return tree, bldr


def check_equal_to_host(tree, bldr, node_idx, device="cpu"):
    """node_observations(node_idx) == history_of_nodes per node (np.array_equal), groups as _fill_nodes makes them, legal masks, history lengths"""
    node_idx = np.asarray(node_idx, np.int32)
    obs = tree.node_observations(bldr, node_idx, device=device)
    nodes = [tree.node(int(i)) for i in node_idx]
    want = W.history_of_nodes(bldr, nodes, stack_size=list(tree.stack_size))
    got = [None] * len(nodes)
    for pos, x in obs.groups:
        x = x.cpu().numpy()
        assert x.dtype == np.float32
        for k, p in enumerate(pos):
            got[p] = x[k]
    assert all(g is not None for g in got)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (i, int(node_idx[i]))
    shapes = list(dict.fromkeys(w.shape for w in want))  # _fill_nodes' groups: shapes in first-appearance order, nodes in request order
    assert [tuple(x.shape[1:]) for _p, x in obs.groups] == shapes
    for pos, _x in obs.groups:
        assert list(pos) == [i for i, w in enumerate(want) if w.shape == want[pos[0]].shape]
    legal = obs.legal.cpu().numpy()
    assert legal.shape == (len(nodes), bldr.N_ACTIONS) and legal.dtype == np.bool_
    for i, n in enumerate(nodes):
        assert list(np.flatnonzero(legal[i])) == n.allowed_actions, i
    assert list(obs.hist_len) == [len(W._path_to_root(n)) for n in nodes]
    return obs


def decision_ids(tree):
    return np.flatnonzero(tree._kind == 0).astype(np.int32)


def sample(ids, k, seed=0):
    return ids if len(ids) <= k else np.sort(np.random.RandomState(seed).choice(ids, k, replace=False)).astype(np.int32)


# ---- CPU (emulator build) ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bldr_cls,invert", [(W.VanillaEnvBuilder, False), (W.HistoryEnvBuilder, False), (W.HistoryEnvBuilder, True),
                                             (W.FlatLimitPokerEnvBuilder, False)])
def test_leduc_observations_equal_host_walk_emu(emu_lib, bldr_cls, invert):
    tree, bldr = build(StandardLeduc, bldr_cls, invert=invert)
    check_equal_to_host(tree, bldr, decision_ids(tree))


def test_discretized_nl_leduc_observations_emu(emu_lib):
    tree, bldr = build(DiscretizedNLLeduc, W.HistoryEnvBuilder, bets=bet_sets.B_3)
    check_equal_to_host(tree, bldr, decision_ids(tree))


def test_flop5holdem_fused_observations_emu(emu_lib):
    tree, bldr = build(Flop5Holdem, W.HistoryEnvBuilder, boards=seeded_boards(3), engine="fused")
    assert tree.solver.engine == "fused"
    check_equal_to_host(tree, bldr, decision_ids(tree))


def test_limit_holdem_flat_observations_emu(emu_lib):
    import parity_cases as pc
    tree, bldr = build(LimitHoldem, W.FlatLimitPokerEnvBuilder, boards=pc.multistreet_runouts(1, 1, 1))
    check_equal_to_host(tree, bldr, sample(decision_ids(tree), 1500))


def test_discretized_nl_holdem_mixed_streets_observations_emu(emu_lib):
    """the smoke test's tree: pot-sized raises with 600 chips over run-outs (1, 2, 1) -- street shapes side by side, all-in run-out chains"""
    import parity_cases as pc
    tree, bldr = build(DiscretizedNLHoldem, W.HistoryEnvBuilder, bets=bet_sets.POT_ONLY, stack=600, boards=pc.multistreet_runouts(1, 2, 1))
    assert np.any(tree._kind[tree._parent[tree._parent.clip(0)].clip(0)] == 1)  # chance nodes below chance nodes: run-out chains are there
    check_equal_to_host(tree, bldr, decision_ids(tree))


def test_shuffled_subset_with_repeats_emu(emu_lib):
    tree, bldr = build(StandardLeduc, W.HistoryEnvBuilder)
    ids = decision_ids(tree)
    req = np.random.RandomState(3).choice(ids, 3 * len(ids) // 2, replace=True).astype(np.int32)
    assert len(np.unique(req)) < len(req)
    check_equal_to_host(tree, bldr, req)


def test_argument_errors_emu(emu_lib):
    tree, bldr = build(DiscretizedNLLeduc, W.HistoryEnvBuilder, bets=bet_sets.B_3)
    t = tree.native_tree
    D = bldr.pub_obs_size
    out = np.zeros((64, D), np.float32)
    dec = decision_ids(tree)
    term = int(np.flatnonzero(tree._kind >= 2)[0])

    def call(idx, off, kind=_native.OBS_HISTORY, row_dim=D, n_rows=64, flat=None):
        with pytest.raises(_native.NativeError) as e:
            t.observations_device(kind, False, np.array(idx, np.int32), np.array(off, np.int64), flat, row_dim, n_rows, out.ctypes.data, 0, bldr.N_ACTIONS)
        assert e.value.status == _native.ERR_ARG
        return str(e.value)

    call([term], [0])                                   # a terminal node
    call([t.n_nodes], [0])                              # out of range
    call([-1], [0])
    deep = int(dec[np.argmax(t.obs_hist_len(dec))])
    call([deep], [64 - int(t.obs_hist_len([deep])[0]) + 1])  # its rows overrun n_rows
    call([int(dec[0])], [-1])
    call([int(dec[0])], [0], row_dim=D + 1)             # row_dim wrong for the kind
    call([int(dec[0])], [0], kind=_native.OBS_FLAT_HU_LIMIT, row_dim=D + 8, flat=[0, 4, 2, 2])  # FLAT on a no-limit game
    assert not out.any()                                # nothing was launched
    with pytest.raises(_native.NativeError):
        t.obs_hist_len([term])
    # the same call with good arguments writes
    t.observations_device(_native.OBS_HISTORY, False, np.array([deep], np.int32), np.array([0], np.int64), None, D, 64, out.ctypes.data, 0, bldr.N_ACTIONS)
    assert out.any()


def _count_tree_nodes(monkeypatch):
    from pokerrl_amd.game import PublicTree as PT
    made = [0]
    init = PT.TreeNode.__init__

    def counting(self, tree, idx):
        made[0] += 1
        init(self, tree, idx)

    monkeypatch.setattr(PT.TreeNode, "__init__", counting)
    return made


def _forbid_host_walk(monkeypatch):
    from pokerrl_amd.game import PublicTree as PT

    def boom(*a, **k):
        raise AssertionError("per-node host walk used")

    monkeypatch.setattr(W, "history_of_nodes", boom)
    monkeypatch.setattr(PT.PublicTree, "_env_state_of", boom)


def test_agent_fill_without_per_node_python_emu(emu_lib, monkeypatch, tmp_path):
    """fill_with_agent_policy with TorchPolicyAgent's device path: no host walk, a handful of TreeNode objects, the host path's strategy bit for bit"""
    from test_f1_agents import t_prof_of
    from pokerrl_amd.rl.neural import TorchPolicyAgent

    class HostFill(TorchPolicyAgent):
        DEVICE_RESIDENT_FILL = False

    t_prof = t_prof_of(StandardLeduc, W.HistoryEnvBuilder, tmp_path)
    tree_h, _b = build(StandardLeduc, W.HistoryEnvBuilder)
    tree_d, _b = build(StandardLeduc, W.HistoryEnvBuilder)
    n_dec = len(decision_ids(tree_d))
    assert 100 <= n_dec <= 2000, n_dec
    tree_h.fill_with_agent_policy(HostFill(t_prof))
    agent = TorchPolicyAgent(t_prof)
    _forbid_host_walk(monkeypatch)
    made = _count_tree_nodes(monkeypatch)
    tree_d.fill_with_agent_policy(agent)
    assert made[0] <= 4, made[0]
    assert agent.n_forwards == len(np.unique(tree_d.native_tree.obs_hist_len(decision_ids(tree_d))))
    sh, sd = tree_h.solver.get("strategy"), tree_d.solver.get("strategy")
    assert sh.shape == sd.shape and np.array_equal(sh, sd)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_flop5holdem_4096_boards_observations():
    _native.require_device()
    tree, bldr = build(Flop5Holdem, W.HistoryEnvBuilder, boards=seeded_boards(4096), engine="fused")
    ids = decision_ids(tree)
    assert len(ids) == 24578
    check_equal_to_host(tree, bldr, sample(ids, 3000), device="cuda")
    obs = tree.node_observations(bldr, device="cuda")  # every decision node: the device path's real request
    assert sum(len(p) for p, _x in obs.groups) == len(ids)


@pytest.mark.gpu
def test_gpu_limit_holdem_per_street_tree_observations():
    import parity_cases as pc
    _native.require_device()
    for bldr_cls in (W.HistoryEnvBuilder, W.FlatLimitPokerEnvBuilder):
        tree, bldr = build(LimitHoldem, bldr_cls, boards=pc.multistreet_runouts(1, 1, 1))
        check_equal_to_host(tree, bldr, sample(decision_ids(tree), 3000), device="cuda")


@pytest.mark.gpu
def test_gpu_discretized_nl_holdem_observations():
    import parity_cases as pc
    _native.require_device()
    tree, bldr = build(DiscretizedNLHoldem, W.HistoryEnvBuilder, bets=bet_sets.POT_ONLY, stack=600, boards=pc.multistreet_runouts(1, 2, 1))
    check_equal_to_host(tree, bldr, decision_ids(tree), device="cuda")


@pytest.mark.gpu
def test_gpu_agent_br_at_65536_boards_device_path_only(monkeypatch, tmp_path):
    """BR of TorchPolicyAgent through LocalBRMaster on Flop5Holdem x 65 536 boards with the host walk forbidden: finite positive exploitability, every
    (node, hand) row of the agent's probabilities sums to 1 over the node's legal actions (checked on the device), and 1 000 random nodes' rows equal
    the host walk's"""
    import torch
    from test_f1_agents import br_of, t_prof_of
    from pokerrl_amd.rl.neural import TorchPolicyAgent
    _native.require_device()
    seen = {}

    class Checked(TorchPolicyAgent):
        def get_a_probs_for_each_hand_in_nodes_device(self, nodes):
            probs = super().get_a_probs_for_each_hand_in_nodes_device(nodes)
            t = nodes.tree
            kind, col_node, col_action = t._kind, t.native_tree.field("col_node"), t.native_tree.field("col_action")
            ord_ = np.full(len(kind), -1, np.int64)
            ord_[kind == 0] = np.arange(int(np.sum(kind == 0)))
            mask = np.zeros((len(nodes), self.env_bldr.N_ACTIONS), np.float32)
            mask[ord_[col_node], col_action] = 1.0
            m = torch.from_numpy(mask).to(probs.device)
            err = 0.0
            for lo in range(0, len(nodes), 8192):  # the masked row sums, a slab of nodes at a time (probs is [n, 1326, 3] float32: 6 GB)
                s = (probs[lo:lo + 8192] * m[lo:lo + 8192, None, :]).sum(-1)
                err = max(err, float((s - 1.0).abs().max()))
            seen["err"], seen["n"] = err, len(nodes)
            return probs

    t_prof = t_prof_of(Flop5Holdem, W.HistoryEnvBuilder, tmp_path, device="cuda")
    _forbid_host_walk(monkeypatch)
    expl, br = br_of(t_prof, Checked, boards=seeded_boards(65536), engine="fused")
    monkeypatch.undo()
    assert np.isfinite(expl) and expl > 0
    assert seen["err"] <= 1e-5, seen
    tree = br._game_trees[0]
    assert seen["n"] == len(decision_ids(tree)) > 350000
    check_equal_to_host(tree, tree.env_bldr, sample(decision_ids(tree), 1000, seed=7), device="cuda")
