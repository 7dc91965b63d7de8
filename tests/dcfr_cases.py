"""Checks of Discounted CFR (include/pokerrl_hip.h: PRL_VARIANT_DISCOUNTED, prl_dcfr_factors) shared by the emulator tests and the GPU tests of
tests/test_dcfr.py. DCFR has no class in the reference and no oracle; its anchor is HookedDCFR below: the update written against the reference's
hook protocol the way the reference writes LinearCFR.py, float32 NumPy on the host, with the tree passes (pinned to the reference elsewhere) on the
device. Everything else compares engines of the library with each other, bit for bit."""
import math
import os
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import parity_cases as pc
from helpers import GAMES, all_single_card_boards, env_args
from pokerrl_amd import _native
from pokerrl_amd.cfr._CFRBase import CFRBase
from pokerrl_amd.cfr.DiscountedCFR import DiscountedCFR
from pokerrl_amd.game import bet_sets
from pokerrl_amd.game import games as G
from pokerrl_amd.rl.base_cls.workers.ChiefBase import ChiefBase

HERE = os.path.dirname(os.path.abspath(__file__))
PARAM_SETS = [(1.5, 0.0, 2.0), (1.0, 1.0, 1.0), (2.0, -math.inf, 3.0), (0.5, 0.5, 0.0)]
COLS = ("regret", "avg", "avg_sum")


class HookedDCFR(CFRBase):
    """Discounted CFR against the hook protocol (_VARIANT = None: level-synchronous tree passes on the device, these four formulas in NumPy)"""

    def __init__(self, name, chief_handle, game_cls, agent_bet_set, starting_stack_sizes=None, alpha=1.5, beta=0.0, gamma=2.0, **kw):
        self._abg = (alpha, beta, gamma)
        super().__init__(name=name, chief_handle=chief_handle, game_cls=game_cls, starting_stack_sizes=starting_stack_sizes,
                         agent_bet_set=agent_bet_set, algo_name="HookedDCFR", **kw)
        self.reset()

    def _factors(self):
        return _native.dcfr_factors(self._iter_counter, *self._abg)  # three float32

    def _regret_formula_first_it(self, ev_all_actions, strat_ev):
        return ev_all_actions - strat_ev

    def _regret_formula_after_first_it(self, ev_all_actions, strat_ev, last_regrets):
        d_pos, d_neg, _ = self._factors()
        return last_regrets * np.where(last_regrets > 0, d_pos, d_neg) + (ev_all_actions - strat_ev)

    def _compute_new_strategy(self, p_id):
        for t_idx, tree in enumerate(self._trees):
            R = self._env_bldrs[t_idx].rules.RANGE_SIZE
            for node in tree.nodes():
                if node.p_id_acting_next == p_id and not node.is_terminal:
                    n = len(node.children)
                    pos = np.maximum(node.data["regret"], 0)
                    s = np.expand_dims(np.sum(pos, axis=1), axis=1).repeat(n, axis=1)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        node.strategy = np.where(s > 0.0, pos / s, np.full(shape=(R, n), fill_value=1.0 / n, dtype=np.float32))

    def _add_strategy_to_average(self, p_id):
        for tree in self._trees:
            for node in tree.nodes():
                if node.p_id_acting_next == p_id and not node.is_terminal:
                    contrib = node.strategy * np.expand_dims(node.reach_probs[p_id], axis=1)
                    if self._iter_counter > 0:
                        node.data["avg_strat_sum"] = node.data["avg_strat_sum"] * self._factors()[2] + contrib
                    else:
                        node.data["avg_strat_sum"] = contrib
                    s = np.expand_dims(np.sum(node.data["avg_strat_sum"], axis=1), axis=1)
                    n = len(node.allowed_actions)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        node.data["avg_strat"] = np.where(s == 0, np.full(shape=n, fill_value=1.0 / n), node.data["avg_strat_sum"] / s)


# ---- 1. the factors ---------------------------------------------------------------------------------------------------------------------------------
def expected_factors(it, a, b, g):
    def d(e):
        x = math.pow(float(it), e)
        return np.float32(x / (x + 1.0))
    return d(a), d(b), np.float32(math.pow(float(it) / float(it + 1), g))


def check_factors():
    for abg in PARAM_SETS:
        for it in range(1, 1001):
            got, want = _native.dcfr_factors(it, *abg), expected_factors(it, *abg)
            assert got.dtype == np.float32 and got[0] == want[0] and got[1] == want[1] and got[2] == want[2], (abg, it, got, want)
        f1 = _native.dcfr_factors(1, *abg)
        assert f1[0] == np.float32(0.5) and f1[1] == np.float32(0.5), (abg, f1)
    assert all(_native.dcfr_factors(it, 1.5, 0.0, 2.0)[1] == np.float32(0.5) for it in range(1, 1001))
    assert all(_native.dcfr_factors(it, 2.0, -math.inf, 3.0)[1] == 0.0 for it in range(2, 1001))
    for bad in [(math.inf, 0.0, 2.0), (math.nan, 0.0, 2.0), (-math.inf, 0.0, 2.0), (1.5, 0.0, math.inf), (1.5, 0.0, math.nan), (1.5, math.inf, 2.0),
                (1.5, math.nan, 2.0)]:
        with pytest.raises(_native.NativeError) as e:
            _native.dcfr_factors(3, *bad)
        assert e.value.status == _native.ERR_ARG and "alpha and gamma must be finite, beta finite or -inf" in str(e.value), (bad, str(e.value))


# ---- 2. / 3. the built-in variant against the restatement --------------------------------------------------------------------------------------------
def _series(chief, game_cls):
    vals, _ = chief.get_new_values()
    metric = "Evaluation/" + game_cls.WIN_METRIC
    curr = [v for k, v in vals.items() if "_Curr_S" in k][0][metric]
    avg = [v for k, v in vals.items() if "_Avg_total_S" in k][0][metric]
    return np.array(curr, np.float64), np.array(avg, np.float64)


def _hooked_columns(cfr):
    """the hooked run's node.data as [n_cols, R] arrays in the solver's column order"""
    tree = cfr._trees[0]
    R = tree.solver.R
    out = {"regret": np.zeros((tree.solver.n_cols, R), np.float32), "avg_sum": np.zeros((tree.solver.n_cols, R), np.float32),
           "avg": np.zeros((tree.solver.n_cols, R), np.float64)}
    n_dec = 0
    for node in tree.nodes():
        if node.is_terminal or node.p_id_acting_next == tree.CHANCE_ID:
            continue
        c0 = int(tree._first_col[node._i])
        for key, name in (("regret", "regret"), ("avg_strat_sum", "avg_sum"), ("avg_strat", "avg")):
            a = node.data[key]
            assert a.dtype == out[name].dtype, (key, a.dtype)
            out[name][c0:c0 + a.shape[1]] = a.T
        n_dec += 1
    assert n_dec > 0
    return out


def check_builtin_vs_restatement(game_cls, bets, abg, n_iters, expect_graph_replay=None, **kw):
    """DiscountedCFR (through iteration() and through iterations(n)) against HookedDCFR: the logged exploitability of the current and the average
    strategy after every iteration, then every decision node's regret / avg_sum / avg, bit for bit"""
    a, b, g = abg
    mk = lambda cls, tag: (lambda chief: (chief, cls(name=tag, chief_handle=chief, game_cls=game_cls, agent_bet_set=bets, alpha=a, beta=b, gamma=g, **kw)))(ChiefBase(t_prof=None))  # noqa: E731
    ch_h, hooked = mk(HookedDCFR, "hook")
    ch_s, single = mk(DiscountedCFR, "single")
    ch_b, batched = mk(DiscountedCFR, "batched")
    assert single._trees[0].solver.discount == (a, b, g)
    for _ in range(n_iters):
        hooked.iteration()
        single.iteration()
    batched.iterations(n_iters)
    curr_h, avg_h = _series(ch_h, game_cls)
    curr_s, avg_s = _series(ch_s, game_cls)
    curr_b, avg_b = _series(ch_b, game_cls)
    assert curr_h.shape == (n_iters + 1, 2) and avg_h.shape == (n_iters, 2)
    assert np.array_equal(curr_s, curr_h), (curr_s, curr_h)
    assert np.array_equal(avg_s, avg_h), (avg_s, avg_h)
    assert np.array_equal(curr_b, curr_h), (curr_b, curr_h)
    assert avg_b.shape == (1, 2) and np.array_equal(avg_b[-1], avg_h[-1])  # iterations(n) evaluates the average after the last one only
    want = _hooked_columns(hooked)
    for cfr, tag in ((single, "iteration()"), (batched, "iterations(n)")):
        s = cfr._trees[0].solver
        for k in COLS:
            got = s.get(k)
            assert np.array_equal(got, want[k]), "%s: %s differs in %d entries" % (tag, k, int(np.sum(got != want[k])))
    if expect_graph_replay is not None:
        assert batched._trees[0].solver.graph_replay == expect_graph_replay
    return single, batched


# ---- 4. fused = levels, single deal ------------------------------------------------------------------------------------------------------------------
def fused_vs_levels(L, n_boards, n_iters, abg=None, seed=11):
    """pc.check_fused_vs_levels for the discounted variant: the same Flop5Holdem tree on the board pass and on the level-synchronous engine. With
    n_iters >= 3 the run covers iteration 0 (no discount), iteration 1 (factor 1/2) and, from the second iteration on, seat 1's average update that
    the board pass applies one walk late (with the factor of the iteration it belongs to)."""
    t = pc.fhp_tree_of(L, pc.fhp_boards(n_boards, seed=seed))
    a = _native.NativeSolver(t, "discounted", 0, engine="fused", _lib=L, discount=abg)
    b = _native.NativeSolver(t, "discounted", 0, engine="levels", _lib=L, discount=abg)
    assert (a.engine, b.engine) == ("fused", "levels")
    assert a.discount == b.discount == (tuple(abg) if abg else (1.5, 0.0, 2.0))
    a.iterations(n_iters)
    b.iterations(n_iters)
    assert np.array_equal(a.get("expl_history"), b.get("expl_history"))
    for k in COLS:
        x, y = a.get(k), b.get(k)
        assert np.array_equal(x, y), "%s differs in %d entries" % (k, int(np.sum(x != y)))
    assert np.array_equal(a.eval_avg(), b.eval_avg())
    # iterations(n) takes the pass's steady-state kind from the second iteration on; single iteration() calls open every iteration with the generic
    # kernel (UPDATE0), which carries the same arithmetic behind run-time switches
    c = _native.NativeSolver(t, "discounted", 0, engine="fused", _lib=L, discount=abg)
    for _ in range(min(n_iters, 3)):
        c.iteration()
    c.iterations(n_iters - min(n_iters, 3))
    assert np.array_equal(c.get("expl_history"), b.get("expl_history"))
    for k in COLS:
        assert np.array_equal(c.get(k), b.get(k)), "single iterations: " + k
    return a, b


# ---- 5. per-street = levels --------------------------------------------------------------------------------------------------------------------------
def streets_vs_levels(L, game_cls, stack, bets, runouts, n_iters, max_raises=None):
    game = game_cls.native_game(env_args(game_cls, stack, bets))
    if max_raises is not None:
        for i, v in enumerate(max_raises):
            game.max_raises[i] = v
    t = _native.NativeTree(game, game_cls.native_rules(), runouts, _lib=L)
    a = _native.NativeSolver(t, "discounted", 0, engine="auto", _lib=L)
    b = _native.NativeSolver(t, "discounted", 0, engine="levels", _lib=L)
    assert (a.engine, b.engine) == ("fused", "levels")
    a.iterations(n_iters)
    b.iterations(n_iters)
    for k in ("regret", "avg"):
        x, y = a.get(k), b.get(k)
        assert np.array_equal(x, y), "%s differs in %d entries" % (k, int(np.sum(x != y)))
    assert np.array_equal(a.get("expl_history"), b.get("expl_history"))
    assert np.array_equal(a.exploitability(), b.exploitability())
    assert np.array_equal(a.eval_avg(), b.eval_avg())


# ---- 6. iterations_many ------------------------------------------------------------------------------------------------------------------------------
def check_iterations_many(L):
    cls = G.StandardLeduc
    cases = [(5, "discounted", None), (7, "plus", None), (13, "linear", None), (20, "vanilla", None), (13, "discounted", (2.0, -math.inf, 3.0))]

    def make(stack, variant, abg):
        t = _native.NativeTree(cls.native_game(env_args(cls, stack, None)), cls.native_rules(), all_single_card_boards(cls), _lib=L)
        return _native.NativeSolver(t, variant, 0, engine="levels", _lib=L, discount=abg)

    many, alone = [make(*c) for c in cases], [make(*c) for c in cases]
    _native.NativeSolver.iterations_many(many, 3)
    _native.NativeSolver.iterations_many(many, 2)
    for i, (m, s) in enumerate(zip(many, alone)):
        s.iterations(5)
        assert m.iter == s.iter == 5
        for k in ("regret", "avg", "expl_history") + (() if cases[i][1] == "plus" else ("avg_sum",)):
            assert np.array_equal(m.get(k), s.get(k)), (i, k)
    assert not np.array_equal(many[2].get("regret"), many[4].get("regret"))  # (same tree, Linear CFR and DCFR: different runs)


# ---- 7. weighted boards ------------------------------------------------------------------------------------------------------------------------------
def check_weighted_ones(L, n_iters=3):
    """multiplicity 1 for every board, no symmetrisation = the unweighted fused solve, bit for bit"""
    t = pc.fhp_tree_of(L, pc.fhp_boards(4))
    a = _native.NativeSolver(t, "discounted", 0, _lib=L, board_mult=np.ones(4, np.int32), symmetrize=False)
    b = _native.NativeSolver(t, "discounted", 0, engine="fused", _lib=L)
    assert (a.engine, b.engine) == ("fused", "fused")
    a.iterations(n_iters)
    b.iterations(n_iters)
    for k in COLS + ("expl_history",):
        assert np.array_equal(a.get(k), b.get(k)), k
    assert np.array_equal(a.eval_avg(), b.eval_avg())


def check_iso_subset(L, n_iters=3):
    def S(boards, mult):
        t = pc.fhp_tree_of(L, boards)
        if mult is None:
            return _native.NativeSolver(t, "discounted", 0, engine="fused", _lib=L)
        return _native.NativeSolver(t, "discounted", 0, _lib=L, board_mult=mult, symmetrize="subset")
    pc.iso_vs_full(S, S, 3, n_iters)  # (the helper's own rtol, as for the other variants)


# ---- 8. checkpoints ----------------------------------------------------------------------------------------------------------------------------------
def _ckpt_tree(L, fused):
    if fused:
        return pc.fhp_tree_of(L, pc.fhp_boards(3)), "fused"
    cls, stack, bets = GAMES["StandardLeduc"]
    return _native.NativeTree(cls.native_game(env_args(cls, stack, bets)), cls.native_rules(), all_single_card_boards(cls), _lib=L), "levels"


def check_checkpoint(L, fused):
    t, engine = _ckpt_tree(L, fused)
    abg = (2.0, -math.inf, 3.0)
    mk = lambda d=abg, v="discounted": _native.NativeSolver(t, v, 0, engine=engine, _lib=L, discount=d)  # noqa: E731
    whole, first = mk(), mk()
    whole.iterations(5)
    first.iterations(3)
    blob = first.save_state()
    resumed = mk()
    resumed.load_state(blob)
    assert resumed.iter == 3 and resumed.discount == abg
    resumed.iterations(2)
    for k in COLS + ("expl_history",):
        assert np.array_equal(whole.get(k), resumed.get(k)), k
    with pytest.raises(_native.NativeError) as e:  # other parameters: refused like another variant / delay
        mk((1.5, 0.0, 2.0)).load_state(blob)
    assert e.value.status == _native.ERR_STATE and "different discount parameters" in str(e.value)
    with pytest.raises(_native.NativeError) as e:
        resumed.set_discount(1.0, 1.0, 1.0)
    assert e.value.status == _native.ERR_STATE
    one = mk()
    one.iterations(1)
    with pytest.raises(_native.NativeError) as e:
        one.set_discount(1.0, 1.0, 1.0)
    assert e.value.status == _native.ERR_STATE
    one.reset()  # keeps the parameters, and they may change again
    assert one.discount == abg
    one.set_discount(1.0, 1.0, 1.0)
    assert one.discount == (1.0, 1.0, 1.0)
    plus = mk(None, "plus")
    with pytest.raises(_native.NativeError) as e:
        plus.set_discount(1.5, 0.0, 2.0)
    assert e.value.status == _native.ERR_UNSUPPORTED
    # the blobs of the other variants are what they were -- header, columns, flags, history -- and a DCFR blob is that plus its three doubles
    # (the sizes come from the blob's own header: format version 3, 64 bytes -- magic, version, then variant, delay, fused, iter, full_cols, R,
    # trunk_cols, trunk_nodes ... as int32; the single-deal fused engine stores a board column as 1088 sorted positions, the trunk's as R hands)
    al = lambda b: (b + 15) & ~15  # noqa: E731
    blob = plus.save_state()
    hdr = blob[:64].view(np.int32)
    variant, is_fused, it, full_cols, R, trunk_cols, trunk_nodes = (int(hdr[i]) for i in (2, 4, 5, 6, 7, 8, 9))
    assert (variant, is_fused, it, full_cols, R) == (1, int(fused), 0, plus.n_cols, plus.R)
    assert trunk_cols == (plus.n_cols - 3 * 14 if fused else plus.n_cols)
    nc = trunk_cols * R + (full_cols - trunk_cols) * 1088
    want_plus = 64 + al(nc * 4) + al(nc * 8) + al(trunk_cols * R * 8) + 2 * al(trunk_nodes) + al((it + 1) * 2 * 4)  # (regret, avg, strategy; no avg_sum)
    assert blob.shape[0] == want_plus, (blob.shape[0], want_plus)
    lin = mk(None, "linear")
    assert mk().save_state().shape[0] == lin.save_state().shape[0] + 32  # three doubles, padded to 16 bytes


# ---- 9. sharded --------------------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def check_sharded_world2(lib_path, device, timeout=900):
    """4 boards over 2 ranks, 4 iterations: every rank's regrets and the exploitability history equal the unsharded solve's"""
    world, n_local, n_iters, seed = 2, 2, 4, 21
    port = _free_port()
    with tempfile.TemporaryDirectory() as d:
        procs = []
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dcfr_sharded_worker.py"), lib_path, device, d, str(n_local), str(n_iters),
                                           str(seed)], env=env))
        try:
            for p in procs:
                assert p.wait(timeout=timeout) == 0
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
        ranks = [dict(np.load(os.path.join(d, "rank%d.npz" % r))) for r in range(world)]
    L = _native.bind(lib_path)
    t = pc.fhp_tree_of(L, pc.fhp_boards(world * n_local, seed=seed, with_special=False))
    s = _native.NativeSolver(t, "discounted", 0, engine="fused", _lib=L, discount=(2.0, -math.inf, 3.0))
    s.iterations(n_iters)
    hist, per = s.get("expl_history"), n_local * 14
    for r, out in enumerate(ranks):
        nt = int(out["n_trunk_cols"])
        assert np.array_equal(out["expl_history"], hist), r
        for k in ("regret", "avg_sum"):
            full = s.get(k)
            assert np.array_equal(out[k][:nt], full[:nt]), (r, k)
            assert np.array_equal(out[k][nt:], full[nt + r * per: nt + (r + 1) * per]), (r, k)


# ---- 10. DCFR(1, 1, 1) against Linear CFR ------------------------------------------------------------------------------------------------------------
def dcfr111_vs_linear(n_iters=50):
    """relative difference of the average-strategy exploitability after n_iters iterations on StandardLeduc"""
    from pokerrl_amd.cfr.LinearCFR import LinearCFR
    out = []
    for cls, kw in ((LinearCFR, {}), (DiscountedCFR, dict(alpha=1.0, beta=1.0, gamma=1.0))):
        cfr = cls(name="x", chief_handle=ChiefBase(t_prof=None), game_cls=G.StandardLeduc, agent_bet_set=bet_sets.POT_ONLY, **kw)
        cfr.iterations(n_iters, log=False)
        out.append(float(np.mean(np.asarray(cfr._trees[0].solver.eval_avg(), np.float64))))
    lin, dcfr = out
    return abs(dcfr - lin) / abs(lin), lin, dcfr


# ---- 11. surface -------------------------------------------------------------------------------------------------------------------------------------
def check_cfr_surface(n_boards, n_iters):
    """DiscountedCFR the way CFRPlus is used on Flop5Holdem (boards dealt by the builder, engine="auto" -> the board pass), and the suit-class path
    of PublicTree (board_mult + symmetrisation: the whole game's code path on a few classes) with the parameters handed through build_tree / copy"""
    from pokerrl_amd.game.PublicTree import PublicTree
    from pokerrl_amd.game.wrappers import HistoryEnvBuilder
    cfr = DiscountedCFR(name="wg", chief_handle=ChiefBase(t_prof=None), game_cls=G.Flop5Holdem, agent_bet_set=bet_sets.POT_ONLY, n_boards=n_boards,
                        alpha=2.0, beta=-math.inf, gamma=3.0)
    s = cfr._trees[0].solver
    assert s.engine == "fused" and cfr.algo_name == "DCFR" and s.discount == (2.0, -math.inf, 3.0)
    cfr.iterations(n_iters)
    h = s.get("expl_history")
    assert s.iter == n_iters and h.shape == (n_iters + 1, 2) and np.all(np.isfinite(h)) and np.all(np.isfinite(s.eval_avg()))
    reps, mult = pc.iso_classes(3)
    args = env_args(G.Flop5Holdem, 20000, bet_sets.POT_ONLY)
    tree = PublicTree(env_bldr=HistoryEnvBuilder(env_cls=G.Flop5Holdem, env_args=args), stack_size=args.starting_stack_sizes_list, stop_at_street=None,
                      boards=reps, board_mult=mult, suit_isomorphism="subset")
    tree.build_tree(variant="discounted", discount=(1.0, 1.0, 1.0))
    assert tree.solver.engine == "fused" and tree.solver.discount == (1.0, 1.0, 1.0)
    tree.solver.iterations(2)
    twin = tree.copy()  # rebuilds its solver with the same parameters: the checkpoint that moves the state over would be refused otherwise
    assert twin.solver.discount == (1.0, 1.0, 1.0) and twin.solver.iter == 2
    assert np.array_equal(twin.solver.get("regret"), tree.solver.get("regret"))
    return cfr


def check_policy_table():
    from pokerrl_amd.rl.tabular_agent import PolicyTable
    cfr = DiscountedCFR(name="tab", chief_handle=ChiefBase(t_prof=None), game_cls=G.DiscretizedNLHoldem, agent_bet_set=bet_sets.POT_ONLY,
                        starting_stack_sizes=[600], max_outcomes=(2, 2, 1))
    for _ in range(3):
        cfr.iteration()
    host, dev = PolicyTable.from_cfr(cfr), PolicyTable.from_solver(cfr)
    assert (dev.n_rows, dev.n_actions, dev.range_size) == (host.n_rows, host.n_actions, host.range_size)
    assert np.array_equal(dev.keys, host.keys) and np.array_equal(dev.rows, host.rows)
    for r in range(host.n_rows):
        assert np.array_equal(dev.row_probs(r), host.probs[r]), r
    host.close(), dev.close()
