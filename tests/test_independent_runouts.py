"""
All-in run-outs and multi-street deals against the INDEPENDENT solver (tests/independent_fhp.py): the float64 dense-matrix solver written from the
game's definition, fed only reference-made fixtures (tests/golden/indep_<case>.npz, `make_golden.py indep`: the betting template walked out of the
reference env, the run-out rows, the reference evaluator's ranks). What the oracle shares with the kernels -- the host tree builder's continuations
under an all-in call or a turn, the chance weights the oracle derives from that tree -- is checked here from outside.

    case     game                 stack  run-outs F x T x R  template nodes  reaches
    nl600    DiscretizedNLHoldem    600  2 x 2 x 2           169             all-ins before the flop (dealt 3 + 1 + 1), on the flop and the turn;
                                                                             mixed street shapes
    nl20000  DiscretizedNLHoldem  20000  1 x 2 x 2           2 581           the 27- and 33-node street shapes, the run-out forest at deep stacks
    lh6      LimitHoldem              6  2 x 2 x 2           139             short-stack all-ins in a limit game, pre-flop included
    lh48     LimitHoldem             48  1 x 2 x 2           17 221          several outcomes on the turn and the river below the first deal

TEACHER-FORCED throughout (free-running runs part on regret matching's cliffs, tests/test_independent_fhp.py): the uniform exploitability, seat 0's
regrets after the first half-iteration, a seeded random profile, and the implementation's own current and average profiles after every iteration
re-evaluated by the independent solver, relative 1e-5. On nl600 and lh6 also every decision node and every node an all-in call leads to (the
product's run-out chain, the template's all-in SHOWDOWN at that prefix), per seat and hand: the oracle on the CPU, the LEVELS engine on the GPU.
"""
import numpy as np
import pytest

from helpers import env_args, golden
from independent_fhp import IndependentSolver, deals_of_runouts
from pokerrl_amd import _native
from pokerrl_amd.game import bet_sets
from pokerrl_amd.game import games as G
from test_independent_fhp import close, random_profile, regrets_close, table_of_columns

CASES = {"nl600": (G.DiscretizedNLHoldem, bet_sets.POT_ONLY), "nl20000": (G.DiscretizedNLHoldem, bet_sets.POT_ONLY),
         "lh6": (G.LimitHoldem, None), "lh48": (G.LimitHoldem, None)}
N_ITERS = {"nl600": 5, "nl20000": 4, "lh6": 5, "lh48": 2, "nl600_1x2x1": 2}
NODE_CASES = ("nl600", "lh6")
EMU_ROWS = [0, 2]  # nl600's first flop, both its turns, the first river of each: 1 x 2 x 1

_CACHE = {}  # (case, rows) -> the independent solver and its numbers, shared by the oracle, emulator and GPU tests of that case


def _tree(case, rows, _lib=None):
    cls, bets = CASES[case]
    f = golden("indep_%s.npz" % case)
    return _native.NativeTree(cls.native_game(env_args(cls, int(f["stack"]), bets)), cls.native_rules(), f["runouts"][rows], _lib=_lib)


def independent(case, rows=slice(None)):
    """{ind, uniform, regrets0, random, table (of the random profile); nodes_uniform / nodes_random on NODE_CASES}"""
    key = (case, str(rows))
    if key not in _CACHE:
        f = golden("indep_%s.npz" % case)
        ranks = {frozenset(int(c) for c in r): f["ranks"][i] for i, r in enumerate(f["runouts"])}
        tpl = {k[len("tpl_"):]: v for k, v in f.items() if k.startswith("tpl_")}
        ind = IndependentSolver(tpl, f["hole_cards"], deals_of_runouts(f["runouts"][rows]), ranks)
        t = _tree(case, rows)
        c = {"ind": ind}
        nodes = {} if case in NODE_CASES else None
        ev, br, _ = ind.evaluate({}, nodes=nodes)
        c["uniform"], c["uniform_ev_br"], c["nodes_uniform"] = (br - ev).sum(axis=1) / ind.R, (ev, br), nodes
        _, _, inst = ind.evaluate({}, seat=0)
        c["regrets0"] = {k: np.maximum(v, 0.0) for k, v in inst.items()}
        cols, table = random_profile(ind, t, 7)
        nodes = {} if case in NODE_CASES else None
        ev, br, _ = ind.evaluate(table, nodes=nodes)
        c["random"], c["random_cols"], c["nodes_random"] = (br - ev).sum(axis=1) / ind.R, cols, nodes
        _CACHE[key] = c
    return _CACHE[key]


def flat_node_of(ind, t):
    """{(template node, board prefix): flat node} for decision nodes, chance nodes and terminals; a template SHOWDOWN below an incomplete board (an
    all-in call) maps to the chance node that starts the product's run-out chain, with the same pot"""
    kind, pot, par = t.field("kind"), t.field("main_pot"), t.field("parent")
    kids = [[] for _ in par]
    for n, p in enumerate(par):
        if p >= 0:
            kids[p].append(n)
    out = {}

    def walk(n, f, b):
        k = ind.kind[n]
        out[(n, b)] = f
        if k == 1:
            assert kind[f] == 1 and len(kids[f]) == len(ind.deals[b])
            for i, o in enumerate(ind.deals[b]):
                walk(ind.kids[n][0], kids[f][i], b + tuple(o))
        elif k == 0:
            assert kind[f] == 0 and len(kids[f]) == len(ind.kids[n])
            for c, cf in zip(ind.kids[n], kids[f]):
                walk(c, cf, b)
        else:
            all_in = k == 3 and len(b) < ind.n_board
            assert kind[f] == (1 if all_in else k) and pot[f] == ind.pot[n], (n, b, f, kind[f], pot[f], ind.pot[n])

    walk(0, 0, ())
    return out


def nodes_close(ind, t, ev, ev_br, want, what):
    """every decision node and every all-in call's node, per seat and hand. Units: the implementation's reach starts at 1/R and its terminal equity
    carries eq_const = R / C(50,2), so its node value is sum over h' of P(h' | h) * chance weights * opponent reach * utility -- the independent
    solver's, factor 1 at every node. Absolute tolerance on the scale of the tree's largest |value|, as regrets_close."""
    m = flat_node_of(ind, t)
    keys = [k for k in m if ind.kind[k[0]] == 0 or (ind.kind[k[0]] == 3 and len(k[1]) < ind.n_board)]
    assert any(ind.kind[k[0]] == 3 for k in keys), "the case must reach all-in calls before the river"
    scale = max(max(np.abs(want[k][0]).max(), np.abs(want[k][1]).max()) for k in keys)
    ev, ev_br = np.asarray(ev, np.float64), np.asarray(ev_br, np.float64)
    for k in keys:
        f = m[k]
        for name, mine, theirs in (("ev", ev[f], want[k][0]), ("ev_br", ev_br[f], want[k][1])):
            err = float(np.max(np.abs(mine - theirs)))
            assert err <= 2e-6 * scale, (what, name, k, f, err, scale)


def uniform_cols(t, R):
    nch, fc, kind = t.field("n_children"), t.field("first_col"), t.field("kind")
    cols = np.zeros((t.n_cols, R))
    for n in np.where(kind == 0)[0]:
        cols[fc[n]:fc[n] + nch[n]] = 1.0 / nch[n]
    return cols


@pytest.mark.parametrize("case", list(CASES))
def test_independent_solver_is_self_consistent_on_runouts(case):
    """zero-sum under the uniform prior and BR >= EV, all-in run-outs and several outcomes per street included"""
    c = independent(case)
    ev, br = c["uniform_ev_br"]
    assert abs(np.sum(ev) / c["ind"].R) < 1e-9 * np.max(np.abs(ev))
    assert np.all(br - ev >= -1e-9 * np.max(np.abs(ev)))
    assert np.all(c["uniform"] > 0)


def _oracle(case, t):
    import oracle
    r = CASES[case][0].RULES
    o = oracle.Oracle({k: t.field(k) for k in oracle.Oracle.FIELDS}, t.board_rows, r.N_HOLE_CARDS, r.N_CARDS_IN_DECK, r.N_SUITS, r._RANK_RULE)
    o.cfr_reset(1, 0)
    return o


def teacher_forced(c, t, imp, what, n_iters):
    """imp: the oracle or a NativeSolver (CFR state reset), behind a small common interface"""
    ind = c["ind"]
    close(imp.exploitability(), c["uniform"], "%s, uniform strategy" % what)
    r = imp.regrets0()
    if r is not None:  # the first half-iteration (seat 0 against the uniform profile): the regrets the definition gives
        regrets_close(table_of_columns(ind, t, r), c["regrets0"], "%s, seat 0 regrets after the first half-iteration" % what)
    imp.evaluate(c["random_cols"])
    close(imp.exploitability(), c["random"], "%s, seeded random profile" % what)
    imp.reset()
    for it in range(1, n_iters + 1):
        imp.iteration()
        close(imp.exploitability(), ind.exploitability(table_of_columns(ind, t, imp.get("strategy"))), "%s, its current profile after iteration %d" % (what, it))
        close(imp.eval_avg(), ind.exploitability(table_of_columns(ind, t, imp.get("avg"))), "%s, its average profile after iteration %d" % (what, it))


class _OracleImp:
    def __init__(self, o):
        self.o = o

    def exploitability(self):
        return self.o.exploitability

    def regrets0(self):
        self.o.compute_regrets(0)
        r = np.array(self.o.regret)
        self.reset()
        return r

    def evaluate(self, cols):
        self.o.set_strategy(cols, True)
        self.o.update_reach()
        self.o.compute_ev()

    def reset(self):
        self.o.cfr_reset(1, 0)

    def iteration(self):
        self.o.cfr_iteration()

    def get(self, name):
        return {"strategy": self.o.strategy, "avg": self.o.avg}[name]

    def eval_avg(self):
        return self.o.eval_avg()


class _SolverImp:
    def __init__(self, s, variant):
        self.s, self.variant = s, variant

    def exploitability(self):
        return self.s.exploitability()

    def regrets0(self):
        """CFR+ only: seat 0 updates first, on the uniform profile, so its clamped regrets after iteration 1 are the first half-iteration's"""
        if self.variant != "plus":
            return None
        self.s.iteration()
        r = self.s.get("regret")
        self.reset()
        return r

    def evaluate(self, cols):
        self.s.set_strategy(cols)
        self.s.compute_ev()

    def reset(self):
        self.s.reset()

    def iteration(self):
        self.s.iteration()

    def get(self, name):
        return self.s.get(name)

    def eval_avg(self):
        return self.s.eval_avg()


@pytest.mark.parametrize("case", list(CASES))
def test_oracle_agrees_with_the_independent_solver_on_runouts(case):
    c = independent(case)
    t = _tree(case, slice(None))
    o = _oracle(case, t)
    if case in NODE_CASES:  # node by node, before anything else moves the oracle's state
        o.set_strategy(uniform_cols(t, c["ind"].R), True)
        o.update_reach()
        o.compute_ev()
        nodes_close(c["ind"], t, o.ev, o.ev_br, c["nodes_uniform"], "%s/oracle, uniform profile" % case)
        o.set_strategy(c["random_cols"], True)
        o.update_reach()
        o.compute_ev()
        nodes_close(c["ind"], t, o.ev, o.ev_br, c["nodes_random"], "%s/oracle, seeded random profile" % case)
        o.cfr_reset(1, 0)
    teacher_forced(c, t, _OracleImp(o), "%s/oracle" % case, N_ITERS[case])


@pytest.fixture(scope="module")
def L():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import build_emu
    lib = _native.bind(build_emu.build())
    assert lib.prl_build_flavor().startswith(b"emu")
    return lib


def test_emu_streets_engine_agrees_with_the_independent_solver(L):
    """the per-street fused engine's kernel sources on the SIMT emulator (tests/test_emu_kernels.py), nl600 on 1 x 2 x 1 run-outs: all-in calls on
    every street before the river, each a run-out chain, two turns below the flop -- a kernel mistake the oracle shares fails here"""
    c = independent("nl600", EMU_ROWS)
    t = _tree("nl600", EMU_ROWS, _lib=L)
    s = _native.NativeSolver(t, "plus", 0, engine="auto", _lib=L)
    assert s.engine == "fused"
    teacher_forced(c, t, _SolverImp(s, "plus"), "nl600 1x2x1/emulator", N_ITERS["nl600_1x2x1"])


@pytest.mark.gpu
@pytest.mark.parametrize("case,variant", [("nl600", "plus"), ("nl20000", "plus"), ("lh6", "plus"), ("lh48", "plus"), ("lh6", "linear")])
def test_gpu_streets_engine_agrees_with_the_independent_solver(case, variant):
    """the per-street fused engine (engine=auto), teacher-forced on every case"""
    _native.require_device()
    c = independent(case)
    t = _tree(case, slice(None))
    s = _native.NativeSolver(t, variant, 0, engine="auto")
    assert s.engine == "fused", "engine=auto must take the per-street fused engine"
    teacher_forced(c, t, _SolverImp(s, variant), "%s/fused/%s" % (case, variant), N_ITERS[case])


@pytest.mark.gpu
@pytest.mark.parametrize("case", NODE_CASES)
def test_gpu_levels_engine_nodes_agree_with_the_independent_solver(case):
    """LEVELS exposes every node's vectors; the per-street engine is bit-equal to it (test_gpu_streets_engine_vs_levels_engine_bench_tree)"""
    _native.require_device()
    c = independent(case)
    t = _tree(case, slice(None))
    s = _native.NativeSolver(t, "plus", 0, engine="levels")
    assert s.engine == "levels"
    for name, cols, want in (("uniform", uniform_cols(t, c["ind"].R), c["nodes_uniform"]), ("seeded random", c["random_cols"], c["nodes_random"])):
        s.set_strategy(cols)
        s.compute_ev()
        close(s.exploitability(), c["uniform" if name == "uniform" else "random"], "%s/levels, %s profile" % (case, name))
        nodes_close(c["ind"], t, s.get("ev"), s.get("ev_br"), want, "%s/levels, %s profile" % (case, name))
