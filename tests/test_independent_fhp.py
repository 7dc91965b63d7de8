"""
Pins the 2-hole-card generalisation (eq_const = R / C(N-H,H), the chance weights, blocked-hand zeroing, main_pot / 2 through chance
levels) INDEPENDENTLY of the oracle/kernel pair: tests/independent_fhp.py is a float64 dense-matrix solver written from the game's definition, fed only
reference-made fixtures (tree walked out of the reference env, ranks of the reference binary, the reference's hole-card table). The oracle (float32,
canonical summation orders, sorted-prefix equity) and -- on the GPU -- the HIP engines must agree with it to 1e-5 relative:
  * Flop5Holdem on 3 boards, FREE-RUNNING: uniform-strategy exploitability, current- and average-strategy exploitability after 5 CFR+ iterations of
    each side on its own;
  * one LimitHoldem run-out (three chance levels), TEACHER-FORCED: uniform-strategy exploitability, a seeded random profile, and after each of 5
    CFR+ iterations of the oracle / the GPU solver the exploitability of ITS current and average profile re-evaluated by the independent solver,
    plus its regrets after the first half-iteration against the definition's. Free-running comparison is not meaningful there, and that is
    a property of the game, not of an implementation: after the first iteration 1.75 M of the 8.46 M (node, hand) regret rows are all-zero
    (blocked hands, and action values that tie exactly on a single run-out), regret matching's `sum > 0` test is a cliff there (uniform on
    one side, pure on the other), and the best response can steer into those nodes: relative noise of 1e-7 on the instantaneous regrets
    of the independent solver ITSELF moves its exploitability after ONE iteration by 5e-4 (1.87659 -> 1.87754; the float32 oracle: 1.87770).
    The reference's own float32 loop stands on the same cliff. On three 5-card boards the free-running runs agree to 1e-5 over 5 iterations.
"""
import numpy as np
import pytest

from helpers import env_args, golden
from independent_fhp import IndependentSolver
from pokerrl_amd import _native
from pokerrl_amd.game import bet_sets
from pokerrl_amd.game import games as G

RTOL = 1e-5
N_ITERS = 5


def _fixture_inputs(n_boards):
    hr = golden("handrank.npz")
    boards = [tuple(int(c) for c in b) for b in hr["boards"][:n_boards]]
    ranks = {frozenset(b): hr["ranks"][i] for i, b in enumerate(boards)}
    hole = golden("luts.npz")["Flop5Holdem_IDX_2_HOLE_CARDS"]
    return boards, ranks, hole


def fhp_case():
    """(independent solver on the REFERENCE's tree replicated over 3 boards, product tree of the same game)"""
    boards, ranks, hole = _fixture_inputs(3)
    ind = IndependentSolver(golden("tree_Flop5Holdem_1board.npz"), hole, {(): boards}, ranks)
    b = np.array([sorted(x) for x in boards], np.int8)
    t = _native.NativeTree(G.Flop5Holdem.native_game(env_args(G.Flop5Holdem, 20000, bet_sets.POT_ONLY)), G.Flop5Holdem.native_rules(), b)
    return ind, t


def lh_case():
    """one LimitHoldem run-out (stacks 48, full betting: 17 221 nodes) dealt flop / turn / river from fixture board 0"""
    boards, ranks, hole = _fixture_inputs(1)
    b = boards[0]
    deals = {(): [b[:3]], b[:3]: [b[3:4]], b[:4]: [b[4:5]]}
    ind = IndependentSolver(golden("tree_LimitHoldem_1runout.npz"), hole, deals, ranks)
    t = _native.NativeTree(G.LimitHoldem.native_game(env_args(G.LimitHoldem, 48, None)), G.LimitHoldem.native_rules(), np.array([b], np.int8))
    return ind, t


def table_of_columns(ind, t, cols):
    """{(template node, board prefix): [R, A]} from flat-tree action columns [n_cols][R] (the oracle's / the solver's layout: column
    first_col[node] + a): template and flat tree walked side by side, chance children in the order the outcomes were listed"""
    first_col, par = t.field("first_col"), t.field("parent")
    kids = [[] for _ in par]
    for n, p in enumerate(par):
        if p >= 0:
            kids[p].append(n)
    table = {}

    def walk(n, f, b):
        k = ind.kind[n]
        if k == 1:
            assert len(kids[f]) == len(ind.deals[b])
            for i, o in enumerate(ind.deals[b]):
                walk(ind.kids[n][0], kids[f][i], b + tuple(o))
        elif k == 0:
            a = len(ind.kids[n])
            assert a == len(kids[f])
            table[(n, b)] = np.asarray(cols[first_col[f]:first_col[f] + a], np.float64).T.copy()
            for c, cf in zip(ind.kids[n], kids[f]):
                walk(c, cf, b)

    walk(0, 0, ())
    return table


def random_profile(ind, t, seed):
    """a seeded strictly positive float64 profile as flat columns [n_cols][R] + the same as the independent solver's table"""
    rng = np.random.RandomState(seed)
    cols = np.zeros((t.n_cols, ind.R))
    first_col, n_ch, kind = t.field("first_col"), t.field("n_children"), t.field("kind")
    for n in np.where(kind == 0)[0]:
        x = 0.05 + rng.random_sample((n_ch[n], ind.R))
        cols[first_col[n]:first_col[n] + n_ch[n]] = x / x.sum(axis=0, keepdims=True)
    return cols, table_of_columns(ind, t, cols)


def independent_numbers(ind, n_iters=N_ITERS):
    out = {"uniform": ind.exploitability()}
    for _ in range(n_iters):
        ind.cfr_plus_iteration()
    out["current"] = ind.exploitability()
    out["average"] = ind.exploitability(ind.avg)
    return out


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(np.abs(a - b) <= RTOL * np.abs(b)), "%s: %s against the independent solver's %s (relative %s)" % (what, a, b, np.abs(a - b) / np.abs(b))


def test_independent_solver_is_self_consistent():
    """zero-sum, BR >= EV, and -- the normalisation from first principles -- the three boards' likelihood ratios: a pair of disjoint hands sees
    n_compatible_boards / 3 * C(52,5) / C(48,5) of chance mass, so the root values of an always-fold profile are exactly +-pot/2-weighted"""
    ind, _ = fhp_case()
    ev, br, _ = ind.evaluate({})
    assert abs(np.sum(ev) / ind.R) < 1e-9                       # zero-sum under the uniform prior
    assert np.all(br - ev >= -1e-12)
    always_fold = {(0, ()): np.tile([1.0, 0.0], (ind.R, 1))}    # SB folds pre-flop with every hand: BB wins the 50 of `main_pot 100 / 2`
    ev, _, _ = ind.evaluate(always_fold)
    assert np.allclose(ev[1], 50.0, rtol=0, atol=1e-9) and np.allclose(ev[0], -50.0, rtol=0, atol=1e-9)
    # the chance weights of a run-out dealt street by street (all-in calls): with every remaining card listed, the completed boards that touch
    # neither of two disjoint hands carry a total weight of exactly 1 (1 / C(52-n_b-4, k) per outcome) -- under one turn, and under one flop
    flop, turn = (3, 17, 40), (22,)
    rest = [c for c in range(52) if c not in flop]
    deals = {flop: [(c,) for c in rest]}
    deals.update({flop + (c,): [(r,) for r in rest if r != c] for c in rest})
    ind = IndependentSolver(golden("tree_Flop5Holdem_1board.npz"), ind.hole, deals, {})
    rng = np.random.RandomState(3)
    for prefix in (flop + turn, flop):
        done = ind.completions(prefix)
        assert len(done) == (48 if len(prefix) == 4 else 49 * 48)
        hands = [set(h) for h in ind.hole[rng.permutation(ind.R)] if not set(h) & set(prefix)]
        pairs = [(h, h2) for h, h2 in zip(hands[0::2], hands[1::2]) if not h & h2][:20]
        assert len(pairs) == 20
        for h, h2 in pairs:
            mass = sum(w for b, w in done if not set(b) & (h | h2))
            assert abs(mass - 1.0) < 1e-12, (prefix, h, h2, mass)


def _oracle(case, t):
    import oracle
    r = (G.Flop5Holdem if case == "fhp3" else G.LimitHoldem).RULES
    o = oracle.Oracle({k: t.field(k) for k in oracle.Oracle.FIELDS}, t.board_rows, r.N_HOLE_CARDS, r.N_CARDS_IN_DECK, r.N_SUITS, r._RANK_RULE)
    o.cfr_reset(1, 0)
    return o


def test_oracle_agrees_with_the_independent_solver_free_running():
    ind, t = fhp_case()
    want = independent_numbers(ind)
    o = _oracle("fhp3", t)
    close(o.exploitability, want["uniform"], "oracle, uniform strategy")
    for _ in range(N_ITERS):
        o.cfr_iteration()
    close(o.exploitability, want["current"], "oracle, current strategy after %d CFR+ iterations" % N_ITERS)
    close(o.eval_avg(), want["average"], "oracle, average strategy after %d CFR+ iterations" % N_ITERS)


def regrets_close(mine, theirs, what):
    """regrets are continuous in the values (the clamp at 0 is): absolute tolerance on the scale of the largest regret of the tree"""
    scale = max(float(np.max(v)) for v in theirs.values())
    for key, want in theirs.items():
        assert np.all(np.abs(mine[key] - want) <= 2e-6 * scale), (what, key, float(np.max(np.abs(mine[key] - want))), scale)


@pytest.mark.parametrize("case", ["fhp3", "lh1"])
def test_oracle_agrees_with_the_independent_solver_teacher_forced(case):
    ind, t = fhp_case() if case == "fhp3" else lh_case()
    o = _oracle(case, t)
    close(o.exploitability, ind.exploitability(), "oracle, uniform strategy")
    # the first half-iteration (seat 0 against the uniform profile): the regrets the definition gives
    _, _, inst = ind.evaluate({}, seat=0)
    o.compute_regrets(0)
    regrets_close(table_of_columns(ind, t, o.regret), {k: np.maximum(v, 0.0) for k, v in inst.items()}, "seat 0 regrets after the first half-iteration")
    o.cfr_reset(1, 0)
    # a seeded random float64 profile: expected values and best response of an arbitrary strategy (LocalBRMaster semantics)
    cols, table = random_profile(ind, t, 7)
    o.set_strategy(cols, True)
    o.update_reach()
    o.compute_ev()
    close(o.exploitability, ind.exploitability(table), "oracle, seeded random profile")
    o.cfr_reset(1, 0)
    for it in range(1, N_ITERS + 1):  # the oracle's OWN profiles after every iteration, re-evaluated from the definition
        o.cfr_iteration()
        close(o.exploitability, ind.exploitability(table_of_columns(ind, t, o.strategy)), "oracle, its current profile after iteration %d" % it)
        close(o.eval_avg(), ind.exploitability(table_of_columns(ind, t, o.avg)), "oracle, its average profile after iteration %d" % it)


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["fused", "levels"])
def test_gpu_engines_agree_with_the_independent_solver_free_running(engine):
    """the HIP path against the definition itself (no oracle in between)"""
    _native.require_device()
    ind, t = fhp_case()
    want = independent_numbers(ind)
    s = _native.NativeSolver(t, "plus", 0, engine=engine)
    assert s.engine == engine
    close(s.exploitability(), want["uniform"], "fhp3/%s, uniform strategy" % engine)
    s.iterations(N_ITERS)
    close(s.exploitability(), want["current"], "fhp3/%s, current strategy" % engine)
    close(s.eval_avg(), want["average"], "fhp3/%s, average strategy" % engine)


@pytest.mark.gpu
@pytest.mark.parametrize("case,engine", [("fhp3", "fused"), ("lh1", "fused"), ("lh1", "levels")])
def test_gpu_engines_agree_with_the_independent_solver_teacher_forced(case, engine):
    """single-deal fused engine, per-street fused engine and LEVELS engine: their own profiles after every CFR+ iteration (and a seeded random one
    through set_strategy) re-evaluated from the definition"""
    _native.require_device()
    ind, t = fhp_case() if case == "fhp3" else lh_case()
    s = _native.NativeSolver(t, "plus", 0, engine=engine)
    assert s.engine == engine
    close(s.exploitability(), ind.exploitability(), "%s/%s, uniform strategy" % (case, engine))
    cols, table = random_profile(ind, t, 7)
    s.set_strategy(cols)
    s.compute_ev()
    close(s.exploitability(), ind.exploitability(table), "%s/%s, seeded random profile" % (case, engine))
    s.reset()
    for it in range(1, N_ITERS + 1):
        s.iteration()
        close(s.exploitability(), ind.exploitability(table_of_columns(ind, t, s.get("strategy"))), "%s/%s, its current profile after iteration %d" % (case, engine, it))
        close(s.eval_avg(), ind.exploitability(table_of_columns(ind, t, s.get("avg"))), "%s/%s, its average profile after iteration %d" % (case, engine, it))
    scale_regrets = table_of_columns(ind, t, s.get("regret"))
    assert all(np.all(v >= 0) for v in scale_regrets.values())
