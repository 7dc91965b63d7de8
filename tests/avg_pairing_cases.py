"""
Paired CFR+ average updates (prl_solver_iterations; csrc/prl_fhp_pass.inc, FhpCtxT kinds 5 / 6): of two consecutive iterations of one call the
first leaves the boards' float64 average alone and the second applies both steps in registers. Same operations, same order, same roundings --
so every case here compares a solver that pairs against one that does not (PRL_FHP_NO_AVG_PAIR=1, the path the other suites pin to the oracle)
BIT FOR BIT: regrets, the float64 average's bit patterns, the strategy, the exploitability history, eval_avg() and the checkpoint blob. No
tolerance anywhere. Shared by the emulator suite (test_avg_pairing.py) and the GPU suite (test_avg_pairing_gpu.py).
"""
import numpy as np

import parity_cases as pc
from pokerrl_amd import _native
from pokerrl_amd.game import games as G

SWITCH = "PRL_FHP_NO_AVG_PAIR"
FIELDS = ("regret", "avg", "strategy", "expl_history")

_REF = {}  # (library, case key, calls) -> snapshot of the unpaired run: computed once, shared, never modified


def expected_pairs(calls, delay):
    """the pairing rule restated: inside a call, (t, t + 1) is a pair when another iteration of the call follows, both seats play regret-matched
    strategies (from iteration 1 of a fresh solver on) and the average is being blended at t (t > delay)"""
    t = pairs = 0
    for n in calls:
        i = 0
        while i < n:
            step = 2 if (i + 1 < n and t >= 1 and t > delay) else 1
            pairs += step == 2
            i += step
            t += step
    return pairs


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def snapshot(s, state=True):
    out = {k: s.get(k) for k in FIELDS}
    out["eval_avg"] = s.eval_avg()
    if state:  # (no checkpoints for solvers with the float32 running average)
        out["state"] = s.save_state()
    out["pairs"] = int(s.get("avg_pairs")[0])
    return out


def run(monkeypatch, make, calls, paired, state=True):
    """the switch is read at every prl_solver_iterations call, so it is set around the calls, not around the solver's creation"""
    s = make()
    if paired:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "1")
    for n in calls:
        s.iterations(n)
    monkeypatch.delenv(SWITCH, raising=False)
    return snapshot(s, state)


def reference(L, monkeypatch, key, make, calls, state=True):
    k = (id(L), key, tuple(calls))
    if k not in _REF:
        _REF[k] = run(monkeypatch, make, calls, paired=False, state=state)
        assert _REF[k]["pairs"] == 0
    return _REF[k]


def assert_identical(got, want, what):
    assert got.keys() == want.keys()
    for k in FIELDS + ("eval_avg",) + (("state",) if "state" in want else ()):
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        assert np.array_equal(bits(a), bits(b)), "%s: %s differs in %d entries" % (what, k, int(np.sum(bits(a) != bits(b))))


def check(L, monkeypatch, key, make, calls, delay=0, pairs=None, state=True):
    """`calls` with pairing against ONE call of the same total without (the unpaired path); the number of pairs taken is the rule's"""
    want = reference(L, monkeypatch, key, make, (sum(calls),), state)
    got = run(monkeypatch, make, calls, paired=True, state=state)
    assert got["pairs"] == (expected_pairs(calls, delay) if pairs is None else pairs), (key, calls, got["pairs"])
    assert_identical(got, want, "%s %s" % (key, list(calls)))
    return got


# ---- solvers ---------------------------------------------------------------------------------------------------------------------------
def fhp_solver(L, n_boards=3, delay=0, variant="plus", stack=20000, flop_raises=None, nodes_per_board=15, **kw):
    def make():
        t = _native.NativeTree(pc.fhp_game(stack, flop_raises), G.Flop5Holdem.native_rules(), pc.fhp_boards(n_boards), _lib=L)
        assert t.n_nodes == 5 + nodes_per_board * n_boards
        s = _native.NativeSolver(t, variant, delay, engine="fused", _lib=L, **kw)
        assert s.engine == "fused"
        return s
    return make


def weighted_solver(L):
    reps, mult = pc.iso_classes(4)

    def make():
        s = _native.NativeSolver(pc.fhp_tree_of(L, reps), "plus", 0, _lib=L, board_mult=mult, symmetrize="subset")
        assert s.engine == "fused"
        return s
    return make


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
# case 1: n iterations in one call after a fresh solver (pairs start at iteration 1, with and without a leftover), and the same totals as
# iterations(k) + iterations(n - k): the second call's first iteration is then the deferred half of a pair and runs its seat-0 pass through the
# generic UPDATE0 kernel (in one call, iteration 1 runs through the generic UPDATE0_EVAL)
CASE1 = [(n, None) for n in (2, 3, 4, 5)] + [(n, k) for n in (2, 3, 4, 5) for k in (1, 2) if k < n]


def case1(L, monkeypatch, n, k):
    check(L, monkeypatch, "fhp15", fhp_solver(L), (n,) if k is None else (k, n - k))


def case2_delay(L, monkeypatch):
    """delay 2, 7 iterations: modes 0 (iterations 0, 1) and 1 (iteration 2) are never paired; pairs (3, 4), (5, 6)"""
    got = check(L, monkeypatch, "fhp15-delay2", fhp_solver(L, delay=2), (7,), delay=2)
    assert got["pairs"] == 2


def case3_no_steady(L, monkeypatch):
    """PRL_FHP_NO_STEADY: every pass is the generic instantiation, which takes the deferred and the catch-up form at run time"""
    monkeypatch.setenv("PRL_FHP_NO_STEADY", "1")  # (read when the solver is created)
    got = check(L, monkeypatch, "fhp15-nosteady", fhp_solver(L), (5,))
    assert got["pairs"] == 2
    # ... and equals the steady-state kernels' result (the reference of case 1)
    monkeypatch.delenv("PRL_FHP_NO_STEADY")
    assert_identical(got, reference(L, monkeypatch, "fhp15", fhp_solver(L), (5,)), "generic against steady kernels")


CASE4 = [("fhp9", dict(stack=700, nodes_per_board=9)), ("fhp21", dict(flop_raises=3, nodes_per_board=21))]


def case4_shape(L, monkeypatch, key, kw):
    got = check(L, monkeypatch, key, fhp_solver(L, **kw), (5,))
    assert got["pairs"] == 2


def case5_boards_per_workgroup(L, monkeypatch):
    """33 boards on two workgroups with block sums: the prefetch and the pipeline of old-average requests cross board boundaries, and a summation block
    boundary"""
    monkeypatch.setenv("PRL_FHP_GRID", "2")
    monkeypatch.setenv("PRL_FHP_BLOCK_SUM", "1")
    got = check(L, monkeypatch, "fhp15-33", fhp_solver(L, n_boards=33), (4,))
    assert got["pairs"] == 1


def case6_weighted(L, monkeypatch):
    got = check(L, monkeypatch, "weighted", weighted_solver(L), (4,))
    assert got["pairs"] == 1


CASE7 = [("f32", dict(avg_dtype="f32")), ("linear", dict(variant="linear")), ("vanilla", dict(variant="vanilla"))]


def case7_not_taken(L, monkeypatch, key, kw):
    """the float32 average, Linear and vanilla CFR are never paired: the switch changes nothing"""
    check(L, monkeypatch, "fhp15-" + key, fhp_solver(L, **kw), (4,), pairs=0, state="avg_dtype" not in kw)


def case8_checkpoint(L, monkeypatch):
    """save_state after iterations(4), byte for byte -- and the blob resumes: nothing of a pair is pending when a call returns"""
    make = fhp_solver(L)
    want = reference(L, monkeypatch, "fhp15", make, (4,))
    got = run(monkeypatch, make, (4,), paired=True)
    assert got["pairs"] == 1 and np.array_equal(got["state"], want["state"])
    s = make()
    s.load_state(got["state"])
    s.iterations(1)
    assert_identical(snapshot(s), reference(L, monkeypatch, "fhp15", make, (5,)), "resumed from the paired run's checkpoint")


def case_oracle(L, monkeypatch, n_iters, delay):
    """the paired path against the CPU oracle directly (iterations(n - 1) + iterations(1))"""
    monkeypatch.delenv(SWITCH, raising=False)
    pc.check_fused_batched_vs_oracle(L, 3, n_iters, delay=delay)
