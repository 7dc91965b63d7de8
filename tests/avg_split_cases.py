"""
Split CFR+ average pairs (prl_solver_iterations; csrc/prl_fhp_pass.inc, fhp_avg_set / fhp_steady_pair): a seat's decision nodes form set A and set B,
A's pairs of iterations are where whole-board pairing puts them and B's run one iteration behind, so the steady kind of a board pass is a pair
(kind of A, kind of B) of U (unpaired), D (deferred), C (catch-up):

    r = 0            (D,U)   -- (U,U) if the call has no further iteration        r counts from the call's first pairable iteration
    r odd            (C,D)   -- (C,U) if it is the call's last
    r even > 0       (D,C)   -- (U,C) if it is the call's last

Per column the operations, their order and their roundings are the unpaired pass's, so every case compares against the run that does not pair at all
(PRL_FHP_NO_AVG_PAIR=1, the path the other suites pin to the oracle) BIT FOR BIT: regrets, the float64 average's bit patterns, the strategy, the
exploitability history, eval_avg() and the checkpoint blob. No tolerance anywhere. Shared by the emulator suite (test_avg_split.py) and the GPU suite
(test_avg_split_gpu.py); the helpers are avg_pairing_cases.py's.
"""
import numpy as np

import avg_pairing_cases as ac
import parity_cases as pc

NO_PAIR = ac.SWITCH
NO_SPLIT = "PRL_FHP_NO_AVG_SPLIT"

_REF = {}  # (library, case key, total) -> snapshot of the unpaired run: computed once, shared, never modified


def expected_counts(calls, delay, split=True):
    """the schedule restated: (pairs of set A, pairs of set B completed one iteration behind). A call's first pairable iteration is the first one that
    another iteration of the call follows, at which both seats play regret-matched strategies (from iteration 1 of a fresh solver on) and the average is
    being blended (t > delay); A completes a pair at every odd r, B at every even r > 0"""
    t = a = b = 0
    for n in calls:
        r = -1
        for i in range(n):
            if r >= 0:
                r += 1
            elif i + 1 < n and t >= 1 and t > delay:
                r = 0
            a += r >= 0 and r % 2 == 1
            b += split and r > 0 and r % 2 == 0
            t += 1
    return int(a), int(b)


def kinds_run(calls, delay):
    """the (kind of A, kind of B) of every pairable iteration of `calls`, by the table above"""
    t, out = 0, []
    for n in calls:
        r = -1
        for i in range(n):
            last = i == n - 1
            if r >= 0:
                r += 1
            elif not last and t >= 1 and t > delay:
                r = 0
            if r == 0:
                out.append("DU")
            elif r > 0:
                out.append(("CU" if last else "CD") if r % 2 else ("UC" if last else "DC"))
            t += 1
    return out


def snapshot(s, state=True):
    out = ac.snapshot(s, state)
    out["split_pairs"] = int(s.get("avg_split_pairs")[0])
    return out


def run(monkeypatch, make, calls, env=(), state=True):
    """the switches are read at every prl_solver_iterations call, so they are set around the calls, not around the solver's creation"""
    s = make()
    for k in (NO_PAIR, NO_SPLIT):
        monkeypatch.delenv(k, raising=False)
    for k in env:
        monkeypatch.setenv(k, "1")
    for n in calls:
        s.iterations(n)
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return snapshot(s, state)


def reference(L, monkeypatch, key, make, total, state=True):
    k = (id(L), key, total)
    if k not in _REF:
        _REF[k] = run(monkeypatch, make, (total,), env=(NO_PAIR,), state=state)
        assert (_REF[k]["pairs"], _REF[k]["split_pairs"]) == (0, 0)
    return _REF[k]


def check(L, monkeypatch, key, make, calls, delay=0, counts=None, state=True, env=()):
    """`calls` on the default path (split pairs) against ONE call of the same total that does not pair; both pair counters are the schedule's"""
    want = reference(L, monkeypatch, key, make, sum(calls), state)
    got = run(monkeypatch, make, calls, env=env, state=state)
    assert (got["pairs"], got["split_pairs"]) == (expected_counts(calls, delay) if counts is None else counts), (key, calls, got["pairs"], got["split_pairs"])
    ac.assert_identical(got, want, "%s %s" % (key, list(calls)))
    return got


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
# case 1: one call of n = 2 .. 7 on a fresh solver (pairable from iteration 1 on, so r runs to n - 2), and the same totals as iterations(k) +
# iterations(n - k): the second call starts at r = 0 again
CASE1 = [(n, None) for n in range(2, 8)] + [(n, k) for n in range(2, 8) for k in (1, 2, 3) if k < n]


def schedule_selfcheck():
    """the restated schedule against the table: case 1's single calls run every kind, a fresh solver's iteration 0 is never pairable"""
    assert {k for n, _ in CASE1[:6] for k in kinds_run((n,), 0)} == {"DU", "CD", "DC", "CU", "UC"}
    assert kinds_run((1,), 0) == [] and kinds_run((2,), 0) == [] and kinds_run((3,), 0) == ["DU", "CU"] and kinds_run((4,), 0) == ["DU", "CD", "UC"]
    assert kinds_run((2, 1), 0) == [] and kinds_run((1, 2), 0) == ["DU", "CU"]  # a call of one iteration pairs nothing: (U,U)
    assert expected_counts((7,), 0) == (3, 2) and expected_counts((20,), 0, split=False) == (9, 0) and expected_counts((1, 20), 0) == (10, 9)


def case1(L, monkeypatch, n, k):
    check(L, monkeypatch, "fhp15", ac.fhp_solver(L), (n,) if k is None else (k, n - k))


def case2_delay(L, monkeypatch):
    """delay 2, 8 iterations: modes 0 (iterations 0, 1) and 1 (iteration 2) are never paired; r = 0 at iteration 3: A pairs (3, 4), (5, 6), B pairs
    (4, 5), (6, 7) -- the call ends on (U,C)"""
    got = check(L, monkeypatch, "fhp15-delay2", ac.fhp_solver(L, delay=2), (8,), delay=2)
    assert (got["pairs"], got["split_pairs"]) == (2, 2) and kinds_run((8,), 2) == ["DU", "CD", "DC", "CD", "UC"]


def case3_no_steady(L, monkeypatch):
    """PRL_FHP_NO_STEADY: every pass is the generic instantiation, which asks for each set's kind at run time"""
    monkeypatch.setenv("PRL_FHP_NO_STEADY", "1")  # (read when the solver is created)
    got = check(L, monkeypatch, "fhp15-nosteady", ac.fhp_solver(L), (6,))
    assert (got["pairs"], got["split_pairs"]) == (2, 2)
    # ... and equals the steady-state kernels' result (the reference of case 1)
    monkeypatch.delenv("PRL_FHP_NO_STEADY")
    ac.assert_identical(got, reference(L, monkeypatch, "fhp15", ac.fhp_solver(L), 6), "generic against steady kernels")


CASE4 = ac.CASE4  # FHP9 (stack 700), FHP21 (three flop raises)


def case4_shape(L, monkeypatch, key, kw):
    """FHP9 splits 2 | 2 columns per seat. FHP21 (5 | 5) keeps whole-board pairs: its (catch-up, deferred) kind would spill more registers than its
    whole-board kinds do, so the library does not build its pair kinds and set B follows set A"""
    split = key != "fhp21"
    got = check(L, monkeypatch, key, ac.fhp_solver(L, **kw), (6,), counts=expected_counts((6,), 0, split=split))
    assert (got["pairs"], got["split_pairs"]) == ((2, 2) if split else (2, 0))


def case5_boards_per_workgroup(L, monkeypatch):
    """33 boards on two workgroups with block sums, 5 iterations: the pipeline of old-average requests crosses board and block boundaries with fewer
    nodes in it than the whole seat's"""
    monkeypatch.setenv("PRL_FHP_GRID", "2")
    monkeypatch.setenv("PRL_FHP_BLOCK_SUM", "1")
    got = check(L, monkeypatch, "fhp15-33", ac.fhp_solver(L, n_boards=33), (5,))
    assert (got["pairs"], got["split_pairs"]) == (2, 1)


def case6_weighted(L, monkeypatch):
    got = check(L, monkeypatch, "weighted", ac.weighted_solver(L), (5,))
    assert (got["pairs"], got["split_pairs"]) == (2, 1)


CASE7 = ac.CASE7  # float32 average, Linear CFR, vanilla CFR


def case7_not_taken(L, monkeypatch, key, kw):
    """the float32 average, Linear and vanilla CFR are never paired: both counters stay 0 and the switches change nothing"""
    check(L, monkeypatch, "fhp15-" + key, ac.fhp_solver(L, **kw), (5,), counts=(0, 0), state="avg_dtype" not in kw)


def case8_checkpoint(L, monkeypatch):
    """save_state after iterations(5), byte for byte -- and the blob resumes: neither set has a step pending when a call returns"""
    make = ac.fhp_solver(L)
    want = reference(L, monkeypatch, "fhp15", make, 5)
    got = run(monkeypatch, make, (5,))
    assert (got["pairs"], got["split_pairs"]) == (2, 1) and np.array_equal(got["state"], want["state"])
    s = make()
    s.load_state(got["state"])
    s.iterations(2)
    ac.assert_identical(snapshot(s), reference(L, monkeypatch, "fhp15", make, 7), "resumed from the split run's checkpoint")


def case9_switch(L, monkeypatch):
    """PRL_FHP_NO_AVG_SPLIT=1: whole-board pairs (set B follows set A, its own counter stays 0) -- the same bits as the default"""
    make = ac.fhp_solver(L)
    whole = check(L, monkeypatch, "fhp15", make, (6,), counts=expected_counts((6,), 0, split=False), env=(NO_SPLIT,))
    assert (whole["pairs"], whole["split_pairs"]) == (2, 0)
    split = run(monkeypatch, make, (6,))
    assert (split["pairs"], split["split_pairs"]) == (2, 2)
    ac.assert_identical({k: v for k, v in split.items() if k != "split_pairs"}, {k: v for k, v in whole.items() if k != "split_pairs"}, "split against whole-board pairs")


def case_oracle(L, monkeypatch):
    """the split path against the CPU oracle directly, 6 iterations (iterations(5) + iterations(1))"""
    for k in (NO_PAIR, NO_SPLIT):
        monkeypatch.delenv(k, raising=False)
    pc.check_fused_batched_vs_oracle(L, 3, 6)
