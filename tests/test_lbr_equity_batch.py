"""A round's LBR equity requests answered in one batch on the device (prl_lbr_checkdown_equity_batch, prl_lbr_equity_batch.hip).
The reference of every request is the single call prl_lbr_checkdown_equity, which tests/test_lbr.py pins to the reference's rollout manager and
to the oracle: the batch must return its float32 bits. The batched engine's request / replay rounds go through the same core: same per-hand
winnings as the host worker / the reference, and no request answered by a per-request host call. CPU: the emulator build of the library."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import lbr_fixture_agent as fx  # noqa: E402
import test_lbr as T  # noqa: E402
from pokerrl_amd import _native  # noqa: E402
from pokerrl_amd.eval.lbr import BatchedLBR, LocalLBRWorker, checkdown_equity_batch  # noqa: E402
from pokerrl_amd.game import bet_sets  # noqa: E402
from pokerrl_amd.game.games import DiscretizedNLHoldem, StandardLeduc  # noqa: E402
from pokerrl_amd.rl.base_cls.EvalAgentBase import EvalAgentBase  # noqa: E402

PRL_ERR_ARG = -1
SENTINEL = np.float32(-7.25)


@pytest.fixture()
def emu_lib(monkeypatch):
    sys.path.insert(0, os.path.join(HERE, "emu"))
    import build_emu
    L = _native.bind(build_emu.build())
    monkeypatch.setattr(_native, "lib", lambda: L)
    monkeypatch.setattr(_native, "require_device", lambda: None)
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def same_bits(a, b):
    """array_equal with NaN == NaN (check_equity_kernel's comparison, element-wise)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


class Requests:
    """n_req decisions in the batch call's layout; expected(L): request by request through the single call, slots at or beyond n_q = SENTINEL"""

    def __init__(self, rules, q_stride):
        self.rules, self.q_stride, self.R, self.n_hole = rules, q_stride, int(rules.range_size), int(rules.n_hole_cards)
        self.boards, self.n_dealt, self.hands, self.ranges, self.n_q = [], [], [], [], []

    def add(self, board, hand, ranges):
        ranges = np.asarray(ranges, np.float32).reshape(-1, self.R)
        b = np.zeros(5, np.int8)
        b[:len(board)] = board
        rg = np.full((self.q_stride, self.R), np.float32(np.nan))  # rows at or beyond n_q: never read
        rg[:ranges.shape[0]] = ranges
        self.boards.append(b), self.n_dealt.append(len(board)), self.hands.append(np.asarray(hand, np.int8)), self.ranges.append(rg), self.n_q.append(ranges.shape[0])

    def arrays(self, sel=None):
        sel = range(len(self.n_q)) if sel is None else sel
        return (np.stack([self.boards[i] for i in sel]), np.array([self.n_dealt[i] for i in sel], np.int32), np.stack([self.hands[i] for i in sel]),
                np.stack([self.ranges[i] for i in sel]).astype(np.float32), np.array([self.n_q[i] for i in sel], np.int32))

    def expected(self, L):
        out = np.full((len(self.n_q), self.q_stride), SENTINEL, np.float32)
        for i in range(len(self.n_q)):
            nd, nq = self.n_dealt[i], self.n_q[i]
            board = np.ascontiguousarray(self.boards[i][:nd])
            hand = np.ascontiguousarray(self.hands[i])
            rg = np.ascontiguousarray(self.ranges[i][:nq], dtype=np.float32)
            wp = np.zeros(nq, np.float32)
            assert L.prl_lbr_checkdown_equity(ctypes.byref(self.rules), _p(board), nd, _p(hand), _p(rg), nq, _p(wp)) == 0
            out[i, :nq] = wp
        return out

    def batch(self, sel=None):
        boards, n_dealt, hands, ranges, n_q = self.arrays(sel)
        out = np.full((len(n_q), self.q_stride), SENTINEL, np.float32)
        return checkdown_equity_batch(self.rules, boards, n_dealt, hands, ranges, n_q, out=out)


def prepared_ranges(rs, cards, n):
    """agent ranges as LocalLBRWorker hands them over: LBR's cards and the board removed, normalised"""
    ranges = (rs.random_sample((n, 1326)) ** 3).astype(np.float32)
    c1, c2 = np.triu_indices(52, 1)
    ranges[:, np.isin(c1, list(cards)) | np.isin(c2, list(cards))] = 0
    ranges /= ranges.sum(axis=1, keepdims=True)
    return ranges


def holdem_requests(to_come_and_n_q, q_stride, seed=11, zero_range_at=None, descending_at=None, duplicate=None):
    rs = np.random.RandomState(seed)
    req = Requests(DiscretizedNLHoldem.native_rules(), q_stride)
    for i, (k, nq) in enumerate(to_come_and_n_q):
        cards = rs.choice(52, 2 + 5 - k, replace=False)
        hand, board = np.sort(cards[:2]), cards[2:]
        ranges = prepared_ranges(rs, cards, nq) if k > 2 else (rs.random_sample((nq, 1326)) ** 4).astype(np.float32)
        if zero_range_at == i:
            ranges[-1] = 0  # an all-zero range becomes uniform
        if descending_at == i:
            hand = hand[::-1]  # an unsorted hand is sorted by the call
        req.add(board, hand, ranges)
    if duplicate is not None:
        d = duplicate
        req.add(req.boards[d][:req.n_dealt[d]], req.hands[d], req.ranges[d][:req.n_q[d]])
    return req


def leduc_requests(n, seed=5):
    rs = np.random.RandomState(seed)
    req = Requests(StandardLeduc.native_rules(), 3)
    for _ in range(n):
        cards = rs.choice(6, 2, replace=False)
        nd = int(rs.randint(0, 2))
        ranges = (rs.random_sample((int(rs.randint(1, 4)), 6)) ** 2).astype(np.float32)
        if rs.randint(0, 8) == 0:
            ranges[0] = 0
        req.add(cards[1:1 + nd], cards[:1], ranges)
    return req


# requests with 0, 1, 2, 3 and 4 cards to come and ONE with 5; n_q 1 / 2 / 3 under q_stride 4; an all-zero range; a hand given in descending
# order; request 1 sent twice
HOLDEM_MIX = dict(to_come_and_n_q=[(0, 1), (1, 2), (2, 3), (3, 1), (4, 2), (5, 1)], q_stride=4, zero_range_at=2, descending_at=4, duplicate=1)
_gpu_ref = {}


def gpu_holdem_mix():
    """the mixed hold'em call and its request-by-request reference: computed once, shared by the tests that need it"""
    if "mix" not in _gpu_ref:
        req = holdem_requests(**HOLDEM_MIX)
        want = req.expected(_native.lib())
        want.setflags(write=False)
        _gpu_ref["mix"] = (req, want)
    return _gpu_ref["mix"]


def check_leduc(L):
    req = leduc_requests(40)
    want = req.expected(L)
    assert sorted(set(req.n_dealt)) == [0, 1] and sorted(set(req.n_q)) == [1, 2, 3]
    got = req.batch()
    assert same_bits(got, want), (got, want)
    assert np.all(got[np.arange(3)[None, :] >= np.array(req.n_q)[:, None]] == SENTINEL)
    assert same_bits(req.batch([7]), want[7:8])  # n_req = 1


@pytest.mark.gpu
def test_gpu_equity_batch_holdem_equals_the_single_call():
    _native.require_device()
    req, want = gpu_holdem_mix()
    assert sorted(5 - nd for nd in req.n_dealt) == [0, 1, 1, 2, 3, 4, 5] and req.hands[4][0] > req.hands[4][1]
    got = req.batch()
    assert same_bits(got, want), (got, want)
    untouched = np.arange(4)[None, :] >= np.array(req.n_q)[:, None]
    assert np.all(got[untouched] == SENTINEL) and not np.any(got[~untouched] == SENTINEL)
    assert same_bits(got[6], got[1])  # the duplicated request
    # (no "< 1": the first board's win / tie lists serve every board -- the reference's quirk -- so a hand that beats everything there sums a whole range)
    assert np.all(np.isfinite(got[3:6][~untouched[3:6]]) & (got[3:6][~untouched[3:6]] > 0))


@pytest.mark.gpu
def test_gpu_equity_batch_leduc_equals_the_single_call():
    _native.require_device()
    check_leduc(_native.lib())


@pytest.mark.gpu
def test_gpu_equity_batch_in_chunks(monkeypatch):
    """PRL_LBR_EQ_BATCH_MB=1: one request per chunk, and the request larger than the budget (five cards to come: 8.5 MB) still runs. Same bits."""
    _native.require_device()
    req, want = gpu_holdem_mix()
    monkeypatch.setenv("PRL_LBR_EQ_BATCH_MB", "1")
    assert same_bits(req.batch(), want)


@pytest.mark.gpu
def test_gpu_equity_batch_before_the_flop_vs_reference():
    """the REFERENCE's rollout manager at hold'em's first decision (lbr_equity_preflop.npz): its three ranges as ONE request and as THREE requests"""
    _native.require_device()
    g = T._preflop_fixture()
    rules = DiscretizedNLHoldem.native_rules()
    ranges = np.ascontiguousarray(g["range"], dtype=np.float32)
    n = ranges.shape[0]
    hand = np.asarray(g["hand"], np.int8).reshape(1, 2)
    one = checkdown_equity_batch(rules, np.zeros((1, 5), np.int8), [0], hand, ranges[None], [n])
    assert np.array_equal(one[0], g["wp"]), (one, g["wp"])
    three = checkdown_equity_batch(rules, np.zeros((n, 5), np.int8), [0] * n, np.repeat(hand, n, axis=0), ranges[:, None, :], [1] * n)
    assert np.array_equal(three[:, 0], g["wp"]), (three, g["wp"])


def test_equity_batch_leduc_emu(emu_lib):
    check_leduc(emu_lib)


def test_equity_batch_holdem_emu(emu_lib):
    """one, two and three cards to come, one range each (nothing deeper: the emulator is slow)"""
    req = holdem_requests([(1, 1), (2, 1), (3, 1)], q_stride=2)
    want = req.expected(emu_lib)
    got = req.batch()
    assert same_bits(got, want), (got, want)
    assert np.all(got[:, 1] == SENTINEL) and np.isfinite(got[2, 0]) and float(got[2, 0]) > 0.0


def test_equity_batch_argument_errors_emu(emu_lib):
    L = emu_lib
    req = leduc_requests(4)
    boards, n_dealt, hands, ranges, n_q = req.arrays()
    out = np.full((4, 3), SENTINEL, np.float32)
    rules = ctypes.byref(req.rules)
    assert L.prl_lbr_checkdown_equity_batch(rules, 4, _p(boards), _p(n_dealt), _p(hands), _p(ranges), _p(n_q), 3, _p(out)) == 0
    assert not np.all(out == SENTINEL)
    out[:] = SENTINEL
    assert L.prl_lbr_checkdown_equity_batch(rules, 0, _p(boards), _p(n_dealt), _p(hands), _p(ranges), _p(n_q), 3, _p(out)) == PRL_ERR_ARG
    assert L.prl_lbr_checkdown_equity_batch(rules, 4, _p(boards), _p(n_dealt), _p(hands), _p(ranges), _p(n_q), int(n_q.max()) - 1, _p(out)) == PRL_ERR_ARG
    assert L.prl_lbr_checkdown_equity_batch(rules, 4, _p(boards), _p(n_dealt), _p(hands), None, _p(n_q), 3, _p(out)) == PRL_ERR_ARG
    assert L.prl_lbr_checkdown_equity_batch(rules, 4, _p(boards), _p(n_dealt), _p(hands), _p(ranges), _p(n_q), 3, None) == PRL_ERR_ARG
    assert L.prl_lbr_checkdown_equity_batch(None, 4, _p(boards), _p(n_dealt), _p(hands), _p(ranges), _p(n_q), 3, _p(out)) == PRL_ERR_ARG
    assert np.all(out == SENTINEL)  # nothing ran
    assert L.prl_lbr_batch_last_info(None) == PRL_ERR_ARG


# ---- the batched engine plays the same hands ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_batched_lbr_before_the_flop_answers_its_requests_on_the_device(tmp_path):
    """T.check_batched_before_the_flop_vs_host with the counters of the rounds: BatchedLBR (lbr_check_to_round = None on DiscretizedNLHoldem) = the host
    LocalLBRWorker hand for hand, every equity request answered in a batch"""
    _native.require_device()
    n_hands = 16
    t_prof = T.make_t_prof(DiscretizedNLHoldem, bet_sets.B_2, dict(lbr_bet_set=bet_sets.B_2, lbr_check_to_round=None), n_hands, tmp_path)
    record = []
    w = LocalLBRWorker(t_prof=t_prof, chief_handle=None, eval_agent_cls=fx.make_agent_cls(EvalAgentBase, seed=7, record=record))
    b = BatchedLBR(t_prof, agent_kind="hash", agent_seed=7)
    lut = DiscretizedNLHoldem.get_lut_holder()
    for seat in (0, 1):
        np.random.seed(300 + seat)
        n0 = len(record)
        host = w.run(agent_seat_id=seat, n_iterations=n_hands, mode="HASH", stack_size=[DiscretizedNLHoldem.DEFAULT_STACK_SIZE] * 2)
        decks = T.decks_from_record(record[n0:], lut, b.n_deal - 2 * b._rules.n_hole_cards)
        got = b.run(agent_seat_id=seat, n_hands=n_hands, decks=decks)
        assert np.array_equal(got, host), "seat %d: %d of %d hands differ" % (seat, int(np.sum(got != host)), n_hands)
        s = b.last_stats
        assert s["equity_requests"] > 0 and s["equity_host_calls"] == 0 and s["equity_rounds"] >= 2 and s["equity_ms"] > 0.0, s


def check_small_game_through_the_rounds(tag, tmp_path, monkeypatch, n=60):
    """StandardLeduc / DiscretizedNLLeduc with PRL_LBRB_PF_MIN=1 (their one-card-to-come decisions go through the cache, the requests and the batched
    core) against the reference's per-hand winnings -- as is; with two requests accepted per round (more are asked: hands are dropped and replayed);
    and with a cache that starts at eight slots on top (it grows mid-run)"""
    game_cls, agent_bets, lbr_kwargs = T.CASES[tag]
    g = np.load(os.path.join(HERE, "golden", "lbr_%s.npz" % tag))
    n = min(int(g["n_hands"]), n)
    t_prof = T.make_t_prof(game_cls, agent_bets, lbr_kwargs, n, tmp_path)
    b = BatchedLBR(t_prof, agent_kind="hash", agent_seed=7)
    lut = game_cls.get_lut_holder()
    record = []
    w = LocalLBRWorker(t_prof=t_prof, chief_handle=None, eval_agent_cls=fx.make_agent_cls(EvalAgentBase, seed=7, record=record))
    w._lbr_action = lambda **kw: 1  # decks only: LBR just calls, no equity work
    decks = []
    for seat in (0, 1):
        np.random.seed(int(g["np_seed"]) + seat)
        n0 = len(record)
        w.run(agent_seat_id=seat, n_iterations=n, mode="HASH", stack_size=[game_cls.DEFAULT_STACK_SIZE] * 2)
        decks.append(T.decks_from_record(record[n0:], lut, b.n_deal - 2 * b._rules.n_hole_cards))
    monkeypatch.setenv("PRL_LBRB_PF_MIN", "1")
    rounds = []
    for env in ({}, {"PRL_LBRB_MAX_REQ": "2"}, {"PRL_LBRB_MAX_REQ": "2", "PRL_LBRB_PF_CAP": "8"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        rounds.append([])
        for seat in (0, 1):
            got = b.run(agent_seat_id=seat, n_hands=n, decks=decks[seat])
            want = g["winnings_agent_seat%d" % seat][:n]
            assert np.array_equal(got, want), "%s %s seat %d: %d of %d hands differ" % (tag, env, seat, int(np.sum(got != want)), n)
            s = b.last_stats
            assert s["equity_host_calls"] == 0 and s["equity_requests"] > 2, s
            rounds[-1].append(s["equity_rounds"])
    for seat in (0, 1):
        assert rounds[1][seat] > rounds[0][seat] >= 2 and rounds[2][seat] > rounds[0][seat], rounds


@pytest.mark.parametrize("tag", ["StandardLeduc", "DiscretizedNLLeduc"])
def test_batched_lbr_small_games_through_the_rounds_emu(emu_lib, monkeypatch, tag, tmp_path):
    check_small_game_through_the_rounds(tag, tmp_path, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["StandardLeduc", "DiscretizedNLLeduc"])
def test_gpu_batched_lbr_small_games_through_the_rounds(monkeypatch, tag, tmp_path):
    _native.require_device()
    check_small_game_through_the_rounds(tag, tmp_path, monkeypatch)
