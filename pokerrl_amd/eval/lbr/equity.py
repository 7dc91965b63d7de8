"""
The check-down equities of many independent LBR decisions in one library call (prl_lbr_checkdown_equity_batch): request i is what
LocalLBRWorker._checkdown_equity computes for (boards[i][:n_dealt[i]], hands[i], ranges[i][:n_q[i]]), bit for bit, but the requests share the launches
and their running float32 sums advance side by side on the device.
"""
import ctypes

import numpy as np

from pokerrl_amd import _native


def checkdown_equity_batch(rules, boards, n_dealt, hands, ranges, n_q, out=None):
    """rules: the game's PrlRules (env_cls.native_rules()); boards: int8 [n_req, 5] 1d cards, the first n_dealt[i] of row i count (deal order);
    hands: int8 [n_req, n_hole_cards] 1d cards; ranges: float32 [n_req, q_stride, range_size]; n_q: int32 [n_req], 1 <= n_q[i] <= q_stride.
    Returns float32 [n_req, q_stride]: P(LBR wins the check-down) per candidate range; slots at or beyond n_q[i] keep the value of `out` (zeros
    when no `out` is given)."""
    L = _native.lib()
    _native.require_device()
    ranges = np.ascontiguousarray(ranges, dtype=np.float32)
    assert ranges.ndim == 3, "ranges: [n_req, q_stride, range_size]"
    n_req, q_stride = int(ranges.shape[0]), int(ranges.shape[1])
    boards = np.ascontiguousarray(boards, dtype=np.int8).reshape(n_req, 5)
    hands = np.ascontiguousarray(hands, dtype=np.int8).reshape(n_req, -1)
    n_dealt = np.ascontiguousarray(n_dealt, dtype=np.int32).reshape(n_req)
    n_q = np.ascontiguousarray(n_q, dtype=np.int32).reshape(n_req)
    assert ranges.shape[2] == rules.range_size and hands.shape[1] == rules.n_hole_cards
    if out is None:
        out = np.zeros((n_req, q_stride), np.float32)
    assert out.dtype == np.float32 and out.shape == (n_req, q_stride) and out.flags.c_contiguous
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    _native.check(L.prl_lbr_checkdown_equity_batch(ctypes.byref(rules), n_req, p(boards), p(n_dealt), p(hands), p(ranges), p(n_q), q_stride, p(out)), L)
    return out
