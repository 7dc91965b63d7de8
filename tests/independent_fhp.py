"""
INDEPENDENT float64 solver for 2-hole-card public trees, written from the game's definition only (test infrastructure).

Nothing here comes from oracle/ or pokerrl_amd/: no import, no shared helper, none of their formulas (no sorted-rank prefix sums, no
per-card blocker corrections, no eq_const / chance-weight constants, no float32, no canonical summation order). Terminal values are dense
1326 x 1326 matrix products over explicit compatibility masks, the recursion is the textbook one, everything is float64. Inputs are reference-made
fixtures only: the flat tree (tests/golden/tree_*.npz, walked out of the reference env), hand ranks (handrank.npz, the reference binary), the
hole-card table (luts.npz). It pins what the oracle and the kernels share by construction: SURVEY Appendix C's constants end to end.

The game (reference semantics, generalised the only way that collapses to first principles on the full deck):
  * both seats get two hole cards from 52; P(h) = 1/R, P(h' | h) = [h' disjoint from h] / C(50,2)   (ValueFiller.py:19,103-125: N/(N-1) for one card)
  * a chance node that deals k cards onto a board of n_b cards lists nc outcomes, each with prior 1/nc; given two hands that the outcome does not
    touch its likelihood ratio is C(52-n_b, k) / C(52-n_b-4, k) -- for the full list (nc = C(52-n_b, k)) that is P(outcome | both hands) =
    1 / C(52-n_b-4, k), StrategyFiller.py:159-166 with its "N_CARDS - 2" read as "cards left once both hands are out"
  * terminal utility of seat p: +-main_pot/2 (fold: the folder loses, ValueFiller.py:112; showdown: higher rank wins, ties 0, :145-155), 0 for a
    hand that shares a card with the board (:57-59); main_pot as the reference env reports it before the money moves (PublicTree.py:244-251)
  * ev[p][h] = E[utility | own hand h] under the strategy profile; best response = max over own actions per hand; exploitability[p] = sum_h P(h) (br - ev)[h]
  * an all-in call ends the betting below an incomplete board (the env runs the board out inside the step): its SHOWDOWN node is the expectation
    over the listed continuations of that board prefix, dealt street by street with the chance-node weight above (prior 1/nc of the
    continuations listed at that prefix, times C(left, k) / C(left-4, k)), each completed board paying +-main_pot/2 with the main_pot recorded
    at the all-in node
  * CFR+ as CFRPlus.py:37-87 / _CFRBase.py:122-134: seat 0 then seat 1, each on freshly computed values; regrets clamped at 0; unweighted blend average.

Inputs of the multi-deal cases (tests/golden/indep_<case>.npz, `make_golden.py indep`): the betting template walked out of the reference env
(one child per chance node), the run-out rows (deals = the distinct continuations of every prefix in row order, deals_of_runouts), the
reference evaluator's rank of every hand on every row and the reference's hole-card table.
"""
from math import comb

import numpy as np

DECISION, CHANCE, FOLD, SHOWDOWN = 0, 1, 2, 3


def deals_of_runouts(rows, streets=(3, 1, 1)):
    """{board prefix: [cards dealt next, one tuple per distinct continuation, in row order]} of full run-out rows dealt `streets` cards at a time"""
    deals = {}
    for r in rows:
        r, n = tuple(int(c) for c in r), 0
        for k in streets:
            outs = deals.setdefault(r[:n], [])
            if r[n:n + k] not in outs:
                outs.append(r[n:n + k])
            n += k
    return deals


class IndependentSolver:
    def __init__(self, tree, hole_cards, deals, ranks_of_board, delay=0):
        """tree: dict of flat arrays (kind, actor, parent, acted_last, main_pot, n_children) with ONE child per chance node (the template that is
        replicated under every listed outcome); deals: {board prefix tuple: [outcome tuples]}; ranks_of_board: {frozenset of 5 cards: int[R]}"""
        self.kind, self.actor, self.pot, self.last = (np.asarray(tree[k]) for k in ("kind", "actor", "main_pot", "acted_last"))
        self.kids = [[] for _ in self.kind]
        for n, p in enumerate(np.asarray(tree["parent"])):
            if p >= 0:
                self.kids[p].append(n)  # DFS pre-order ids: ascending id = the reference's child order
        self.hole = np.asarray(hole_cards, np.int64)
        self.R = len(self.hole)
        h = self.hole
        self.disjoint = (h[:, None, :, None] != h[None, :, None, :]).all(axis=(2, 3)).astype(np.float64)  # [R, R] hands that share no card
        self.deals, self.ranks, self.delay = deals, ranks_of_board, delay
        self.n_board = max(len(b) + len(o) for b, outs in deals.items() for o in outs)
        self.regret, self.sigma, self.avg, self.iter, self._mats = {}, {}, {}, 0, {}

    def matrix(self, kind, board):
        """U[h, h'] = utility sign of h against h' on this board (before +-pot/2), 0 where the two hands and the board are not disjoint"""
        key = (kind, board)
        if key not in self._mats:
            alive = (~np.isin(self.hole, board).any(axis=1)).astype(np.float64) if board else np.ones(self.R)
            m = self.disjoint * alive[:, None] * alive[None, :]
            if kind == SHOWDOWN:
                r = np.asarray(self.ranks[frozenset(board)], np.int64)
                m = m * np.sign(r[:, None] - r[None, :])
            self._mats[key] = m
        return self._mats[key]

    def outcome_weight(self, b, o):
        """chance weight of dealing the cards o onto the board b: prior 1 / (outcomes listed at b) times the likelihood ratio for two untouched hands"""
        left = 52 - len(b)
        return comb(left, len(o)) / comb(left - 4, len(o)) / len(self.deals[b])

    def completions(self, b):
        """[(completed board, weight)] of the listed run-outs below the prefix b, in deal order (an all-in showdown: street by street)"""
        if len(b) == self.n_board:
            return [(b, 1.0)]
        return [(f, self.outcome_weight(b, o) * w) for o in self.deals[b] for f, w in self.completions(b + tuple(o))]

    def strategy(self, table, n, b):
        a = len(self.kids[n])
        return table.get((n, b), np.full((self.R, a), 1.0 / a))

    def evaluate(self, table, seat=None, nodes=None):
        """root (ev[2,R], br[2,R]) of the profile `table`; with seat: also {(node, board): instantaneous regrets [R, A]} of that seat's nodes;
        a dict `nodes` receives every node's (ev[2,R], br[2,R]) keyed by (template node, board prefix)"""
        terms = []

        def down(n, b, w, pi):
            k = self.kind[n]
            if k == FOLD:
                terms.append((n, b, w, pi))
            elif k == SHOWDOWN:  # below an incomplete board: an all-in call, run out over the listed continuations
                for f, wf in self.completions(b):
                    terms.append((n, f, w * wf, pi))
            elif k == CHANCE:
                assert len(self.kids[n]) == 1
                for o in self.deals[b]:
                    down(self.kids[n][0], b + tuple(o), w * self.outcome_weight(b, o), pi)
            else:
                s = self.strategy(table, n, b)
                for a, c in enumerate(self.kids[n]):
                    q = list(pi)
                    q[self.actor[n]] = pi[self.actor[n]] * s[:, a]
                    down(c, b, w, q)

        down(0, (), 1.0, [np.ones(self.R), np.ones(self.R)])
        vals = [None] * len(terms)
        groups = {}
        for i, (n, b, w, pi) in enumerate(terms):
            groups.setdefault((int(self.kind[n]), b), []).append(i)
        for (k, b), idx in groups.items():  # one matrix product per (terminal kind, board): columns = the opponents' reach at those terminals
            u = self.matrix(k, b)
            for p in (0, 1):
                x = u @ np.stack([terms[i][3][1 - p] for i in idx], axis=1)
                for j, i in enumerate(idx):
                    n, _, w, _ = terms[i]
                    sgn = 1.0 if k == SHOWDOWN else (-1.0 if self.last[n] == p else 1.0)
                    if vals[i] is None:
                        vals[i] = np.zeros((2, self.R))
                    vals[i][p] = sgn * x[:, j] * w / comb(50, 2) * self.pot[n] / 2.0
        it = iter(vals)
        inst = {}

        def up(n, b):
            k = self.kind[n]
            if k >= FOLD:
                v = next(it) if k == FOLD else sum(next(it) for _ in self.completions(b))
                ev, br = v, v
            elif k == CHANCE:
                res = [up(self.kids[n][0], b + tuple(o)) for o in self.deals[b]]
                ev, br = sum(r[0] for r in res), sum(r[1] for r in res)
            else:
                p, s = self.actor[n], self.strategy(table, n, b)
                res = [up(c, b) for c in self.kids[n]]
                ev, br = np.zeros((2, self.R)), np.zeros((2, self.R))
                ev[p] = sum(s[:, a] * r[0][p] for a, r in enumerate(res))
                ev[1 - p] = sum(r[0][1 - p] for r in res)
                br[p] = np.max([r[1][p] for r in res], axis=0)
                br[1 - p] = sum(r[1][1 - p] for r in res)
                if p == seat:
                    inst[(n, b)] = np.stack([r[0][p] for r in res], axis=1) - ev[p][:, None]
            if nodes is not None:
                nodes[(n, b)] = (ev, br)
            return ev, br

        ev, br = up(0, ())
        return ev, br, inst

    def exploitability(self, table=None):
        ev, br, _ = self.evaluate(self.sigma if table is None else table)
        return (br - ev).sum(axis=1) / self.R

    def cfr_plus_iteration(self):
        for p in (0, 1):
            _, _, inst = self.evaluate(self.sigma, seat=p)
            for key, d in inst.items():
                r = np.maximum(self.regret.get(key, 0.0) + d, 0.0)
                tot = r.sum(axis=1, keepdims=True)
                self.regret[key] = r
                self.sigma[key] = np.where(tot > 0, r / np.where(tot > 0, tot, 1.0), 1.0 / r.shape[1])
                if self.iter > self.delay:
                    cur, new = sum(range(self.delay + 1, self.iter + 1)), self.iter - self.delay + 1
                    self.avg[key] = cur / (cur + new) * self.avg[key] + new / (cur + new) * self.sigma[key]
                elif self.iter == self.delay:
                    self.avg[key] = self.sigma[key].copy()
        self.iter += 1
