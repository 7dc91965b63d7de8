"""Discounted CFR (Brown & Sandholm 2019, "Solving Imperfect-Information Games via Discounted Regret Minimization"; the reference has no such
class -- it generalises its LinearCFR.py: DCFR(1, 1, 1) is Linear CFR up to a scale of the regrets).

With the 0-based iteration counter t >= 1, positive regrets are multiplied by t^alpha / (t^alpha + 1), negative ones by t^beta / (t^beta + 1) and
the reach-weighted strategy sum by (t / (t + 1))^gamma before the new terms are added; iteration 0 discounts nothing. The arithmetic is compiled
into the kernels of every engine (include/pokerrl_hip.h, prl_dcfr_factors), so it takes everything CFRPlus takes: boards= / n_boards=, engine=,
the whole game through its suit classes, checkpoints, iterations(n)."""
from pokerrl_amd.cfr._CFRBase import CFRBase as _CFRBase


class DiscountedCFR(_CFRBase):
    _VARIANT = "discounted"

    def __init__(self, name, chief_handle, game_cls, agent_bet_set, starting_stack_sizes=None, alpha=1.5, beta=0.0, gamma=2.0, **kw):
        super().__init__(name=name, chief_handle=chief_handle, game_cls=game_cls, starting_stack_sizes=starting_stack_sizes,
                         agent_bet_set=agent_bet_set, algo_name="DCFR", discount=(alpha, beta, gamma), **kw)
        self.alpha, self.beta, self.gamma = alpha, beta, gamma
        self.reset()
