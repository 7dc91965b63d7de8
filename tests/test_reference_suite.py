"""This package side by side with the reference at the env boundary, against values captured from the reference itself
(tests/golden/reference_boundary.json, written by tests/golden/make_reference_boundary_golden.py): the observation entry names of four
games and 200 seeded random NoLimitHoldem episodes."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _item(x):
    """numpy scalars as the exact Python int / float (JSON)"""
    return x.item()


def _golden(key):
    with open(os.path.join(HERE, "golden", "reference_boundary.json")) as f:
        return json.load(f)[key]


def test_observation_entry_names_match_the_reference():
    """PokerEnv.obs_idx_dict / obs_parts_idxs_dict (what print_obs and the reference's neural modules index observations by)"""
    from pokerrl_amd.game import bet_sets as mb
    from pokerrl_amd.game import games as MG
    golden = _golden("obs_idx")
    for name, bets in (("StandardLeduc", None), ("DiscretizedNLHoldem", "B_5"), ("LimitHoldem", None), ("Flop5Holdem", None)):
        mcls = getattr(MG, name)
        ma = mcls.ARGS_CLS(n_seats=2, bet_sizes_list_as_frac_of_pot=getattr(mb, bets)) if bets else mcls.ARGS_CLS(n_seats=2)
        ours = mcls(env_args=ma, is_evaluating=True, lut_holder=mcls.get_lut_holder())
        assert [[k, int(v)] for k, v in ours.obs_idx_dict.items()] == golden[name]["obs_idx_dict"], name  # names, indices and their order
        assert json.loads(json.dumps(ours.obs_parts_idxs_dict, default=_item)) == golden[name]["obs_parts_idxs_dict"], name


def test_no_limit_holdem_random_episodes_match_the_reference():
    """Heads-up NoLimitHoldem side by side with the reference for 200 seeds: the stacks a freshly constructed env shows, the stacks after
    reset(), the (type, chips) actions get_random_action draws, the rewards and the final stacks of whole random episodes -- with equal
    and with randomised starting stacks -- and get_fraction_of_pot_raise / get_frac_from_chip_amt along the way, also after the hand is over."""
    from pokerrl_amd.game.games import NoLimitHoldem as MN
    golden = _golden("nlh_episodes")

    def mk(cls, randomise):
        args = cls.ARGS_CLS(n_seats=2, stack_randomization_range=((100 - 1000) if randomise else 0, 0), starting_stack_sizes_list=[1000, 1000])
        return cls(env_args=args, is_evaluating=True, lut_holder=cls.get_lut_holder())

    for trial in range(200):
        outs = []
        for cls in (MN,):
            np.random.seed(trial)
            env = mk(cls, trial % 2 == 1)
            rec = [[p.stack for p in env.seats]]
            env.reset()
            rec.append([p.stack for p in env.seats])
            done = False
            while not done:
                a = env.get_random_action()
                nxt = env.current_player.seat_id
                rec.append((a, env.get_fraction_of_pot_raise(fraction=0.7, player_that_bets=env.seats[nxt]),
                            round(env.get_frac_from_chip_amt(amt=233, player_that_bets=env.seats[nxt]), 12)))
                _o, r, done, _i = env.step(action=a)
            rec.append(([float(x) for x in r], [p.stack for p in env.seats], env.get_fraction_of_pot_raise(fraction=1.4, player_that_bets=env.seats[0])))
            outs.append(rec)
        assert json.loads(json.dumps(outs[0], default=_item)) == golden[trial], trial
