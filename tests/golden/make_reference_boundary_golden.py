"""
Generates tests/golden/reference_boundary.json by RUNNING THE REFERENCE (read-only, imported through ref_harness with its test-only shims):
what tests/test_reference_suite.py and tests/test_f1_agents.py compare this package with, stored so that those tests need nothing outside
the repository.
  obs_idx        PokerEnv.obs_idx_dict (as a list of pairs, in order) and obs_parts_idxs_dict of four games
  nlh_episodes   heads-up NoLimitHoldem: 200 seeded random episodes (stacks, drawn actions, pot-fraction conversions, rewards)
  br_hash_agent  LocalBRMaster.evaluate of the hash agent (pokerrl_amd.rl.hash_agent, seed 7) on two games: the logged value

    python tests/golden/make_reference_boundary_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

import ref_harness  # noqa: E402

np = ref_harness.setup()


def _item(x):
    """numpy scalars as the exact Python int / float (JSON)"""
    return x.item()


def obs_idx():
    from PokerRL.game import bet_sets as rb
    from PokerRL.game import games as RG
    out = {}
    for name, bets in (("StandardLeduc", None), ("DiscretizedNLHoldem", "B_5"), ("LimitHoldem", None), ("Flop5Holdem", None)):
        cls = getattr(RG, name)
        args = cls.ARGS_CLS(n_seats=2, bet_sizes_list_as_frac_of_pot=getattr(rb, bets)) if bets else cls.ARGS_CLS(n_seats=2)
        env = cls(env_args=args, is_evaluating=True, lut_holder=cls.get_lut_holder())
        out[name] = {"obs_idx_dict": [[k, int(v)] for k, v in env.obs_idx_dict.items()],
                     "obs_parts_idxs_dict": json.loads(json.dumps(env.obs_parts_idxs_dict, default=_item))}
    return out


def nlh_episodes(cls, n_trials=200):
    """the record tests/test_reference_suite.py builds for both packages (the same code on either side)"""
    def mk(randomise):
        args = cls.ARGS_CLS(n_seats=2, stack_randomization_range=((100 - 1000) if randomise else 0, 0), starting_stack_sizes_list=[1000, 1000])
        return cls(env_args=args, is_evaluating=True, lut_holder=cls.get_lut_holder())

    recs = []
    for trial in range(n_trials):
        np.random.seed(trial)
        env = mk(trial % 2 == 1)
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
        recs.append(rec)
    return json.loads(json.dumps(recs, default=_item))


def br_hash_agent(tmp):
    import PokerRL.game.bet_sets as ref_bets
    from PokerRL.eval.br.LocalBRMaster import LocalBRMaster as RefBR
    from PokerRL.game import games as ref_games
    from PokerRL.game.wrappers import HistoryEnvBuilder as RefHistoryEnvBuilder
    from PokerRL.rl.base_cls.EvalAgentBase import EvalAgentBase as RefEvalAgentBase
    from PokerRL.rl.base_cls.TrainingProfileBase import TrainingProfileBase as RefTProf
    from PokerRL.rl.base_cls.workers.ChiefBase import ChiefBase as RefChiefBase
    from pokerrl_amd.rl import hash_agent

    class RefChief(RefChiefBase):
        def pull_current_eval_strategy(self, last):
            return None, last

    Agent = hash_agent.make_agent_cls(RefEvalAgentBase, seed=7)
    out = {}
    for game_name, bets_name in (("StandardLeduc", None), ("DiscretizedNLLeduc", "POT_ONLY")):
        ref_game = getattr(ref_games, game_name)
        ref_args = ref_game.ARGS_CLS(n_seats=2, bet_sizes_list_as_frac_of_pot=getattr(ref_bets, bets_name)) if bets_name else ref_game.ARGS_CLS(n_seats=2)
        prof = RefTProf(name="x", log_verbose=False, log_export_freq=1, checkpoint_freq=10 ** 9, eval_agent_export_freq=10 ** 9,
                        game_cls=ref_game, env_bldr_cls=RefHistoryEnvBuilder, start_chips=None, eval_modes_of_algo=("HASH",),
                        eval_stack_sizes=None, module_args={"env": ref_args}, path_data=os.path.join(tmp, game_name))
        rc = RefChief(prof)
        br = RefBR(t_prof=prof, chief_handle=rc, eval_agent_cls=Agent)
        br.update_weights()
        br.evaluate(iter_nr=0)
        (_e, graphs), = rc.get_new_values()[0].items()
        (_g, series), = graphs.items()
        out[game_name] = float(series[0][1])
    return out


if __name__ == "__main__":
    import tempfile
    from PokerRL.game.games import NoLimitHoldem
    with tempfile.TemporaryDirectory() as tmp:
        data = {"obs_idx": obs_idx(), "nlh_episodes": nlh_episodes(NoLimitHoldem), "br_hash_agent": br_hash_agent(tmp)}
    path = os.path.join(HERE, "reference_boundary.json")
    with open(path, "w") as f:
        json.dump(data, f, separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes;", data["br_hash_agent"])
