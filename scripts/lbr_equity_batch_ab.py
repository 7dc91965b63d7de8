"""Same-box A/B of LBR from the first decision (bench_lbr.py --lbr-from-the-start): the present library against another build of it (the parent
commit's, whose request rounds take one synchronous prl_lbr_checkdown_equity call per request), alternated for a number of rounds, a fresh process per
run (POKERRL_AMD_LIB picks the library). Prints every run's wall time of the timed region, hands/s, kernel seconds and the request counters, and a JSON
summary (last line): the means, the spreads (max - min) and whether the new wall time is below the other's by more than the larger spread.
Usage: python scripts/lbr_equity_batch_ab.py OTHER_LIB.so [rounds] [hands per seat] [extra bench_lbr.py arguments ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
other = os.path.abspath(sys.argv[1])
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
hands = int(sys.argv[3]) if len(sys.argv) > 3 else 262144
extra = sys.argv[4:] or ["--game", "Flop5Holdem", "--agent", "table"]
cmd = [sys.executable, os.path.join(ROOT, "bench_lbr.py"), "--lbr-from-the-start", "--hands", str(hands), "--cpu-hands", "0"] + extra
res = {"other": [], "new": []}
for r in range(rounds):
    for name in ("other", "new"):
        env = dict(os.environ)
        env.pop("POKERRL_AMD_LIB", None)
        if name == "other":
            env["POKERRL_AMD_LIB"] = other
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=900)
        if p.returncode != 0:
            sys.exit("round %d %s: bench_lbr.py exited with %d" % (r, name, p.returncode))
        c = json.loads(p.stdout.decode().strip().splitlines()[-1])
        cfg = c["config"]
        row = {"wall_s": cfg["wall_s"], "hands_per_s": c["value"], "kernel_s": cfg["device_seconds_rank0"], "equity_rounds": cfg["equity_rounds"],
               "equity_requests": cfg["equity_requests"], "equity_host_calls": cfg["equity_host_calls"], "equity_ms": cfg["equity_ms"],
               "lbr_winnings_mbb_per_g": cfg["lbr_winnings_mbb_per_g"]}
        res[name].append(row)
        print("round %d %-5s %s" % (r, name, json.dumps(row)), flush=True)
out = {"command": " ".join(cmd[1:]), "rounds": rounds}
for name, rows in res.items():
    w = [x["wall_s"] for x in rows]
    out[name] = {"wall_s_mean": sum(w) / len(w), "wall_s_min": min(w), "wall_s_max": max(w), "wall_s_spread": max(w) - min(w), "wall_s_all": w}
out["same_winnings"] = len({x["lbr_winnings_mbb_per_g"] for rows in res.values() for x in rows}) == 1
gap = out["other"]["wall_s_mean"] - out["new"]["wall_s_mean"]
out["wall_s_gap"] = gap
out["new_is_faster_by_more_than_the_larger_spread"] = gap > max(out["other"]["wall_s_spread"], out["new"]["wall_s_spread"])
print(json.dumps(out))
