"""A/B of the split CFR+ average pairs on ONE solver object (same memory, same stream): PRL_FHP_NO_AVG_SPLIT is read at every
prl_solver_iterations call, so time_iterations_ex(20) is called alternately with the switch set (whole-board pairs: catch-up and deferred launches
alternate) and unset (set B's pairs one iteration behind set A's: every launch carries half a seat's float64 columns). One object repeats to ~0.1 %,
while different objects differ by up to 15 % from physical placement ("Spread") -- which is why the comparison stays on one.
Prints the board-pass kernel ms per iteration of every repeat and a JSON summary (last line) with the acceptance figures: the two ranges must not
overlap and the mean gain must be at least ten times the larger of the two settings' spreads.
Usage: python scripts/avg_split_toggle.py [rounds] [boards] [iterations per timing]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from pokerrl_amd import _native  # noqa: E402

SWITCH = "PRL_FHP_NO_AVG_SPLIT"
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 6
n_boards = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
n_it = int(sys.argv[3]) if len(sys.argv) > 3 else 20
_native.require_device()
tree = bench.fhp_tree(bench.seeded_boards(n_boards, 0), None)
s = _native.NativeSolver(tree, "plus", 0, engine="fused")
s.iterations(4)
os.environ[SWITCH] = "1"
s.time_iterations_ex(n_it)  # warm both paths' kernels
del os.environ[SWITCH]
s.time_iterations_ex(n_it)
res = {"whole": {"kernel_ms": [], "device_ms": []}, "split": {"kernel_ms": [], "device_ms": []}}
for r in range(rounds):
    for name in ("whole", "split"):
        if name == "whole":
            os.environ[SWITCH] = "1"
        else:
            os.environ.pop(SWITCH, None)
        pairs0, split0 = int(s.get("avg_pairs")[0]), int(s.get("avg_split_pairs")[0])
        dev_ms, pass_ms, n_pass = s.time_iterations_ex(n_it)
        assert int(s.get("avg_pairs")[0]) - pairs0 == n_it // 2
        assert int(s.get("avg_split_pairs")[0]) - split0 == ((n_it - 1) // 2 if name == "split" else 0)
        res[name]["kernel_ms"].append(pass_ms / n_it)
        res[name]["device_ms"].append(dev_ms / n_it)
        print("round %d %-6s board-pass kernels %.4f ms / iteration, device %.4f ms / iteration (%d launches)" % (r, name, pass_ms / n_it, dev_ms / n_it, n_pass), flush=True)
os.environ.pop(SWITCH, None)
out = {"boards": n_boards, "iterations_per_timing": n_it, "rounds": rounds, "iterations_done": s.iter}
for name, d in res.items():
    for k, v in d.items():
        out["%s_%s" % (name, k)] = {"mean": sum(v) / len(v), "min": min(v), "max": max(v), "all": v}
w, p = out["whole_kernel_ms"], out["split_kernel_ms"]
out["kernel_ms_ratio_split_over_whole"] = p["mean"] / w["mean"]
out["device_ms_ratio_split_over_whole"] = out["split_device_ms"]["mean"] / out["whole_device_ms"]["mean"]
spread = max(w["max"] - w["min"], p["max"] - p["min"])
out["kernel_ms_gain"] = w["mean"] - p["mean"]
out["kernel_ms_larger_spread"] = spread
out["ranges_overlap"] = not (p["max"] < w["min"])
out["bar_met"] = p["max"] < w["min"] and out["kernel_ms_gain"] >= 10 * spread
print(json.dumps(out))
