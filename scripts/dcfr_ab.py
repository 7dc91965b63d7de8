"""Board-pass cost of Discounted CFR against Linear CFR at the benchmark size (Flop5Holdem, 262 144 seeded boards, single-deal fused engine).

DCFR moves Linear CFR's bytes (regrets, avg_sum; the average is materialised on demand), so its board pass should cost what Linear's costs. Solver
objects of one process differ by up to 15 % with where their arrays land ("Spread"), so two objects side by side prove nothing:
ONE solver is alive at a time -- a destroyed solver's memory is taken again by the next one -- and the variants alternate, Linear, DCFR, three times.
Every object: three warm-up iterations, then time_iterations_ex(20); printed: the summed board-pass kernel milliseconds per iteration.

    python scripts/dcfr_ab.py [--boards 262144] [--rounds 3] [--steps 20] [--with-generic]

The yardstick: DCFR's median no worse than Linear's median plus Linear's own spread (max - min over its objects of the run), the noise floor of this
comparison. On the generic board-pass kernel (STEADY == 0) DCFR missed it by 17 %, so it has a steady-state kind of its own (STEADY == 7, as Linear's
2 and Vanilla's 3), with which it is 1.2 % behind Linear (profiles/dcfr_ab.txt); --with-generic adds three DCFR objects created under PRL_FHP_NO_STEADY (the generic kernel in the steady state too) for the record."""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402
from pokerrl_amd import _native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--with-generic", action="store_true")
    args = ap.parse_args()
    _native.require_device()
    tree = bench.fhp_tree(bench.seeded_boards(args.boards, 0))
    ms = {"linear": [], "discounted": [], "discounted-generic": []}
    order = [v for _ in range(args.rounds) for v in ("linear", "discounted")] + (["discounted-generic"] * args.rounds if args.with_generic else [])
    for n, variant in enumerate(order):
        if variant == "discounted-generic":
            os.environ["PRL_FHP_NO_STEADY"] = "1"  # (read when the solver is created)
        s = _native.NativeSolver(tree, variant.split("-")[0], 0, engine="fused")
        os.environ.pop("PRL_FHP_NO_STEADY", None)
        s.iterations(3)
        s.sync()
        total_ms, pass_ms, n_pass = s.time_iterations_ex(args.steps)
        ms[variant].append(pass_ms / args.steps)
        print("object %d %-18s board-pass %.3f ms/iteration (%d launches, whole iteration %.3f ms)"
              % (n, variant, pass_ms / args.steps, n_pass, total_ms / args.steps), flush=True)
        del s
        gc.collect()
    lin, dcfr = np.array(ms["linear"]), np.array(ms["discounted"])
    spread = float(lin.max() - lin.min())
    out = {"boards": args.boards, "steps": args.steps, "linear_ms": [float(x) for x in lin], "discounted_ms": [float(x) for x in dcfr],
           "linear_median": float(np.median(lin)), "discounted_median": float(np.median(dcfr)), "linear_spread": spread,
           "discounted_within_linear_median_plus_spread": bool(np.median(dcfr) <= np.median(lin) + spread)}
    if args.with_generic:
        out["discounted_generic_kernel_ms"] = [float(x) for x in ms["discounted-generic"]]
        out["discounted_generic_kernel_median"] = float(np.median(ms["discounted-generic"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
