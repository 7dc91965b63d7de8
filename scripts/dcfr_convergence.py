"""Average-strategy exploitability of the WHOLE Flop5Holdem game (its 134 459 suit classes, prl_solver_create_weighted) after 10, 50 and 100
iterations, for CFR+ and for Discounted CFR (1.5, 0, 2): the figure in mbb/g that users ask for. One solver alive at a time.

    python scripts/dcfr_convergence.py [--out profiles/dcfr_convergence.json] [--n-classes N]   (N: a subset of the classes, for a dry run)"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import bench  # noqa: E402
from pokerrl_amd import _native  # noqa: E402
from pokerrl_amd.game import board_enum  # noqa: E402
from pokerrl_amd.game import games as G  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n-classes", type=int, default=None)
    ap.add_argument("--checkpoints", default="10,50,100")
    args = ap.parse_args()
    _native.require_device()
    reps, mult = board_enum.single_deal_board_classes(G.Flop5Holdem)
    sym = True
    if args.n_classes:
        reps, mult, sym = reps[:args.n_classes], mult[:args.n_classes], "subset"
    tree = bench.fhp_tree(reps)
    marks = [int(x) for x in args.checkpoints.split(",")]
    out = {"game": "Flop5Holdem", "classes": int(len(reps)), "boards": int(mult.sum()), "unit": "mbb/g (mean over seats x EV_NORMALIZER)", "series": {}}
    for variant in ("plus", "discounted"):
        t0 = time.perf_counter()
        s = _native.NativeSolver(tree, variant, 0, board_mult=mult, symmetrize=sym)
        rows, done = [], 0
        for m in marks:
            s.iterations(m - done)
            done = m
            avg = float(np.mean(s.eval_avg()) * G.Flop5Holdem.EV_NORMALIZER)
            cur = float(np.mean(s.exploitability()) * G.Flop5Holdem.EV_NORMALIZER)
            rows.append({"iterations": m, "average_strategy": avg, "current_strategy": cur})
            print(variant, m, "avg %.4f current %.4f (%.0f s)" % (avg, cur, time.perf_counter() - t0), flush=True)
        out["series"]["CFR+" if variant == "plus" else "DCFR(1.5, 0, 2)"] = rows
        del s
        gc.collect()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
