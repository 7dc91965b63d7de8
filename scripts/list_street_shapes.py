"""
Lists the street shapes of a multi-street public tree the way csrc/prl_st.cpp::list_instance does (DFS pre-order below every chance
outcome that is a decision; chance nodes and showdowns are kind-3 leaves), from the library's own tree builder, and prints every
distinct shape as the three arrays of a PrlFhpSpec (csrc/prl_fhp.h) together with (nodes, max actions, decisions, leaves, folds,
columns) and whether a registered spec has the same listing. Runs on the emulator build of the library: no GPU.

    python scripts/list_street_shapes.py --bets B_2 --stacks 300 600 1200 2500 5000
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))


def registered_specs():
    """{name: (K, A, C)} parsed from the PrlFhpSpec structs of prl_fhp.h"""
    text = open(os.path.join(ROOT, "pokerrl_amd", "csrc", "prl_fhp.h")).read()
    out = {}
    for m in re.finditer(r"struct (PrlFhpSpec\w+) \{(.*?)\n\};", text, re.S):
        arrs = re.findall(r"static constexpr int ([KAC])\(int n\) \{ constexpr int t\[N_NODES\] = \{([^}]*)\}", m.group(2))
        out[m.group(1)] = {k: tuple(int(x) for x in v.split(",")) for k, v in arrs}
    return out


def shapes_of(t):
    kind, actor, nch = t.field("kind"), t.field("actor"), t.field("n_children")
    cs, cl, parent = t.field("child_start"), t.field("child_list"), t.field("parent")
    seen = {}
    for n in range(t.n_nodes):
        if kind[n] != 0 or parent[n] < 0 or kind[parent[n]] != 1:  # PRL_NODE_DECISION below PRL_NODE_CHANCE: an instance root
            continue
        K, A, C, stack = [], [], [], [n]
        while stack:
            m = stack.pop()
            if kind[m] == 0:
                K.append(0); A.append(int(actor[m])); C.append(int(nch[m]))
                stack.extend(int(cl[cs[m] + i]) for i in range(nch[m] - 1, -1, -1))
            else:
                K.append(3 if kind[m] in (1, 3) else 2); A.append(-1); C.append(0)
        key = (tuple(K), tuple(A), tuple(C))
        seen[key] = seen.get(key, 0) + 1
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", default="DiscretizedNLHoldem")
    ap.add_argument("--bets", default="B_2")
    ap.add_argument("--stacks", type=int, nargs="+", default=[300, 600, 1200, 2500, 5000])
    a = ap.parse_args()
    import build_emu
    import parity_cases as pc
    from helpers import env_args
    from pokerrl_amd import _native
    from pokerrl_amd.game import bet_sets
    from pokerrl_amd.game import games as G
    L = _native.bind(build_emu.build())
    game_cls = getattr(G, a.game)
    specs = registered_specs()
    printed = set()
    for stack in a.stacks:
        args = env_args(game_cls, stack, getattr(bet_sets, a.bets))
        t = _native.NativeTree(game_cls.native_game(args), game_cls.native_rules(), pc.multistreet_runouts(1, 1, 1), _lib=L)
        kinds = t.field("kind")
        trunk_a = 0
        nchs, n = t.field("n_children"), 0
        ss = t.field("subtree_size")
        while n < t.n_nodes:  # the trunk: everything above the first chance nodes
            if kinds[n] == 1:
                n += int(ss[n])
                continue
            if kinds[n] == 0:
                trunk_a = max(trunk_a, int(nchs[n]))
            n += 1
        print("%s %s stack %d: %d nodes, trunk max actions %d" % (a.game, a.bets, stack, t.n_nodes, trunk_a))
        for (K, A, C), count in sorted(shapes_of(t).items(), key=lambda kv: -len(kv[0][0])):
            dec = [i for i, k in enumerate(K) if k == 0]
            fig = (len(K), max(C), len(dec), K.count(3), K.count(2), sum(C[i] for i in dec))
            name = next((nm for nm, s in specs.items() if (s["K"], s["A"], s["C"]) == (K, A, C)), None)
            print("  %s x%d  %s" % (fig, count, name or "NOT REGISTERED"))
            if name is None and (K, A, C) not in printed:
                printed.add((K, A, C))
                for nm, arr in (("K", K), ("A", A), ("C", C)):
                    print("    static constexpr int %s(int n) { constexpr int t[N_NODES] = {%s}; return t[n]; }" % (nm, ", ".join(str(x) for x in arr)))


if __name__ == "__main__":
    main()
