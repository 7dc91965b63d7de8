"""One rank of the sharded Discounted CFR test (spawned by tests/dcfr_cases.py: check_sharded_world2).

argv: lib_path device out_dir n_local n_iters seed   (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT from the env)
Solves the r-th contiguous block of fhp_boards(world * n_local, seed) with DCFR(2, -inf, 3) through NativeSolver(shard=...) and writes the rank's
state to out_dir/rank<r>.npz."""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    lib_path, device, out_dir = sys.argv[1:4]
    n_local, n_iters, seed = (int(x) for x in sys.argv[4:7])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world,
                            init_method="tcp://%s:%s" % (os.environ.get("MASTER_ADDR", "127.0.0.1"), os.environ["MASTER_PORT"]))
    from pokerrl_amd import _native
    from pokerrl_amd.dist import TorchExchange
    import parity_cases as pc

    L = _native.bind(lib_path)
    boards = pc.fhp_boards(world * n_local, seed=seed, with_special=False)[rank * n_local:(rank + 1) * n_local]
    t = pc.fhp_tree_of(L, boards)
    s = _native.NativeSolver(t, "discounted", 0, _lib=L, shard=(world, rank, TorchExchange(device)), discount=(2.0, -math.inf, 3.0))
    assert s.engine == "fused" and s.discount == (2.0, -math.inf, 3.0)
    s.iteration()
    s.iterations(n_iters - 1)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), expl_history=s.get("expl_history"), regret=s.get("regret"), avg_sum=s.get("avg_sum"),
             n_trunk_cols=np.int64(t.n_cols - len(boards) * 14))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
