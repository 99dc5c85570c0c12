"""Worker of test_gpu_likelihood.test_two_ranks_return_the_one_rank_estimate: one rank of a 2-process run of
Model.log_likelihood on ONE GPU (gloo carries the per-window results through the host)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clvae_amd  # noqa: F401,E402
from likelihood_case import vrnn_case  # noqa: E402


def main():
    rank, world, out = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), sys.argv[1]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    model, x, y, _ = vrnn_case(torch.device("cuda:0"), B=8)
    r = model.log_likelihood(x, y, k=5, seed=3, per_window=True)
    torch.cuda.synchronize()
    np.savez(out % rank, **r['windows'])
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
