"""What train.py and evaluate.py share: the rank setup, the two header lines
and the operating-point CSV.  Importing this module does not import torch."""
from __future__ import annotations

import csv
import os
from collections import namedtuple

import numpy as np

# dist: torch.distributed once the process group is up, None for one process;
# coll_dev: where small host-side collectives (seed, metric sums, replica
# digests) live -- device tensors under RCCL, host tensors under gloo
Ranks = namedtuple("Ranks", "rank world local backend dist coll_dev")


def ranks(versions_first: bool = False) -> Ranks:
    """This process's place among the ranks torchrun started (WORLD_SIZE, RANK,
    LOCAL_RANK), with the process group initialised when there is more than one.
    versions_first: rank 0 prints the header lines (print_versions) before the
    group comes up -- train.py's order; gloo announces its peers on stdout.
    Rehearsal knobs for the N > 1 path on a one-GPU box (as bench.py's):
    JR_ONE_DEVICE=1 (or JR_BENCH_ONE_DEVICE=1) puts every rank on cuda:0,
    JR_DIST_BACKEND=gloo replaces RCCL (which refuses two ranks on one device)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if versions_first and rank == 0:
        print_versions()
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("JR_ONE_DEVICE") == "1" or os.environ.get("JR_BENCH_ONE_DEVICE") == "1":
        local = 0
    backend = os.environ.get("JR_DIST_BACKEND", "nccl")
    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    return Ranks(rank, world, local, backend, dist, "cuda" if backend == "nccl" else "cpu")


def print_versions() -> None:
    """The reference's two header lines."""
    import torch
    print(f"Numpy version: {np.__version__}")
    print(f"Torch version: {torch.__version__} (libjr / MI355X backend)")


def write_operating_points(path, thresholds, specificities, sensitivities, n) -> None:
    """The space-delimited CSV of the first n thresholds: threshold, specificity, sensitivity."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        w = csv.writer(f, delimiter=" ")
        w.writerow(["threshold", "specificity", "sensitivity"])
        for idx in range(n):
            w.writerow(["{:0.4f}".format(v) for v in (thresholds[idx], specificities[idx], sensitivities[idx])])
