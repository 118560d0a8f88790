"""DistributedSmoother.quality_sets on N ranks (torch.distributed.run): every rank writes its sets, before and after 3 iterations,
to <out>/sets<r>.npz (tests/test_gpu_quality_sets_decomposed.py compares them with LocalMultiSmoother's).  On a 1-GPU box:
SMOOTHMESH_SHARE_GPU=1 SMOOTHMESH_BACKEND=gloo python -m torch.distributed.run --nproc-per-node 2 scripts/check_dist_quality_sets.py <out>"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch, torch.distributed as dist
from smoothmesh_amd import default_params
from smoothmesh_amd.decompose import grid_partition, decompose
from smoothmesh_amd.halo import DistributedSmoother
from smoothmesh_amd.meshgen import hex_block

out = sys.argv[1]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
local = int(os.environ.get("LOCAL_RANK", "0"))
if os.environ.get("SMOOTHMESH_SHARE_GPU"):
    local %= torch.cuda.device_count()
torch.cuda.set_device(local)
backend = os.environ.get("SMOOTHMESH_BACKEND", "nccl")
dist.init_process_group(backend, **({"device_id": torch.device("cuda", local)} if backend == "nccl" else {}))
thr = dict(nonOrthThreshold=25.0, skewThreshold=0.35, aspectThreshold=2.2)
m = hex_block(12, 10, 8, jitter=0.4, seed=31)
subs = decompose(m, grid_partition(m, (world, 1, 1)), world)
ds = DistributedSmoother(subs[rank], device=local)
ds.set_params(default_params(ds.global_min_edge()))
rec = {f"before_{k}": v for k, v in ds.quality_sets(**thr).items()}
ds.iterate(3, 0.0)
rec.update({f"after_{k}": v for k, v in ds.quality_sets(**thr).items()})
np.savez(os.path.join(out, f"sets{rank}.npz"), **rec)
ds.close()
dist.barrier()
dist.destroy_process_group()
print(f"rank {rank}: ok", flush=True)
