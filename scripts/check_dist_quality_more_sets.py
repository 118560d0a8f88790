"""DistributedSmoother.quality_geometry_sets / quality_motion_sets on N ranks (torch.distributed.run): every rank writes its sets of
both kinds, before and after 3 iterations, to <out>/more_sets<r>.npz (tests/test_gpu_quality_more_sets_decomposed.py compares them
with LocalMultiSmoother's).  On a 1-GPU box: SMOOTHMESH_SHARE_GPU=1 SMOOTHMESH_BACKEND=gloo python -m torch.distributed.run
--nproc-per-node 2 scripts/check_dist_quality_more_sets.py <out> '<json of {"geometry": thresholds, "motion": thresholds}>'"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch, torch.distributed as dist
from smoothmesh_amd import default_params
from smoothmesh_amd.decompose import bfs_partition, decompose
from smoothmesh_amd.halo import DistributedSmoother
from smoothmesh_amd.meshgen import hex_block

out, thr = sys.argv[1], json.loads(sys.argv[2])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
local = int(os.environ.get("LOCAL_RANK", "0"))
if os.environ.get("SMOOTHMESH_SHARE_GPU"):
    local %= torch.cuda.device_count()
torch.cuda.set_device(local)
backend = os.environ.get("SMOOTHMESH_BACKEND", "nccl")
dist.init_process_group(backend, **({"device_id": torch.device("cuda", local)} if backend == "nccl" else {}))
m = hex_block(12, 10, 8, jitter=0.3, seed=31)
subs = decompose(m, bfs_partition(m, world, seed=2), world)
ds = DistributedSmoother(subs[rank], device=local)
ds.set_params(default_params(ds.global_min_edge()))
both = lambda when: {f"{when}_{k}": v for d in (ds.quality_geometry_sets(**thr["geometry"]), ds.quality_motion_sets(**thr["motion"]))  # noqa: E731
                     for k, v in d.items()}
rec = both("before")
ds.iterate(3, 0.0)
rec.update(both("after"))
np.savez(os.path.join(out, f"more_sets{rank}.npz"), **rec)
ds.close()
dist.barrier()
dist.destroy_process_group()
print(f"rank {rank}: ok", flush=True)
