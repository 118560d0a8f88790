"""DistributedSmoother.mesh_quality_geometry / mesh_quality_motion on N ranks (torch.distributed.run): every rank writes its two
reports of the decomposed mesh to <out>/rank<r>.json (tests/test_gpu_quality_geometry_motion_decomposed.py compares them with
LocalMultiSmoother's).  On a 1-GPU box: SMOOTHMESH_SHARE_GPU=1 SMOOTHMESH_BACKEND=gloo python -m torch.distributed.run
--nproc-per-node 2 scripts/check_dist_quality_geometry_motion.py <out> '<json of {"geometry": thresholds, "motion": thresholds}>'"""
import dataclasses, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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
both = lambda: {"geometry": dataclasses.asdict(ds.mesh_quality_geometry(**thr["geometry"])),  # noqa: E731
                "motion": dataclasses.asdict(ds.mesh_quality_motion(**thr["motion"]))}
rec = {"before": both()}
ds.iterate(3, 0.0)
rec["after"] = both()
with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
    json.dump({k: {w: {n: (v.hex() if isinstance(v, float) else v) for n, v in d.items()} for w, d in r.items()} for k, r in rec.items()}, f)
ds.close()
dist.barrier()
dist.destroy_process_group()
print(f"rank {rank}: ok", flush=True)
