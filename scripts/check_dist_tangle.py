"""DistributedSmoother with the tangle constraint (DESIGN.md "Mesh quality", 10.13) on two ranks (torch.distributed.run) against
its CPU restatement (tests/tangle_multi_reference.py): the dented block cut (1, 1, 2), where from iteration 7 on rank 1 has no bad
cell of its own and must put back shared points the loop had moved.  Per iteration the points (rel_linf <= 1e-13), at the end
this rank's records, the combined records and the summed exempt count; in order and with an exchange stream
(SMOOTHMESH_EXCHANGE=push: the peer-store transport, which has no exchange stream -- both legs then run in order).
On a 1-GPU box: SMOOTHMESH_SHARE_GPU=1 SMOOTHMESH_BACKEND=gloo python -m torch.distributed.run --nproc-per-node 2 ... (the
engines are the real ones; only the transport is gloo).  Exit code 1 on a mismatch."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch, torch.distributed as dist
from oracle import oracle_ffi
from smoothmesh_amd.halo import DistributedSmoother
from tangle_multi_reference import FIELDS, MARGIN, TangleMultiReference
from test_gpu_quality_trace import dented_block

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
assert world == 2
local = int(os.environ.get("LOCAL_RANK", "0"))
if os.environ.get("SMOOTHMESH_SHARE_GPU"):
    local %= torch.cuda.device_count()
torch.cuda.set_device(local)
backend = os.environ.get("SMOOTHMESH_BACKEND", "nccl")
dist.init_process_group(backend, **({"device_id": torch.device("cuda", local)} if backend == "nccl" else {}))
oracle_ffi.build()
N = 8
bad = 0
for overlap in (False, True):
    ref = TangleMultiReference(oracle_ffi, dented_block(), (1, 1, 2), 2, "com", False, maxStepLength=1.0, minEdgeLength=1e-4)
    want = ref.run(N)
    assert ref.minMargin > MARGIN
    assert any(r == 1 and moved > 0 for _, _, r, _, moved in ref.foreign)      # the case is the one its docstring names
    ds = DistributedSmoother(ref.subs[rank], device=local, overlap=overlap)
    ds.set_params(ref.prm)
    ds.set_tangle_constraint(2)
    ok = ds.tangle_state().nExemptCells == sum(ref.nExemptCells)
    worst = 0.0
    for k in range(N):
        n, res, frz = ds.iterate(1, 0.0)
        p, q = ds.get_points(), want["pts"][k][rank]
        worst = max(worst, float(np.max(np.abs(p - q)) / np.max(np.abs(q))))
        ok = ok and n == 1 and int(frz[0]) == int(want["frz"][k])
    per_rank = ds.tangle_records(per_rank=True)
    mine = [{f: getattr(r, f) for f in FIELDS} for r in per_rank[rank]]
    ok = ok and worst <= 1e-13 and mine == want["per_rank"][rank]
    ds.iterate(1, 0.0)
    comb = [{f: getattr(r, f) for f in FIELDS} for r in ds.tangle_records()]
    ok = ok and [c["iteration"] for c in comb] == [N + 1]
    transport = "peer stores" if ds.pushbuf is not None else backend
    print(f"rank {rank} overlap {overlap} [{transport}]: {'ok' if ok else 'BAD'} rel_linf {worst:.2e} reverted {[r['nPointsReverted'] for r in mine]}", flush=True)
    bad += 0 if ok else 1
    ds.close()
    del ds
dist.barrier()
dist.destroy_process_group()
sys.exit(1 if bad else 0)
