"""DistributedSmoother with the quality constraint's scaling passes (DESIGN.md "Mesh quality", 10.20) on two ranks, one process each
(RANK, WORLD_SIZE, MASTER_ADDR, MASTER_PORT in the environment, as torch.distributed.run sets them), against its CPU restatement
(tests/quality_constraint_scaled_multi_reference.py): the dented block cut (2, 1, 1) under an internal skewness limit, as
scripts/check_dist_quality_constraint.py, with S = 2, r = 0.75, n = 4, P = 2 -- the marks of the points on the cut become scales on
both ranks, and every sweep moves the partial sums of the shared points as exchange S (set up from both ranks' shared-shared
edges, gathered once).  Per iteration the points (rel_linf <= 1e-13), at the end this rank's scaled records, the combined records
and the state; in order and with an exchange stream.
On a 1-GPU box: SMOOTHMESH_SHARE_GPU=1 SMOOTHMESH_BACKEND=gloo (the engines are the real ones; only the transport is gloo).
Exit code 1 on a mismatch."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch, torch.distributed as dist
from oracle import oracle_ffi
from smoothmesh_amd.halo import DistributedSmoother
from quality_constraint_multi_reference import FACE_MARGIN, MARGIN, OFF
from quality_constraint_scaled_multi_reference import QualityConstraintScaledMultiReference
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
LIM = {**OFF, "maxInternalSkewness": 0.4}
SCALING = dict(scalePasses=2, errorReduction=0.75, nSmoothScale=4)
bad = 0
for overlap in (False, True):
    ref = QualityConstraintScaledMultiReference(oracle_ffi, dented_block(), (2, 1, 1), LIM, 2, "com", False, **SCALING, maxStepLength=1.0, minEdgeLength=1e-4)
    want = ref.run(N)
    assert ref.minMargin > MARGIN and ref.minSkewGap > FACE_MARGIN
    assert ref.uncounted > 0 and any(r["nPointsScaled"] > 0 for r in want["recs"])   # the case is the one its docstring names
    fields = list(want["per_rank"][0][0])
    ds = DistributedSmoother(ref.subs[rank], device=local, overlap=overlap)
    ds.set_params(ref.prm)
    ds.set_quality_constraint(passes=2, **LIM)
    ds.set_quality_constraint_scaling(**SCALING)
    st = ds.quality_constraint_state_scaled()
    ok = st.on and st.nExemptCells == sum(ref.nExemptCells) and st.nExemptFaces == sum(ref.nExemptFaces) and st.scalePasses == 2 and st.nSmoothScale == 4
    worst = 0.0
    for k in range(N):
        n, res, frz = ds.iterate(1, 0.0)
        p, q = ds.get_points(), want["pts"][k][rank]
        worst = max(worst, float(np.max(np.abs(p - q)) / np.max(np.abs(q))))
        ok = ok and n == 1 and int(frz[0]) == int(want["frz"][k])
    per_rank = ds.quality_constraint_records_scaled(per_rank=True)
    mine = [{f: getattr(r, f) for f in fields} for r in per_rank[rank]]
    ok = ok and worst <= 1e-13 and mine == want["per_rank"][rank]
    ds.iterate(1, 0.0)
    comb = ds.quality_constraint_records_scaled()
    ok = ok and [c.iteration for c in comb] == [N + 1]
    print(f"rank {rank} overlap {overlap} [{backend}]: {'ok' if ok else 'BAD'} rel_linf {worst:.2e} scaled {[r['nPointsScaled'] for r in mine]} "
          f"reverted {[r['nPointsReverted'] for r in mine]} minScale {[r['minScale'] for r in mine]}", flush=True)
    bad += 0 if ok else 1
    ds.close()
    del ds
dist.barrier()
dist.destroy_process_group()
sys.exit(1 if bad else 0)
