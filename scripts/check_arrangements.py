"""GPU check that every arrangement of the multi-rank iteration gives the same bits: one rank of eight (2 x 2 x 2 cut of a hex
block: face, edge and corner sharers) with its real halo tables and a self-exchange standing in for the seven peers (RCCL send /
recv groups with the one rank a 1-GPU box offers; SMOOTHMESH_EXCHANGE=push: the peer-store transport onto the rank's own receive
slots) -- the one-kernel-per-step form (SMGPU_HALO_MERGED=0) in order and with an exchange stream, the multi-role launches
(k_geom_halo / k_smooth_halo) in order, and their flagged arrangement (exchanges ordered by flag words next to the launches).
With the self-exchange a shared point is combined with its own record, so the result is no mesh anybody wants -- but it is a fixed
function of the inputs that every arrangement must reproduce bit for bit.  Prints 'arrangements: ok' or exits non-zero.

usage: check_arrangements.py [n [iters [set]]] -- set "knobs" runs, against the same one-kernel-per-step reference, the knobs that
decide where the pack role and the fix role sit inside the two multi-role launches: SMGPU_HALO_FIX_INSIDE, SMGPU_HALO_FIX_AT (hs.nA in
runMergedSmooth, rounded with & ~7: on a rank with fewer than 8 smoothing tiles it is 0 whatever the knob says, and the fix role
runs ahead of every regular tile -- n = 6) and SMGPU_HALO_PACK_AFTER (nI1 in runMergedGeomPack: 0, every interior tile ahead of
the pack role, and 8 tiles).

Why no value of these knobs can make a launch wait for itself (kernels_tiled.hpp; workgroups are dispatched in index order, so a
workgroup that waits only for lower indices, or for work of an earlier launch, waits for something that is running or done):
 * k_geom_halo is [geometry tiles with a shared point] [nI1 interior tiles] [pack role] [the other interior tiles].  Only the pack
   role waits (roleWait), and only for the first role, which sits at index 0 whatever nI1 is: SMGPU_HALO_PACK_AFTER moves tiles
   between the second and the fourth role, which wait for nobody.  Every role's size is rounded up to a multiple of 8
   (tileGrid), so each starts at a multiple of 8 as roleDone's per-XCD counts need.
 * k_smooth_halo is [multi-sharer combine] [shared points' tiles] [hs.nA regular tiles] [fix role] [the other regular tiles].
   The first two roles wait for exchange A, which the pack role of the EARLIER launch released (peer stores: its flag; flagged:
   the relay on the exchange stream behind the host's exchange, which waits for nothing but that pack role); the shared points'
   tiles also wait for the first role.  The fix role waits for the shared points' tiles -- lower indices for every hs.nA >= 0 --
   and for exchange F, which those same tiles release when the last of them signals (peer stores: the flag word; flagged: the
   relay behind the host's exchange F, which waits for that signal alone).  The regular tiles wait for nobody, so workgroups
   that spin never keep the exchange stream's kernels from a slot for longer than a tile takes.
 * SMGPU_HALO_FIX_INSIDE=0 takes the fix role out: k_shared_fix is a launch of its own behind k_smooth_halo and carries the wait
   for exchange F, released by a launch that has been enqueued before it.
Every wait is bounded besides (roleWait: 2 s; pushWait and the relays: SMGPU_PUSH_TIMEOUT_S) and ends with the engine's error
word, which stops this script at the case that raised it."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch, torch.distributed as dist
for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29589")):
    os.environ.setdefault(k, v)
torch.cuda.set_device(0)
dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
from smoothmesh_amd import default_params
from smoothmesh_amd import halo
from smoothmesh_amd.meshgen import hex_subdomain
n = int(sys.argv[1]) if len(sys.argv) > 1 else 26
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 14
case_set = sys.argv[3] if len(sys.argv) > 3 else "default"
assert case_set in ("default", "knobs"), case_set
KNOBS = ("SMGPU_HALO_FIX_INSIDE", "SMGPU_HALO_FIX_AT", "SMGPU_HALO_PACK_AFTER")
grid = (2, 2, 2)
subs = [hex_subdomain((n, n, n), grid, r, jitter=0.25, seed=77) for r in range(8)]
cands = [s.processor_patch_point_lists() for s in subs]
sub = subs[0]
sub.nRanks = 1
dist.all_gather_object = lambda out, obj: out.__setitem__(slice(None), [cands[0]])
t = halo.HaloTables(0, sub.pointProcAddressing, cands)
halo.HaloTables = lambda rank, ppa, c: t
push = os.environ.get("SMOOTHMESH_EXCHANGE", "") == "push"
REFERENCE = ("one kernel per step, in order", {"SMGPU_HALO_MERGED": "0"}, False)
cases = [REFERENCE, ("multi-role launches, in order", {}, False)]
if not push:
    cases += [("one kernel per step, exchange stream", {"SMGPU_HALO_MERGED": "0"}, True),
              ("exchange stream without the flag words (SMGPU_HALO_FLAGGED=0: back to one kernel per step)", {"SMGPU_HALO_FLAGGED": "0"}, True),
              ("multi-role launches, flagged", {}, True)]


def knob_cases(tiles):
    """the arrangement knobs, each case named after the path it must take: "multi-role" always; "flagged" with an exchange stream;
    "fix inside" where k_shared_fix's work is a role of k_smooth_halo.  PACK_AFTER just above the first role's size: nI1 = 8"""
    above = (tiles["geom_shared"] + 7) // 8 * 8 + 8
    out = []
    if push:
        for at in (0, 50, 100):
            out.append((f"multi-role launches, peer stores, fix inside at {at} %", {"SMGPU_HALO_FIX_INSIDE": "1", "SMGPU_HALO_FIX_AT": str(at)}, False))
        out.append(("multi-role launches, peer stores, k_shared_fix behind the launch", {"SMGPU_HALO_FIX_INSIDE": "0"}, False))
        for after in (0, 2 ** 30, above):
            out.append((f"multi-role launches, peer stores, fix inside, pack after {after}", {"SMGPU_HALO_PACK_AFTER": str(after)}, False))
        return out
    for at in (0, 50, 100):
        out.append((f"multi-role launches, flagged, fix inside at {at} %", {"SMGPU_HALO_FIX_INSIDE": "1", "SMGPU_HALO_FIX_AT": str(at)}, True))
    out.append(("multi-role launches, flagged, fix inside", {"SMGPU_HALO_FIX_INSIDE": "1"}, True))
    for after in (0, 2 ** 30, above):
        out.append((f"multi-role launches, in order, pack after {after}", {"SMGPU_HALO_PACK_AFTER": str(after)}, False))
        out.append((f"multi-role launches, flagged, pack after {after}", {"SMGPU_HALO_PACK_AFTER": str(after)}, True))
    return out


if case_set == "knobs":
    cases = [REFERENCE]
ref = None
bad = 0
while cases:
    name, env, overlap = cases.pop(0)
    for k in ("SMGPU_HALO_MERGED", "SMGPU_HALO_FLAGGED") + KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    ds = halo.DistributedSmoother(sub, device=0, probe_slots=t.nSend, overlap=overlap)
    ds.set_params(default_params(ds.global_min_edge(), edgeAngleConstraint=False, faceAngleConstraint=False))
    done, res, frz = ds.iterate(iters, 0.0)
    pts = ds.get_points()
    hm = ds.engine.debug_halo_mode()
    want = {"multi_role": "multi-role" in name, "flagged": "flagged" in name}
    if case_set == "knobs":
        want["fix_inside"] = "fix inside" in name
    if any(hm[k] != v for k, v in want.items()):
        print(f"{name}: the engine took another path: {hm}")
        bad += 1
    if case_set == "knobs" and ref is None:
        tiles = ds.engine.debug_halo_tiles()
        print(f"tiles: {tiles}" + (" -- fewer than 8 smoothing tiles: the fix role runs ahead of every regular tile (hs.nA = 0)" if tiles["smooth_tiles"] < 8 else ""))
        cases += knob_cases(tiles)
    ds.close()
    got = (done, res.copy(), frz.copy(), pts.copy())
    if ref is None:
        ref = got
        print(f"{name}: reference ({t.nSend} send slots, {len(t.sharedLocal)} shared points, nFrozenPoints {frz[:4].tolist()} ..., residual {res[-1]:.6g})")
        continue
    same = got[0] == ref[0] and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    print(f"{name}: {'same bits' if same else 'DIFFERENT: max |dx| = %.3e' % float(np.max(np.abs(got[3] - ref[3])))}")
    bad += 0 if same else 1
dist.destroy_process_group()
if bad:
    sys.exit(1)
print("arrangements: ok")
