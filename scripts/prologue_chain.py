#!/usr/bin/env python3
"""The memory chain of the tile kernels' prologues, from the compiler's gfx950 assembly (no GPU needed).

    scripts/prologue_chain.py [--asm FILE] [--all] [kernel-name-substring ...]

Compiles csrc/smgpu.hip with the build's own flags to assembly (device side only, into a scratch directory; --asm FILE reads
an assembly file built that way instead) and prints, for every instantiation of the tile kernels (k_geom_tile, k_geom_tile_bnd,
k_smooth_tile, k_pack_tile, k_geom_halo, k_smooth_halo; --all: the instantiations of every tile width, not only 256), the scalar
loads, vector loads and waits a workgroup passes between kernel entry and the staging barrier on the main path, with the
kernel's registers, scratch and code size.  Only loads, s_waitcnt and s_barrier are read.

The staging barrier: the s_barrier behind which most of the kernel lies (the barrier block that dominates the most code) --
barriers of optional work in front of the tile (the deferred finish of the previous iteration) and those of the later phases
dominate less.
The main path: among the loop-free paths from the entry to that barrier which pass no other barrier, the one with the highest
score (vector loads issued) - 3 x (waits on vmcnt), the shorter one on a tie: the batched prologue of a tile within the fixed
staging rounds issues many loads per wait, while the fall-back paths (staging loops, set by set) wait behind nearly every load
and a path that skips an optional load issues fewer.  The labels of the path's blocks are printed, to check the choice
against the assembly.

Per kernel, after the sequence: how many waits on lgkmcnt(0) lie in front of the first vector load (each is one scalar round
trip the workgroup sits through, as far as a load was issued since the wait before), and the vmcnt waits between the first and
the last vector load of the prologue (round 1 -> round 2).
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "smoothmesh_amd", "csrc", "smgpu.hip")
KERNELS = ("k_geom_tile<", "k_geom_tile_bnd<", "k_smooth_tile<", "k_pack_tile<", "k_geom_halo<", "k_smooth_halo<")


def flags():
    mk = open(os.path.join(ROOT, "smoothmesh_amd", "csrc", "Makefile")).read()
    m = re.search(r"^HIPFLAGS\s*[:?]?=\s*(.*)$", mk, re.M)
    fl = m.group(1).split() if m else ["-O3", "-std=c++17", "-ffp-contract=off"]
    fl = [f.replace("$(ARCH)", "gfx950") for f in fl if not f.startswith(("-shared", "-o", "-fPIC"))]
    if not any(f.startswith("--offload-arch=") for f in fl):
        fl.append("--offload-arch=gfx950")
    return fl


def build_asm():
    out = os.path.join(tempfile.mkdtemp(prefix="prologue_chain_"), "smgpu.s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc] + flags() + ["--cuda-device-only", "-S", SRC, "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr[-2000:])
    return out


def functions(path):
    """mangled name -> (instruction lines, info dict of the 'Kernel info' comments)"""
    funcs = collections.OrderedDict()
    cur = info = None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            funcs[cur] = ([], {})
            info = None
            continue
        if line.startswith(".Lfunc_end") and cur:
            info = funcs[cur][1]
            cur = None
            continue
        if cur is not None:
            funcs[cur][0].append(line.rstrip("\n"))
        elif info is not None:
            m = re.match(r"^; (codeLenInByte|TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy)\s*[:=]\s*(\d+)", line)
            if m:
                info[m.group(1)] = int(m.group(2))
            elif line.startswith("\t.section\t.text"):
                info = None
    return funcs


class Block:
    def __init__(self, label):
        self.label, self.ins, self.succ = label, [], []


def cfg(lines):
    """basic blocks in layout order; a block ends at a label or behind a branch"""
    blocks = [Block("entry")]
    for line in lines:
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            blocks.append(Block(m.group(1)))
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):
            continue
        blocks[-1].ins.append(t)
        if t.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc")):
            blocks.append(Block(None))
    index = {b.label: i for i, b in enumerate(blocks) if b.label}
    for i, b in enumerate(blocks):
        last = b.ins[-1] if b.ins else ""
        op = last.split()[0] if last else ""
        nxt = [i + 1] if i + 1 < len(blocks) else []
        if op == "s_branch":
            b.succ = [index[last.split()[-1]]]
        elif op in ("s_endpgm", "s_setpc_b64"):
            b.succ = []
        elif op.startswith("s_cbranch"):
            b.succ = nxt + [index[last.split()[-1]]]
        else:
            b.succ = nxt
    return blocks


def dominators(blocks):
    n = len(blocks)
    pred = [[] for _ in range(n)]
    for i, b in enumerate(blocks):
        for s in b.succ:
            pred[s].append(i)
    # reachable blocks in reverse post-order
    seen, order, stack = {0}, [], [(0, iter(blocks[0].succ))]
    while stack:
        v, it = stack[-1]
        for s in it:
            if s not in seen:
                seen.add(s)
                stack.append((s, iter(blocks[s].succ)))
                break
        else:
            order.append(v)
            stack.pop()
    rpo = order[::-1]
    num = {v: k for k, v in enumerate(rpo)}
    idom = {0: 0}

    def meet(a, b):
        while a != b:
            while num[a] > num[b]:
                a = idom[a]
            while num[b] > num[a]:
                b = idom[b]
        return a

    changed = True
    while changed:
        changed = False
        for v in rpo[1:]:
            ps = [p for p in pred[v] if p in idom]
            new = ps[0]
            for p in ps[1:]:
                new = meet(new, p)
            if idom.get(v) != new:
                idom[v] = new
                changed = True
    return idom, num


def chain_of(v, idom):
    c = [v]
    while v != 0:
        v = idom[v]
        c.append(v)
    return c[::-1]


def is_vload(op):
    return op.startswith(("global_load", "buffer_load", "flat_load")) and "lds" not in op


def main_path(blocks):
    """(list of instructions from the entry up to and including the staging barrier) or None"""
    idom, num = dominators(blocks)
    weight = collections.Counter()
    for v in idom:
        for a in chain_of(v, idom):
            weight[a] += len(blocks[v].ins)
    barriers = [v for v in idom if any(t.startswith("s_barrier") for t in blocks[v].ins)]
    if not barriers:
        return None
    heavy = max(weight[v] for v in barriers)
    target = min((v for v in barriers if weight[v] == heavy), key=lambda v: num[v])
    # blocks of loops: a backward edge u -> h, h and whatever reaches u without passing h
    pred = collections.defaultdict(list)
    for v in idom:
        for s_ in blocks[v].succ:
            pred[s_].append(v)
    looped = set()
    for u in idom:
        for h in blocks[u].succ:
            if num[h] > num[u]:
                continue
            body, work = {h, u}, [u] if u != h else []
            while work:
                for q in pred[work.pop()]:
                    if q in idom and q not in body:
                        body.add(q)
                        work.append(q)
            looped |= body

    def upto_barrier(b):
        k = next(k for k, t in enumerate(b.ins) if t.startswith("s_barrier"))
        return b.ins[:k + 1]

    # best path by (vector loads - 3 x vmcnt waits, -instructions) over the forward edges (reverse post-order numbers rise along them)
    best = {0: ((0, 0), None)}
    for v in sorted(idom, key=lambda v: num[v]):
        if v not in best or v in looped:
            continue
        ins = upto_barrier(blocks[v]) if v == target else blocks[v].ins
        if v != target and any(t.startswith("s_barrier") for t in ins):
            continue                       # a path through another barrier
        (loads, neg), _ = best[v]
        here = (loads + sum(is_vload(t.split()[0]) for t in ins) - 3 * sum(t.startswith("s_waitcnt") and "vmcnt" in t for t in ins), neg - len(ins))
        if v == target:
            continue
        for s in blocks[v].succ:
            if num[s] <= num[v]:
                continue                   # a backward edge: loops are not part of the prologue's main path
            if s not in best or here > best[s][0]:
                best[s] = (here, v)
    if target not in best:
        return None
    path, v = [], target
    while v is not None:
        path.append(v)
        v = best[v][1]
    out = []
    for v in path[::-1]:
        out += upto_barrier(blocks[v]) if v == target else blocks[v].ins
    return out, [blocks[v].label for v in path[::-1] if blocks[v].label]


def report(short, lines, info):
    blocks = cfg(lines)
    path = main_path(blocks)
    print(f"== {short}")
    print(f"   NumVgprs {info.get('NumVgprs', -1)}  NumAgprs {info.get('NumAgprs', -1)}  TotalNumSgprs {info.get('TotalNumSgprs', -1)}  "
          f"ScratchSize {info.get('ScratchSize', -1)}  Occupancy {info.get('Occupancy', -1)}  codeLenInByte {info.get('codeLenInByte', -1)}")
    if path is None:
        print("   (no staging barrier found)")
        return
    path, labels = path
    print("   path: " + " ".join(labels))
    seq = []
    for t in path:
        op = t.split()[0]
        if op.startswith("s_load") or op.startswith("s_buffer_load"):
            seq.append(("S", t))
        elif is_vload(op):
            seq.append(("V", t))
        elif op == "s_waitcnt":
            seq.append(("W", t))
        elif op.startswith("s_barrier"):
            seq.append(("B", t))
    # runs of the same kind on one line
    k = 0
    while k < len(seq):
        kind = seq[k][0]
        j = k
        while j < len(seq) and seq[j][0] == kind and kind in "SV":
            j += 1
        j = max(j, k + 1)
        if kind == "S":
            parts = []
            for _, t in seq[k:j]:
                a = t.replace(",", " ").split()
                parts.append(f"{a[0][len('s_load_'):]} {a[2]}+{a[3]}")
            print(f"   scalar loads x{j - k}: " + ", ".join(parts))
        elif kind == "V":
            cnt = collections.Counter(t.split()[0][len("global_load_"):] if t.startswith("global_load_") else t.split()[0] for _, t in seq[k:j])
            print(f"   vector loads x{j - k}: " + ", ".join(f"{n} {w}" for w, n in cnt.items()))
        elif kind == "W":
            print(f"   wait  {seq[k][1][len('s_waitcnt '):]}")
        else:
            print("   s_barrier")
        k = j
    first_v = next((i for i, (kd, _) in enumerate(seq) if kd == "V"), len(seq))
    last_v = max((i for i, (kd, _) in enumerate(seq) if kd == "V"), default=-1)
    # a wait counts as a round trip only if a scalar load was issued since the last full wait
    trips, pending = 0, False
    for kd, t in seq[:first_v]:
        if kd == "S":
            pending = True
        elif kd == "W" and "lgkmcnt(0)" in t and pending:
            trips += 1
            pending = False
    mid = [t[len("s_waitcnt "):] for kd, t in seq[first_v:last_v] if kd == "W" and "vmcnt" in t]
    print(f"   -> scalar round trips (lgkmcnt(0) waits with a load outstanding) before the first vector load: {trips}")
    print(f"   -> vmcnt waits between the first and the last vector load: {len(mid)}" + (f" ({', '.join(mid)})" if mid else ""))


def main():
    args = sys.argv[1:]
    asm = None
    if "--asm" in args:
        k = args.index("--asm")
        asm = args[k + 1]
        del args[k:k + 2]
    every = "--all" in args
    args = [a for a in args if a != "--all"]
    asm = asm or build_asm()
    funcs = functions(asm)
    names = subprocess.run(["c++filt"], input="\n".join(funcs), capture_output=True, text=True).stdout.split("\n")
    for mangled, name in zip(funcs, names):
        short = name.split("(")[0].replace("void ", "").replace("smgpu::", "")
        if not short.startswith(KERNELS) or not funcs[mangled][0]:
            continue
        if args and not any(a in short for a in args):
            continue
        if not every and "256" not in short:
            continue
        report(short, *funcs[mangled])


if __name__ == "__main__":
    main()
