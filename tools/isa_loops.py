"""Diagnostic: per-loop instruction counts of a kernel in a hipcc -save-temps .s file (the
chain kernels' 16-step block loops).
  python tools/isa_loops.py FILE.s KERNEL_SYMBOL [N]        the N largest loops by category
  python tools/isa_loops.py edge FILE.s KERNEL_SYMBOL       the banded chains' whole-block loops:
      per loop, the instructions / issue slots from each `v_readlane_b32 ..., 63` (the end of a
      step's wave reduction) to the next one inside the unrolled block, and on the edge path: from
      the block's last one, round the loop's back edge, to the first one of the next block
      (shortest path through the loop's branches: the path a whole block takes), with the scalar /
      branch, wait, barrier and LDS instructions on it.  The edge's cost in slots is that figure
      less a steady step's."""
import heapq
import re
import sys
from collections import Counter


def cat(op):
    if op.startswith("v_"): return "valu"
    if op.startswith("s_waitcnt"): return "waitcnt"
    if op.startswith("s_nop"): return "nop"
    if op.startswith("s_barrier"): return "barrier"
    if op.startswith(("s_branch", "s_cbranch")): return "branch"
    if op.startswith("s_"): return "salu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("global_", "buffer_", "flat_")): return "vmem"
    return "other"


def function_lines(src, name):
    a = src.index(name + ":")
    b = src.index(".Lfunc_end", a)
    return src[a:b].split("\n")


def parse(lines):
    """the instructions of a function's lines as (op, operands) and, per label, the index of the
    instruction it stands ahead of"""
    ins, labels = [], {}
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        t = l.strip()
        if not l.startswith("\t") or not t or t.startswith((";", ".")):
            continue
        t = t.split(";")[0].strip()
        op, _, rest = t.partition(" ")
        ins.append((op, rest.strip()))
    return ins, labels


def slots(ins_item):
    """issue slots of an instruction: s_nop N stands for N + 1"""
    op, rest = ins_item
    if op == "s_nop":
        return int(rest, 0) + 1
    return 1


def branch_target(ins_item):
    op, rest = ins_item
    return rest.split()[0].rstrip(",") if cat(op) == "branch" else None


def is_red_end(ins_item):
    op, rest = ins_item
    return op == "v_readlane_b32" and rest.replace(" ", "").endswith(",63")


def chain_loops(ins, labels):
    """the innermost loops (head, tail) that hold a straight-line run of at least 16 reduction
    ends, with that run"""
    found = {}
    heads = set(labels.values())
    for i, it in enumerate(ins):
        tgt = branch_target(it)
        if tgt is None or tgt not in labels or labels[tgt] > i:
            continue
        h = labels[tgt]
        run, best = [], []
        for k in range(h, i + 1):
            if k in heads or cat(ins[k][0]) == "branch":
                if len(run) > len(best): best = run
                run = []
            if is_red_end(ins[k]):
                run = run + [k]
        if len(run) > len(best): best = run
        if len(best) >= 16:
            key = tuple(best)
            if key not in found or i - h < found[key][1] - found[key][0]:
                found[key] = (h, i)
    return [(h, t, list(k)) for k, (h, t) in sorted(found.items(), key=lambda kv: kv[1])]


def shortest_path(ins, labels, h, t, src, dst):
    """the instruction indices of the shortest path src -> dst inside the loop [h, t], every
    branch followed both ways (the back edge included), dst excluded"""
    dist, prev = {src: 0}, {}
    pq = [(0, src)]
    while pq:
        d, u = heapq.heappop(pq)
        if d > dist.get(u, 1 << 60): continue
        nxt = []
        op = ins[u][0]
        tgt = branch_target(ins[u])
        if tgt is not None and tgt in labels and h <= labels[tgt] <= t:
            nxt.append(labels[tgt])
        if op != "s_branch" and u + 1 <= t:
            nxt.append(u + 1)
        for v in nxt:
            if d + 1 < dist.get(v, 1 << 60):
                dist[v], prev[v] = d + 1, u
                heapq.heappush(pq, (d + 1, v))
    if dst not in prev: return None
    path, u = [], prev[dst]
    while u != src:
        path.append(u)
        u = prev[u]
    return [src] + path[::-1]


def count(ins, idxs):
    c = Counter(cat(ins[k][0]) for k in idxs)
    return len(idxs), sum(slots(ins[k]) for k in idxs), c


def edge_report(lines):
    """per chain loop: (steps, edge) -- steps the (instructions, slots) from each reduction end to
    the next inside the block, edge (instructions, slots, Counter by category) of the edge path"""
    ins, labels = parse(lines)
    out = []
    for h, t, run in chain_loops(ins, labels):
        steps = [count(ins, range(a, b))[:2] for a, b in zip(run, run[1:])]
        path = shortest_path(ins, labels, h, t, run[-1], run[0])
        out.append((h, t, len(run), steps, count(ins, path) if path else None))
    return out


def main(argv):
    if argv[1:2] == ["edge"]:
        lines = function_lines(open(argv[2]).read(), argv[3])
        for h, t, n, steps, edge in edge_report(lines):
            ss = sorted(s for _, s in steps)
            med = ss[len(ss) // 2]
            print(f"chain loop instr {h}-{t}: {n} reduction ends; slots between them " + " ".join(str(s) for _, s in steps))
            if edge:
                ni, ns, c = edge
                print(f"   steady step (median) {med} slots; edge path {ni} instr / {ns} slots = steady + {ns - med}; on it: "
                      f"scalar+branch {c['salu'] + c['branch']}  waitcnt {c['waitcnt']}  barrier {c['barrier']}  lds {c['lds']}  "
                      f"valu {c['valu']}  nop slots {ns - ni + c['nop']}")
        return
    src = open(argv[1]).read()
    name = argv[2]
    lines = function_lines(src, name)
    labels = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)|^\s+s_branch\s+(\.LBB\d+_\d+)", l)
        if m:
            tgt = m.group(1) or m.group(2)
            if tgt in labels and labels[tgt] < i:
                loops.append((labels[tgt], i))
    for s0, s1 in sorted(loops, key=lambda x: x[1] - x[0], reverse=True)[:int(argv[3]) if len(argv) > 3 else 12]:
        ins = [l.strip().split()[0] for l in lines[s0:s1 + 1] if l.startswith("\t") and not l.strip().startswith((";", "."))]
        c = Counter("salu" if cat(o) == "branch" else cat(o) for o in ins)
        ops = Counter(ins)
        dpp = sum(1 for l in lines[s0:s1 + 1] if "_dpp" in l or "row_bcast" in l or "quad_perm" in l or "row_" in l and l.strip().startswith("v_"))
        print(f"loop lines {s0}-{s1}: {len(ins)} instr  {dict(c)}  dpp={dpp}  top={ops.most_common(8)}")


if __name__ == "__main__":
    main(sys.argv)
