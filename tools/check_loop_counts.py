#!/usr/bin/env python
"""Development: per-class instruction counts of one solve kernel's check loop, from the .s of tools/kernel_resources.sh (no GPU).

    python tools/check_loop_counts.py FILE.s [substring of the mangled kernel name] [--blocks] [--quiet] [--path=LABEL,LABEL,...]

The check loop is the loop around the plain-iteration loops (the loops at depth 3 with 8 to 12 v_fma_f64) - the body of
`for (it = 0;;)` in pdlp_solve_kernel - counted WITHOUT those loops; the loops are the ones the compiler's comments name.  Classes:
FP64 VALU (v_*_f64, conversions to and from f64 included), spill lanes (v_readlane_b32 / v_writelane_b32 of a VGPR that
v_writelane_b32 writes: the SGPR spills), other lane reads (the reductions' v_readlane_b32), v_mov_b32 (the DPP moves of the
reductions included), v_mov_b64, other VALU, scratch, LDS (ds_*), SALU, other.
--blocks lists every basic block of the loop with its counts and where it ends; --quiet adds the counts of the straight-line path
of a check on which no event fires (the cheapest way from the residual to the Halpern step and the loop's header); --path=L1,L2,...
sums the blocks named.
"""
import re
import sys

CLASSES = ("fp64", "spill_lane", "lane", "v_mov", "v_mov64", "valu", "scratch", "lds", "salu", "other")
SPILL_VGPRS = set()          # VGPRs that hold spilled SGPRs: the destinations of v_writelane_b32


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_readlane") or op.startswith("v_writelane"):
        return "spill_lane" if set(re.findall(r"\bv\d+\b", ins)) & SPILL_VGPRS else "lane"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("v_mov_b32"):
        return "v_mov"
    if op.startswith("v_mov_b64"):
        return "v_mov64"
    if op.startswith("v_"):
        return "fp64" if "f64" in op else "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


def function_body(text, key):
    names = [m.group(1) for m in re.finditer(r"^(_Z\w*pdlp_solve_kernel\w*):", text, re.M)]
    name = next(n for n in names if key in n)
    i = text.index("\n" + name + ":")
    return name, text[i:text.index(".Lfunc_end", i)].split("\n")[2:]


def blocks_of(body):
    """[(label, [instructions], header of the innermost loop the block lies in, or None)] in layout order; a block ends at a label or
    behind a branch.  The loops are the compiler's own: it comments every block with `in Loop: Header=BB0_n` or `This ... Loop Header`."""
    out, cur, label, n, loop, parent = [], [], "entry", 0, None, {}
    lines = iter(range(len(body)))
    for k in lines:
        line = body[k]
        s = line.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s) or re.match(r"^; %bb\.(\d+):", line.strip())
        if m:
            if cur or label != "entry":
                out.append((label, cur, loop))
            if s:
                label, n = m.group(1), 0
            else:
                n += 1
                label = "%s+%d" % (label.split("+")[0], n)
            cur = []
            note, j = line, k + 1                   # the comment may run over the lines that follow
            while j < len(body) and body[j].strip().startswith(";") and not body[j].strip().startswith("; %bb"):
                note += body[j]
                j += 1
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            if h:
                loop = ".L" + h.group(1)
            elif "Loop Header" in note:
                loop = label
                up = re.findall(r"Parent Loop (BB\d+_\d+)", note)
                parent[label] = ".L" + up[-1] if up else None
            else:
                loop = None
            continue
        if not s or s.startswith("."):
            continue
        cur.append(s)
        if s.startswith("s_cbranch") or s.startswith("s_branch") or s.startswith("s_endpgm"):
            out.append((label, cur, loop))            # (a conditional branch may be followed by a plain one without a comment)
            n += 1
            label, cur = "%s+%d" % (label.split("+")[0], n), []
    if cur:
        out.append((label, cur, loop))
    return out, parent


def count(instrs):
    c = dict.fromkeys(CLASSES, 0)
    for s in instrs:
        c[classify(s)] += 1
    return c


def fmt(c):
    return " ".join("%s %4d" % (k, c[k]) for k in CLASSES) + " | all %4d" % sum(c.values())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    key = args[1] if len(args) > 1 else "Li4ELi2ELb0ELj4403ELj68ELb0ELb0E"
    name, body = function_body(open(args[0]).read(), key)
    blocks, parent = blocks_of(body)
    written = [m.group(1) for _, ins, _ in blocks for s in ins if (m := re.match(r"v_writelane_b32 (v\d+),", s))]
    SPILL_VGPRS.update(v for v in written if written.count(v) >= 4)         # (a reduction's scratch register may see a stray one)
    index = {lab: i for i, (lab, _, _) in enumerate(blocks)}
    of = lambda h: [i for i, b in enumerate(blocks) if b[2] == h]
    fma = lambda L: sum("v_fma_f64" in s for i in L for s in blocks[i][1])
    plain = [of(h) for h in parent if 8 <= fma(of(h)) <= 12 and parent[h] and parent.get(parent[h])]
    outer = parent[blocks[plain[0][0]][2]]
    inside = of(outer)
    print(name)
    print("whole kernel        ", fmt(count([s for _, ins, _ in blocks for s in ins])))
    for p in plain:
        print("plain loop %-9s" % blocks[min(p)][0], fmt(count([s for i in sorted(p) for s in blocks[i][1]])))
    print("check loop          ", fmt(count([s for i in inside for s in blocks[i][1]])), "(header %s, %d blocks)" % (outer, len(inside)))
    if "--blocks" in sys.argv:
        for i in inside:
            lab, ins, _ = blocks[i]
            print("  %-14s" % lab, fmt(count(ins)), "->", ins[-1] if ins and "branch" in ins[-1] else "(falls through)")
    if "--quiet" in sys.argv:
        # the cheapest way through a check: from the block of the residual (the PDHG step, the half product and the reduction: LDS
        # gathers and DPP moves in one block) through the restart test (the block that converts k for the artificial criterion and
        # tests r0 against infinity) to the Halpern step of the check iteration (v_rcp_f64 right behind v_cvt_f64_i32) and on to the
        # loop's header, by instruction count over the loop's own blocks - no KKT test, no restart, no ray jump
        succ = {}
        for pos, i in enumerate(inside):
            ins = blocks[i][1]
            last = ins[-1] if ins else ""
            m = re.search(r"s_c?branch\w* (\.LBB\d+_\d+)", last)
            out = [index[m.group(1)]] if m and m.group(1) in index else []
            if not last.startswith("s_branch") and i + 1 < len(blocks):
                out.append(i + 1)
            succ[i] = [j for j in out if j in succ or j in inside]
        has = lambda i, *ops: all(any(s.startswith(op) for s in blocks[i][1]) for op in ops)
        base = next(i for i in inside if has(i, "v_mov_b32_dpp") and sum(s.startswith("ds_") for s in blocks[i][1]) >= 30)
        halpern = next(i for i in inside if any(a.startswith("v_cvt_f64_i32") and b.startswith("v_rcp_f64") for a, b in zip(blocks[i][1], blocks[i][1][1:])))

        def cheapest(a, b):
            import heapq
            dist, prev, heap = {a: len(blocks[a][1])}, {}, [(len(blocks[a][1]), a)]
            while heap:
                d, i = heapq.heappop(heap)
                if i == b:
                    break
                for j in succ.get(i, []):
                    if j in succ and d + len(blocks[j][1]) < dist.get(j, 1 << 30):
                        dist[j], prev[j] = d + len(blocks[j][1]), i
                        heapq.heappush(heap, (dist[j], j))
            way = [b]
            while way[-1] != a:
                way.append(prev[way[-1]])
            return way[::-1]
        tests = next(i for i in inside if has(i, "v_cvt_f64_i32") and any("0x7ff00000" in s for s in blocks[i][1]) and i != halpern)
        way = cheapest(base, tests) + cheapest(tests, halpern)[1:] + cheapest(halpern, index[outer])[1:-1]
        print("quiet check         ", fmt(count([s for i in way for s in blocks[i][1]])), "(%d blocks: %s)" % (len(way), " ".join(blocks[i][0] for i in way if blocks[i][1])))
    for a in sys.argv[1:]:
        if a.startswith("--path="):
            labs = a[7:].split(",")
            print("path of %d blocks    " % len(labs), fmt(count([s for lab in labs for s in blocks[index[lab]][1]])))


if __name__ == "__main__":
    main()
