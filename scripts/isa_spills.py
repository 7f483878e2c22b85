"""Developer tool, sibling of isa_regions.py: where the pipelined search kernel's SGPR spills are stored and reloaded, what each
spilled value is, and which reload sites lie on the laid-out path of a tile job.
  hipcc <the Makefile's flags for astar_tile.hip> -S --cuda-device-only astar_tile.hip -o /tmp/astar_tile.s -I../../include
  python scripts/isa_spills.py /tmp/astar_tile.s [kernel symbol] [astar_tile.hip]

A spilled SGPR lives in one lane of a spill VGPR (v_writelane_b32 vN, sK, lane / v_readlane_b32 sK, vN, lane).  The assembly carries
no comment for these, so a slot is named by the instruction that produced the value stored into it (looked up backwards from the
store, through scalar copies): a scalar load names its base and offset -- `kernarg+0x58` is a field of TsaLaunch -- anything else is
quoted as it stands.
A site is counted per `; TSA_MARK` region and as
  path   on the path the block placement laid out for the region: from its mark along fall-throughs and unconditional branches to
         the next mark -- what a job executes when every conditional branch goes the way the compiler expected,
  side   in any other block of the region (a block belongs to the region of the mark a wavefront passed last), which a job enters
         by a TAKEN conditional branch: the bodies of TSA_UNLIKELY branches, a row's scan -- and whatever else the placement put
         out of line, likely or not (the odd rows' stores of the results phase are such blocks).
Blocks that are reached from the end of the job before the next job_begin (finish, the queue, the bucket loop, the backtrace, and
the way out of a turn that found nothing) are `outside`.  The counts are static: sites, not executions."""
import collections
import hashlib
import re
import sys

path = sys.argv[1]
kern = sys.argv[2] if len(sys.argv) > 2 else "_ZN3rna17tsa_search_kernelILi8ELb0EEEvNS_9TsaLaunchE"
L = open(path).read().split("\n")
start = [i for i, l in enumerate(L) if l.startswith(kern + ":")][0]
end = next(i for i in range(start, len(L)) if L[i].strip().startswith("s_endpgm"))
K = [l.strip() for l in L[start:end + 1]]

if len(sys.argv) > 3:
    print("kernel_source_sha %s" % hashlib.sha256(open(sys.argv[3], "rb").read()).hexdigest()[:12])   # as bench.py quotes it
meta = "\n".join(L)
m = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % re.escape(kern), meta, re.S)
if m:
    f = dict(re.findall(r"\.(\w+):\s+(\d+)", m[1]))
    print("%s: vgpr_count %s sgpr_spill_count %s vgpr_spill_count %s private_segment_fixed_size %s" % (
        kern, f.get("vgpr_count"), f.get("sgpr_spill_count"), f.get("vgpr_spill_count"), f.get("private_segment_fixed_size")))

# ---- the spill VGPRs: registers that take v_writelane from an SGPR with a literal lane outside inline assembly ----
WR = re.compile(r"v_writelane_b32 (v\d+), (s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi), (\d+)$")
RD = re.compile(r"v_readlane_b32 (s\d+|vcc_lo|vcc_hi), (v\d+), (\d+)$")
in_asm, wcount = False, collections.Counter()
for t in K:
    if t.startswith(";;#ASMSTART"):
        in_asm = True
    elif t.startswith(";;#ASMEND"):
        in_asm = False
    elif not in_asm:
        m = WR.match(t)
        if m:
            wcount[m[1]] += 1
spill_regs = {r for r, n in wcount.items() if n >= 8}   # (the job's own v_writelane, lanes 0 / 63 of a row, are inline assembly)

# ---- basic blocks, regions ----
marks = [(i, t[11:].strip()) for i, t in enumerate(K) if t.startswith("; TSA_MARK")]
names = [n for _, n in marks]
job0, job1 = marks[0][0], marks[-1][0]
is_label = lambda t: re.match(r"(\.LBB\d+_\d+):", t)
is_instr = lambda t: t and t[0] not in ";." and not is_label(t) and not t.endswith(":")
bstart = sorted({0} | {i for i, t in enumerate(K) if is_label(t)} | {i for i, _ in marks})
bidx = {}
for k, s in enumerate(bstart):
    for i in range(s, bstart[k + 1] if k + 1 < len(bstart) else len(K)):
        bidx[i] = k
label_block = {is_label(K[s])[1]: k for k, s in enumerate(bstart) if is_label(K[s])}
succ = collections.defaultdict(set)
for k, s in enumerate(bstart):
    e = bstart[k + 1] if k + 1 < len(bstart) else len(K)
    ins = [t for t in K[s:e] if is_instr(t)]
    for t in ins:
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", t)
        if m and m[1] in label_block:
            succ[k].add(label_block[m[1]])
    last = ins[-1].split()[0] if ins else ""
    if last not in ("s_branch", "s_endpgm", "s_setpc_b64") and k + 1 < len(bstart):
        succ[k].add(k + 1)


mark_block = {bidx[i]: n for i, n in marks}
# a block belongs to the region of the mark a wavefront passed last on its way there; what is reached from job_end before the next
# job_begin is outside the job (the no-op turn's way out of the halo step included: it is the way every turn ends)
region_of, outside = {}, set()
todo = list(succ[bidx[job1]])
while todo:
    k = todo.pop()
    if k in outside or k in mark_block:
        continue
    outside.add(k)
    todo.extend(succ[k])
for i, n in marks[:-1]:
    todo = [bidx[i]]
    while todo:
        k = todo.pop()
        if k in region_of or k in outside or (k in mark_block and k != bidx[i]):
            continue
        region_of[k] = [n, "side"]
        todo.extend(succ[k])
    # the path the block placement laid out: from the mark along fall-throughs and unconditional branches to the next mark
    k, seen = bidx[i], set()
    while k is not None and k not in seen and region_of.get(k, [None])[0] == n:
        seen.add(k)
        region_of[k][1] = "path"
        s_, e_ = bstart[k], bstart[k + 1] if k + 1 < len(bstart) else len(K)
        ins = [t for t in K[s_:e_] if is_instr(t)]
        if ins and ins[-1].split()[0] == "s_branch":
            k = label_block.get(ins[-1].split()[1])
        elif ins and ins[-1].split()[0] in ("s_endpgm", "s_setpc_b64"):
            k = None
        else:
            k = k + 1
region_of = {k: tuple(v) for k, v in region_of.items()}


# ---- what a slot holds: the producer of the SGPR stored into it ----
def producer(i, reg, depth=0):
    n = int(reg[1:]) if reg[0] == "s" and reg[1:].isdigit() else None
    for j in range(i - 1, max(i - 400, -1), -1):
        t = K[j]
        if not is_instr(t):
            continue
        ops = t.replace(",", " ").split()
        if len(ops) < 2:
            continue
        d = ops[1]
        hit = d == reg
        m = re.match(r"s\[(\d+):(\d+)\]", d)
        if m and n is not None and int(m[1]) <= n <= int(m[2]):
            hit = True
        if not hit or ops[0].startswith(("s_cmp", "s_cbranch", "s_bitcmp", "v_writelane", "s_waitcnt")):
            continue
        if ops[0] in ("s_mov_b32", "s_mov_b64") and re.match(r"s(\d+|\[)", ops[2]) and depth < 3:
            src = ops[2]
            if m and src.startswith("s["):
                src = "s%d" % (int(re.match(r"s\[(\d+)", src)[1]) + n - int(m[1]))
            return producer(j, src, depth + 1)
        if ops[0].startswith("s_load") or ops[0].startswith("s_buffer_load"):
            off = ops[3] if len(ops) > 3 else "0"
            base = "kernarg" if ops[2] in ("s[0:1]", "s[4:5]", "s[2:3]") and j < job0 else ops[2]
            word = (n - int(m[1])) if m and n is not None else 0
            try:
                return "%s+0x%x (%s)" % (base, int(off, 0) + 4 * word, ops[0])
            except ValueError:
                return t
        if ops[0].startswith("v_readlane") and ops[2] in spill_regs:
            return "copy of slot %s[%s]" % (ops[2], ops[3])
        return t
    return "?"


slots = collections.defaultdict(lambda: {"w": [], "r": []})
in_asm = False
for i, t in enumerate(K):
    if t.startswith(";;#ASMSTART"):
        in_asm = True
    elif t.startswith(";;#ASMEND"):
        in_asm = False
    if in_asm:
        continue
    m = WR.match(t)
    if m and m[1] in spill_regs:
        slots[(m[1], int(m[3]))]["w"].append(i)
    m = RD.match(t)
    if m and m[2] in spill_regs:
        slots[(m[2], int(m[3]))]["r"].append(i)


def where(i):
    k = bidx[i]
    if k in region_of:
        return region_of[k]
    return ("outside", "")


print("spill VGPRs: %s; %d slots, %d store sites, %d reload sites" % (
    " ".join(sorted(spill_regs)), len(slots), sum(len(s["w"]) for s in slots.values()), sum(len(s["r"]) for s in slots.values())))
tot = collections.Counter()
for s in slots.values():
    for kind in "wr":
        for i in s[kind]:
            tot[(where(i), kind)] += 1
print("\n%-16s %10s %10s %10s %10s" % ("region", "reload/path", "reload/side", "store/path", "store/side"))
for n in names[:-1] + ["outside"]:
    if n == "outside":
        print("%-16s %10d %10s %10d" % (n, tot[(("outside", ""), "r")], "", tot[(("outside", ""), "w")]))
    else:
        print("%-16s %10d %10d %10d %10d" % (n, tot[((n, "path"), "r")], tot[((n, "side"), "r")], tot[((n, "path"), "w")], tot[((n, "side"), "w")]))
print("job, path: %d reloads %d stores; job, side: %d reloads %d stores" % (
    sum(v for (w, k), v in tot.items() if w[1] == "path" and k == "r"), sum(v for (w, k), v in tot.items() if w[1] == "path" and k == "w"),
    sum(v for (w, k), v in tot.items() if w[1] == "side" and k == "r"), sum(v for (w, k), v in tot.items() if w[1] == "side" and k == "w")))

# outside the job, by the loop the block stands in (the compiler's "Depth=" comment on the block label): 1 = once per bucket, 2 = once
# per job TAKEN (the turn that pops a tile: a sticky turn does not pass here), 3 = the job loop's own blocks outside the marks
depth_of, d = {}, 0
for i, t in enumerate(K):
    m = is_label(t)
    if m:
        dm = re.search(r"Depth=(\d+)", t)
        d = int(dm[1]) if dm else 0
    depth_of[i] = d
od = collections.Counter()
for s in slots.values():
    for kind in "wr":
        for i in s[kind]:
            if where(i)[0] == "outside":
                od[(depth_of[i], kind)] += 1
sc = collections.Counter((depth_of[i], "load" if "scratch_load" in t else "store") for i, t in enumerate(K) if t.startswith("scratch_"))
print("outside the job by loop depth (0 = straight-line kernel code): " + "; ".join(
    "depth %d: %d reloads %d stores, scratch %d loads %d stores" % (k, od[(k, "r")], od[(k, "w")], sc[(k, "load")], sc[(k, "store")]) for k in range(4)))
print("\nslots reloaded inside the job (reload sites per region as path+side), and what they hold:")
for key in sorted(slots, key=lambda k: (k[0], k[1])):
    s = slots[key]
    c = collections.Counter(where(i) for i in s["r"])
    if not any(w[0] != "outside" for w in c):
        continue
    per = " ".join("%s:%d+%d" % (n, c[(n, "path")], c[(n, "side")]) for n in names[:-1] if c[(n, "path")] + c[(n, "side")])
    held = sorted({producer(i, WR.match(K[i])[2]) for i in s["w"]})
    print("  %s[%2d] %-70s <- %s" % (key[0], key[1], per, " | ".join(held[:3]) + (" | ..." if len(held) > 3 else "")))
