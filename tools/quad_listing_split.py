"""Static account of one hh_k_world_quad instance from the compiler's listing (.s of a -save-temps / -S --offload-device-only build with the
product's flags): the simulation wave's tick loop split at its barriers (head -> X, X -> Y, Y -> the loop's last branch, which takes in the cold
blocks the compiler lays out behind the usual path), counted by the classes of profiles/r08_quad_before_x.md; and the loop of the envelope drain on its own.
    python tools/quad_listing_split.py LISTING.s ['_Z15hh_k_world_quadILi1ELi1ELb1ELi8ELb1ELb1EE']"""
import collections
import re
import sys

path = sys.argv[1]
name = sys.argv[2] if len(sys.argv) > 2 else "_Z15hh_k_world_quadILi1ELi1ELb1ELi8ELb1ELb1EE"
body, inside = [], False
for line in open(path):
    if line.startswith(name) and line.split(";")[0].rstrip().endswith(":"):
        inside = True
        continue
    if inside:
        if line.startswith(".Lfunc_end"):
            break
        body.append(line.rstrip("\n"))
ins = []     # (index, text) of instructions; labels kept as ("label", name)
labels = {}
for l in body:
    t = l.split(";")[0].strip()
    if not t:
        continue
    m = re.match(r"^(\.LBB\d+_\d+):", t)
    if m:
        labels[m.group(1)] = len(ins)
        continue
    if t.startswith(".") or t.endswith(":"):
        continue
    ins.append(t)
bar = [i for i, t in enumerate(ins) if t.startswith("s_barrier")]
# the simulation wave's loop: the last backward branch that spans two barriers
loops = []
for i, t in enumerate(ins):
    m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", t)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        a = labels[m.group(1)]
        nb = [b for b in bar if a <= b <= i]
        if len(nb) >= 2:
            loops.append((a, i, nb))
if not loops:
    sys.exit(f"{name}: no loop with two barriers in it (not a two-wave instance, or not in {path})")
# several loops may hold two barriers (the output wave's too): the simulation wave's is the one with more FP64 in it
a, e, nb = max(loops, key=lambda lp: sum("_f64" in t for t in ins[lp[0]:lp[1] + 1]))
X, Y = nb[0], nb[1]


def account(seg):
    c = collections.Counter()
    for t in seg:
        op = t.split()[0]
        c["instructions"] += 1
        c["FP64"] += "_f64" in op
        c["branches"] += op.startswith(("s_cbranch", "s_branch"))
        c["exec-mask regions"] += bool(re.match(r"s_(and|or)_saveexec_b64", op))
        c["s_mov_b32 literal"] += bool(re.match(r"s_mov_b32 s\d+, 0x[0-9a-f]+", t))
        c["scalar mask ops"] += bool(re.match(r"s_(and|or|xor|andn2|orn2|nand|nor|xnor)_b64", op))
        c["v_readlane"] += op.startswith("v_readlane")
        c["v_writelane"] += op.startswith("v_writelane")
        c["v_cmp*"] += op.startswith("v_cmp")
        c["v_cndmask*"] += op.startswith("v_cndmask")
        c["s_nop"] += op == "s_nop"
        c["v_accvgpr_*"] += op.startswith("v_accvgpr")
        c["scratch_*"] += op.startswith("scratch_")
    return c


rows = ["instructions", "FP64", "branches", "exec-mask regions", "s_mov_b32 literal", "scalar mask ops", "v_readlane", "v_writelane", "v_cmp*", "v_cndmask*", "s_nop",
        "v_accvgpr_*", "scratch_*"]
segs = {"head -> X": ins[a:X], "X -> Y": ins[X:Y], "Y -> loop end": ins[Y:e + 1], "whole kernel": ins}
acc = {k: account(v) for k, v in segs.items()}
print(f"{name}: {len(ins)} instructions, loop {a}..{e}, barrier X at {X}, barrier Y at {Y}")
print("| | " + " | ".join(segs) + " |")
for r in rows:
    print(f"| {r} | " + " | ".join(str(acc[k][r]) for k in segs) + " |")
if len(sys.argv) > 3:   # where one opcode prefix occurs from the loop head to barrier Y (index from the head; X and Y marked)
    for i in range(a, Y):
        if ins[i].startswith(sys.argv[3]):
            print(i - a, "head -> X" if i < X else f"X + {i - X}", ins[i])

# the drain of the envelope queue on its own (drain_envelope_queue_t, `#pragma unroll 1`): every basic block the listing's own loop comments place in the
# depth-2 loop that holds the verdict's `ds_or_b32`, its inner loops (the Karney fallback's iterations) included
blocks, cur = [], None      # (label, comment text, instructions)
for l in body:
    t = l.split(";")[0].strip()
    c = l.split(";", 1)[1] if ";" in l else ""
    m = re.match(r"^(\.LBB\d+_\d+):", t) or re.match(r"^\s*%bb\.(\d+):", c.strip())
    if m:
        cur = [m.group(1), c, []]
        blocks.append(cur)
    elif cur is not None:
        if not t:
            cur[1] += c       # continuation lines of the block's loop comment
        elif not t.startswith(".") and not t.endswith(":"):
            cur[2].append(t)
hdr = None
for lab, c, bi in blocks:
    if any(x.startswith("ds_or_b32") for x in bi):
        m = re.search(r"Header=(BB\d+_\d+) Depth=2", c) or re.search(r"Parent Loop (BB\d+_\d+) Depth=2", c)
        if m:
            hdr = m.group(1)
            break
if hdr:
    seg = [x for lab, c, bi in blocks if lab == ".L" + hdr or re.search(hdr + r"\b", c) for x in bi]
    d = account(seg)
    extra = {"v_sqrt/rsq/rcp_f64 + v_div_*": sum(x.split()[0].startswith(("v_sqrt_f64", "v_rsq_f64", "v_rcp_f64", "v_div_")) for x in seg)}
    print(f"drain loop (header {hdr}): " + ", ".join(f"{r} {d[r]}" for r in rows) + "".join(f", {k} {v}" for k, v in extra.items()))
