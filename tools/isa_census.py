"""isa_census.py FILE.s KERNEL_SUBSTRING [--fwd N --rev N]: instruction census of one kernel of a gfx950 assembly file
(hipcc ... -save-temps), per basic block and per sched_barrier-delimited segment, by instruction class.

The tile kernel's source phases are delimited by its `sched_barrier(0)`s (each leaves a `; sched_barrier` comment) and by
the labels of its two layer loops.  Loops are found from the backward branches; a block's dynamic weight per 16-point tile
is the trip count of the innermost layer loop that holds it (--fwd / --rev: L - 1 iterations of the forward / reverse
layer loop, told apart by their MFMA counts: the reverse body holds the GEMM and the weight gradient), 1 for the rest of
the tile loop and 0 outside it.  Spin loops (the gradient lock) hold no MFMA and count once.

Classes: mfma | v_pk_* | v_accvgpr_* | v_mov | v_cndmask | transcendental (v_exp/v_rcp/v_log/v_rsq/v_sqrt/v_sin/v_cos) |
other VALU | ds_* | vector memory (global_/buffer_/flat_/scratch_) | scalar (s_*, with s_waitcnt and s_nop broken out).
Output: one line per (block, segment) with static counts, then the per-tile dynamic totals per class.

Last column, `memrun`: the longest run of LDS or vector-memory instructions that nothing but scalar and non-MFMA vector
instructions separate — the wave issues in order, so during such a run the matrix pipe drains and idles.  A run is cut by
an MFMA and by a label, not by a sched_barrier; it is booked to the segment that holds its last instruction.  The last line
gives the longest run of the segments that hold MFMAs (the GEMM streams and the weight gradient's quantity loop), where a
run that ends in a segment's last MFMA-free stretch (what follows the last MFMA: the next phase's business) is left out."""
import argparse
import collections
import re

CLASSES = ("mfma", "v_pk", "v_accvgpr", "v_mov", "v_cndmask", "trans", "valu_other", "ds", "vmem", "s_waitcnt", "s_nop", "salu")
TRANS = ("v_exp", "v_rcp", "v_log", "v_rsq", "v_sqrt", "v_sin", "v_cos")


def classify(op):
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith("v_pk_"):
        return "v_pk"
    if op.startswith("v_accvgpr"):
        return "v_accvgpr"
    if op.startswith("v_mov"):
        return "v_mov"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith(TRANS):
        return "trans"
    if op.startswith("v_"):
        return "valu_other"
    if op.startswith("ds_"):
        return "ds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_"):
        return "salu"
    return None


def kernel_lines(path, name):
    out, on = [], False
    for line in open(path, errors="replace"):
        if not on:
            if re.match(r"^[A-Za-z_][\w$.]*:", line) and name in line.split(":")[0]:
                on = True
            continue
        out.append(line.rstrip("\n"))
        if line.strip().startswith("s_endpgm"):
            break
    if not out:
        raise SystemExit(f"no kernel matching {name!r} in {path}")
    return out


def parse(lines):
    """-> blocks: list of dict(label, segs: [Counter], ops: Counter of mnemonics, branches: [target labels])"""
    blocks = [dict(label="entry", segs=[collections.Counter()], ops=collections.Counter(), branches=[])]
    run = 0          # LDS / vector-memory instructions since the last MFMA or label
    for line in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            blocks.append(dict(label=m.group(1), segs=[collections.Counter()], ops=collections.Counter(), branches=[]))
            run = 0
            continue
        s = line.strip()
        if s.startswith("; sched_barrier"):
            blocks[-1]["segs"].append(collections.Counter())
            continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        op = s.split()[0]
        c = classify(op)
        if c is None:
            continue
        seg = blocks[-1]["segs"][-1]
        seg[c] += 1
        blocks[-1]["ops"][op] += 1
        if c == "mfma":
            seg["memrun_mfma"] = max(seg["memrun_mfma"], run)     # the runs that an MFMA of this segment ends
            run = 0
        elif c in ("ds", "vmem"):
            run += 1
            seg["memrun"] = max(seg["memrun"], run)
        if op.startswith(("s_cbranch", "s_branch")):
            blocks[-1]["branches"].append(s.split()[1])
    return blocks


def loops(blocks):
    idx = {b["label"]: i for i, b in enumerate(blocks)}
    out = []
    for i, b in enumerate(blocks):
        for t in b["branches"]:
            if t in idx and idx[t] <= i:
                out.append((idx[t], i))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm"); ap.add_argument("kernel")
    ap.add_argument("--fwd", type=int, default=7, help="trips of the forward layer loop per tile (L - 1)")
    ap.add_argument("--rev", type=int, default=7, help="trips of the reverse layer loop per tile (L - 1)")
    ap.add_argument("--ops", action="store_true", help="also print the mnemonic histogram of every weighted block")
    a = ap.parse_args()
    blocks = parse(kernel_lines(a.asm, a.kernel))
    lp = loops(blocks)
    mf = lambda lo, hi: sum(s["mfma"] for b in blocks[lo:hi + 1] for s in b["segs"])
    with_mfma = sorted((l for l in lp if mf(*l) > 0), key=lambda l: l[1] - l[0])
    if not with_mfma:
        raise SystemExit("no loop with MFMAs found")
    tile = with_mfma[-1]                               # the outermost loop that holds MFMAs: the tile loop
    inner = [l for l in with_mfma if l != tile and tile[0] <= l[0] and l[1] <= tile[1]]
    inner.sort(key=lambda l: l[0])
    weight = [0] * len(blocks)
    for i in range(tile[0], tile[1] + 1):
        weight[i] = 1
    names = {}
    if len(inner) >= 2:                                # forward loop comes first in program order
        for (lo, hi), trips, nm in ((inner[0], a.fwd, "fwd-loop"), (inner[-1], a.rev, "rev-loop")):
            for i in range(lo, hi + 1):
                weight[i] = trips; names[i] = nm
    print("block weight segment " + " ".join(CLASSES) + " memrun")
    total = collections.Counter()
    longest = (0, "-")
    for i, b in enumerate(blocks):
        for j, s in enumerate(b["segs"]):
            if not s:
                continue
            where = f"{b['label']} {weight[i]} {names.get(i, 'tile' if weight[i] else 'outside')}#{j}"
            print(where + " " + " ".join(str(s[c]) for c in CLASSES) + f" {s['memrun']}")
            if weight[i] and s["mfma"] >= 2 and s["memrun_mfma"] > longest[0]:
                longest = (s["memrun_mfma"], where)
            for c in CLASSES:
                total[c] += weight[i] * s[c]
        if a.ops and weight[i]:
            print("   ops:", ", ".join(f"{k} {v}" for k, v in sorted(b["ops"].items(), key=lambda kv: -kv[1])))
    print("per tile (dynamic): " + " ".join(f"{c}={total[c]}" for c in CLASSES))
    valu = sum(total[c] for c in ("v_pk", "v_accvgpr", "v_mov", "v_cndmask", "trans", "valu_other"))
    print(f"per tile: MFMA {total['mfma']}, other VALU {valu}, LDS {total['ds']}, vector memory {total['vmem']}, "
          f"non-MFMA vector + LDS + vector memory {valu + total['ds'] + total['vmem']}")
    print(f"longest LDS / vector-memory run in front of an MFMA, segments of the tile loop with MFMAs: {longest[0]} ({longest[1]})")


if __name__ == "__main__":
    main()
