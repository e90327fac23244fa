"""kernel_resources.py LOG [LOG2]: the register / scratch / spill / LDS lines of every kernel in a compiler log made with
    make -C pinn_depthestimation_amd/csrc -B -j16 -Otarget HIPCC="/opt/rocm/bin/hipcc -Rpass-analysis=kernel-resource-usage" \\
         all > LOG 2>&1
(-Otarget keeps each unit's remarks together; without it parallel compiles interleave them and -j1 is needed.  Name
objects instead of `all`, e.g. pinn_fused_w64.o pinn_fused_adj_w64.o, for the units of interest only.)  With one log: one
line per kernel.  With two (the same command in a checkout of the parent commit and in this tree): every kernel of LOG
whose lines differ in LOG2, then the counts — the check that a change to fused_kernel.h, or to how its instances are
built, left the existing instances as the compiler made them before."""
import collections, re, sys

KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]",
        "LDS Size [bytes/block]")


def parse(path):
    out, cur = collections.OrderedDict(), None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(.*?)\s*\[-Rpass", line)   # (newer clang puts file:line:col in front)
        if not m:
            continue
        body = m.group(1)
        f = re.match(r"Function Name: (\S+)", body)
        if f:
            cur = f.group(1); out[cur] = {}
        elif cur:
            k, _, v = body.rpartition(":")
            out[cur][k.strip()] = v.strip()
    return out


def nice(n):
    m = re.search(r"k_fusedILi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)", n)
    return "k_fused<WP=%s,K1=%s,GRAD=%s,LDSACC=%s,ACT=%s,EPI=%s,KRO=%s,DROP=%s>" % m.groups() if m else n


a = parse(sys.argv[1])
if len(sys.argv) == 2:
    print("kernel | " + " | ".join(KEYS))
    for k, r in a.items():
        print(nice(k) + " | " + " | ".join(r.get(x, "?") for x in KEYS))
else:
    b = parse(sys.argv[2])
    same = 0
    for k, r in a.items():
        if b.get(k) == r:
            same += 1
        else:
            print("DIFFERENT" if k in b else "MISSING", nice(k), r, b.get(k))
    print(f"{len(a)} kernels in {sys.argv[1]}, {same} with identical lines in {sys.argv[2]}, {len(a) - same} different or missing; "
          f"{len(b) - len(set(a) & set(b))} kernels only in {sys.argv[2]}")
