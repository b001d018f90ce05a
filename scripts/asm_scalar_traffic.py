"""Scalar traffic of one sampler kernel instantiation per marked action, from a
-DFITOCT_ASM_MARKS listing (sibling of asm_actions.py: same attribution, code belongs to the
most recent mark in text order).

    python scripts/asm_scalar_traffic.py [family [template arguments [existing listing]]]

Default: the headline instantiation, family 2, "double, 8, 15, 1, 0, 2, true, true, false".
Without a third argument the kernel is compiled alone (seconds): a temporary translation
unit repeats nuts_device.hip's includes and pragmas and instantiates that one kernel.

Per action it prints
  (a) the SGPR spill slots (spill VGPR, lane) it reloads (v_readlane) and writes
      (v_writelane), with counts;
  (b) its v_readfirstlane count, by source register;
  (c) plain v_mov_b32 whose source is an SGPR, an inline constant or a literal (the LDS
      base and sub-bases arrive this way), by source;
  (d) its s_load groups (runs of s_load with no other scalar-memory wait between them)
      with the number of loads, and whether an "s_waitcnt lgkmcnt(0)" follows before the
      next group.
A spill VGPR is one that v_writelane targets from an SGPR at least four times."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fitoct_amd", "csrc")

fam = sys.argv[1] if len(sys.argv) > 1 else "2"
targs = sys.argv[2] if len(sys.argv) > 2 else "double, 8, 15, 1, 0, 2, true, true, false"
listing = sys.argv[3] if len(sys.argv) > 3 else None


def compile_one():
    """nuts_device.hip's include block (first #include to the last layer header) plus one
    explicit instantiation, compiled device-only to a listing."""
    src = open(os.path.join(CSRC, "nuts_device.hip")).read().split("\n")
    first = next(i for i, l in enumerate(src) if l.startswith("#include"))
    last = max(i for i, l in enumerate(src) if l.startswith('#include "'))
    tmp = tempfile.mkdtemp(prefix="fitoct_asm_")
    unit, out = os.path.join(tmp, "one.hip"), os.path.join(tmp, "one.s")
    with open(unit, "w") as f:
        f.write("\n".join(src[first:last + 1]))
        f.write(f"\ntemplate __global__ void nuts_kernel<{targs}>(const KParams*, const int*);\n"
                "}  // namespace fitoct\n")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-DFITOCT_FAMILY={fam}",
                    "-DFITOCT_ASM_MARKS", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", "-S",
                    "--cuda-device-only", unit, "-o", out], check=True)
    return out


L = open(listing or compile_one()).read().split("\n")
st = next(i for i, l in enumerate(L) if l.startswith("_ZN6fitoct11nuts_kernel"))
en = next(i for i in range(st, len(L)) if L[i].startswith(".Lfunc_end"))
body = [l.strip() for l in L[st:en]]


def operands(s):
    return [o.strip() for o in s.split(None, 1)[1].split(",")] if " " in s else []


writes = collections.Counter()
for s in body:
    if s.startswith("v_writelane_b32"):
        o = operands(s)
        if o[1].startswith("s"):
            writes[o[0]] += 1
SPILL = {v for v, n in writes.items() if n >= 4}

A = collections.defaultdict(lambda: {"rd": collections.Counter(), "wr": collections.Counter(),
                                     "rfl": collections.Counter(), "mov": collections.Counter(),
                                     "groups": [], "valu": 0, "salu": 0, "smem": 0})
cur, group = "entry", None   # group: [action, loads, waited]


def close(waited):
    global group
    if group:
        A[group[0]]["groups"].append((group[1], waited))
    group = None


for s in body:
    if ";MARK" in s:
        cur = s.split("MARK")[1].strip()
        continue
    if not s or s.startswith((";", ".")) or s.endswith(":"):
        continue
    op, o, a = s.split()[0], operands(s), A[cur]
    a["valu"] += op.startswith("v_")
    a["salu"] += op.startswith("s_") and not op.startswith(("s_load", "s_buffer_load"))
    if op.startswith(("s_load", "s_buffer_load")):
        a["smem"] += 1
        if group is None:
            group = [cur, 0, False]
        group[1] += 1
    elif op == "s_waitcnt" and "lgkmcnt(0)" in s:
        close(True)
    elif op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_endpgm")):
        close(False)   # a group ends at the block's end
    elif op == "v_readlane_b32" and o[1] in SPILL:
        a["rd"][f"{o[1]}[{o[2]}]"] += 1
    elif op == "v_writelane_b32" and o[0] in SPILL:
        a["wr"][f"{o[0]}[{o[2]}]"] += 1
    elif op == "v_readfirstlane_b32":
        a["rfl"][o[1]] += 1
    elif op == "v_mov_b32_e32" and not o[1].startswith(("v", "a")):
        kind = "sgpr" if re.match(r"s\d+|s\[|vcc|exec|m0", o[1]) else "const"
        a["mov"][f"{kind} {o[1]}"] += 1
close(False)


def fmt(c, n=12):
    items = sorted(c.items(), key=lambda kv: (-kv[1], kv[0]))
    tail = f" … +{len(items) - n} more" if len(items) > n else ""
    return ", ".join(f"{k}x{v}" if v > 1 else k for k, v in items[:n]) + tail


print(f"# nuts_kernel<{targs}>, family {fam}; spill VGPRs: {', '.join(sorted(SPILL)) or 'none'} "
      f"({sum(writes[v] for v in SPILL)} slot writes in the kernel)")
print(f"{'action':22s} {'valu':>5s} {'salu':>5s} {'smem':>4s} | {'reload':>6s} {'slots':>5s} {'spill':>5s} "
      f"{'rfl':>4s} {'movS':>4s} {'movC':>4s} | s_load groups (loads/waited)")
tot = collections.Counter()
for k, a in sorted(A.items(), key=lambda kv: -(sum(kv[1]["rd"].values()) + sum(kv[1]["wr"].values())
                                                  + sum(kv[1]["mov"].values()) + sum(kv[1]["rfl"].values()))):
    ms = sum(v for m, v in a["mov"].items() if m.startswith("sgpr"))
    mc = sum(a["mov"].values()) - ms
    row = dict(valu=a["valu"], salu=a["salu"], smem=a["smem"], reload=sum(a["rd"].values()),
               slots=len(a["rd"]), spill=sum(a["wr"].values()), rfl=sum(a["rfl"].values()), movS=ms, movC=mc)
    tot.update(row)
    g = " ".join(f"{n}{'w' if w else '-'}" for n, w in a["groups"])
    print(f"{k:22s} {row['valu']:5d} {row['salu']:5d} {row['smem']:4d} | {row['reload']:6d} {row['slots']:5d} "
          f"{row['spill']:5d} {row['rfl']:4d} {row['movS']:4d} {row['movC']:4d} | {g}")
print(f"{'TOTAL':22s} {tot['valu']:5d} {tot['salu']:5d} {tot['smem']:4d} | {tot['reload']:6d} {'':5s} "
      f"{tot['spill']:5d} {tot['rfl']:4d} {tot['movS']:4d} {tot['movC']:4d} |")
print("\n# per action: (a) slots reloaded / written, (b) v_readfirstlane sources, (c) v_mov_b32 sources")
for k, a in A.items():
    if not (a["rd"] or a["wr"] or a["rfl"] or a["mov"]):
        continue
    print(f"## {k}")
    if a["rd"]:
        print("  reload:", fmt(a["rd"], 40))
    if a["wr"]:
        print("  spill :", fmt(a["wr"], 40))
    if a["rfl"]:
        print("  rfl   :", fmt(a["rfl"]))
    if a["mov"]:
        print("  mov   :", fmt(a["mov"]))
