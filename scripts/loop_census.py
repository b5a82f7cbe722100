#!/usr/bin/env python
"""Static census of ONE kernel's gfx950 code by LOOP-NEST LEVEL (no GPU needed):

    python scripts/loop_census.py inst_f64_t0 'k_nuts<double, 64, 2, 0, 0>' [--json out.json]
    python scripts/loop_census.py path/to/unit.o 'k_nuts<double, 64, 2, 3, 0>'
    python scripts/loop_census.py ... --diff before.json     # per level (matched in order), the mnemonics whose counts differ from an earlier --json
    AHMC_OBJ_DIR=<object cache>/variants/<name> python scripts/loop_census.py inst_f64_t0b ...   # another build's objects

The unit is disassembled (llvm-objdump, as scripts/isa_digest.py does), the kernel whose demangled name contains the given text is cut
out, its control-flow graph is built from the branch targets, and the natural loops (back edges to a dominating header; loops with one
header merged) are nested by containment.  Every instruction is counted ONCE, at the innermost loop that holds it — so the row of a
loop is the code that runs once per iteration of THAT loop outside the loops inside it, and `(none)` is what runs once per launch.

Per level: VALU, memory instructions (VMEM / LDS / SMEM apart), and the two classes DESIGN §4.1 "once per transition" is about:
  restores  v_readlane_b32 from one of the VGPRs the kernel fills with v_writelane_b32 — the restore of a spilled SGPR, one dword each
            (`parks`: the v_writelane_b32 into them)
  addr64    v_lshl_add_u64 — 64-bit per-lane address arithmetic
and tell-tale signatures to recognise the level (philox = v_mul_hi_u32, xlane = permlane swaps / DPP = a reduction, ...).
Static counts: a level's row counts every block of the level once, rarely taken branches included."""
import json
import os
import re
import subprocess
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LLVM = "/opt/rocm/lib/llvm/bin"


def disassemble(obj, tmp="/tmp/isa"):
    import shutil

    os.makedirs(tmp, exist_ok=True)
    cp = os.path.join(tmp, os.path.basename(obj))
    shutil.copyfile(obj, cp)  # llvm-objdump --offloading writes the device image next to its input
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", cp], capture_output=True, check=True)
    co = cp + ".0.hipv4-amdgcn-amd-amdhsa--gfx950"
    return subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout


def kernel_slice(text, want):
    """[(addr, mnemonic, operands, branch target or None)] of the kernel whose demangled name contains `want` (blanks ignored)"""
    heads = [(m.start(), int(m.group(1), 16), m.group(2)) for m in re.finditer(r"^([0-9a-f]+) <(.+)>:$", text, flags=re.M)]
    names = subprocess.run(["c++filt"], input="\n".join(h[2] for h in heads), capture_output=True, text=True).stdout.splitlines()
    key = want.replace(" ", "")
    hit = [i for i, n in enumerate(names) if key in n.replace(" ", "") and not heads[i][2].endswith(".kd")]
    if len(hit) != 1:
        raise SystemExit(f"{len(hit)} kernels match {want!r}: {[names[i] for i in hit][:8]}")
    i = hit[0]
    body = text[heads[i][0]:heads[i + 1][0] if i + 1 < len(heads) else len(text)]
    base, ins = heads[i][1], []
    for line in body.splitlines()[1:]:
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if not m:
            continue
        mn, ops, addr = m.group(1), m.group(2), int(m.group(3), 16)
        tgt = None
        if mn.startswith(("s_branch", "s_cbranch")):
            t = re.search(r"\+0x([0-9a-f]+)>", line)
            tgt = base + int(t.group(1), 16) if t else None
        ins.append((addr, mn, ops, tgt))
    return names[i], ins


def klass(mn):
    if mn.startswith(("s_branch", "s_cbranch")):
        return "BR"
    if mn.startswith(("s_waitcnt", "s_nop", "s_endpgm", "s_barrier", "s_sleep", "s_setprio", "s_clause")):
        return "MISC"
    if mn.startswith(("s_load", "s_buffer_load")):
        return "SMEM"
    if mn.startswith("s_"):
        return "SALU"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(("global_", "scratch_", "buffer_", "flat_")):
        return "VMEM"
    if mn.startswith("v_"):
        return "VALU"
    return "MISC"


SIG = [("permlane", "xlane"), ("v_mul_hi_u32", "philox"), ("v_ldexp", "ldexp"), ("v_rcp", "rcp"), ("v_sqrt", "sqrt"), ("v_rsq", "rsq"), ("v_log", "log"),
       ("v_exp", "exp"), ("v_div_", "div"), ("scratch_", "scratch"), ("v_readfirstlane", "rfl")]


def census(ins):
    addrs = [a for a, *_ in ins]
    idx = {a: i for i, a in enumerate(addrs)}
    leaders = {addrs[0]}
    for i, (a, mn, ops, tgt) in enumerate(ins):
        if tgt is not None:
            leaders.add(tgt)
        if (tgt is not None or mn in ("s_endpgm", "s_setpc_b64")) and i + 1 < len(ins):
            leaders.add(addrs[i + 1])
    leaders = sorted(x for x in leaders if x in idx)
    blocks = [ins[idx[s]:(idx[leaders[k + 1]] if k + 1 < len(leaders) else len(ins))] for k, s in enumerate(leaders)]
    bidx = {s: k for k, s in enumerate(leaders)}
    n = len(blocks)
    succ = [[] for _ in range(n)]
    for k, body in enumerate(blocks):
        a, mn, ops, tgt = body[-1]
        if tgt is not None:
            if tgt in bidx:
                succ[k].append(bidx[tgt])
            if not mn.startswith("s_branch") and k + 1 < n:
                succ[k].append(k + 1)
        elif mn not in ("s_endpgm", "s_setpc_b64") and k + 1 < n:
            succ[k].append(k + 1)
    pred = [[] for _ in range(n)]
    for k in range(n):
        for s in succ[k]:
            pred[s].append(k)
    # dominators (iterative, over the blocks reachable from the entry, in reverse post-order)
    order, seen, stack = [], {0}, [(0, iter(succ[0]))]
    while stack:
        k, it = stack[-1]
        for s in it:
            if s not in seen:
                seen.add(s)
                stack.append((s, iter(succ[s])))
                break
        else:
            order.append(k)
            stack.pop()
    rpo = order[::-1]
    pos = {b: i for i, b in enumerate(rpo)}
    idom = {0: 0}
    changed = True
    while changed:
        changed = False
        for b in rpo[1:]:
            new = None
            for p_ in pred[b]:
                if p_ not in idom:
                    continue
                if new is None:
                    new = p_
                    continue
                x, y = p_, new
                while x != y:
                    while pos[x] > pos[y]:
                        x = idom[x]
                    while pos[y] > pos[x]:
                        y = idom[y]
                new = x
            if new is not None and idom.get(b) != new:
                idom[b] = new
                changed = True

    def dominates(h, b):
        while True:
            if b == h:
                return True
            if b == 0 or b not in idom:
                return False
            b = idom[b]

    loops = defaultdict(set)  # header -> body
    for t in seen:
        for h in succ[t]:
            if h in seen and dominates(h, t):
                body, work = {h, t}, [t]
                while work:
                    x = work.pop()
                    if x == h:
                        continue
                    for p_ in pred[x]:
                        if p_ in seen and p_ not in body:
                            body.add(p_)
                            work.append(p_)
                loops[h] |= body
    heads = sorted(loops, key=lambda h: len(loops[h]))  # innermost first
    owner = {}
    for h in heads:
        for b in loops[h]:
            owner.setdefault(b, h)
    parent = {}
    for i, h in enumerate(heads):
        parent[h] = next((g for g in heads[i + 1:] if h in loops[g] and g != h), None)

    def depth(h):
        d = 0
        while h is not None:
            d, h = d + 1, parent[h]
        return d

    park = set()
    for a, mn, ops, tgt in ins:
        if mn.startswith("v_writelane_b32"):
            park.add(ops.split(",")[0].strip())
    rows = defaultdict(lambda: defaultdict(int))
    hist = defaultdict(lambda: defaultdict(int))
    for k in seen:
        row = rows[owner.get(k)]
        row["blocks"] += 1
        for a, mn, ops, tgt in blocks[k]:
            row[klass(mn)] += 1
            hist[owner.get(k)][mn] += 1
            if mn.startswith("v_readlane_b32") and ops.split(",")[1].strip() in park:
                row["restores"] += 1
            if mn.startswith("v_writelane_b32"):
                row["parks"] += 1
            if mn.startswith("v_lshl_add_u64"):
                row["addr64"] += 1
            for pat, name in SIG:
                if pat in mn:
                    row["sig_" + name] += 1
            if "dpp" in ops or "quad_perm" in ops or "row_" in ops:
                row["sig_dpp"] += 1
    out = []
    for h in [None] + sorted(loops, key=lambda h: leaders[h]):
        r = rows[h]
        out.append({"loop": "(none)" if h is None else "+0x%x" % (leaders[h] - addrs[0]), "depth": 0 if h is None else depth(h),
                    "parent": None if h is None or parent[h] is None else "+0x%x" % (leaders[parent[h]] - addrs[0]),
                    "blocks": r["blocks"], "valu": r["VALU"], "vmem": r["VMEM"], "lds": r["LDS"], "smem": r["SMEM"], "salu": r["SALU"],
                    "mem": r["VMEM"] + r["LDS"] + r["SMEM"], "restores": r["restores"], "parks": r["parks"], "addr64": r["addr64"],
                    "signature": {k[4:]: v for k, v in sorted(r.items()) if k.startswith("sig_")}, "mnemonics": dict(sorted(hist[h].items()))})
    return {"instructions": len(ins), "spill_vgprs": sorted(park), "levels": out}


def main():
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in ("--json", "--diff")]
    unit, want = args[0], args[1]
    if not os.path.exists(unit):
        from ahmc_amd import build as _B

        unit = os.path.join(os.environ.get("AHMC_OBJ_DIR") or _B.OBJ, unit + ".o")
    name, ins = kernel_slice(disassemble(unit), want)
    res = {"kernel": name, **census(ins)}
    print(f"# {name}: {res['instructions']} instructions; SGPR spills parked in {len(res['spill_vgprs'])} VGPR(s) {' '.join(res['spill_vgprs'])}")
    print("# loop (offset of its header)  depth  parent      blocks   VALU  VMEM   LDS  SMEM  SALU  restores parks addr64  signature")
    for r in res["levels"]:
        print("%-30s %5d  %-10s %7d %6d %5d %5d %5d %5d %9d %5d %6d  %s" % (
            "  " * r["depth"] + r["loop"], r["depth"], r["parent"] or "-", r["blocks"], r["valu"], r["vmem"], r["lds"], r["smem"], r["salu"],
            r["restores"], r["parks"], r["addr64"], " ".join(f"{k}:{v}" for k, v in r["signature"].items())))
    if "--diff" in sys.argv:
        old = json.load(open(sys.argv[sys.argv.index("--diff") + 1]))
        if [r["depth"] for r in old["levels"]] != [r["depth"] for r in res["levels"]]:
            print("# --diff: the loop nests differ, levels cannot be matched")
        else:
            for a, b in zip(old["levels"], res["levels"]):
                d = {m: (a["mnemonics"].get(m, 0), b["mnemonics"].get(m, 0)) for m in set(a["mnemonics"]) | set(b["mnemonics"])}
                d = {m: v for m, v in sorted(d.items()) if v[0] != v[1] and klass(m) not in ("MISC",)}
                if d:
                    print(f"# {b['loop']} (depth {b['depth']}): " + "  ".join(f"{m} {v[0]}->{v[1]}" for m, v in d.items()))
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
