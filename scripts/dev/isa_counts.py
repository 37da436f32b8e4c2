"""Instruction-class counts of the headline kernels' ISA (no GPU needed: hipcc -S --cuda-device-only with the library's flags).

A wavefront alone on a SIMD issues one instruction every ~5 cycles whatever it is (LAB_NOTES.md, round 4), so these kernels
are bound by what they issue, and an instruction that only moves a value costs what an FMA costs.  Per kernel, and for its
largest loop (natural loop of the control-flow graph), this prints CLASS COUNTS only:

  total        instructions
  fp64         every v_*_f64 instruction but moves (arithmetic, comparisons, conversions: the work in double)
  agpr         v_accvgpr_read / v_accvgpr_write / v_accvgpr_mov: traffic with the second register file
  spill_lane   v_writelane_b32 of an SGPR into a lane given as a literal, and v_readlane_b32 back from such a VGPR: the
               register allocator's SGPR spills (a readlane of a reduction reads a VGPR no such writelane targets)
  v_mov        v_mov_b32 / v_mov_b64 (DPP moves excluded: they are the lane exchange)
  s_nop, s_waitcnt
  registers    from the kernel descriptor's comment block: VGPRs, AGPRs, SGPRs, scratch bytes per lane

usage: python scripts/dev/isa_counts.py [--json] [kernel-name-substring ...]
       (default: the sampler, the re-score and the team kernel of the headline call)
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from esac_amd import build as B  # noqa: E402

# kernel (substring of the mangled name) -> source
HEADLINE = {
    "k_sampleILi256ELi2E": "esac_kernels.hip",
    "k_rescoreILi1024E": "esac_kernels.hip",
    "k_refine_teamILi2ELi0ELi16EE": "esac_refine_team.hip",
    "k_refine_team_routeILi2ELi16EE": "esac_refine_team_route.hip",
    "k_sample_routeILi256ELi2E": "esac_front_route.hip",
    "k_rescore_routeILi1024ELi5E": "esac_front_route.hip",
}
FP64_ARITH = re.compile(r"^v_(?!mov)\w*_f64")
CLASSES = ("total", "fp64", "agpr", "spill_lane", "v_mov", "s_nop", "s_waitcnt")


def hipcc():
    for cand in ("/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def assemble(source, out_dir):
    """hipcc -S of one source of the library, with the library's flags."""
    asm = os.path.join(out_dir, os.path.splitext(source)[0] + ".s")
    cmd = [hipcc()] + [f for f in B.FLAGS if f not in ("-shared", "-fPIC")] + ["-S", "--cuda-device-only", os.path.join(B.CSRC, source), "-o", asm]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return asm


def functions(asm_path):
    """{mangled name: {"ins": [(label or None, instruction)], "regs": {...}}}: labels are kept as entries with instruction None."""
    funcs, cur, name = {}, None, None
    with open(asm_path) as fh:
        for line in fh:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                name = m.group(1)
                cur = funcs.setdefault(name, {"ins": [], "regs": {}})["ins"]
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize): (\d+)", line)
            if m and name is not None:
                funcs[name]["regs"][m.group(1)] = int(m.group(2))
                continue
            if cur is None:
                continue
            s = line.split(";")[0].strip()
            if not s or s.startswith("."):
                m = re.match(r"^(\.LBB\w+):", s)
                if m:
                    cur.append((m.group(1), None))
                continue
            if s.endswith(":"):
                continue
            cur.append((None, s))
    return funcs


def spill_vgprs(ins):
    """VGPRs that hold SGPR spills: targets of `v_writelane_b32 vN, sX, <literal lane>`."""
    regs = set()
    for i in ins:
        m = re.match(r"^v_writelane_b32 (v\d+), (s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi), \d+$", i)
        if m:
            regs.add(m.group(1))
    return regs


def classify(ins, spills):
    c = dict.fromkeys(CLASSES, 0)
    for i in ins:
        c["total"] += 1
        if FP64_ARITH.match(i):
            c["fp64"] += 1
        elif i.startswith("v_accvgpr_"):
            c["agpr"] += 1
        elif i.startswith("v_writelane_b32") or i.startswith("v_readlane_b32"):
            ops = [o.strip() for o in i.split(None, 1)[1].split(",")]
            v = ops[0] if i.startswith("v_writelane") else ops[1]
            if v in spills and re.match(r"^\d+$", ops[2]):
                c["spill_lane"] += 1
        elif re.match(r"^v_mov_b(32|64)(_e32|_e64)? ", i):
            c["v_mov"] += 1
        elif i.startswith("s_nop"):
            c["s_nop"] += 1
        elif i.startswith("s_waitcnt"):
            c["s_waitcnt"] += 1
    return c


def largest_loop(entries):
    """Instructions of the largest natural loop of the function's control-flow graph: basic blocks from the labels and
    branches, back edges by a depth-first walk from the entry, a loop = its header and every block that reaches the back
    edge's source without passing the header.  (Where a block sits in the file says nothing: the compiler lays join blocks
    and cold paths out far from the code around them, and a branch up the file need not close a loop.)"""
    blocks, cur, label_at = [[]], 0, {}
    for label, i in entries:
        if i is None:
            if blocks[-1]:
                blocks.append([])
            label_at[label] = len(blocks) - 1
            continue
        blocks[-1].append(i)
        if re.match(r"^s_c?branch|^s_endpgm|^s_setpc", i):
            blocks.append([])
    succ = []
    for n, blk in enumerate(blocks):
        out, last = [], blk[-1] if blk else ""
        m = re.match(r"^s_(c?)branch\w* (\.LBB\w+)$", last)
        if m and m.group(2) in label_at:
            out.append(label_at[m.group(2)])
        if not last.startswith(("s_branch", "s_endpgm", "s_setpc")) and n + 1 < len(blocks):
            out.append(n + 1)
        succ.append(out)
    pred = [[] for _ in blocks]
    for n, out in enumerate(succ):
        for t in out:
            pred[t].append(n)
    # iterative depth-first walk: an edge to a block still on the walk's stack is a back edge
    state, back, stack = [0] * len(blocks), [], [(0, 0)]
    state[0] = 1
    while stack:
        n, k = stack.pop()
        if k < len(succ[n]):
            stack.append((n, k + 1))
            t = succ[n][k]
            if state[t] == 1:
                back.append((n, t))
            elif state[t] == 0:
                state[t] = 1
                stack.append((t, 0))
        else:
            state[n] = 2
    loops = {}
    for src, head in back:
        body, work = loops.setdefault(head, {head}), [src]
        while work:
            n = work.pop()
            if n not in body:
                body.add(n)
                work.extend(pred[n])
    best = max(loops.values(), key=lambda body: sum(len(blocks[n]) for n in body), default=set())
    return [i for n in sorted(best) for i in blocks[n]]


def count_kernels(wanted=None, asm_dir=None):
    wanted = wanted or list(HEADLINE)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        cache = {}
        for want in wanted:
            sources = [HEADLINE[want]] if want in HEADLINE else B.SOURCES
            for src in sources:
                if src not in cache:
                    pre = os.path.join(asm_dir, os.path.splitext(src)[0] + ".s") if asm_dir else None
                    cache[src] = functions(pre if pre and os.path.exists(pre) else assemble(src, tmp))
                for name, f in cache[src].items():
                    if want not in name:
                        continue
                    ins = [i for _, i in f["ins"] if i is not None]
                    spills = spill_vgprs(ins)
                    out[name] = {"kernel": classify(ins, spills), "largest_loop": classify(largest_loop(f["ins"]), spills), "registers": f["regs"]}
    return out


def main(argv):
    as_json = "--json" in argv
    asm_dir = None
    if "--asm-dir" in argv:  # assembly already made (one <source>.s per source)
        asm_dir = argv[argv.index("--asm-dir") + 1]
        argv = [a for a in argv if a not in ("--asm-dir", asm_dir)]
    wanted = [a for a in argv if not a.startswith("--")]
    res = count_kernels(wanted, asm_dir)
    if as_json:
        print(json.dumps(res, indent=1, sort_keys=True))
        return
    for name, r in sorted(res.items()):
        print(name)
        print("  %-13s" % "" + "".join("%11s" % c for c in CLASSES))
        for part in ("kernel", "largest_loop"):
            print("  %-13s" % part + "".join("%11d" % r[part][c] for c in CLASSES))
        print("  registers    " + ", ".join("%s %d" % kv for kv in sorted(r["registers"].items())))


if __name__ == "__main__":
    main(sys.argv[1:])
