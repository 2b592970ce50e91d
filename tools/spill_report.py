#!/usr/bin/env python3
"""Static count of the SGPR spill traffic of one kernel, from the compiler's assembly.

  python tools/spill_report.py [--kernel SUBSTR] [--define -DX ...] [FILE.s]

Without FILE.s the env kernels' translation unit (csrc/vnl_lib.hip) is compiled to assembly with the product's flags
(csrc/build.py, device side only; nothing is run).  Prints, for the kernel whose mangled name holds SUBSTR (default: the
specialised step kernel, `vnl_step_kernelI13VnlSpecRodent`):

  * lane writes (v_writelane_b32) and lane reads (v_readlane_b32), split into SGPR spill traffic and other uses.  A spill VGPR
    is one that v_writelane_b32 writes: the compiler parks SGPRs there, the product writes no lane by hand.  A lane read from
    any other VGPR is work (wave sums, VNL_GETF);
  * the spill reads and writes by region: in front of the substep loop / in its body outside the solver loop / inside the
    solver's iteration loop / behind the substep loop ("glue").  The substep loop is the largest natural loop of the kernel's
    control-flow graph, the solver loop the largest loop nested in it (loops_of below);
  * s_nop, and how many of them stand directly in front of a v_writelane_b32 / a v_cndmask_b32;
  * the instruction total and the resource lines the compiler prints behind every env kernel of the file.

It counts lane reads and writes, s_nop and totals, nothing else.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vnl-brax-imitation_amd", "csrc")
RES = ("NumSgprs", "NumVgprs", "ScratchSize", "Occupancy")
ENV_KERNELS = ("vnl_step_kernel", "vnl_reset_kernel", "vnl_reset_done_kernel")


def compile_asm(defines: list[str]) -> str:
    sys.path.insert(0, CSRC)
    import build as B  # the product's flags, from the one place that has them

    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17",
           "-fPIC"] + B.VARIANTS["product"][1] + defines + ["--cuda-device-only", "-S", os.path.join(CSRC, "vnl_lib.hip"), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def kernels(lines: list[str]) -> dict:
    """{mangled name: (first line, end line)} of every function of the file."""
    out, name, start = {}, None, 0
    for i, l in enumerate(lines):
        mm = re.match(r"(_Z\w+):", l)
        if mm:
            name, start = mm.group(1), i
        elif l.startswith(".Lfunc_end") and name:
            out[name] = (start, i)
            name = None
    return out


def resources(lines: list[str], end: int) -> dict:
    res = {}
    for l in lines[end:end + 400]:
        mm = re.match(r"\s*;\s*(\w+):\s*(\d+)", l)
        if mm and mm.group(1) in RES and mm.group(1) not in res:
            res[mm.group(1)] = int(mm.group(2))
        if l.startswith("_Z"):
            break
    return res


def loops_of(ins: list, labels: dict) -> tuple:
    """(instructions of the substep loop, instructions of the solver loop): natural loops of the kernel's control-flow graph.
    A back edge is a branch to a block that dominates it; its loop is every block that reaches the branch without passing the
    head (where the lines stand does not matter: the compiler places blocks of a loop behind its back edge, and branches
    backwards into blocks that are no loop heads).  The substep loop is the largest loop, the solver's iteration loop the
    largest loop nested in it."""
    n = len(ins)
    is_br = [op.startswith(("s_cbranch", "s_branch")) and rest in labels and labels[rest] < n for op, rest in ins]
    leaders = sorted({0} | {labels[r] for (o, r), b in zip(ins, is_br) if b} | {i + 1 for i, b in enumerate(is_br) if b and i + 1 < n}
                     | {i + 1 for i, (o, r) in enumerate(ins) if o.startswith("s_endpgm") and i + 1 < n})
    blk_of, bounds = {}, []
    for k, a in enumerate(leaders):
        e = leaders[k + 1] if k + 1 < len(leaders) else n
        bounds.append((a, e))
        blk_of[a] = k
    succ = [[] for _ in bounds]
    for k, (a, e) in enumerate(bounds):
        op, rest = ins[e - 1]
        if is_br[e - 1]:
            succ[k].append(blk_of[labels[rest]])
        if not op.startswith(("s_branch", "s_endpgm", "s_setpc")) and e < n:
            succ[k].append(blk_of[e])
    pred = [[] for _ in bounds]
    for k, ss in enumerate(succ):
        for t in ss:
            pred[t].append(k)
    # reverse post-order, then the iterative dominator algorithm (Cooper, Harvey, Kennedy)
    order, seen, stack = [], {0}, [(0, iter(succ[0]))]
    while stack:
        k, it = stack[-1]
        for t in it:
            if t not in seen:
                seen.add(t)
                stack.append((t, iter(succ[t])))
                break
        else:
            order.append(k)
            stack.pop()
    rpo = order[::-1]
    num = {k: i for i, k in enumerate(rpo)}
    idom = {0: 0}
    changed = True
    while changed:
        changed = False
        for k in rpo[1:]:
            new = None
            for q in pred[k]:
                if q in idom:
                    if new is None:
                        new = q
                    else:
                        x, y = q, new
                        while x != y:
                            while num[x] > num[y]:
                                x = idom[x]
                            while num[y] > num[x]:
                                y = idom[y]
                        new = x
            if new is not None and idom.get(k) != new:
                idom[k], changed = new, True

    def dominates(h: int, k: int) -> bool:
        while k != h and k != 0:
            k = idom[k]
        return k == h

    loops = {}
    for k in rpo:
        for h in succ[k]:
            if h in idom and dominates(h, k):
                body = loops.setdefault(h, {h})
                todo = [k]
                while todo:
                    q = todo.pop()
                    if q not in body:
                        body.add(q)
                        todo.extend(x for x in pred[q] if x in idom)
    size = lambda body: sum(bounds[k][1] - bounds[k][0] for k in body)
    by_size = sorted(loops.values(), key=size, reverse=True)
    sub = by_size[0] if by_size else set()
    inner = [b for b in by_size[1:] if b < sub]
    expand = lambda body: {i for k in body for i in range(*bounds[k])}
    return expand(sub), expand(inner[0] if inner else set())


def report(lines: list[str], name: str, span: tuple) -> str:
    body = lines[span[0]:span[1]]
    ins, labels = [], {}  # (mnemonic, operand text), label -> index of the next instruction
    for l in body:
        t = l.split(";")[0].strip()
        if not t or t[0] == ".":
            if t.endswith(":"):
                labels[t[:-1]] = len(ins)
            continue
        if t.endswith(":"):
            labels[t[:-1]] = len(ins)
            continue
        op, _, rest = t.partition(" ")
        ins.append((op, rest.strip()))
    sub, cg = loops_of(ins, labels)
    first = min(sub, default=0)

    def region(i: int) -> str:
        if i in cg:
            return "solver loop"
        if i in sub:
            return "substep body"
        return "front" if i < first else "glue"

    spill_v = {rest.split(",")[0].strip() for op, rest in ins if op == "v_writelane_b32"}
    slots = {tuple(x.strip() for x in rest.split(",")[::2]) for op, rest in ins if op == "v_writelane_b32"}
    regs = ("front", "substep body", "solver loop", "glue")
    rd, wr = dict.fromkeys(regs, 0), dict.fromkeys(regs, 0)
    other_rd = 0
    for i, (op, rest) in enumerate(ins):
        if op == "v_writelane_b32":
            wr[region(i)] += 1
        elif op == "v_readlane_b32":
            if rest.split(",")[1].strip() in spill_v:
                rd[region(i)] += 1
            else:
                other_rd += 1
    nop = sum(op == "s_nop" for op, _ in ins)
    nop_wl = sum(op == "s_nop" and ins[i + 1][0] == "v_writelane_b32" for i, (op, _) in enumerate(ins[:-1]))
    nop_cm = sum(op == "s_nop" and ins[i + 1][0].startswith("v_cndmask_b32") for i, (op, _) in enumerate(ins[:-1]))
    res = resources(lines, span[1])
    out = [f"kernel {name}",
           f"  instructions {len(ins)}   substep loop {len(sub)}   solver loop {len(cg)}",
           f"  spill VGPRs {len(spill_v)} ({', '.join(sorted(spill_v, key=lambda v: int(v[1:])))})   spill slots {len(slots)}",
           f"  v_writelane_b32 {sum(wr.values())} (all spill)   v_readlane_b32 {sum(rd.values()) + other_rd}: spill {sum(rd.values())}, other {other_rd}",
           "  region          spill reads  spill writes"]
    out += [f"  {r:<15} {rd[r]:>11} {wr[r]:>13}" for r in regs]
    out += [f"  s_nop {nop}   in front of v_writelane {nop_wl}   in front of v_cndmask {nop_cm}",
            f"  flat_ instructions {sum(op.startswith('flat_') for op, _ in ins)}",
            "  " + "  ".join(f"{k}={v}" for k, v in res.items())]
    return "\n".join(out)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", nargs="?", help="assembly of csrc/vnl_lib.hip (default: compile it)")
    ap.add_argument("--kernel", default="vnl_step_kernelI13VnlSpecRodent")
    ap.add_argument("--define", action="append", default=[], help="extra compiler flag, e.g. --define=-DVNL_SGPR_PLAIN")
    a = ap.parse_args()
    path = a.asm or compile_asm(a.define)
    lines = open(path).read().split("\n")
    ks = kernels(lines)
    hit = [n for n in ks if a.kernel in n]
    if not hit:
        sys.exit(f"no function whose name holds {a.kernel!r} in {path}")
    for n in hit:
        print(report(lines, n, ks[n]))
    print("env kernels of the file:")
    for n, sp in ks.items():
        if any(k in n for k in ENV_KERNELS):
            print(f"  {n[:60]:<60} " + "  ".join(f"{k}={v}" for k, v in resources(lines, sp[1]).items()))
    if not a.asm:
        os.remove(path)


if __name__ == "__main__":
    main()
