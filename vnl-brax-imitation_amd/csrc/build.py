"""Build libvnl.so for gfx950 with hipcc (in-tree, next to the sources)."""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# (vnl_domain.hip last: the randomised env kernels, a translation unit of their own -- vnl_env_set_domain -- listed after the
# existing kernels in the resource report; vnl_eval.hip: the step kernels that score an evaluation, vnl_env_step_post_eval,
# apart for the same reason; vnl_record.hip last: the kernel and entry of the recorded rollouts, vnl_env_record, likewise)
SOURCES = ["vnl_lib.hip", "vnl_policy.hip", "vnl_ppo.hip", "vnl_domain.hip", "vnl_eval.hip", "vnl_record.hip"]
DEPS = SOURCES + ["vnl_env_kernels.h", "vnl_body.h", "vnl_types.h", "vnl_inertial.h", "vnl_philox.h", "vnl_policy_train.h", "../../include/vnl.h"]
OUT = os.path.join(HERE, "libvnl.so")

# Diagnostic / regression builds of the SAME sources (never the product library, only loaded by tools/ and tests/):
#   prof   -DVNL_PROFILE      per-stage s_memtime stamps (tools/stage_profile.py)
#   knobs  -DVNL_STAGE_KNOBS  stage-repeat knob VNL_DBG_REPEAT + LDS padding knob (tools/stage_cost.py, tools/pmc_stage.sh)
#   noblk  -DVNL_NO_BLK: the products with the factor / its inverse one lane per row / column (regression build for the
#          balanced blocked form, EnvWave::blk_apply: same sums in another order)
#   tail   -DVNL_SOLVER_TAIL: the solver's last permitted iteration computes its gradient / M^-1 grad / search update
#          although nothing reads them (regression build for the skipped tail of EnvWave::solve: the same bits on every output)
#   plain  -DVNL_SOLVER_PLAIN: the solver loop as it was before its per-lane constants were staged -- index tables and friction
#          read from global memory, a block-descriptor load per product (regression build and bisecting tool for the staged
#          form, EnvWaveT::with_solve_regs / load_tables: the same values from another place, the same bits on every output)
#   vmemplain -DVNL_VMEM_PLAIN: the vector-memory accesses of a substep outside the solver loop as they were before they were
#          taken off the critical path -- factor_aba's schedule byte and 1/D2 store per step, euler()'s element-wise reload of
#          the second inverse factor, forward()'s copy of the warm start through LO(tmp) (regression build and bisecting tool:
#          the same values by another route, the same bits on every output; tests/test_gpu_vmem_schedule.py)
#   ldsplain -DVNL_LDS_PLAIN: the serial LDS round trips of a substep as they were before they were taken out -- blk_apply one
#          trip after the other (indices, gathers, the writer's operands: three dependent round trips each), factor_aba's
#          pivot block writing V = U / D and 1/D1 inside the step chain and its lane sets reading their lines one after the
#          other, the solver's qg1 / qg2 / Gauss scalars in per-dof passes of their own (regression build and bisecting tool:
#          the same operations in another order of issue, the same bits on every output; tests/test_gpu_lds_chain.py)
#   sgprplain -DVNL_SGPR_PLAIN: the lane predicates of a substep as the compiler used to carry them -- `u < n` of blk_apply's
#          selects, the debug trace's literal row addresses and the masks lane < 64 / lane > 63 of every one-trip region found
#          loop-invariant, hoisted to the top of the kernel, parked in VGPR lanes for want of SGPRs and read back with
#          v_readlane at every use (regression build for VNL_LOCAL / VNL_ROLLED / VNL_LANE_RANGE of csrc/vnl_body.h: the same
#          compares on the same operands issued in another place or not needed, the same bits on every output;
#          tests/test_gpu_sgpr_plain.py, tools/spill_report.py)
#   xlaneplain -DVNL_XLANE_PLAIN: the cross-lane glue of a substep as it was -- every row_bcast step of a wave sum or scan as
#          the builtin with old = 0 and an add (v_mov_b32 0, v_mov_b32_dpp, v_add_f32) instead of one masked v_add_f32_dpp, every
#          sum and scan a sequence of its own, the last trip of dof_prefix (nine dofs of the rodent's 73) as six full scans
#          (regression build for vnl_rows_join / VNL_WAVE_SUMS / VNL_SCAN6 and dof_prefix's tail form of csrc/vnl_body.h: the
#          same adds on the same operands, the same bits on every output; tests/test_gpu_xlane_plain.py)
#   treeplain -DVNL_TREE_PLAIN: the two subtree sums of a substep (composite inertias, cfrc child into parent) in the
#          specialised kernels as the generic ones still do them -- a walk that reads the parent bytes from LDS and decides per
#          body with compares and selects whether it is a chain link, which register of its group of eight is the parent, or
#          whether the parent lies below the group (regression build for EnvWaveT::tree_accumulate_const of csrc/vnl_body.h,
#          the walk unrolled over VnlSpecRodent::body_parent: the same adds on the same operands in the same order, the same
#          bits on every output; tests/test_gpu_tree_const.py)
#   spill  env kernels compiled under a 128-VGPR cap, which forces ~230 registers per lane to spill to scratch
#          memory: results must not depend on spilling (tests/test_gpu_spill.py)
#   nospec -DVNL_NO_SPEC: the generic kernels (dims and LDS offsets read at run time) on the rodent too: the specialised ones
#          must agree bit for bit (tests/test_gpu_spill.py)
#
# The product holds its env kernels to two waves per SIMD: the specialised instantiations, every bound a constant, are
# unrolled further by the compiler and would otherwise take a 257th register -- half the occupancy.  The diagnostic and
# regression variants carry extra code: held to the same two waves so that their timings stay comparable.
TWO_WAVES = "-DVNL_KERNEL_ATTR=__attribute__((amdgpu_waves_per_eu(2,2)))"
_DEFINES = {"prof": "VNL_PROFILE", "knobs": "VNL_STAGE_KNOBS", "noblk": "VNL_NO_BLK", "tail": "VNL_SOLVER_TAIL",
            "plain": "VNL_SOLVER_PLAIN", "vmemplain": "VNL_VMEM_PLAIN", "ldsplain": "VNL_LDS_PLAIN",
            "sgprplain": "VNL_SGPR_PLAIN", "xlaneplain": "VNL_XLANE_PLAIN", "treeplain": "VNL_TREE_PLAIN",
            "nospec": "VNL_NO_SPEC"}
VARIANTS = {
    "product": ("libvnl.so", [TWO_WAVES]),
    "spill": ("libvnl_spill.so", ["-DVNL_KERNEL_ATTR=__attribute__((amdgpu_waves_per_eu(4,4)))"]),
    **{v: (f"libvnl_{v}.so", ["-D" + d, TWO_WAVES]) for v, d in _DEFINES.items()},
}
# What the driver entry builds (__graft_entry__.build): the product and the regression builds the tests load.  A new
# regression build is a paragraph above, an entry of _DEFINES and a name here; its device test is a few calls into
# tests/variant_cases.py, its host test (tests/helpers.py HOSTSIM_VARIANTS) into tests/hostsim_cases.py.
DRIVER_VARIANTS = ("product", "spill", "noblk", "nospec", "tail", "plain", "vmemplain", "ldsplain", "sgprplain", "xlaneplain",
                   "treeplain")
ENV_KERNELS = ("vnl_step_kernel", "vnl_reset_kernel", "vnl_reset_done_kernel")


def resource_usage(stderr_text: str) -> dict:
    """{kernel name: {remark: int}} parsed from -Rpass-analysis=kernel-resource-usage."""
    out, name = {}, None
    for line in stderr_text.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
            out[name] = {}
        elif name and "remark:" in line:
            body = line.split("remark:")[1].split("[-Rpass")[0].strip()  # e.g. "Occupancy [waves/SIMD]: 2"
            key, _, val = body.rpartition(":")
            try:
                out[name][key.strip()] = int(val.strip())
            except ValueError:
                pass
    return out


def build(force: bool = False, verbose: bool = False, profile: bool = False, knobs: bool = False,
          variant: str | None = None) -> str:
    variant = variant or ("prof" if profile else ("knobs" if knobs else "product"))
    fname, defs = VARIANTS[variant]
    out = os.path.join(HERE, fname)
    deps = [os.path.join(HERE, d) for d in DEPS] + [os.path.abspath(__file__)]
    newest = max(os.path.getmtime(d) for d in deps)
    if not force and os.path.exists(out) and os.path.getmtime(out) >= newest:
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # One object per source, kept under _obj/<variant>/ with the compiler's resource-usage remarks beside it: a change to the
    # PPO or policy kernels does not recompile the env kernels (two minutes), and the register-budget check below still sees
    # every kernel's remarks.
    objdir = os.path.join(HERE, "_obj", variant)
    os.makedirs(objdir, exist_ok=True)
    flags = ["-Rpass-analysis=kernel-resource-usage", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "-fPIC"] + \
        defs + os.environ.get("VNL_HIPCC_EXTRA", "").split()
    stamp = " ".join(flags)
    headers = [d for d in deps if not d.endswith(".hip")]
    SRC_DEPS = {"vnl_lib.hip": headers, "vnl_policy.hip": [h for h in headers if h.endswith("vnl.h")] + [os.path.join(HERE, "vnl_policy_train.h"), os.path.join(HERE, "vnl_philox.h")],
                "vnl_ppo.hip": [h for h in headers if h.endswith("vnl.h")] + [os.path.join(HERE, "vnl_policy_train.h")]}
    objs, remarks = [], ""
    for src in SOURCES:
        obj = os.path.join(objdir, src + ".o")
        rem = obj + ".remarks.txt"
        srcdeps = [os.path.join(HERE, src)] + [h for h in SRC_DEPS.get(src, headers) if os.path.exists(h)]
        fresh = (not force and os.path.exists(obj) and os.path.exists(rem) and
                 os.path.getmtime(obj) >= max(os.path.getmtime(d) for d in srcdeps) and
                 open(rem).readline().rstrip("\n") == stamp)
        if not fresh:
            cmd = [hipcc] + flags + ["-c", os.path.join(HERE, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
            if verbose or r.returncode:
                sys.stderr.write(r.stderr)
            if r.returncode:
                raise subprocess.CalledProcessError(r.returncode, cmd)
            with open(rem, "w") as f:
                f.write(stamp + "\n" + r.stderr)
        objs.append(obj)
        remarks += open(rem).read().split("\n", 1)[1]
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise subprocess.CalledProcessError(r.returncode, cmd)

    # Register budget of the env kernels: a PERFORMANCE check (two waves per SIMD and no private-memory stack are what
    # the measured numbers assume), not a correctness one -- the spill variant runs the parity tests with hundreds of bytes of
    # scratch per lane.  Fails closed: if the compiler's remarks for the env kernels are not found, the build is
    # rejected rather than waved through.
    usage = resource_usage(remarks)  # (of all objects, cached or not)
    seen = {k: [u for n, u in usage.items() if k in n] for k in ENV_KERNELS}
    missing = [k for k, v in seen.items() if not v or "Occupancy [waves/SIMD]" not in v[0]]
    if missing:
        os.remove(out)
        raise RuntimeError(f"no resource-usage remark for {missing}: cannot check the register budget of this build")
    if variant == "product":
        for k, u in ((k, u) for k, v in seen.items() for u in v):
            # (a few dwords of scratch are values that live across the whole launch -- rtrunk, a scratch pointer -- parked
            # once and fetched once per substep: the specialised step kernel has 20 B; more than 64 B means spilling in loops)
            if u.get("ScratchSize [bytes/lane]", 0) > 64 or u["Occupancy [waves/SIMD]"] < 2:
                if os.environ.get("VNL_ALLOW_SPILL") != "1":
                    os.remove(out)
                    raise RuntimeError(
                        f"{k}: {u.get('VGPRs')} VGPRs, {u.get('ScratchSize [bytes/lane]')} B scratch per lane, "
                        f"{u['Occupancy [waves/SIMD]']} waves/SIMD -- below the two waves per SIMD without spilling that the "
                        "published numbers were measured with.  Results do not depend on spilling (tests/test_gpu_spill.py); "
                        "this gate keeps a performance regression from shipping silently: set VNL_ALLOW_SPILL=1 to build anyway")
                sys.stderr.write(f"[build] WARNING (performance): {k} uses {u.get('VGPRs')} VGPRs, "
                                 f"{u.get('ScratchSize [bytes/lane]')} B scratch per lane, "
                                 f"{u['Occupancy [waves/SIMD]']} waves/SIMD: below the two waves per SIMD without "
                                 "spilling that the published numbers were measured with\n")
    with open(os.path.join(HERE, fname + ".resources.txt"), "w") as f:
        for n, u in usage.items():
            f.write(n + " " + " ".join(f"{a}={b}" for a, b in sorted(u.items())) + "\n")
    return out


if __name__ == "__main__":
    v = next((k for k in VARIANTS if "--" + k in sys.argv), None)
    if "--profile" in sys.argv:
        v = "prof"
    print(build(force="--force" in sys.argv, verbose=True, variant=v))
