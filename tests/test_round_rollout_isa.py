"""CPU-only guard on the round kernel's rollout step after its stage cost was
pinned inside the step.  `round_n4_kernel<25, true>`
is compiled to ISA with the Makefile's flags, as tests/test_round_step_isa.py
does, and

* the four-steps-a-trip rollout loop stays at the instruction count this
  change reached (the parent: 87.0 per step by this count - the loop's closing
  s_mov / s_branch included - 75.0 of them vector);
* the state is updated in place on the quad the candidate row's store reads:
  no `v_mov` in the loop (the parent: 2.5 per step) and no `s_nop`;
* the packed count is the parent's 13 per step: the Euler updates as two
  packed multiply-adds were built and measured, and not kept (their results'
  wait states cost what the shorter stream saved);
* no scalar register spilled to a vector lane is read or written inside the
  rollout loop or inside the sweep's unrolled step block;
* the kernel needs no more vector registers than its parent, spills none and
  has no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pddp_amd", "csrc")
KERNEL = "round_n4_kernelILj25ELb1E"

# what the in-place state reached (parent: 87.0 / 75.0 / 13)
STEP_MAX = 84.75
STEP_VALU_MAX = 72.5
PACKED = 13.0
# spilled scalars' lane moves inside the two step loops: there were none in
# the parent either - the kernel's 250 spilled scalars are moved at the
# phases' boundaries and in the rounds' prologue, outside both chains
LANE_MOVES = 0
VGPR_MAX = 178  # the parent's
SWEEP_BLOCK = 16
SWEEP_STEP_SPAN = 120


def _flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*?)(?<!\\)\n", mk, re.S | re.M).group(1)
    flags = flags.replace("\\\n", " ").replace("$(ARCH)", "gfx950")
    own = re.search(r"^FLAGS_round_n4 := (.*)$", mk, re.M).group(1)
    return flags.split() + own.split()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the round kernel cannot be compiled")
    out = tmp_path_factory.mktemp("isa") / "round_n4.s"
    subprocess.check_call([hipcc] + _flags() + [
        "--cuda-device-only", "-S", os.path.join(CSRC, "round_n4.hip"),
        "-o", str(out)], cwd=CSRC)
    return out.read_text()


def _kernel_body(text):
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines)
                 if re.match(r"^_Z\S*%s\S*:" % KERNEL, l))
    end = next(i for i in range(start + 1, len(lines))
               if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def _instructions(lines):
    out = []
    for l in lines:
        t = l.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        out.append(t.split()[0])
    return out


def _rollout_loop(body):
    """The search's rollout loop, header to back branch: the first loop that
    runs four range reductions (`v_rndne_f64`) a trip."""
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\S+):", l)
        if not m or i + 1 >= len(body) or "Loop Header" not in body[i + 1]:
            continue
        end = next((j for j in range(i + 1, len(body))
                    if body[j].strip() == "s_branch " + m.group(1)), None)
        if end is None:
            continue
        ins = _instructions(body[i:end + 1])
        if sum(x.startswith("v_rndne_f64") for x in ins) == 4:
            return ins
    raise AssertionError("the rollout loop (four steps a trip) was not found")


def _sweep_steps(ins):
    """The steps of the sweep's unrolled block: from one pair of
    `ds_bpermute_b32` transposes to the next, sixteen pairs in a row."""
    at = [k for k, x in enumerate(ins) if x == "ds_bpermute_b32"]
    starts = [k for n, k in enumerate(at) if n == 0 or k - at[n - 1] > 4]
    for n in range(len(starts) - SWEEP_BLOCK + 1):
        run = starts[n:n + SWEEP_BLOCK]
        steps = [ins[a:b] for a, b in zip(run, run[1:])]
        if all(len(s) < SWEEP_STEP_SPAN for s in steps):
            return steps
    raise AssertionError("the unrolled sweep block was not found")


def _metadata(text, key):
    md = text[text.index("amdhsa.kernels"):]
    for blk in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if KERNEL in name:
            return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
    raise AssertionError("no metadata for " + KERNEL)


def _lane_moves(ins):
    return sum(x.startswith(("v_readlane", "v_writelane")) for x in ins)


def test_rollout_step_is_shorter_than_the_parents(isa):
    ins = _rollout_loop(_kernel_body(isa))
    per_step = len(ins) / 4
    valu = sum(x.startswith("v_") for x in ins) / 4
    assert per_step <= STEP_MAX, (per_step, valu)
    assert valu <= STEP_VALU_MAX, (per_step, valu)


def test_rollout_step_packed_count_and_no_moves(isa):
    ins = _rollout_loop(_kernel_body(isa))
    assert sum(x.startswith("v_pk_") for x in ins) / 4 == PACKED
    # the candidate row's quad is the state's own registers, and nothing in
    # the step waits out a hazard
    assert sum(x.startswith("v_mov_") for x in ins) == 0
    assert sum(x == "s_nop" for x in ins) == 0
    # one 16-byte store per step
    assert sum(x == "global_store_dwordx4" for x in ins) == 4
    assert sum(x.startswith("global_store") for x in ins) == 4


def test_no_spilled_scalar_moves_in_the_step_loops(isa):
    ins = _instructions(_kernel_body(isa))
    assert _lane_moves(_rollout_loop(_kernel_body(isa))) == LANE_MOVES
    assert sum(_lane_moves(s) for s in _sweep_steps(ins)) == LANE_MOVES


def test_round_kernel_registers(isa):
    assert _metadata(isa, "vgpr_count") <= VGPR_MAX
    assert _metadata(isa, "vgpr_spill_count") == 0
    assert _metadata(isa, "private_segment_fixed_size") == 0
