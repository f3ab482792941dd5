"""CPU-only guard on the round kernel's sweep step: the
cartpole f32 round kernel `round_n4_kernel<25, true>` is compiled to ISA with
the Makefile's flags, and the steps of its unrolled 16-step block - each one
opens with the two `ds_bpermute_b32` transposes - must stay at the paired
step's instruction count, keep their packed operations, need no `s_nop` more
than before, and the kernel must spill no vector register and hold no
scalar-memory store or scalar atomic."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pddp_amd", "csrc")
KERNEL = "round_n4_kernelILj25ELb1E"
BLOCK = 16  # steps of the unrolled block

# the paired step: 83 instructions, 5 of them packed, 2 s_nop (the scalar
# one was 88 with 2 s_nop: the pairing may not bring back a wait state)
STEP_MAX = 83
PACKED_MIN = 5
NOP_MAX = 2
# longer than any step, shorter than a step and a block boundary (~160)
STEP_SPAN = 120


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


def _sweep_steps(ins):
    """The steps of the unrolled block, in the order the code lays them out:
    from one pair of transposes to the next, for BLOCK pairs in a row."""
    at = [k for k, x in enumerate(ins) if x == "ds_bpermute_b32"]
    # a step's two transposes are issued back to back
    starts = [k for n, k in enumerate(at) if n == 0 or k - at[n - 1] > 4]
    for n in range(len(starts) - BLOCK + 1):
        run = starts[n:n + BLOCK]
        steps = [ins[a:b] for a, b in zip(run, run[1:])]
        # (a block boundary - gains out, barrier - is far longer than a step)
        if all(len(s) < STEP_SPAN for s in steps):
            return steps
    raise AssertionError("the unrolled sweep block (%d steps) was not found"
                         % BLOCK)


def _metadata(text, key):
    md = text[text.index("amdhsa.kernels"):]
    for blk in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if KERNEL in name:
            return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
    raise AssertionError("no metadata for " + KERNEL)


def test_sweep_step_instruction_count(isa):
    steps = _sweep_steps(_instructions(_kernel_body(isa)))
    n = len(steps)
    per_step = sum(len(s) for s in steps) / n
    packed = sum(x.startswith("v_pk_") for s in steps for x in s) / n
    nops = sum(x == "s_nop" for s in steps for x in s) / n
    assert per_step <= STEP_MAX, (per_step, packed, nops)
    # (the pairs are there: the Newton point's gaps to the box, Q x + c and
    # Q x / 2 + c at both iterates, Luu + p1 / Lu + p2, -s Quzc / Quzr Quzc)
    assert packed >= PACKED_MIN, (per_step, packed, nops)
    # every DPP source still two instructions behind its write
    assert nops <= NOP_MAX, (per_step, packed, nops)


def test_round_kernel_spills_no_vector_registers(isa):
    assert _metadata(isa, "vgpr_spill_count") == 0
    assert _metadata(isa, "private_segment_fixed_size") == 0


def test_round_kernel_has_no_scalar_memory_writes(isa):
    ins = _instructions(_kernel_body(isa))
    bad = sorted({x for x in ins if re.match(
        r"^s_(buffer_|scratch_)?(store|atomic)|^s_dcache_(?!inv)", x)})
    assert not bad, bad
