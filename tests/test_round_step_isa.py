"""CPU-only guard on the round kernel's rollout step: the
cartpole f32 round kernel `round_n4_kernel<25, true>` is compiled to ISA with
the Makefile's flags, and its unrolled rollout loop (four steps, one
`v_rndne_f64` each - the sine / cosine range reduction) must stay at the
paired step's instruction count, spill no more registers, and hold no
scalar-memory store or scalar atomic."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pddp_amd", "csrc")
KERNEL = "round_n4_kernelILj25ELb1E"

# the paired step: 86 instructions (the scalar one was 100), 75 of them vector
STEP_MAX = 88
STEP_VALU_MAX = 77
# the kernel's metadata with the paired step
VGPR_SPILL_MAX = 0


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
    """The rollout loop's hot path: from a loop header to the branch back to
    it, for the loop that runs four range reductions a trip."""
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\S+):", l)
        if not m or i + 1 >= len(body) or "Loop Header" not in body[i + 1]:
            continue
        lab = m.group(1)
        end = next((j for j in range(i + 1, len(body))
                    if body[j].strip() == "s_branch " + lab), None)
        if end is None:
            continue
        ins = _instructions(body[i:end + 1])
        if sum(x.startswith("v_rndne_f64") for x in ins) == 4:
            return ins
    raise AssertionError("the rollout loop (four steps a trip) was not found")


def _metadata(text, key):
    md = text[text.index("amdhsa.kernels"):]
    for blk in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if KERNEL in name:
            return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
    raise AssertionError("no metadata for " + KERNEL)


def test_rollout_step_instruction_count(isa):
    ins = _rollout_loop(_kernel_body(isa))
    per_step = len(ins) / 4
    valu = sum(x.startswith("v_") for x in ins) / 4
    packed = sum(x.startswith("v_pk_") for x in ins) / 4
    assert per_step <= STEP_MAX, (per_step, valu)
    assert valu <= STEP_VALU_MAX, (per_step, valu)
    # (the pairs are there: sine / cosine polynomials, differences, cost,
    # dynamics)
    assert packed >= 10, packed


def test_round_kernel_spills_no_more(isa):
    assert _metadata(isa, "vgpr_spill_count") <= VGPR_SPILL_MAX
    assert _metadata(isa, "private_segment_fixed_size") == 0


def test_round_kernel_has_no_scalar_memory_writes(isa):
    ins = _instructions(_kernel_body(isa))
    bad = sorted({x for x in ins if re.match(
        r"^s_(buffer_|scratch_)?(store|atomic)|^s_dcache_(?!inv)", x)})
    assert not bad, bad
