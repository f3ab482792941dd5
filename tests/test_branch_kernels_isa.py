"""CPU-only guard on the kernels of the cartpole's other gain branches
(csrc/cartpole_branches.hip): the translation unit is compiled
to ISA with the Makefile's flags; every kernel it adds must spill no vector
register, use no scratch and hold no scalar-memory store or scalar atomic, and
the steps of the unrolled 16-step block of each branch's sweep kernel must
stay at the instruction count measured when they were written."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pddp_amd", "csrc")
NEW_KERNELS = ("sweep_n4_branch_kernel", "sweep_n4_branch_f64_kernel",
               "round_n4_branch_kernel")
# 3 branches x 2 cost masks x (2 f32 sweep forms + 1 f64 sweep + 2 round forms)
N_KERNELS = 30
BLOCK = 16
# instructions per step of sweep_n4_branch_kernel<25, true, BR> (mean over the
# unrolled block; the scheduler moves a few across step boundaries), measured
# from the ISA: 57.3 eig-clamp unbounded (BR 1), 72.5 V_zz-regularised
# unbounded (BR 2), 103.3 V_zz-regularised bounded (BR 3).  Bound: + 2.
STEP_MEASURED = {1: 57.3, 2: 72.5, 3: 103.3}
STEP_SLACK = 2.0
STEP_SPAN = 160  # longer than any step, shorter than a block boundary


def _flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*?)(?<!\\)\n", mk, re.S | re.M).group(1)
    flags = flags.replace("\\\n", " ").replace("$(ARCH)", "gfx950")
    own = re.search(r"^FLAGS_cartpole_branches := (.*)$", mk, re.M).group(1)
    return flags.split() + own.split()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the kernels cannot be compiled")
    out = tmp_path_factory.mktemp("isa") / "cartpole_branches.s"
    subprocess.check_call([hipcc] + _flags() + [
        "--cuda-device-only", "-S",
        os.path.join(CSRC, "cartpole_branches.hip"), "-o", str(out)], cwd=CSRC)
    return out.read_text()


def _new(name):
    return any(re.search(r"\d%sI" % k, name) for k in NEW_KERNELS)


def _metadata(text):
    md = text[text.index("amdhsa.kernels"):]
    rows = {}
    for blk in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if _new(name):
            rows[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))
                          for k in ("vgpr_spill_count",
                                    "private_segment_fixed_size")}
    return rows


def _bodies(text):
    lines = text.split("\n")
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\S+):", l)
        if m and _new(m.group(1)):
            end = next(k for k in range(i + 1, len(lines))
                       if lines[k].startswith(".Lfunc_end"))
            out[m.group(1)] = lines[i:end]
    return out


def _instructions(lines):
    out = []
    for l in lines:
        t = l.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        out.append(t.split()[0])
    return out


def test_new_kernels_spill_nothing_and_use_no_scratch(isa):
    rows = _metadata(isa)
    assert len(rows) == N_KERNELS, sorted(rows)
    bad = {k: v for k, v in rows.items() if any(v.values())}
    assert not bad, bad


def test_new_kernels_have_no_scalar_memory_writes(isa):
    bodies = _bodies(isa)
    assert len(bodies) == N_KERNELS, sorted(bodies)
    for name, lines in bodies.items():
        bad = sorted({x for x in _instructions(lines) if re.match(
            r"^s_(buffer_|scratch_)?(store|atomic)|^s_dcache_(?!inv)", x)})
        assert not bad, (name, bad)


@pytest.mark.parametrize("br", [1, 2, 3])
def test_branch_sweep_step_instruction_count(isa, br):
    key = "sweep_n4_branch_kernelILj25ELb1ELi%dE" % br
    body = [v for k, v in _bodies(isa).items() if key in k]
    assert len(body) == 1
    ins = _instructions(body[0])
    # a step opens with its transposes (two, and a third a few instructions
    # later in the V_zz-regularised branches)
    at = [k for k, x in enumerate(ins) if x == "ds_bpermute_b32"]
    starts = [k for n, k in enumerate(at) if n == 0 or k - at[n - 1] > 30]
    for n in range(len(starts) - BLOCK + 1):
        run = starts[n:n + BLOCK]
        steps = [ins[a:b] for a, b in zip(run, run[1:])]
        if all(len(s) < STEP_SPAN for s in steps):
            break
    else:
        raise AssertionError("the unrolled sweep block was not found")
    per_step = sum(len(s) for s in steps) / len(steps)
    print("BR", br, "instructions per step", per_step)
    assert per_step <= STEP_MEASURED[br] + STEP_SLACK, per_step
