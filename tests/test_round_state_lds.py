"""CPU-only guard on the static LDS of the one-launch round.  With several
rounds per launch the kernel keeps one record per trajectory (accept.hpp
RoundState), the action's bounds and the step sizes in STATIC LDS, next to the
search's decisions; the dynamic size is the plan's (tests/test_nominal_plan.py
pins it) and the two together must fit a CU's 160 KB at the longest horizons
the launch serves.  The kernels are compiled to ISA with the Makefile's flags,
as tests/test_round_rollout_isa.py does, and

* every `round_n4_kernel` / `round_n4_branch_kernel` instantiation has at most
  128 + 960 bytes of static LDS, spills no vector register, and fits 163 840
  bytes together with the plan's dynamic size at N = 123 with the carried rows
  and at N = 127 without;
* in `round_n4_kernel<25, true>` no wait on the vector memory counter sits
  between the round loop's header and the sweep's first barrier outside a
  block that issued a load itself (the launch's first round), and in the
  search's short tail none follows the first store: on gfx950 loads and stores
  return through one in-order counter, and such a wait is a wait for every
  store the last round's tail issued."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pddp_amd", "csrc")
STATIC_MAX = 128 + 960
CU_LDS = 163840
FLAGSHIP = "round_n4_kernelILj25ELb1E"


def _round_lds(N, carry):  # n4_nominal_plan's, as tests/test_nominal_plan.py
    return 16 * (6880 + 24 * N + (340 if carry else 0))


def _flags(unit):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*?)(?<!\\)\n", mk, re.S | re.M).group(1)
    flags = flags.replace("\\\n", " ").replace("$(ARCH)", "gfx950")
    own = re.search(r"^FLAGS_%s := (.*)$" % unit, mk, re.M).group(1)
    return flags.split() + own.split()


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the round kernels cannot be compiled")
    d = tmp_path_factory.mktemp("isa")
    procs = []
    for unit in ("round_n4", "cartpole_branches"):
        procs.append(subprocess.Popen([hipcc] + _flags(unit) + [
            "--cuda-device-only", "-S", os.path.join(CSRC, unit + ".hip"),
            "-o", str(d / (unit + ".s"))], cwd=CSRC))
    assert all(p.wait() == 0 for p in procs)
    return {u: (d / (u + ".s")).read_text()
            for u in ("round_n4", "cartpole_branches")}


def _round_kernels(text):
    """name -> metadata block of every one-launch round kernel."""
    md = text[text.index("amdhsa.kernels"):]
    out = {}
    for blk in md.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "round_n4_kernel" in name or "round_n4_branch_kernel" in name:
            out[name] = blk
    return out


def _field(blk, key):
    return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))


def test_static_lds_fits_and_nothing_spills(isa):
    kernels = {}
    for text in isa.values():
        kernels.update(_round_kernels(text))
    # two cost masks x one or several rounds, for each of the four branches
    assert len(kernels) == 16, sorted(kernels)
    for name, blk in kernels.items():
        static = _field(blk, "group_segment_fixed_size")
        assert static <= STATIC_MAX, (name, static)
        assert static + _round_lds(123, True) <= CU_LDS, (name, static)
        assert static + _round_lds(127, False) <= CU_LDS, (name, static)
        assert _field(blk, "vgpr_spill_count") == 0, name


def _kernel_body(text):
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines)
                 if re.match(r"^_Z\S*%s\S*:" % FLAGSHIP, l))
    end = next(i for i in range(start + 1, len(lines))
               if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def _is_label(line):
    return bool(re.match(r"^(\.LBB\S+:|; %bb\.)", line))


def test_no_store_wait_at_the_start_of_a_round(isa):
    body = _kernel_body(isa["round_n4"])
    head = next(i for i, l in enumerate(body) if "Loop Header: Depth=1" in l)
    first_barrier = next(i for i in range(head, len(body))
                         if body[i].strip() == "s_barrier")
    loaded = False  # a global load earlier in this basic block
    waits = 0
    for l in body[head:first_barrier]:
        if _is_label(l):
            loaded = False
        t = l.strip()
        if t.startswith("global_load"):
            loaded = True
        if t.startswith("s_waitcnt") and "vmcnt" in t:
            waits += 1
            assert loaded, t
    assert waits <= 1  # (the first round's terminal state, from global memory)


def test_nothing_waits_for_the_tails_stores(isa):
    body = _kernel_body(isa["round_n4"])
    end = next(i for i, l in enumerate(body) if l.strip() == "s_endpgm")
    bars = [i for i, l in enumerate(body[:end]) if l.strip() == "s_barrier"]
    # the last three barriers of the round: the decisions' hand-over, the end
    # of the tail, the round loop's
    tail = [l.strip() for l in body[bars[-3]:bars[-2]]]
    assert sum(t.startswith("global_load_dwordx4") for t in tail) == 4, \
        "the short tail (four rows requested per lane) was not found"
    first_store = next(i for i, t in enumerate(tail)
                       if t.startswith("global_store"))
    assert sum(t.startswith("global_store") for t in tail) >= 8
    late = [t for t in tail[first_store:]
            if t.startswith("s_waitcnt") and "vmcnt" in t]
    assert late == []
    # and nothing after the tail, up to the round loop's barrier
    assert [l for l in body[bars[-2]:bars[-1]] if "vmcnt" in l] == []
