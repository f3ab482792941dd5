"""CPU-only guard on what the round kernel's two chains issue besides their
steps' arithmetic.  `round_n4_kernel<25,
true>` is compiled to ISA with the Makefile's flags, as the other ISA tests do,
and

* the rollout step stays at the instruction count this reached, with the
  quadrant of its sine / cosine selected bitwise: one `v_cndmask` per step
  (the action's clamp), where the parent had three behind a compare;
* the rollout loops wait for their LDS row no more often than the parent's:
  one `s_waitcnt lgkmcnt(0)` per step was built, measured inside the spread
  of the box and not kept, so these pins stand at the parent's figures;
* the sweep's block loop issues, on its shortest way round, no more
  instructions outside the sixteen steps than it did (its boundary was
  budgeted and not rebuilt);
* the sweep step stays at the count this reached, without an `s_nop`.

Beside each pin: the parent's figure, from these counters on the parent's
source."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pddp_amd", "csrc")
KERNEL = "round_n4_kernelILj25ELb1E"
BLOCK = 16        # steps of the sweep's unrolled block
STEP_SPAN = 120   # longer than a sweep step, shorter than a block boundary

# s_waitcnt per trip of the four-step loop, of its remainder loop, and of the
# retry rollout's two loops: the parent's figures (one per step - 4, 1, 4, 1,
# every one lgkmcnt(0) - was built and not kept)
TRIP_WAITS = 15           # parent: 15 (lgkmcnt(2), (1), (0) staged per step)
REMAINDER_WAITS = 3       # parent: 3
RETRY_TRIP_WAITS = 9      # parent: 9
RETRY_REMAINDER_WAITS = 3  # parent: 3
ROLLOUT_STEP_MAX = 81.75  # parent: 82.75 (80.0 with one wait per step)
ROLLOUT_CNDMASK = 1.0     # parent: 3.0 per step
# loop header -> the block's first transposes, plus the block's last
# transposes -> the back branch, the fewest instructions any path issues.  The
# boundary itself was not rebuilt: the parent's figure less the s_nop that
# left the sixteenth step's end, which lies behind the last transposes
BOUNDARY_MAX = 123        # parent: 124 (48 + 76)
# (over the fifteen spans from one step's transposes to the next's, as
# tests/test_sweep_step_isa.py counts: thirteen of 81, one of 83, one of 76)
SWEEP_STEP_MAX = 1209 / 15  # 80.6; parent: 1238 / 15 = 82.53 (thirteen of 83)
SWEEP_NOP_MAX = 0.0       # parent: 29 / 15 = 1.93


def _flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS \?= (.*?)(?<!\\)\n", mk, re.S | re.M).group(1)
    flags = flags.replace("\\\n", " ").replace("$(ARCH)", "gfx950")
    own = re.search(r"^FLAGS_round_n4 := (.*)$", mk, re.M).group(1)
    return flags.split() + own.split()


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    """The kernel's lines, label to end of function."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.fail("hipcc not found: the round kernel cannot be compiled")
    out = tmp_path_factory.mktemp("isa") / "round_n4.s"
    subprocess.check_call([hipcc] + _flags() + [
        "--cuda-device-only", "-S", os.path.join(CSRC, "round_n4.hip"),
        "-o", str(out)], cwd=CSRC)
    lines = out.read_text().split("\n")
    start = next(i for i, l in enumerate(lines)
                 if re.match(r"^_Z\S*%s\S*:" % KERNEL, l))
    end = next(i for i in range(start + 1, len(lines))
               if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def _is_instruction(line):
    t = line.strip()
    return bool(t) and not t.startswith((";", ".")) and not t.endswith(":")


def _instructions(lines):
    """(mnemonic, operands) of every instruction line."""
    out = []
    for l in lines:
        if _is_instruction(l):
            parts = l.split(";")[0].split(None, 1)
            out.append((parts[0], parts[1].strip() if len(parts) > 1 else ""))
    return out


def _loops(body):
    """Every loop the compiler marks, in layout order: (label, lines from its
    header to its last branch back to the header)."""
    out = []
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\S+):", l)
        if not m or i + 1 >= len(body) or "Loop Header" not in body[i + 1]:
            continue
        back = [j for j in range(i + 1, len(body)) if re.match(
            r"\s*s_c?branch\S*\s+%s\s*$" % re.escape(m.group(1)), body[j])]
        if back:
            out.append((m.group(1), body[i:back[-1] + 1]))
    return out


def _rollout_loops(body):
    """The search's rollout loops, in layout order: the four-steps-a-trip loop
    (four range reductions, `v_rndne_f64`, a trip: the first such loop is the
    rollout's, as in tests/test_round_rollout_isa.py, the second the retry
    rollout's) and, behind each, its remainder loop (one a trip)."""
    loops = [(lab, _instructions(ls)) for lab, ls in _loops(body)]
    rnd = [sum(op.startswith("v_rndne_f64") for op, _ in ins)
           for _, ins in loops]
    trips = [k for k, n in enumerate(rnd) if n == 4]
    assert len(trips) == 2, "rollout and retry rollout: %r" % (rnd,)
    out = []
    for k in trips:
        rem = next((r for r in range(k + 1, len(loops)) if rnd[r] == 1), None)
        assert rem is not None, "no remainder loop behind " + loops[k][0]
        out += [loops[k][1], loops[rem][1]]
    return out  # trip, remainder, retry trip, retry remainder


def _waits(ins):
    return [args for op, args in ins if op == "s_waitcnt"]


def _sweep_block(body):
    """(the block loop's lines, the line indices - within them - of the first
    transpose of each of the unrolled block's sixteen steps and of the last
    transpose of the sixteenth)."""
    for _, ls in _loops(body):
        at = [k for k, l in enumerate(ls)
              if _is_instruction(l) and l.split()[0] == "ds_bpermute_b32"]
        if len(at) < 2 * BLOCK:
            continue
        n_ins = {k: n for n, k in enumerate(
            k for k, l in enumerate(ls) if _is_instruction(l))}
        # a step's two transposes are issued back to back
        starts = [k for n, k in enumerate(at)
                  if n == 0 or n_ins[k] - n_ins[at[n - 1]] > 4]
        for n in range(len(starts) - BLOCK + 1):
            run = starts[n:n + BLOCK]
            if all(n_ins[b] - n_ins[a] < STEP_SPAN
                   for a, b in zip(run, run[1:])):
                last = max(k for k in at if k - run[-1] <= 4 and k >= run[-1])
                return ls, run, last
    raise AssertionError("the unrolled sweep block was not found")


def _shortest(ls, src, dst):
    """The fewest instructions issued on a path through the loop's control
    flow from line `src` (counted) to line `dst` (not counted)."""
    label_at = {}
    for k, l in enumerate(ls):
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            label_at[m.group(1)] = k
    dist = {src: 0}
    todo = collections.deque([src])
    while todo:  # (0 / 1 weights: a deque keeps the order)
        k = todo.popleft()
        if k == dst:
            return dist[k]
        d = dist[k]
        nxt = []
        if _is_instruction(ls[k]):
            d += 1
            op, _, arg = ls[k].split(";")[0].strip().partition(" ")
            if op.startswith(("s_branch", "s_cbranch")):
                tgt = label_at.get(arg.strip())
                if tgt is not None:
                    nxt.append(tgt)
            if op != "s_branch":
                nxt.append(k + 1)
        else:
            nxt.append(k + 1)
        for j in nxt:
            if j < len(ls) and (j not in dist or d < dist[j]):
                dist[j] = d
                if d == dist[k]:
                    todo.appendleft(j)
                else:
                    todo.append(j)
    raise AssertionError("no path from line %d to line %d" % (src, dst))


def test_rollout_loops_wait_no_more_often(body):
    trip, rem, retry, retry_rem = _rollout_loops(body)
    for ins, most in ((trip, TRIP_WAITS), (rem, REMAINDER_WAITS),
                      (retry, RETRY_TRIP_WAITS),
                      (retry_rem, RETRY_REMAINDER_WAITS)):
        w = _waits(ins)
        print("s_waitcnt:", w)
        assert len(w) <= most, w
        # (LDS only: no wait in these loops names another counter)
        assert all(re.fullmatch(r"lgkmcnt\(\d+\)", x) for x in w), w


def test_rollout_step_count(body):
    trip = _rollout_loops(body)[0]
    cnd = sum(op.startswith("v_cndmask") for op, _ in trip) / 4
    print("rollout step: %.2f, v_cndmask %.2f" % (len(trip) / 4, cnd))
    assert len(trip) / 4 <= ROLLOUT_STEP_MAX
    assert cnd <= ROLLOUT_CNDMASK
    assert sum(op == "s_nop" for op, _ in trip) == 0


def test_sweep_block_boundary(body):
    ls, run, last = _sweep_block(body)
    head = _shortest(ls, 0, run[0])
    # (from behind the last transpose to the loop's closing branch, counted)
    tail = _shortest(ls, last + 1, len(ls) - 1) + 1
    print("block boundary: %d + %d" % (head, tail))
    assert head + tail <= BOUNDARY_MAX, (head, tail)


def test_sweep_step_count_and_padding(body):
    ls, run, _ = _sweep_block(body)
    steps = [_instructions(ls[a:b]) for a, b in zip(run, run[1:])]
    per_step = sum(len(s) for s in steps) / len(steps)
    nops = sum(op == "s_nop" for s in steps for op, _ in s) / len(steps)
    print("sweep step: %.2f, s_nop %.2f" % (per_step, nops))
    assert per_step <= SWEEP_STEP_MAX, (per_step, nops)
    assert nops <= SWEEP_NOP_MAX, (per_step, nops)
