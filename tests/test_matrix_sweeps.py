"""The matrix-core Riccati sweeps (csrc/riccati_mfma16.hpp, riccati_mfma32.hpp,
riccati_mfma32s.hpp and the texts they share) on the MI355X at EVERY state
size they admit - float32 n = 1 .. 30, float64 n = 1 .. 14 - in every form the
launcher admits there, against the float64 oracle.  n is a runtime argument of
these kernels: the operand map, the zeroed slot padding, the number of LDS-DMA
instructions per record and the lane mask of the last one all depend on it.

The batch of a launch is sweep_records.ROLES: plain, indefinite, bounds and
fault trajectories side by side, one of them inactive, B = 17 so that the last
workgroup of either form is partly empty.  Per (n, dtype): N in {1, 2, 5}
(N = 2 is shorter than riccati_mfma16's ring of three), both gain branches,
unbounded / bounded / bounded with bounds that are never active, reg in {1e-3,
1} (a plain trajectory and one with Q_uu < 0 at t = 0 at reg = 0 throughout),
every admitted variant.

The bars are the suite's own (`_check_gains`: float64 1e-9; float32 the error
against the float64 oracle at most F32_RATIO x the float32 oracle's own on
that trajectory, or the floor of the branch), no new tolerance.  Beside them:
status the oracle's on every trajectory; a step the model calls clamped has
K == 0 and k == bound - U exactly; the inactive trajectory, the guard rows
behind `gains` and the guard words behind `status` untouched; NaN in the
record's pad words (and in U when unbounded) changes no bit; a fault changes
no bit of another trajectory; `auto` is bit for bit the form the dispatcher
says it is.

The outlined BoxQP (n4::boxqp1_outlined).  QpClosed::solve sets `slow` when
iteration 0 is not done (not clamped at the start, Q positive, |g0| >= 1e-8)
and either the full step neither passes the Armijo test nor is cut short by a
bound with a decrease (`pass0 | guard`), or the iterate after it is live on a
bound.  In exact arithmetic no scalar convex QP does either: the Armijo ratio
of a step cut to the fraction a of the Newton step is a - a^2 / 2 > 0, and an
iterate on a bound has the gradient pointing outward.  Finite records reach
it through rounding only, where the decrease f1 - f0 or the product s0 g0
rounds to zero or to the wrong sign.  One such input can be placed without
knowing a kernel's roundings: two consecutive steps with the same scalars
(F_u = L_uz = 0: Q_uu = L_uu, Q_u = L_u exactly), both free.  The first ends
live and inside the box, at x2 = x1 + (newton - x1) = newton exactly; the warm
start of the second is then its own Newton point, s0 = 0, s0 g0 = 0 - the
Armijo test cannot pass, no bound cuts the step - and with Q_u ~ 4e9 the
residual |Q x + Q_u|, a rounding of Q_u, is above 1e-8 in either type, so
iteration 0 is not done: `slow` (test_sweep_records.py checks the residual in
IEEE arithmetic, fused and not).  That is trajectory `repeat`, held like the
others: the loop accepts the zero step (0 / 0 is not below the Armijo bound)
and ends on the objective, free, at the Newton point.  What cannot be seen
from outside is that a form did go through the outlined call.

Measured on the MI355X, float32, worst error against the float64 oracle per
family and gain branch over all sizes, horizons and forms, as kernel / float32
oracle on the same trajectory (`rel_err`, so relative to the largest gain of
the trajectory), and the share of the bar it uses:

  family      branch  k                   share   K                   share
  plain       eig     2.8e-6 / 1.2e-6     0.003   8.0e-7 / 2.8e-7     0.001
  plain       chol    2.0e-6 / 4.5e-8     0.065   7.5e-7 / 2.4e-7     0.025
  indefinite  eig     4.2e-7 / 7.9e-8     0.0004  1.1e-6 / 4.3e-7     0.001
  indefinite  chol    7.9e-7 / 1.3e-7     0.026   6.2e-7 / 3.1e-7     0.021
  bounds      eig     3.4e-6 / 4.1e-6     0.003   7.6e-7 / 7.6e-7     0.001
  bounds      chol    3.3e-6 / 4.1e-6     0.10    7.1e-7 / 5.1e-7     0.024

(40095 rows; per form the worst of k and K is 3.4e-6 for 14, 3.3e-6 for 15 and
auto, 2.8e-6 for 26 and 27.)  The float32 oracle is itself within 1e-7 of the
float64 one on most of these short sweeps, so F32_RATIO x its error is often
the smaller half of the bar: the floor (1e-3 eig, 3e-5 chol) is what passes
k on 1434 of the rows and K on 32, `indefinite` on the eig-clamp branch among
them (k 322 of 7260 rows, K 7).  The largest kernel error among those rows is
2.1e-6 (`indefinite`: 4.1e-7, against 4.9e-8 for the oracle on that row); the
largest ratio kernel / oracle is 2.5e3 (plain, chol, n = 5, a trajectory on
which the oracle is all but exact) and 324 on `indefinite` (eig, n = 15, form
26).  Nothing was raised.
float64: at most 2.6e-15 (n = 8, bounds, chol) against the bar of 1e-9.
"""
import sys

import numpy as np
import pytest
import torch

import oracle as orc
import sweep_records as sr
from golden_util import np_dtype, rel_err
from solver_util import TDT
# (conftest.py dumps sys.modules["test_gpu_parity"].STATS: the fp32
# bookkeeping stays in that module)
from test_gpu_parity import _check_gains, _f32_ok, F32_RATIO

pytestmark = pytest.mark.gpu

B = len(sr.ROLES)
GUARD = 2          # trajectories' worth of gains / words of status behind B
G_SENT, S_SENT = 7.0, -5
HORIZONS = (1, 2, 5)


def admitted(n, dtype, V_zz_reg):
    """(variants the launcher admits, variants it refuses, what `auto` is).
    n = 4: `auto` is the specialised sweep of riccati_n4.hpp, not a
    matrix-core form (and it leaves junk in the gains of an inactive
    trajectory, which include/pddp_hip.h allows): the 16 x 16 form is reached
    by its numbers alone."""
    auto = () if n == 4 else (0,)
    if dtype == "f64":
        return auto + (14,), (15, 26, 27), 14
    if n <= 14 or V_zz_reg:
        return auto + (14, 15), (26, 27), 15
    return (0, 14, 15, 26, 27), (), 27


class Launcher:
    """The packed records of one (n, N, dtype) batch on the device - as
    pddp_pack_records wrote them, with NaN in what must not be read, and with
    the faults removed - and pddp_riccati_backward_variant on them."""

    def __init__(self, n, N, dtype):
        from pddp_amd import _native
        self.nat, self.n, self.N, self.dt = _native, n, N, TDT[dtype]
        self.npd = np_dtype(dtype)
        self.rec, good = sr.launch_batch(n, N, self.npd)
        self.lay = _native.record_layout(n, 1)
        self.stream = _native.stream_handle(torch.device("cuda"))
        self.clean, self.good = self._pack(self.rec), self._pack(good)
        oU, S = self.lay.o_U, self.lay.stride
        assert oU + 1 == 2 * n * n + 3 * n + 3 and S == (oU + 4) // 4 * 4
        self.pad = self.clean.clone()
        self.pad[:, :, oU + 1:] = float("nan")
        self.pad_U = self.pad.clone()
        self.pad_U[:, :, oU] = float("nan")
        act = np.ones(B, np.uint8)
        act[sr.INACTIVE] = 0
        self.active = torch.as_tensor(act).cuda()

    def _pack(self, rec):
        p = self.nat.ptr
        dev = [torch.as_tensor(np.ascontiguousarray(rec[nm])).cuda()
               for nm in sr.ARG_NAMES + ("U",)]
        buf = torch.empty(B, self.N + 1, self.lay.stride, dtype=self.dt,
                          device="cuda")
        self.nat.call("pddp_pack_records", self.dt, B, self.N, self.n, 1,
                      *[p(d) for d in dev], p(buf), self.stream)
        return buf

    def run(self, buf, variant, V_zz_reg, bounds, reg):
        """(return code, gains (B + GUARD, N, 1 + n), status (B + GUARD,))."""
        p = self.nat.ptr
        gains = torch.full((B + GUARD, self.N, self.lay.gain_stride), G_SENT,
                           dtype=self.dt, device="cuda")
        status = torch.full((B + GUARD,), S_SENT, dtype=torch.int32,
                            device="cuda")
        regv = torch.tensor([sr.reg_of(b, reg) for b in range(B)],
                            dtype=torch.float64, device="cuda")
        lo = hi = None
        if bounds is not None:
            lo = torch.full((1,), bounds[0], dtype=self.dt, device="cuda")
            hi = torch.full((1,), bounds[1], dtype=self.dt, device="cuda")
        rc = self.nat.call_rc(
            "pddp_riccati_backward_variant", self.dt, B, self.N, self.n, 1,
            p(buf), p(lo), p(hi), p(regv), int(V_zz_reg), p(self.active),
            p(gains), p(status), self.stream, variant)
        torch.cuda.synchronize()
        return rc, gains.cpu().numpy(), status.cpu().numpy()


def oracle_rows(L, V_zz_reg, bounds, reg):
    """Per trajectory (k, K, status, args, kw) of the oracle in the run's
    dtype; None for the inactive one."""
    o = orc.load(L.npd)
    rows = []
    for b in range(B):
        if b == sr.INACTIVE:
            rows.append(None)
            continue
        args, kw = sr.oracle_call(L.rec, b, V_zz_reg, bounds, reg)
        rows.append(o.backward(*args, **kw) + (args, kw))
    return rows


def same_bits(a, b):
    """Bit for bit (a faulty trajectory's NaN gains included)."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def bounds_name(bounds):
    return "no" if bounds is None else "wide" if bounds[1] == sr.WIDE else "box"


@pytest.mark.parametrize("n,dtype", [(n, "f32") for n in range(1, 31)] +
                         [(n, "f64") for n in range(1, 15)])
def test_every_size_and_form_vs_oracle(n, dtype):
    """Everything of the module docstring at one (n, dtype)."""
    stats = sys.modules["test_gpu_parity"].STATS
    first, worst64 = len(stats), {}
    for N in HORIZONS:
        L = Launcher(n, N, dtype)
        models = {}
        # the conditions on the inputs: status 0, clamped Q_uu at the chosen
        # steps, margins, the three outcomes, the exact steps
        assert sr.broken_conditions(L.rec, N, models) == []
        for V_zz_reg, bounds, reg in sr.CONFIGS:
            key = (n, dtype, N, V_zz_reg, bounds, reg)
            rows = oracle_rows(L, V_zz_reg, bounds, reg)
            model = models[(V_zz_reg, bounds, reg)]
            variants, refused, auto_is = admitted(n, dtype, V_zz_reg)
            unread = L.pad if bounds is not None else L.pad_U
            out = {}
            for v in variants:
                rc, g, st = L.run(L.clean, v, V_zz_reg, bounds, reg)
                assert rc == 0, (key, v)
                out[v] = (g, st)
                check_launch(L, g, st, rows, model, bounds, key + (v,),
                             worst64)
                # nothing read that should not be
                rc, g2, st2 = L.run(unread, v, V_zz_reg, bounds, reg)
                assert rc == 0 and same_bits(st2, st) and same_bits(g2, g), (
                    key, v, "pad words / U read")
                # the faults move no bit of another trajectory
                rc, g3, st3 = L.run(L.good, v, V_zz_reg, bounds, reg)
                others = [b for b in range(B + GUARD) if b not in sr.FAULTS]
                assert rc == 0 and same_bits(st3[others], st[others]) and \
                    same_bits(g3[others], g[others]), (key, v)
                assert st3[list(sr.FAULTS)].tolist() == [0, 0], (key, v)
            if 0 in out:
                assert same_bits(out[0][0], out[auto_is][0]) and \
                    same_bits(out[0][1], out[auto_is][1]), (key, "auto")
            for v in refused:
                rc, g, st = L.run(L.clean, v, V_zz_reg, bounds, reg)
                assert rc == L.nat.E_UNSUPPORTED, (key, v)
                assert (g == G_SENT).all() and (st == S_SENT).all(), (key, v)
    report(n, dtype, stats[first:], worst64)


def family(role):
    return "indefinite" if role in ("indef_last", "indef_t0", "small_quu") \
        else "plain" if role == "plain" else "bounds"


def report(n, dtype, rows, worst64):
    """The figures of the module docstring, printed: per family and branch
    the largest error against the float64 oracle with the float32 oracle's
    own on the same trajectory, and how many rows only the floor passes."""
    for (fam, V), e in sorted(worst64.items()):
        print("SWEEPS n=%d f64 %s %s worst %.3g of 1e-9" % (
            n, fam, "chol" if V else "eig", e))
    by = {}
    for r in rows:
        by.setdefault((family(r["role"]), r["V_zz_reg"]), []).append(r)
    for (fam, V), rs in sorted(by.items()):
        wk = max(rs, key=lambda r: r["k_hip"])
        wK = max(rs, key=lambda r: r["K_hip"])
        floor_only = sum(
            1 for r in rs for q in "kK"
            if _f32_ok(r[q + "_hip"], r[q + "_o32"], V) and
            r[q + "_hip"] > F32_RATIO * r[q + "_o32"])
        print("SWEEPS n=%d f32 %s %s k %.3g/%.3g K %.3g/%.3g "
              "floor-only %d of %d" % (
                  n, fam, "chol" if V else "eig", wk["k_hip"], wk["k_o32"],
                  wK["K_hip"], wK["K_o32"], floor_only, 2 * len(rs)))


def check_launch(L, g, st, rows, model, bounds, key, worst64):
    n, N = L.n, L.N
    dtype = "f64" if L.npd is np.float64 else "f32"
    V_zz_reg, reg, variant = key[3], key[5], key[6]
    # guards and the inactive trajectory
    assert (g[B:] == G_SENT).all() and (st[B:] == S_SENT).all(), key
    assert (g[sr.INACTIVE] == G_SENT).all() and st[sr.INACTIVE] == S_SENT, key
    k, K = g[:B, :, :1], g[:B, :, 1:].reshape(B, N, 1, n)
    for b in range(B):
        if b == sr.INACTIVE:
            continue
        kr, Kr, s_or, args, kw = rows[b]
        assert st[b] == s_or, (key, b, sr.ROLES[b], st[b], s_or)
        if sr.fault_like(b, V_zz_reg):
            continue
        assert s_or == sr.BWD_OK, (key, b)
        if dtype == "f64":
            fv = (family(sr.ROLES[b]), bool(V_zz_reg))
            worst64[fv] = max(worst64.get(fv, 0.0), rel_err(k[b], kr),
                              rel_err(K[b], Kr))
        assert _check_gains(
            dtype, k[b], K[b], kr, Kr, args, kw, test="matrix_sweeps", n=n,
            N=N, variant=variant, V_zz_reg=bool(V_zz_reg),
            bounded=bounds_name(bounds), reg=sr.reg_of(b, reg), b=b,
            role=sr.ROLES[b]), (key, b, "the float64 oracle fails")
        if bounds is None:
            continue
        # exact facts of the steps the model calls clamped
        m = model[b]
        U = L.rec["U"][b, :, 0]
        for t in range(N):
            if m["outcome"][t] == sr.FREE:
                continue
            bound = bounds[0] if m["outcome"][t] == sr.LOWER else bounds[1]
            assert (K[b, t] == 0).all(), (key, b, t, "K of a clamped step")
            assert k[b, t, 0] == L.npd(bound) - U[t], (key, b, t, k[b, t, 0])
        if sr.ROLES[b] == "on_umin" and bounds[1] != sr.WIDE:
            t0 = sr.exact_step(N)
            assert m["outcome"][t0] == sr.LOWER and k[b, t0, 0] == 0, (key, b)
