"""Device-resident batched iLQR engine: owns the HBM buffers of B independent
trajectories and drives the HIP kernels of libpddp_hip.so through the C ABI.

One `round()` = what the reference does in one pass of the retry loop of
`iLQRController.step` (pddp/controllers/ilqr.py:183-235) for EVERY live
trajectory at once:

    derivatives (only trajectories whose nominal changed, ilqr.py:198-209)
    -> backward Riccati sweep (ilqr.py:125-139)
    -> line search over A step sizes + costs (ilqr.py:148-160)
    -> accept / reject, mu schedule, fit-loop bookkeeping (ilqr.py:161-181,
       298-314)

with per-trajectory masks instead of Python control flow, so a round is a
fixed launch sequence with no host synchronisation.

The launches of a round are decided in one place: `ILQRSolver._plan()` names
the sequence a round tries FIRST, round() demotes it when an entry point
answers PDDP_E_UNSUPPORTED, and the `_*_done()` helpers note what a
launch did in the plan's inputs, the tri-states `_one_launch`, `_nominal_sweep`
(None at first only where that sweep applies and pays) and `_fused`: None
untried / allowed, False forbidden or found unsupported, True has applied.
Assign one between two rounds to force a path.  "nominal" below: the variant
is 0 and neither `_nominal_sweep` nor `_fused` is False.

    sequence          launches                        tried first when
    ----------------  ------------------------------  ------------------------
    one_launch        pddp_round_nominal_f32          nominal, `_one_launch`
                                                      is not False, no
                                                      search_events
    nominal+fused     pddp_sweep_nominal,             nominal (and what a
                      pddp_search_accept, L = NULL    refused one_launch
                                                      becomes)
    nominal+separate  pddp_sweep_nominal,             never: a nominal+fused
                      line_search, accept; records    whose search was refused
                      by derivs from then on          (> 16 step sizes)
    records+fused     [sync_records] [derivs]         not nominal (or sweep
                      backward, pddp_search_accept    refused); no plugin,
                                                      `_fused` is not False
    records+separate  derivs, backward, line_search,  plugin, `_fused` is
                      accept                          False, search refused, or
                                                      a per-trajectory problem

`set_batch_problem()` gives every trajectory its own model parameters and
goals (`batch_table`): derivs, nominal rollout and line search are then the
pddp_*_batch_* entry points, and every round is records+separate.

`set_reference()` gives every trajectory a goal per TIME STEP (`reference`,
read from row `ref_start` on): derivs and line search are then the
pddp_*_track_* entry points, every round is records+separate, and
`mpc_closed_loop()` moves the window by one row per control step.

`set_batch_weights()` gives every trajectory its own diagonals of Q, Q_term
and R (`batch_weights`): derivs and line search are then the pddp_*_weighted_*
entry points, with the table's address or NULL, and every round is
records+separate.

Weights and a reference are held at once where the second setter is told to
keep the first (`set_reference(keep_weights=True)`,
`set_batch_weights(keep_reference=True)`): derivs and line search are then the
pddp_*_track_weighted_* entry points (csrc/goal_kernels.hpp), with the table's
address or NULL, the reference window and the weights; every round is
records+separate.  Without the keyword the second setter refuses.
"""
import contextlib
import ctypes
import functools
import numbers
import types

import torch

from .. import _native
from ..utils.encoding import StateEncoding

BRANCH_EIG, BRANCH_CHOLESKY = 0, 1
ONE_LAUNCH, NOMINAL_FUSED, RECORDS_FUSED, RECORDS_SEPARATE = (
    "one_launch", "nominal+fused", "records+fused", "records+separate")


def _on_device(fn):
    """The C ABI takes a stream handle and launches on the CURRENT device: a
    solver that lives on another GPU makes its device current for the call."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        if torch.cuda.current_device() == self.device.index:
            return fn(self, *args, **kwargs)
        with torch.cuda.device(self.device):
            return fn(self, *args, **kwargs)
    return wrapped


def fit_alphas(dtype, device):
    """ilqr.py:282 (the schedule `fit` actually uses):
    `1.025**(-torch.arange(10.0)**2).to(**tensor_opts)` - the `.to` binds to
    the parenthesised exponent, so the (integer-valued) exponents are cast and
    the power is taken in the RUN's dtype: a float64 run sees float64 step
    sizes.  Formed on the host so that every device sees the same bits."""
    return (1.025 ** (-torch.arange(10.0) ** 2).to(dtype)).to(device)


def mpc_alphas(dtype, device):
    """ilqr.py:116,189 default of `step` (used by forward(mpc=True))."""
    return (10.0 ** torch.linspace(0, -3, 11)).to(dtype=dtype, device=device)


class ILQRSolver(object):

    def __init__(self, problem, B, N, dtype, device, u_min=None, u_max=None,
                 alphas=None, branch=BRANCH_EIG, plugin=None, n=None, m=None,
                 kernel_variant=0):
        """`problem`: ctypes PddpProblem of a sample problem (everything in
        HIP), or None together with `plugin` (plugin.TorchProblem) and the
        encoded state / action sizes `n`, `m`: derivatives and the line search
        then come from the plugin modules, the sweep / accept stay HIP."""
        self.problem = problem
        self.plugin = plugin
        self.B, self.N = int(B), int(N)
        if problem is not None:
            self.n, self.m = problem.encoded_size, problem.action_size
        else:
            self.n, self.m = int(n), int(m)
        self.dtype, self.device = dtype, torch.device(device)
        if self.device.type != "cuda":
            raise _native.NativeError(
                "ILQRSolver needs a GPU device (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lay = _native.record_layout(self.n, self.m)
        self.branch = branch
        # backward-sweep kernel of round(): 0 = auto (f32: approximate
        # v_rcp / v_sqrt kernels), `exact_variant()` = the IEEE-division twins
        self.kernel_variant = int(kernel_variant)
        opts = dict(dtype=dtype, device=self.device)
        B, N, n, m = self.B, self.N, self.n, self.m
        S, gs = self.lay.stride, self.lay.gain_stride
        self.u_min = None if u_min is None else \
            torch.as_tensor(u_min).to(**opts).reshape(m).contiguous()
        self.u_max = None if u_max is None else \
            torch.as_tensor(u_max).to(**opts).reshape(m).contiguous()
        self.alphas = (fit_alphas(dtype, self.device) if alphas is None
                       else torch.as_tensor(alphas).to(**opts).contiguous())
        A = self.A = self.alphas.numel()
        self.z0 = torch.zeros(B, n, **opts)
        self.Z = torch.zeros(B, N + 1, n, **opts)
        self.U = torch.zeros(B, N, m, **opts)
        self._rec = torch.zeros(B, N + 1, S, **opts)
        self.L = torch.zeros(B, N + 1, **opts)
        self.J_opt = torch.zeros(B, **opts)
        self.gains = torch.zeros(B, N, gs, **opts)
        self.gains_acc = torch.zeros(B, N, gs, **opts)
        # candidates, time-major like the reference's Z_new / U_new
        self.Zc = torch.zeros(B, N + 1, A, n, **opts)
        self.Uc = torch.zeros(B, N, A, m, **opts)
        self.Jc = torch.zeros(B, A, **opts)
        i32 = dict(dtype=torch.int32, device=self.device)
        u8 = dict(dtype=torch.uint8, device=self.device)
        f64 = dict(dtype=torch.float64, device=self.device)
        self.bwd_status = torch.zeros(B, **i32)
        self.state = torch.zeros(B, **i32)
        self.iter = torch.zeros(B, **i32)
        self.mu = torch.zeros(B, **f64)
        self.delta = torch.full((B,), 2.0, **f64)
        self.active = torch.zeros(B, **u8)
        self.fresh = torch.zeros(B, **u8)
        # PDDP_LIVE_SHARDS counters: running total of "still live after its
        # attempt" since the last reset (bench.py's unit accounting; the fit
        # loop itself looks at `active`)
        self.n_live = torch.zeros(256, **i32)
        self._graph = None  # (key, graph of a round [, round without derivs])
        self._rollout_graph = None
        self._graph_nominal = False  # the captured round writes no records
        self._model_gen = self._cost_gen = None  # the plugin graphs' own
        self.graph_rollout = False  # nominal rollout of a plugin as a hipGraph
        self._fused = self._one_launch = None  # _plan()'s inputs (docstring)
        self._round_args = None  # _buffers()'s cache
        self._jscr = torch.zeros_like(self.J_opt)  # sync_records()'s J_opt
        self.last_search_timed = None
        # int64 [ceil(B / 16)][2] or None: pddp_round_nominal_f32's phase clock
        self.phase_ticks = None
        # False after a search launch that dropped the candidates (large
        # batches without records, pddp_search_candidates): `Zc`, `Uc` are then
        # scratch - only `Jc` and the nominal are results of that round.  (In
        # the record-free rounds of the sample problems `Uc` is never written:
        # the winner's actions are re-evaluated, include/pddp_hip.h)
        self.candidates_kept = True
        self._derivs_due = True
        # (with the sweep from the nominal `rec` is not kept up to date by
        # round(); `sync_records()` brings it up to date for whoever reads it)
        self._nominal_sweep = None if (self._nominal_sweep_possible() and
                                       self._nominal_sweep_pays()) else False
        self._rec_stale = False
        self._pp = None if problem is None else ctypes.addressof(problem)
        # [B][_native.BATCH_ROW] per-trajectory parameters and goals, or None:
        # set_batch_problem()
        self.batch_table = None
        # [B][L][_native.REF_ROW] goals per time step, or None, and the row
        # horizon index 0 reads: set_reference()
        self.reference = None
        self.ref_start = 0
        # [B][n] the plant's state behind the observation in z0, while an
        # mpc_closed_loop(obs_std=) trial can be continued; else None
        self.x_true = None
        # [B][_native.WEIGHT_ROW] per-trajectory diagonals of Q, Q_term, R, or
        # None: set_batch_weights()
        self.batch_weights = None

    def _nominal_sweep_possible(self):
        """pddp_sweep_nominal_*'s domain (include/pddp_hip.h).  At every
        batch: from 12288 trajectories on the quad sweep on records is the
        faster SWEEP, but the round without records is still shorter (no 79 MB
        of records written by the line search and read back)."""
        # include/pddp_problem.h: PDDP_MODEL_CARTPOLE = 1,
        # PDDP_ENC_IGNORE_UNCERTAINTY = 4
        if not (self.plugin is None and self.problem is not None and
                self.m == 1 and self.problem.encoding == 4 and
                self.kernel_variant == 0):
            return False
        if self.problem.model == 1:  # cartpole: csrc/riccati_n4_elem.hpp
            # (f32, and - round 5 - the same mapping in f64; all four gain
            # branches: eig-clamp / V_zz-regularised, bounded or not)
            return (self.n == 4 and
                    (self.u_min is None) == (self.u_max is None))
        # pendulum (3), double cartpole (2): csrc/riccati_mfma16_nominal.hpp -
        # f32 and f64, both branches, bounded or not
        return self.problem.model in (2, 3) and \
            (self.u_min is None) == (self.u_max is None)

    def _nominal_sweep_pays(self):
        """Where round() takes the sweep from the nominal by itself (measured,
        tools/nominal_round_time.py, 4096 trajectories): cartpole f32 1.37x
        the round on records (bounded eig-clamp; the other gain branches,
        tools/cartpole_branch_round_time.py: two launches 1.48x - 1.61x f32,
        1.25x - 1.54x f64, the one-launch round 1.8x - 2.0x),
        pendulum f32 1.04x; pendulum f64 0.95x and the
        double cartpole 0.65x (f32) / 0.74x (f64) - its record is ~1500
        instructions against a step of ~150, and a block of them in LDS leaves
        one workgroup per CU.  `sweep_nominal()` itself works wherever
        `_nominal_sweep_possible()` says so; set `_nominal_sweep = None` to
        make round() use it regardless."""
        return self.problem.model == 1 or (self.problem.model == 3 and
                                           self.dtype == torch.float32)

    # parameters of each sample model, dt included (include/pddp_problem.h)
    _PARAM_COUNT = {1: 6, 2: 8, 3: 5, 4: 3}

    def _batch_problem_possible(self):
        """The domain of the pddp_*_batch_* entry points (check_problem() of
        csrc/problem_args.hpp): a sample model under IGNORE_UNCERTAINTY."""
        return (self.plugin is None and self.problem is not None and
                self.problem.encoding == 4 and
                self.problem.model in self._PARAM_COUNT)

    @_on_device
    def set_batch_problem(self, params=None, x_goal=None, u_goal=None):
        """Per-trajectory model parameters and goals: `params` [B][P] (P: the
        model's parameter count, dt first, in `native_problem`'s order),
        `x_goal` [B][na] in augmented coordinates, `u_goal` [B][m]; a block
        not given stays the shared problem's.  Q, Q_term, R, the model, the
        encoding and the action bounds stay shared.

        Builds `batch_table` ([B][20], include/pddp_hip.h); from then on the
        nominal rollout, the derivative records and the line search read
        trajectory b's row, and every round is derivs, backward, line_search,
        accept (`records+separate`): the sweep from the nominal, the
        one-launch round and the fused search take one problem for the batch.
        The current nominal `Z` is NOT rolled out again: call
        `nominal_rollout()` / `set_nominal()` after changing the table."""
        self._need_sample_problem("set_batch_problem")
        self.batch_table = self._write_fields(
            "set_batch_problem", self._shared_row().repeat(self.B, 1),
            self._row_blocks(params, x_goal, u_goal)).contiguous()
        self._problem_changed(separate=True)

    def _need_sample_problem(self, what):
        if not self._batch_problem_possible():
            raise _native.NativeError(
                "%s needs a sample problem under IGNORE_UNCERTAINTY on the "
                "native path (no plugin, no Gaussian encoding)" % what)

    def _check_active(self, what, active):
        if active is not None and not (
                torch.is_tensor(active) and active.dtype == torch.uint8 and
                active.device == self.device and
                tuple(active.shape) == (self.B,)):
            raise _native.NativeError(
                "%s: active must be a uint8 tensor of shape (%d,) on %s" % (
                    what, self.B, self.device))

    def _out(self, masked, *shape, dtype=None, fill=float("nan")):
        """An output the kernels write: `fill`ed ahead of the launch where a
        mask leaves rows of it unwritten."""
        opts = dict(dtype=dtype or self.dtype, device=self.device)
        return torch.full(shape, fill, **opts) if masked else \
            torch.empty(shape, **opts)

    def _write_fields(self, what, rows, blocks, over_samples=False):
        """Writes the fields the user gave - `blocks`: (name, block or None,
        offset, width), `_row_blocks` / `_weight_blocks` - into `rows`
        ([B][row], or [B][S][row]; `over_samples`: a [B][width] block is then
        the same for every s) and returns `rows`; a field of another shape is
        `what`'s NativeError."""
        lead = tuple(rows.shape[:-1])
        for name, block, off, width in blocks:
            if block is None:
                continue
            block = torch.as_tensor(block)
            if over_samples and block.dim() == 2:
                block = block.unsqueeze(1).expand(-1, lead[1], -1)
            if tuple(block.shape) != lead + (width,):
                want = "(%d, [%d, ]%d)" if over_samples else "(%d, %d)"
                raise _native.NativeError("%s: %s has shape %s, expected %s" % (
                    what, name, tuple(block.shape), want % (lead + (width,))))
            rows[..., off:off + width] = block.to(dtype=self.dtype,
                                                  device=self.device)
        return rows

    def _problem_changed(self, separate=False):
        """The records in `_rec` are another problem's and a captured round is
        dropped; `separate`: per-trajectory data was set, every round is
        records+separate from now on."""
        if separate:
            self._one_launch = self._nominal_sweep = self._fused = False
        self._derivs_due = True
        self._rec_stale = True
        self._graph = None

    def _per_trajectory(self):
        """Is any per-trajectory data set?  (Its kernels are the only ones that
        read it: every other sequence takes one problem for the batch.)"""
        return self.batch_table is not None or self.reference is not None or \
            self.batch_weights is not None

    def _base_table(self):
        """`batch_table`, or the shared problem in every row."""
        return self.batch_table if self.batch_table is not None else \
            self._shared_row().repeat(self.B, 1)

    def _shared_row(self):
        """The shared problem as one row of the table's layout
        (include/pddp_hip.h): double -> T as convert_problem
        (csrc/models.hpp)."""
        N_ = _native
        prob = self.problem
        row = torch.zeros(N_.BATCH_ROW, dtype=torch.float64)
        row[N_.BATCH_PARAMS:N_.BATCH_PARAMS + N_.MAX_PARAMS] = \
            torch.tensor(list(prob.params), dtype=torch.float64)
        row[N_.BATCH_X_GOAL:N_.BATCH_X_GOAL + N_.MAX_AUG] = \
            torch.tensor(list(prob.x_goal), dtype=torch.float64)
        row[N_.BATCH_U_GOAL:N_.BATCH_U_GOAL + N_.MAX_ACTION] = \
            torch.tensor(list(prob.u_goal), dtype=torch.float64)
        return row.to(self.dtype).to(self.device)

    def _row_blocks(self, params, x_goal, u_goal):
        """(name, block, offset in a row, width) of a row's three fields."""
        N_ = _native
        prob = self.problem
        return (("params", params, N_.BATCH_PARAMS,
                 self._PARAM_COUNT[prob.model]),
                ("x_goal", x_goal, N_.BATCH_X_GOAL, prob.aug_size),
                ("u_goal", u_goal, N_.BATCH_U_GOAL, self.m))

    def _weight_matrices(self):
        """(name, matrix, leading dimension, size, offset of its diagonal in a
        row of the weights) of the shared Q, Q_term, R."""
        N_ = _native
        prob = self.problem
        return (("Q", prob.Q, N_.MAX_AUG, prob.aug_size, N_.WEIGHT_Q),
                ("Q_term", prob.Q_term, N_.MAX_AUG, prob.aug_size,
                 N_.WEIGHT_Q_TERM),
                ("R", prob.R, N_.MAX_ACTION, self.m, N_.WEIGHT_R))

    def _shared_weights_row(self):
        """The shared diagonals as one row of the weights' layout: double -> T
        as convert_problem (`_shared_row`)."""
        row = torch.zeros(_native.WEIGHT_ROW, dtype=torch.float64)
        for _, mat, ld, k, off in self._weight_matrices():
            row[off:off + k] = torch.tensor(
                [mat[i * ld + i] for i in range(k)], dtype=torch.float64)
        return row.to(self.dtype).to(self.device)

    def _weight_blocks(self, q, q_term, r):
        """(name, block, offset in a row, width) of a row's three fields."""
        return tuple((name.lower(), block, off, k) for block, (
            name, _, _, k, off) in zip((q, q_term, r),
                                       self._weight_matrices()))

    def clear_batch_problem(self):
        """Back to one problem for the whole batch: the plan's inputs as the
        constructor leaves them (while a reference is set, once that is
        cleared too).  (Nothing to do without a table.)"""
        if self.batch_table is None:
            return
        self.batch_table = None
        self._restore_plan()

    def _restore_plan(self):
        """After a table, a reference or the weights went: the plan's inputs
        as the constructor leaves them, unless another of them is still
        set."""
        if not self._per_trajectory():
            self._fused = self._one_launch = None
            self._nominal_sweep = None if (
                self._nominal_sweep_possible() and
                self._nominal_sweep_pays()) else False
        self._problem_changed()

    @_on_device
    def set_reference(self, x_ref, u_ref=None, start=0, keep_weights=False):
        """A goal per time step (reference tracking): `x_ref` [B][L][na] in
        augmented coordinates, `u_ref` [B][L][m] (default: in every row the
        table's `u_goal` if a table is set, else the shared problem's).
        Horizon index i = 0 .. N of trajectory b takes its goals from row
        min(start + i, L - 1): the last row is held, the terminal step reads
        its row's `x_goal` only.  Q, Q_term, R, the model, the encoding and the
        bounds stay the problem's; the model parameters stay the table's where
        one is set.

        Builds `reference` ([B][L][12], include/pddp_hip.h) and `ref_start`;
        from then on the derivative records and the line search are the
        pddp_*_track_* entry points and every round is derivs, backward,
        line_search, accept (`records+separate`); `mpc_closed_loop()` reads
        the window from `ref_start + t` at control step t.  The sweep from the
        nominal, the one-launch round and the fused search take one goal per
        trajectory and refuse; so does `closed_loop()` unless it is told to
        follow the reference (`track=True`).  The nominal rollout reads no
        goal: the current nominal stays as it is.

        While per-trajectory cost weights are set (`set_batch_weights`) the
        call is refused unless `keep_weights=True`: the reference is then
        tracked under every trajectory's own diagonals - records and line
        search are the pddp_*_track_weighted_* entry points, everything else
        as above.  (`mpc_closed_loop()` and `closed_loop(track=True)` still
        REPORT under the shared Q, Q_term, R.)"""
        self._need_sample_problem("set_reference")
        if self.batch_weights is not None and not keep_weights:
            raise _native.NativeError(
                "set_reference: per-trajectory cost weights are set "
                "(set_batch_weights); keep_weights=True tracks the reference "
                "under them, clear_batch_weights() drops them first")
        N_ = _native
        B, na, m = self.B, self.problem.aug_size, self.m
        opts = dict(dtype=self.dtype, device=self.device)
        x_ref = torch.as_tensor(x_ref)
        if x_ref.dim() != 3 or x_ref.shape[0] != B or x_ref.shape[1] < 1 or \
                x_ref.shape[2] != na:
            raise _native.NativeError(
                "set_reference: x_ref has shape %s, expected (%d, L >= 1, "
                "%d)" % (tuple(x_ref.shape), B, na))
        L = x_ref.shape[1]
        if u_ref is not None:
            u_ref = torch.as_tensor(u_ref)
            if tuple(u_ref.shape) != (B, L, m):
                raise _native.NativeError(
                    "set_reference: u_ref has shape %s, expected (%d, %d, "
                    "%d)" % (tuple(u_ref.shape), B, L, m))
        start = self._ref_start_of(start)
        ref = torch.zeros(B, L, N_.REF_ROW, **opts)
        ref[:, :, N_.REF_U_GOAL:N_.REF_U_GOAL + N_.MAX_ACTION] = \
            self._base_table()[:, None, N_.BATCH_U_GOAL:N_.BATCH_U_GOAL +
                               N_.MAX_ACTION]
        ref[:, :, N_.REF_X_GOAL:N_.REF_X_GOAL + na] = x_ref.to(**opts)
        if u_ref is not None:
            ref[:, :, N_.REF_U_GOAL:N_.REF_U_GOAL + m] = u_ref.to(**opts)
        self.reference = ref.contiguous()
        self.ref_start = start
        self._problem_changed(separate=True)

    def _ref_start_of(self, start):
        if int(start) != start or int(start) < 0 or int(start) > 0x7fffffff:
            raise _native.NativeError(
                "the reference's window starts at a row index >= 0, got %r" %
                (start,))
        return int(start)

    def set_reference_start(self, start):
        """Moves the window: horizon index 0 reads row `start` from now on
        (the records of the nominal are evaluated again, a captured round is
        dropped)."""
        if self.reference is None:
            raise _native.NativeError(
                "set_reference_start: no reference is set")
        self.ref_start = self._ref_start_of(start)
        self._problem_changed()

    def clear_reference(self):
        """Back to one goal per trajectory: what `clear_batch_problem()`
        restores; with a table still set its plan stays.  (Nothing to do
        without a reference.)"""
        if self.reference is None:
            return
        self.reference = None
        self.ref_start = 0
        self._restore_plan()

    @_on_device
    def set_batch_weights(self, q=None, q_term=None, r=None, check=True,
                          keep_reference=False):
        """Per-trajectory cost weights: `q`, `q_term` [B][na] (augmented
        coordinates) and `r` [B][m] REPLACE the diagonals of Q, Q_term and R
        for trajectory b; a block not given keeps the shared diagonal.  The
        off-diagonal entries, the model, the encoding and the action bounds
        stay shared; parameters and goals stay the table's where one is set.

        Builds `batch_weights` ([B][20], include/pddp_hip.h); from then on the
        derivative records and the line search are the pddp_*_weighted_* entry
        points and every round is derivs, backward, line_search, accept
        (`records+separate`): the sweep from the nominal, the one-launch round
        and the fused search take one cost for the batch and refuse.  The
        nominal rollout reads no cost: the current nominal stays as it is.
        `closed_loop()`, `closed_loop_draws()` and `mpc_closed_loop()` stay
        available; the costs they REPORT are under the shared problem's Q,
        Q_term, R.  While a reference is set (`set_reference`) the call is
        refused unless `keep_reference=True`: the reference is then tracked
        under the weights - records and line search are the
        pddp_*_track_weighted_* entry points, the table's goals are not read.

        `check` (default): every trajectory's matrices are tested on the
        host, in float64, once - one copy of [B][20] numbers.  The symmetrised
        Q_b and Q_term_b must have no eigenvalue below -1e-9 max |entry| (nor
        below the shared matrix's own lowest, where that is lower: the shared
        cost is never refused), R_b only positive ones; otherwise NativeError
        names the first offending trajectory and matrix.  (A diagonal lowered
        under an off-diagonal entry makes the cost indefinite, and the solver
        then answers with NOT_PD / MAX_REG states that look like a tuning
        result.)"""
        self._need_sample_problem("set_batch_weights")
        if self.reference is not None and not keep_reference:
            raise _native.NativeError(
                "set_batch_weights: a reference is set (set_reference); "
                "keep_reference=True tracks it under the weights, "
                "clear_reference() drops it first")
        weights = self._write_fields(
            "set_batch_weights", self._shared_weights_row().repeat(self.B, 1),
            self._weight_blocks(q, q_term, r))
        if check:
            self._check_weights(weights)
        self.batch_weights = weights.contiguous()
        self._problem_changed(separate=True)

    def _check_weights(self, weights):
        """set_batch_weights(check=True): the eigenvalues of every
        trajectory's Q, Q_term (symmetrised, >= -1e-9 max |entry| or the
        shared matrix's own lowest) and R (> 0), on the host in float64."""
        w = weights.to(dtype=torch.float64, device="cpu")
        found = None  # (trajectory, matrix) of the first offender
        for name, mat, ld, k, off in self._weight_matrices():
            positive = name == "R"
            M = torch.tensor(list(mat), dtype=torch.float64).reshape(
                ld, ld)[:k, :k]
            M = 0.5 * (M + M.T)
            # (the shared matrix's own lowest eigenvalue is allowed: the
            # double cartpole's Q, rank one in exact arithmetic, has one of
            # -1e-8 from the float32 rounding of its entries)
            slack = max(0.0, -float(torch.linalg.eigvalsh(M)[0]))
            M = M.repeat(self.B, 1, 1)
            idx = torch.arange(k)
            M[:, idx, idx] = w[:, off:off + k]
            finite = torch.isfinite(M).flatten(1).all(1)
            M[~finite] = 0.0  # (a row with inf / NaN offends as it is)
            low = torch.linalg.eigvalsh(M)[:, 0]
            bad = ~finite | ((low <= 0) if positive else (
                low < -torch.clamp(
                    1e-9 * M.abs().flatten(1).max(1).values, min=slack)))
            if bool(bad.any()):
                b = int(torch.nonzero(bad)[0])
                if found is None or b < found[0]:
                    found = (b, name, "" if positive else "semi-")
        if found is not None:
            raise _native.NativeError(
                "set_batch_weights: %s of trajectory %d is not positive "
                "%sdefinite with these weights (check=False skips this "
                "test)" % (found[1], found[0], found[2]))

    def clear_batch_weights(self):
        """Back to the shared cost: what `clear_batch_problem()` restores;
        with a table still set its plan stays.  (Nothing to do without
        weights.)"""
        if self.batch_weights is None:
            return
        self.batch_weights = None
        self._restore_plan()

    def _one_goal(self, what):
        if self.reference is not None:
            raise _native.NativeError(
                "%s takes ONE goal per trajectory; with a reference "
                "(set_reference) a round is derivs, backward, line_search, "
                "accept" % what)

    def _one_problem(self, what):
        if self.reference is not None:  # (no call on the one-launch path)
            self._one_goal(what)
        if self.batch_weights is not None:
            raise _native.NativeError(
                "%s evaluates ONE cost for the whole batch; with "
                "set_batch_weights() a round is derivs, backward, line_search, "
                "accept" % what)
        if self.batch_table is not None:
            raise _native.NativeError(
                "%s evaluates ONE problem for the whole batch; with "
                "set_batch_problem() a round is derivs, backward, line_search, "
                "accept" % what)

    def _problem_call(self, name, *args, goals=False):
        """A problem kernel's entry point, by the per-trajectory data set: the
        `_batch` one, with the table, while a table is set; for a kernel that
        reads the `goals` (records, line search) the `_weighted` one, with the
        table's address or NULL and the weights, while weights are set, and
        the `_track` one, likewise with `_ref_window()`, while a reference is;
        with both the `_track_weighted` one: the table's address or NULL, the
        window, the weights.  The addresses are looked up at the call: a
        tensor may be replaced between two calls."""
        p = _native.ptr
        track = goals and self.reference is not None
        weighted = goals and self.batch_weights is not None
        suffix = ("_track" if track else "") + \
            ("_weighted" if weighted else "")
        if not suffix and self.batch_table is not None:
            suffix = "_batch"
        lead = ()
        if suffix:  # the table, then the window, then the weights
            lead = (p(self.batch_table),) + \
                (self._ref_window() if track else ()) + \
                ((p(self.batch_weights),) if weighted else ())
        return _native.call(name + suffix, self.dtype, self._pp, *lead, *args)

    def _ref_window(self):
        """(address, rows, first row) of the reference, as every pddp_*_track_*
        entry point takes them after the table."""
        return (_native.ptr(self.reference), self.reference.shape[1],
                self.ref_start)

    @property
    def rec(self):
        """The derivative records [B][N+1][S] of the nominal, up to date."""
        self.sync_records()
        return self._rec

    @_on_device
    def sync_records(self):
        """Brings `rec` / `L` up to date with the nominal when round() left
        them behind (the sweep from the nominal writes no records)."""
        if self._rec_stale:
            self._derivs(None, self._jscr, None)
            self._rec_stale = False

    def _derivs(self, mask, J, state):
        p = _native.ptr
        self._problem_call("pddp_derivs", self.B, self.N,
                           p(self.Z), p(self.U), p(self.u_min), p(self.u_max),
                           p(mask), p(self._rec), p(self.L), p(J), p(state),
                           self._s(), goals=True)

    # -- views in the reference's tensor layout -----------------------------
    def record_views(self):
        """(F_z, F_u, L_z, L_u, L_zz, L_uz, L_uu) as zero-copy views of the
        record buffer, shaped like ilqr.py:445-455 with a leading batch."""
        l, n, m, N = self.lay, self.n, self.m, self.N
        r = self.rec
        B = self.B
        F_z = r[:, :N, l.o_Fz:l.o_Fz + n * n].unflatten(-1, (n, n))
        F_u = r[:, :N, l.o_Fu:l.o_Fu + n * m].unflatten(-1, (n, m))
        L_z = r[:, :, l.o_Lz:l.o_Lz + n]
        L_u = r[:, :N, l.o_Lu:l.o_Lu + m]
        L_zz = r[:, :, l.o_Lzz:l.o_Lzz + n * n].unflatten(-1, (n, n))
        L_uz = r[:, :N, l.o_Luz:l.o_Luz + m * n].unflatten(-1, (m, n))
        L_uu = r[:, :N, l.o_Luu:l.o_Luu + m * m].unflatten(-1, (m, m))
        return F_z, F_u, L_z, L_u, L_zz, L_uz, L_uu

    def gain_views(self, accepted=False):
        g = self.gains_acc if accepted else self.gains
        m, n = self.m, self.n
        return g[..., :m], g[..., m:].unflatten(-1, (m, n))

    def exact_variant(self, branch=None, bounded=True):
        """The variant number (include/pddp_hip.h) of the kernel `auto` would
        pick, with IEEE division / square root instead of v_rcp / v_sqrt."""
        branch = self.branch if branch is None else branch
        bounded = bounded and self.u_min is not None
        if self.dtype != torch.float32:
            return 0  # the f64 kernels are IEEE throughout
        if self.n == 4 and self.m == 1:
            return 16 if self.B >= 12288 else 6
        if self.m == 1 and self.n <= 30:
            return 14
        return 0  # generic kernel: IEEE throughout

    # -- kernels --------------------------------------------------------------
    def _s(self):
        return _native.stream_handle(self.device)

    @_on_device
    def set_nominal(self, z0, U):
        """ilqr.py:274-277: new nominal controls, regularisation reset.
        (z0 is the plant's state again: a noisy MPC trial's `x_true` is
        dropped.)"""
        self.x_true = None
        self.z0.copy_(z0.reshape(self.B, self.n))
        self.U.copy_(U.reshape(self.B, self.N, self.m))
        self.reset_controller_state()
        self.nominal_rollout()

    def reset_controller_state(self):
        self._derivs_due = True  # every nominal is new: records at round start
        self.n_live.zero_()
        self.mu.zero_()          # _reset_reg ilqr.py:364-367
        self.delta.fill_(2.0)
        self.state.zero_()       # UNDEFINED
        self.iter.fill_(1)       # first step() call is under way
        self.active.fill_(1)
        self.fresh.fill_(1)

    def _graphs_fresh(self):
        """Plugin graphs hold raw pointers to model-owned tensors
        (normalisation buffers, dropout masks, cached noise); `model.fit()`,
        `resample()` and loading a state replace those tensors and bump the
        model's generation (models/bnn.py).  A graph captured under another
        generation is dropped here and re-captured by its user."""
        if self.plugin is None:
            return
        from ..models.bnn import generation
        gen = generation(self.plugin.model)
        # (and the cost's tensors where launches read converted copies of
        # them: the GP line search, plugin.cost_generation)
        cg = getattr(self.plugin, "cost_generation", lambda: None)()
        if gen != self._model_gen or cg != self._cost_gen:
            self._graph = None
            self._rollout_graph = None
            self._model_gen = gen
        self._cost_gen = cg

    @_on_device
    def nominal_rollout(self, mask=None):
        if self.plugin is not None:
            self._graphs_fresh()
            if self.graph_rollout and self.plugin.capture_ok(self):
                # the N + 1 moment-step / network launch pairs of the nominal
                # rollout as one hipGraph (z0, U, Z are solver-owned buffers)
                if self._rollout_graph is None:
                    self.plugin.rollout(self)  # warm: caches, attributes
                    torch.cuda.synchronize(self.device)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self.plugin.rollout(self)
                    self._rollout_graph = g
                self._rollout_graph.replay()
                return
            return self.plugin.rollout(self)
        p = _native.ptr
        self._problem_call("pddp_nominal_rollout", self.B,
                           self.N, p(self.z0), p(self.U), p(self.u_min),
                           p(self.u_max), p(mask), p(self.Z), self._s())

    @_on_device
    def derivs(self, mask=None, set_state=True, in_graph=False):
        if self.plugin is not None:
            return self.plugin.derivs(self, mask, set_state, in_graph)
        if mask is not None:
            self.sync_records()  # (the rows outside the mask)
        self._rec_stale = False
        self._derivs(mask, self.J_opt, self.state if set_state else None)

    @_on_device
    def backward(self, active=None, reg=None, branch=None, bounded=True,
                 variant=0, events=None):
        """variant: 0 auto, 1 generic kernel; n = 4: 6 / 7 sixteen lanes per
        trajectory (IEEE / approximate division), 16 / 17 / 18 four lanes;
        14 / 15 the matrix-core kernels (m = 1, n <= 30), 26 / 27 their step
        split over two wavefronts - the list in csrc/riccati.hip.  `events`: a
        (start, stop) pair of pddp_event handles to attach to the dispatch."""
        self.sync_records()
        p = _native.ptr
        reg = self.mu if reg is None else reg
        branch = self.branch if branch is None else branch
        umin = self.u_min if bounded else None
        umax = self.u_max if bounded else None
        args = (self.B, self.N, self.n, self.m, p(self._rec), p(umin), p(umax),
                p(reg), int(branch), p(active), p(self.gains),
                p(self.bwd_status), self._s(), int(variant))
        if events is None:
            _native.call("pddp_riccati_backward_variant", self.dtype, *args)
        else:
            _native.call("pddp_riccati_backward_timed", self.dtype, *args,
                         events[0], events[1])

    # -- the round's launch plan ----------------------------------------------
    def _plan(self, variant, search_events=None):
        """The sequence a round tries first (module docstring)."""
        if self._per_trajectory():
            # (the other sequences' kernels take one problem for the batch)
            return RECORDS_SEPARATE
        if variant == 0 and self._nominal_sweep is not False and \
                self._fused is not False:
            one = self._one_launch is not False and search_events is None
            return ONE_LAUNCH if one else NOMINAL_FUSED
        return RECORDS_FUSED if self._fused_allowed() else RECORDS_SEPARATE

    def _fused_allowed(self):
        return self.plugin is None and self._fused is not False and \
            not self._per_trajectory()

    def _one_launch_applied(self):
        return self._one_launch is True

    def _nominal_sweep_applied(self):
        return self._nominal_sweep is True

    def _records_due(self, always):
        # (the fused search writes the records of the nominals it accepts)
        return self._derivs_due or always or self._fused is not True

    def _round_nominal_done(self, ok):  # (ok False: PDDP_E_UNSUPPORTED)
        self._one_launch = ok
        if ok:
            self._nominal_sweep = self._fused = self._rec_stale = True
            self._derivs_due = False
        return ok

    def _sweep_nominal_done(self, ok):
        self._nominal_sweep = ok
        self._rec_stale |= ok  # (the sweep writes no records)
        return ok

    def _search_accept_done(self, ok, records=True):
        self._fused = ok
        if ok:
            # (pddp_search_candidates: without records the candidates are
            # dropped beyond 200 MB - Zc / Uc are scratch after such a launch,
            # only Jc and the nominal are results)
            mode = _native.lib().pddp_search_candidates(-1)
            nbytes = float(self.B) * self.A * (
                (self.N + 1) * self.n + self.N * self.m) * \
                self.Z.element_size()
            self.candidates_kept = records or self._rec is None or not (
                mode == 2 or (mode == 0 and nbytes > 200e6))
        return ok

    def _launch(self, events, fn, *args):
        """fn(*args) with `events`, a (start, stop) pair or None, attached to
        its launch - detached again if it made none (PDDP_E_UNSUPPORTED)."""
        if events is None:
            return fn(*args)
        attach = _native.lib().pddp_attach_events
        attach(*events)
        rc = fn(*args)
        if rc == _native.E_UNSUPPORTED:
            attach(None, None)
        return rc

    def _buffers(self):
        """Addresses of the round's buffers (the solver's own for its lifetime:
        looked up once - a launch of pddp_round_nominal_f32 is the whole host
        side of a round, and 27 data_ptr() calls were a third of it).  After
        replacing one other than u_min, u_max, alphas: `_round_args = None`."""
        key = (self._rec.data_ptr(), self.Z.data_ptr(), self.U.data_ptr(),
               self.gains.data_ptr(), int(self.branch), id(self.u_min),
               id(self.u_max), id(self.alphas))
        b = self._round_args
        if b is None or b.key != key:
            b = self._round_args = types.SimpleNamespace(
                key=key, keep=(self.u_min, self.u_max, self.alphas),  # (ids)
                branch=key[4], **{
                    k.lstrip("_"): _native.ptr(getattr(self, k)) for k in (
                        "Z", "U", "alphas", "u_min", "u_max", "active",
                        "fresh", "gains", "bwd_status", "L", "J_opt", "Zc",
                        "Uc", "Jc", "gains_acc", "mu", "delta", "state",
                        "iter", "n_live", "_rec")})
            # pddp_round_nominal_f32's around (tol, max_reg, n_iterations)
            b.head = (self._pp, self.B, self.N, self.A, b.Z, b.U, b.alphas,
                      b.u_min, b.u_max, b.branch, b.active, b.fresh, b.gains,
                      b.bwd_status, b.L, b.J_opt, b.Zc, b.Uc, b.Jc)
            b.tail = (b.gains_acc, b.mu, b.delta, b.state, b.iter, b.n_live,
                      b.rec)
        return b

    @_on_device
    def sweep_nominal(self, events=None):
        """Backward sweep straight from the nominal (pddp_sweep_nominal_f32):
        derivative records evaluated in the workgroups, stage costs to `L`,
        J_opt of the fresh nominals.  False when it does not apply."""
        self._one_problem("sweep_nominal")
        b = self._buffers()
        rc = self._launch(
            events, _native.call_rc, "pddp_sweep_nominal", self.dtype,
            self._pp, self.B, self.N, b.Z, b.U, b.u_min, b.u_max, b.mu,
            b.branch, b.active, b.fresh, b.gains, b.bwd_status, b.L, b.J_opt,
            self._s())
        return self._sweep_nominal_done(rc == 0)

    @_on_device
    def round_nominal(self, tol, max_reg, n_iterations, events=None,
                      rounds=1):
        """A whole round in ONE launch (pddp_round_nominal_f32,
        csrc/round_n4.hip): the sweep from the nominal, then line search,
        accept and regularisation schedule in the same workgroups - the two
        launches' results (the sweep's bit for bit, the search's to rounding).
        `rounds` > 1: that many rounds back to back in the one launch (a
        workgroup owns its trajectories; no launch boundary between their
        attempts).  False when it does not apply (the caller then makes the two
        calls)."""
        self._one_problem("round_nominal")
        if self.dtype != torch.float32 or self.plugin is not None or \
                (self.u_min is None) != (self.u_max is None):
            return self._round_nominal_done(False)
        b = self._buffers()
        rc = self._launch(
            events, _native.lib().pddp_round_nominal_f32, *b.head, float(tol),
            float(max_reg), int(n_iterations), *b.tail, int(rounds),
            _native.ptr(self.phase_ticks), self._s())
        if rc != _native.E_UNSUPPORTED:
            _native.check(rc, "pddp_round_nominal_f32")
        return self._round_nominal_done(rc == 0)

    @_on_device
    def line_search(self, active=None, use_status=True):
        if self.plugin is not None:
            return self.plugin.line_search(self, active, use_status)
        b = self._buffers()
        self._problem_call(
            "pddp_line_search", self.B, self.N,
            self.A, b.Z, b.U, b.gains, b.alphas, b.u_min, b.u_max,
            _native.ptr(active), b.bwd_status if use_status else None,
            b.Zc, b.Uc, b.Jc, self._s(), goals=True)

    @_on_device
    def accept(self, tol, max_reg, n_iterations):
        b = self._buffers()
        _native.call("pddp_accept", self.dtype, self.B, self.N, self.n, self.m,
                     self.A, b.Zc, b.Uc, b.Jc, b.gains, b.bwd_status,
                     float(tol), float(max_reg), int(n_iterations), b.Z, b.U,
                     b.gains_acc, b.J_opt, b.mu, b.delta, b.state, b.iter,
                     b.active, b.fresh, b.n_live, self._s())

    def search_accept(self, tol, max_reg, n_iterations, events=None,
                      records=True):
        """`_search_accept`, refused while a reference is set (round() then
        makes the separate calls by itself)."""
        self._one_goal("search_accept")
        return self._search_accept(tol, max_reg, n_iterations, events,
                                   records)

    @_on_device
    def _search_accept(self, tol, max_reg, n_iterations, events=None,
                       records=True):
        """Line search + accept + derivative records of the new nominals in
        one launch (pddp_search_accept_*).  False when the fused kernel does
        not apply; the caller then makes the separate calls.  `events`: a
        (start, stop) pair attached to THIS launch (bench.py); when the fused
        kernel does not apply nothing is attached and `last_search_timed` says
        so."""
        self.last_search_timed = None
        if not self._fused_allowed():
            return False
        b = self._buffers()
        rc = self._launch(
            events, _native.call_rc, "pddp_search_accept", self.dtype,
            self._pp, self.B, self.N, self.A, b.Z, b.U, b.gains, b.alphas,
            b.u_min, b.u_max, b.active, b.bwd_status, b.Zc, b.Uc, b.Jc,
            float(tol), float(max_reg), int(n_iterations), b.gains_acc,
            b.J_opt, b.mu, b.delta, b.state, b.iter, b.fresh, b.n_live, b.rec,
            b.L if records else None, self._s())
        if rc == 0 and events is not None:
            self.last_search_timed = "search_accept"
        return self._search_accept_done(rc == 0, records)

    @_on_device
    def closed_loop(self, samples=None, z0=None, params=None, x_goal=None,
                    u_goal=None, feedback=True, accepted=True, keep=False,
                    active=None, events=None, process_std=None, obs_std=None,
                    seed=0, sample_offset=0, track=False):
        """Runs every trajectory's policy in closed loop, S rollouts each
        (pddp_closed_loop_*: the batched `_apply_controller`, pddp.py:209-245,
        with the sample models as the plant): rollout (b, s) starts at
        `z0[b][s]` ([B][S][n]; default: the nominal's first state), applies
        u = clamp(U + K (x - Z)) and steps the plant of row (b, s).

        Plant fields `params` ([.][P], dt first), `x_goal` ([.][na]), `u_goal`
        ([.][m]) as in `set_batch_problem`, each [B][S][.] or [B][.] (the same
        for every s); a field not given is `batch_table`'s if a table is set,
        else the shared problem's; no field and no table: the shared problem
        for every rollout.  The cost of a rollout uses its row's goals.
        `samples` S defaults to z0.shape[1], else 1.  `accepted`: the gains of
        the accepted nominal (`gains_acc`, the reference's `_K`) or the last
        sweep's; `feedback=False`: open loop, u = clamp(U).  `active` [B]
        uint8: trajectories with 0 are skipped, their outputs NaN (X, U:
        unspecified).  `events`: a (start, stop) pair for the dispatch.

        `process_std`, `obs_std` (each a scalar or [n]; None: none of it):
        noise drawn inside the rollouts (pddp_closed_loop_noisy_*) - the plant
        steps to x' + process_std (.) w_t, the controller sees x + obs_std (.)
        v_t, the cost is the true state's.  w_t, v_t are unit normals, a pure
        function of (`seed`, `sample_offset` + b S + s, t, component): the same
        seed repeats a run and gives another controller the same noise;
        `closed_loop_draws` returns them.  With both None this is the
        noise-free launch, as ever.

        Returns an object with `J` [B][S], `stats` [B][4] = (mean, min, max of
        the finite costs, their number) and, with `keep`, `X` [B][N+1][S][n],
        `U` [B][N][S][m] (None otherwise: only costs leave the chip).
        Stream-ordered on the solver's stream; the controller state, the
        nominal, the plan and a captured graph are not touched.

        While a reference is set (`set_reference`) the call is refused - the
        rollouts would be costed under one goal - unless `track=True`: then
        rollout (b, s) takes the stage cost of step t under reference row
        min(ref_start + t, L - 1) of trajectory b and the terminal cost under
        row min(ref_start + N, L - 1) (pddp_closed_loop_track_*), with or
        without noise; all S rollouts of a trajectory share its reference, and
        the plant fields supply parameters only: `x_goal` / `u_goal` would not
        be read and are refused.  `ref_start` is read, not moved.

        With per-trajectory cost weights (`set_batch_weights`) the call is
        NOT refused and its kernels are unchanged: `J` and `stats` are under
        the shared problem's Q, Q_term, R and the plant row's goals, whatever
        weights each policy was fitted under - the common yardstick (with
        `track=True` while both are set: under the shared matrices along the
        reference)."""
        if track:
            if self.reference is None:
                raise _native.NativeError(
                    "closed_loop(track=True): no reference is set "
                    "(set_reference)")
            if x_goal is not None or u_goal is not None:
                raise _native.NativeError(
                    "closed_loop(track=True) takes the goals of every step "
                    "from the reference; x_goal / u_goal would not be read")
        elif self.reference is not None:
            raise _native.NativeError(
                "closed_loop takes ONE goal per trajectory; with a reference "
                "(set_reference) pass track=True to cost the rollouts along "
                "it")
        self._need_sample_problem("closed_loop")
        B, N, n, m = self.B, self.N, self.n, self.m
        opts = dict(dtype=self.dtype, device=self.device)
        if z0 is not None:
            z0 = torch.as_tensor(z0).to(**opts)
            if z0.dim() != 3 or z0.shape[0] != B or z0.shape[2] != n:
                raise _native.NativeError(
                    "closed_loop: z0 has shape %s, expected (%d, S, %d)" % (
                        tuple(z0.shape), B, n))
        S = int(samples) if samples is not None else \
            (z0.shape[1] if z0 is not None else 1)
        if S < 1 or (z0 is not None and z0.shape[1] != S):
            raise _native.NativeError(
                "closed_loop: %d samples, z0 of shape %s" % (
                    S, None if z0 is None else tuple(z0.shape)))
        plant = None
        if not (self.batch_table is None and params is None and
                x_goal is None and u_goal is None):
            plant = self._write_fields(
                "closed_loop", self._base_table().unsqueeze(1).repeat(1, S, 1),
                self._row_blocks(params, x_goal, u_goal), over_samples=True)
        self._check_active("closed_loop", active)
        gains = None if not feedback else \
            (self.gains_acc if accepted else self.gains)
        masked = active is not None
        out = types.SimpleNamespace(
            J=self._out(masked, B, S), stats=self._out(masked, B, 4),
            X=self._out(False, B, N + 1, S, n) if keep else None,
            U=self._out(False, B, N, S, m) if keep else None)
        p = _native.ptr
        w_std = self._noise_std("process_std", process_std)
        v_std = self._noise_std("obs_std", obs_std)
        # (in ABI order: problem, [reference,] shapes, nominal, plant, [noise])
        nominal = (p(self.Z), p(self.U), p(gains))
        starts = (p(None if z0 is None else z0.contiguous()), p(plant),
                  p(self.u_min), p(self.u_max))
        noise = (p(w_std), p(v_std), int(seed), int(sample_offset))
        outputs = (p(active), p(out.X), p(out.U), p(out.J), p(out.stats),
                   self._s())
        if track:  # (with or without noise: one entry point)
            name, ref = "pddp_closed_loop_track", self._ref_window()
        elif process_std is None and obs_std is None:
            name, ref, noise = "pddp_closed_loop", (), ()
        else:
            name, ref = "pddp_closed_loop_noisy", ()
        self._launch(events, _native.call, name, self.dtype, self._pp, *ref,
                     B, N, S, *nominal, *starts, *noise, *outputs)
        return out

    def _noise_std(self, name, std, what="closed_loop"):
        """[n] device vector of a noise level given as a scalar or [n]."""
        if std is None:
            return None
        # (a Python number goes straight to the run's dtype, not through f32)
        std = torch.as_tensor(std, dtype=self.dtype, device=self.device)
        if std.dim() == 0:
            std = std.repeat(self.n)
        if tuple(std.shape) != (self.n,):
            raise _native.NativeError(
                "%s: %s has shape %s, expected a scalar or (%d,)" % (
                    what, name, tuple(std.shape), self.n))
        return std.contiguous()

    @_on_device
    def closed_loop_draws(self, samples, which="process", seed=0,
                          sample_offset=0, steps=None):
        """The unit normals `closed_loop(samples, seed=, sample_offset=)`
        draws, W [B][N][S][n] (pddp_closed_loop_draws_*; time-major like X):
        `which` "process" for w_t, "obs" for v_t.  To look at, or to replay,
        the noise of a rollout - e.g. process_std * W[b, :T, s] as
        `mpc_closed_loop`'s disturbance.  (No cost is read: per-trajectory
        cost weights, `set_batch_weights`, change nothing here; the costs
        `closed_loop` reports for these draws are under the shared problem's
        Q, Q_term, R and the plant row's goals - the common yardstick.)

        `steps`: the number of time rows in place of N, W [B][steps][S][n] -
        the normals of a T-step `mpc_closed_loop(process_std=, obs_std=,
        seed=)` trial are `closed_loop_draws(1, which, seed, sample_offset,
        steps=T + 1)[:, :, 0]` (row step_offset + t: w of control step t, v of
        the observation y_t)."""
        if which not in ("process", "obs"):
            raise _native.NativeError(
                "closed_loop_draws: which is %r, expected 'process' or 'obs'"
                % (which,))
        B, S = self.B, int(samples)
        N = self.N if steps is None else int(steps)
        if S < 1 or N < 1:
            raise _native.NativeError(
                "closed_loop_draws: %d samples, %d steps" % (S, N))
        W = torch.empty(B, N, S, self.n, dtype=self.dtype, device=self.device)
        _native.call("pddp_closed_loop_draws", self.dtype, B, N, S, self.n,
                     0 if which == "process" else 1, int(seed),
                     int(sample_offset), _native.ptr(W), self._s())
        return W

    def _action_std(self, std, what="shoot"):
        """[m] device vector of a perturbation level given as a scalar or [m]
        (`_noise_std`, of the action's length)."""
        std = torch.as_tensor(std, dtype=self.dtype, device=self.device)
        if std.dim() == 0:
            std = std.repeat(self.m)
        if tuple(std.shape) != (self.m,):
            raise _native.NativeError(
                "%s: std has shape %s, expected a scalar or (%d,)" % (
                    what, tuple(std.shape), self.m))
        return std.contiguous()

    @_on_device
    def shoot(self, samples, std, smooth=0.0, seed=0, sample_offset=0,
              active=None, adopt=True, events=None, objective="shared"):
        """Sampled shooting around the current action sequence
        (pddp_shoot_*, csrc/shoot.hip): S = `samples` candidates per
        trajectory, candidate 0 the sequence `U` itself, candidate s >= 1
        u_t = clamp(U[b][t] + std (.) e_t) with e an AR(1) of unit variance,
        e_t = smooth e_{t-1} + sqrt(1 - smooth^2) xi_t, over the unit normals
        xi of (`seed`, `sample_offset` + b S + s, t) - `shoot_draws` returns
        them.  Each is rolled out open loop from `z0` under the solver's own
        model, cost and bounds (row b of `batch_table` while a table is set);
        the cheapest finite one is found inside the launch and only its
        states and actions are written.  `std`: a scalar or [m]; `smooth` in
        [0, 1); `active` [B] uint8: trajectories with 0 are skipped.

        Returns an object with `J` [B][S], `best` [B] int32 (-1: no candidate
        of that trajectory had a finite cost) and `J_best` [B] (the bits of
        J[b, best[b]]; +inf with best == -1); of a masked trajectory NaN, -1,
        NaN.  Never worse than the start: J_best <= J[:, 0].

        `adopt=True`: `U` and `Z` take the winners' rows in place (a
        device-side select on `best`, no host synchronisation; trajectories
        with best == -1 or masked keep theirs) and the controller state is
        re-armed as `set_nominal` does, so the next round starts with records.
        No rollout is launched: `Z` already is the rollout of `U`.  `z0`,
        `x_true`, the plan, the table and a captured graph's buffers stay.
        `adopt=False`: nothing of the solver is touched; the object also has
        `Z` [B][N+1][n] and `U` [B][N][m], the winners (NaN rows where there
        is none).  `events`: a (start, stop) pair for the dispatch.

        While a reference (`set_reference`) or per-trajectory cost weights
        (`set_batch_weights`) are set the call is refused under
        `objective="shared"` (default): the candidates would be costed under
        another objective than the line search's.  `objective="search"`
        costs every candidate - and the winner's second pass - under whatever
        the line search currently uses (pddp_shoot_track_*, _weighted_*,
        _track_weighted_*, csrc/shoot.hip, mppi.hip): step t under reference
        row min(ref_start + t, L - 1), the terminal step under row
        ref_start + N's `x_goal`, with row b's diagonals of Q, Q_term, R; the
        S candidates of a trajectory share both.  With neither set it is the
        call "shared" makes, the same launch."""
        self._need_sample_problem("shoot")
        goals = self._one_sampled_objective("shoot", objective)
        B, N, n, m = self.B, self.N, self.n, self.m
        S = int(samples)
        if S < 1:
            raise _native.NativeError("shoot: %d samples" % S)
        a_std = self._action_std(std)
        self._check_active("shoot", active)
        masked = active is not None
        out = types.SimpleNamespace(
            J=self._out(masked, B, S),
            best=self._out(masked, B, dtype=torch.int32, fill=-1),
            J_best=self._out(masked, B))
        # (the winners' buffers: the caller's with adopt=False, rows without a
        # winner NaN; else scratch the select below reads)
        Zw = self._out(not adopt, B, N + 1, n)
        Uw = self._out(not adopt, B, N, m)
        p = _native.ptr
        self._launch(events, functools.partial(self._problem_call, goals=goals),
                     "pddp_shoot", B, N, S,
                     p(self.z0), p(self.U), p(self.u_min), p(self.u_max),
                     p(a_std), float(smooth), int(seed), int(sample_offset),
                     p(active), p(out.J), p(out.best), p(out.J_best), p(Zw),
                     p(Uw), self._s())
        if not adopt:
            out.Z, out.U = Zw, Uw
            return out
        won = (out.best >= 0).reshape(B, 1, 1)
        torch.where(won, Uw, self.U, out=self.U)
        torch.where(won, Zw, self.Z, out=self.Z)
        self.reset_controller_state()
        return out

    @_on_device
    def shoot_draws(self, samples, seed=0, sample_offset=0):
        """The unit normals xi `shoot(samples, seed=, sample_offset=)` draws,
        E [B][N][S][m] (pddp_shoot_draws_*): to look at, or to replay, a
        candidate."""
        S = int(samples)
        if S < 1:
            raise _native.NativeError("shoot_draws: %d samples" % S)
        E = torch.empty(self.B, self.N, S, self.m, dtype=self.dtype,
                        device=self.device)
        _native.call("pddp_shoot_draws", self.dtype, self.B, self.N, S, self.m,
                     int(seed), int(sample_offset), _native.ptr(E), self._s())
        return E

    @_on_device
    def mppi(self, samples, std, temperature, smooth=0.0, seed=0,
             sample_offset=0, iterations=1, active=None, adopt=True,
             events=None, objective="shared"):
        """Sampled shooting with a softmin-weighted (MPPI) update of the
        action sequence (pddp_mppi_*, csrc/mppi.hip): `shoot`'s S = `samples`
        candidates, costed by the same law, and instead of the cheapest one
        the sequence U + std (.) sum_s W[b][s] e_s, clamped, with
        W[b][s] = softmin_s(J[b][s] / temperature[b]) over the finite costs;
        that sequence is rolled out and costed inside the launch.  `std`,
        `smooth`, `seed`, `sample_offset`, `active`: as `shoot`.
        `temperature`: a float or [B], in cost units, > 0 (a trajectory whose
        temperature is not is treated as one without a finite candidate).

        `iterations` launches follow each other on private copies of U and Z:
        iteration k draws with `sample_offset` + k B S and takes the weighted
        rows of the trajectories it `improved` (a device-side select, no host
        synchronisation), so the call is never worse than its start.

        Returns an object with `J` [B][S], `best` [B] int32, `J_best` [B],
        `W` [B][S], `J_w` [B] (the cost of the weighted sequence; +inf with
        best == -1), `ess` [B] = 1 / sum_s W^2, `improved` [B] bool =
        isfinite(J_w) & (J_w <= J[:, 0]) - those of the LAST iteration; of a
        masked trajectory NaN / -1 / False - and `J_trace`
        [iterations + 1][B]: the base's cost, then the cost carried after each
        iteration.

        `adopt=True`: `U` and `Z` take the carried rows in place - the
        weighted ones where an iteration improved, their own elsewhere - and
        the controller state is re-armed, as `shoot` does.  `adopt=False`:
        nothing of the solver is touched; the object also has `Z` and `U`, the
        carried rows.  `events`: a (start, stop) pair for the dispatch, with
        one iteration only.

        `objective`: as `shoot` - "shared" refuses while a reference or
        per-trajectory cost weights are set, "search" costs the candidates
        and the weighted sequence under the line search's objective
        (pddp_mppi_track_*, _weighted_*, _track_weighted_*)."""
        self._need_sample_problem("mppi")
        goals = self._one_sampled_objective("mppi", objective)
        B, N, n, m = self.B, self.N, self.n, self.m
        S, K = int(samples), int(iterations)
        if S < 1:
            raise _native.NativeError("mppi: %d samples" % S)
        if K < 1:
            raise _native.NativeError("mppi: %d iterations" % K)
        if events is not None and K > 1:
            raise _native.NativeError(
                "mppi: events time ONE dispatch, %d iterations are %d" % (K, K))
        a_std = self._action_std(std, "mppi")
        lam = self._temperature("mppi", temperature)
        self._check_active("mppi", active)
        masked = active is not None
        p = _native.ptr
        U, Z = self.U.clone(), self.Z.clone()
        J_trace = torch.empty(K + 1, B, dtype=self.dtype, device=self.device)
        for k in range(K):
            out = types.SimpleNamespace(
                J=self._out(masked, B, S),
                best=self._out(masked, B, dtype=torch.int32, fill=-1),
                J_best=self._out(masked, B), W=self._out(masked, B, S),
                J_w=self._out(masked, B))
            # (rows without a weighted sequence are never selected)
            Zw, Uw = self._out(False, B, N + 1, n), self._out(False, B, N, m)
            self._launch(events,
                         functools.partial(self._problem_call, goals=goals),
                         "pddp_mppi", B, N, S,
                         p(self.z0), p(U), p(self.u_min), p(self.u_max),
                         p(a_std), p(lam), float(smooth), int(seed),
                         int(sample_offset) + k * B * S, p(active), p(out.J),
                         p(out.best), p(out.J_best), p(out.W), p(out.J_w),
                         p(Zw), p(Uw), self._s())
            out.improved = torch.isfinite(out.J_w) & (out.J_w <= out.J[:, 0])
            if k == 0:
                J_trace[0] = out.J[:, 0]
            take = out.improved.reshape(B, 1, 1)
            U, Z = torch.where(take, Uw, U), torch.where(take, Zw, Z)
            J_trace[k + 1] = torch.where(out.improved, out.J_w, J_trace[k])
        out.ess = 1.0 / (out.W * out.W).sum(dim=1)
        out.J_trace = J_trace
        if not adopt:
            out.Z, out.U = Z, U
            return out
        self.U.copy_(U)
        self.Z.copy_(Z)
        self.reset_controller_state()
        return out

    def _width(self, what, std):
        """[B][N][m] device tensor, a private copy, of a width given as a
        float, an [m] vector or a [B][N][m] tensor (the `std` a `cem` call
        returned)."""
        shape = (self.B, self.N, self.m)
        std = torch.as_tensor(std, dtype=self.dtype, device=self.device)
        if std.dim() == 0 or tuple(std.shape) == (self.m,):
            return std.expand(shape).contiguous()
        if tuple(std.shape) != shape:
            raise _native.NativeError(
                "%s: std has shape %s, expected a scalar, (%d,) or %s" % (
                    what, tuple(std.shape), self.m, shape))
        return std.clone().contiguous()

    @_on_device
    def cem(self, samples, std, elites, iterations=1, std_min=0.0, mix=0.0,
            smooth=0.0, seed=0, sample_offset=0, active=None, adopt=True,
            events=None, objective="shared"):
        """Sampled shooting with a cross-entropy (CEM) refit of the
        distribution the candidates are drawn from (pddp_cem_*, csrc/cem.hip):
        `shoot`'s S = `samples` candidates around the mean - the current `U` -
        with a width per time step and action component, costed by the same
        law; the K = `elites` cheapest finite ones are ranked out inside the
        launch and the mean and the width are refitted to them, the new mean
        is rolled out and costed in the same launch.  `std`: a float, an [m]
        vector or a [B][N][m] tensor, such as the `std` an earlier call
        returned.  `std_min`: a float or [m], the floor of the refitted width.
        `mix` in [0, 1): the share of the old distribution kept in the new one
        (0: the elites' fit alone).  `smooth`, `seed`, `sample_offset`,
        `active`: as `shoot`.

        `iterations` launches follow each other on private copies: iteration k
        draws with `sample_offset` + k B S around the distribution iteration
        k - 1 left, which moves for every trajectory with an elite (a
        device-side select, no host synchronisation).  Next to the
        distribution the call carries an incumbent: the start, replaced by an
        iteration's mean where isfinite(J_m) & (J_m <= the carried cost) - so
        the call is never worse than its start, as `shoot` and `mppi`.

        Returns an object with `J` [B][S], `rank` [B][S] int32 (-1: not
        finite), `best` [B] int32, `J_best` [B], `n_elite` [B] int32, `J_m`
        [B] (the cost of the refitted mean; +inf without a finite candidate) -
        those of the LAST iteration; of a masked trajectory NaN / -1 / 0 -,
        `mean` [B][N][m] and `std` [B][N][m], the final distribution, and
        `J_trace` [iterations + 1][B]: the start's cost, then the incumbent's
        after each iteration.

        `adopt=True`: `U` and `Z` take the incumbent's rows in place and the
        controller state is re-armed, as `shoot` does.  `adopt=False`: nothing
        of the solver is touched; the object also has `Z` and `U`, the
        incumbent's rows.  `events`: a (start, stop) pair for the dispatch,
        with one iteration only.

        `objective`: as `shoot` - "shared" refuses while a reference or
        per-trajectory cost weights are set, "search" costs the candidates
        and every iteration's mean under the line search's objective
        (pddp_cem_track_*, _weighted_*, _track_weighted_*): `J_trace[0]` is
        then the current nominal's cost under it, and the incumbent is never
        worse than the start under the objective `rounds()` optimises.
        `ref_start` is read, not moved."""
        self._need_sample_problem("cem")
        goals = self._one_sampled_objective("cem", objective)
        B, N, n, m = self.B, self.N, self.n, self.m
        S, K, iters = int(samples), int(elites), int(iterations)
        if S < 1:
            raise _native.NativeError("cem: %d samples" % S)
        if not 1 <= K <= S:
            raise _native.NativeError(
                "cem: %d elites of %d samples" % (K, S))
        if iters < 1:
            raise _native.NativeError("cem: %d iterations" % iters)
        if events is not None and iters > 1:
            raise _native.NativeError(
                "cem: events time ONE dispatch, %d iterations are %d" % (
                    iters, iters))
        sigma = self._width("cem", std)
        floor = self._action_std(std_min, "cem")
        self._check_active("cem", active)
        masked = active is not None
        p = _native.ptr
        mean = self.U.clone()
        U, Z = self.U.clone(), self.Z.clone()  # the incumbent
        J_trace = torch.empty(iters + 1, B, dtype=self.dtype,
                              device=self.device)
        for k in range(iters):
            out = types.SimpleNamespace(
                J=self._out(masked, B, S),
                rank=self._out(masked, B, S, dtype=torch.int32, fill=-1),
                best=self._out(masked, B, dtype=torch.int32, fill=-1),
                J_best=self._out(masked, B),
                n_elite=self._out(masked, B, dtype=torch.int32, fill=0),
                J_m=self._out(masked, B))
            # (rows without a refit are never selected)
            Zm, Um = self._out(False, B, N + 1, n), self._out(False, B, N, m)
            Sm = self._out(False, B, N, m)
            self._launch(events,
                         functools.partial(self._problem_call, goals=goals),
                         "pddp_cem", B, N, S, K,
                         p(self.z0), p(mean), p(self.u_min), p(self.u_max),
                         p(sigma), p(floor), float(smooth), float(mix),
                         int(seed), int(sample_offset) + k * B * S, p(active),
                         p(out.J), p(out.rank), p(out.best), p(out.J_best),
                         p(out.n_elite), p(out.J_m), p(Zm), p(Um), p(Sm),
                         self._s())
            if k == 0:
                J_trace[0] = out.J[:, 0]
            better = torch.isfinite(out.J_m) & (out.J_m <= J_trace[k])
            take = better.reshape(B, 1, 1)
            U, Z = torch.where(take, Um, U), torch.where(take, Zm, Z)
            J_trace[k + 1] = torch.where(better, out.J_m, J_trace[k])
            moved = (out.n_elite > 0).reshape(B, 1, 1)
            mean = torch.where(moved, Um, mean)
            sigma = torch.where(moved, Sm, sigma)
        out.mean, out.std, out.J_trace = mean, sigma, J_trace
        if not adopt:
            out.Z, out.U = Z, U
            return out
        self.U.copy_(U)
        self.Z.copy_(Z)
        self.reset_controller_state()
        return out

    def _one_sampled_objective(self, what, objective="shared"):
        """The `objective` of `shoot`, `mppi`, `cem`, `mppi_closed_loop` and
        `cem_closed_loop` (which has no entry point for True yet and refuses).
        "shared": the refusal while a reference or per-trajectory cost
        weights are set.  "search": True where the candidates are costed
        along the reference and / or under the weights (the entry points of
        csrc/shoot.hip, mppi.hip, cem.hip), False where neither is set - the
        call is then the one "shared" makes."""
        if objective == "search":
            return self.reference is not None or \
                self.batch_weights is not None
        if objective != "shared":
            raise _native.NativeError(
                '%s: objective is %r, expected "shared" or "search"' % (
                    what, objective))
        if self.reference is not None:
            raise _native.NativeError(
                "%s costs its candidates under ONE goal per trajectory; "
                "with a reference (set_reference) the line search's objective "
                'is another one (objective="search" costs them under it)'
                % what)
        if self.batch_weights is not None:
            raise _native.NativeError(
                "%s costs its candidates under the shared Q, Q_term, R; "
                "with per-trajectory weights (set_batch_weights) the line "
                'search\'s objective is another one (objective="search" '
                "costs them under it)" % what)
        return False

    def _temperature(self, what, temperature):
        """[B] device vector of a temperature given as a float or [B]."""
        lam = torch.as_tensor(temperature, dtype=self.dtype,
                              device=self.device)
        if lam.dim() == 0:
            lam = lam.repeat(self.B)
        if tuple(lam.shape) != (self.B,):
            raise _native.NativeError(
                "%s: temperature has shape %s, expected a scalar or (%d,)"
                % (what, tuple(lam.shape), self.B))
        return lam.contiguous()

    @_on_device
    def mppi_closed_loop(self, steps, samples, std, temperature, iterations=1,
                         smooth=0.0, seed=0, candidate_offset=0, z0=None,
                         params=None, x_goal=None, u_goal=None,
                         disturbance=None, process_std=None, obs_std=None,
                         sample_offset=0, step_offset=0, active=None,
                         log_costs=False, events=None, objective="shared"):
        """A receding-horizon MPPI trial of every trajectory on its own plant,
        all `steps` control steps in ONE launch (pddp_mppi_trial_*,
        csrc/mppi_trial.hip): per control step `iterations` iterations of
        `mppi`'s law around the plan `U` from what the controller sees - an
        iteration's weighted sequence replaces the plan where it `took`,
        isfinite(J_w) & (J_w <= J[:, 0]) - then clamp(U[b][0]) is applied to
        plant b, the trial is logged, the next state observed and the plan
        shifted by one (the last row repeated).  `samples`, `std`,
        `temperature`, `smooth`: as `mppi`.  Iteration k of control step c
        draws its candidates as `mppi(seed=, sample_offset=candidate_offset +
        (c iterations + k) B samples)` does.

        The plant (`params`, `x_goal`, `u_goal`), `disturbance`, the noise
        (`process_std`, `obs_std` with `seed`, `sample_offset`, `step_offset`),
        the start (`z0`; with `obs_std` the TRUE start, `x_true` and the first
        observation), continuation with `z0=None` and `active` are
        `mpc_closed_loop`'s, word for word: an MPPI trial and an iLQR trial
        with the same `seed`, `sample_offset` and `step_offset` run under the
        same normals (`seed` also keys the candidates, on a stream of their
        own).

        Returns an object with `X` [B][steps+1][n], `U` [B][steps][m], `J`
        [B], `Y` [B][steps+1][n] (None without `obs_std`) as
        `mpc_closed_loop`; `J0`, `J_w` [B][steps][iterations]: the cost of the
        plan and of the weighted sequence in every iteration; `took` (bool,
        from the two); `ess` [B][steps]: the effective sample size of each
        step's last iteration (0 without a finite candidate); `plans`
        [B][steps][N][m]: the plan each step applied the first row of; with
        `log_costs` `Jc` [B][steps][iterations][samples], else None.  Of a
        masked trajectory NaN / False.  No host synchronisation; `events`: a
        (start, stop) pair attached to the one launch.

        Afterwards `z0` is what the controller sees at step `steps`, `U` the
        shifted plan and `Z` its rollout, all in place, and the controller
        state is re-armed: `rounds()` polishes with iLQR, a second call with
        `z0=None`, `step_offset=steps` and `candidate_offset` advanced by
        steps * iterations * B * samples continues the trial.

        `objective="shared"` (default): refused while a reference or
        per-trajectory cost weights are set, as `mppi` is.
        `objective="search"`: the trial plans under the line search's
        objective (pddp_mppi_trial_goals_*, csrc/mppi_trial.hip).  With a
        reference control step c plans under the window that starts at row
        `ref_start + c`; the applied step is logged as `mpc_closed_loop` logs
        it - the stage cost under that row, the terminal cost under the
        next - and the plant fields supply parameters only: `x_goal` /
        `u_goal` would not be read and are refused.  Afterwards `ref_start`
        has advanced by `steps` and a captured round is dropped, so that a
        continued trial continues the reference.  Per-trajectory weights
        affect the planning only: `J` is under the shared Q, Q_term, R, the
        common yardstick.  With neither set it is the call "shared" makes."""
        what = "mppi_closed_loop"
        self._need_sample_problem(what)
        goals = self._one_sampled_objective(what, objective)
        tracking = goals and self.reference is not None
        if tracking and (x_goal is not None or u_goal is not None):
            raise _native.NativeError(
                "%s: with a reference the trial's cost is evaluated along "
                "it; the plant's x_goal / u_goal would not be read" % what)
        B, N, m = self.B, self.N, self.m
        a_std = self._action_std(std, what)
        lam = self._temperature(what, temperature)
        masked = active is not None
        p = _native.ptr
        with self._sampled_trial(
                what, steps, samples, iterations, None, z0, params, x_goal,
                u_goal, disturbance, process_std, obs_std, seed, sample_offset,
                step_offset, active, log_costs) as (T, S, K, out, plant, tail):
            out.J0, out.J_w = self._out(masked, B, T, K), \
                self._out(masked, B, T, K)
            out.ess = self._out(masked, B, T)
            out.plans = self._out(masked, B, T, N, m)
            U_work = self._out(False, B, N, m)
            name, lead = "pddp_mppi_trial", ()
            if goals:  # (the window and the weights, nullable each, not both)
                name = "pddp_mppi_trial_goals"
                lead = (self._ref_window() if tracking else (None, 0, 0)) + \
                    (p(self.batch_weights),)
            self._launch(
                events, _native.call, name, self.dtype, self._pp,
                p(self.batch_table), p(plant), *lead, B, N, S, K, T, 0, T,
                p(self.z0), p(self.U), p(self.Z), p(U_work), p(self.u_min),
                p(self.u_max), p(a_std), p(lam), float(smooth), int(seed),
                int(candidate_offset), B * S, *tail, p(out.J0), p(out.J_w),
                p(out.ess), p(out.plans), self._s())
        out.took = torch.isfinite(out.J_w) & (out.J_w <= out.J0)
        if tracking:  # the next call's window, as mpc_closed_loop leaves it
            self.ref_start += T
            self._graph = None  # (captured under another window)
        return out

    @_on_device
    def cem_closed_loop(self, steps, samples, std, elites, iterations=1,
                        std_min=0.0, mix=0.0, keep_std=False, smooth=0.0,
                        seed=0, candidate_offset=0, z0=None, params=None,
                        x_goal=None, u_goal=None, disturbance=None,
                        process_std=None, obs_std=None, sample_offset=0,
                        step_offset=0, active=None, log_costs=False,
                        events=None, objective="shared"):
        """A receding-horizon CEM trial of every trajectory on its own plant,
        all `steps` control steps in ONE launch (pddp_cem_trial_*,
        csrc/cem_trial.hip): per control step `iterations` iterations of
        `cem`'s law from what the controller sees, around a mean that starts
        as the plan `U` and a width - with `cem`'s selects between them: the
        incumbent (the plan at the step's start) is replaced by an iteration's
        mean where isfinite(J_m) & (J_m <= the carried cost), the distribution
        moves where the iteration had an elite - then clamp(incumbent[0]) is
        applied to plant b, the trial is logged, the next state observed and
        the plan shifted by one (the last row repeated).  `samples`, `std`,
        `elites`, `std_min`, `mix`, `smooth`: as `cem`.  Iteration k of control
        step c draws its candidates as `cem(seed=, sample_offset=
        candidate_offset + (c iterations + k) B samples)` does.

        `keep_std=False`: every control step starts from the width given, the
        usual CEM-MPC.  `keep_std=True`: a control step starts from the shift
        of the width the step before refitted (never below `std_min`).

        The plant, `disturbance`, the noise, the start, continuation with
        `z0=None` and `active` are `mppi_closed_loop`'s, word for word: the
        three controllers run under the same normals with the same `seed`,
        `sample_offset` and `step_offset`.

        Returns an object with `X`, `U`, `J`, `Y` as `mppi_closed_loop`;
        `J_trace` [B][steps][iterations+1]: the incumbent's cost before
        iteration 0 and after each; `J_m` [B][steps][iterations] and `n_elite`
        (int32) of every iteration; `plans` [B][steps][N][m]; `std_steps`
        [B][steps][N][m]: the width after each step's last iteration; `std`
        [B][N][m]: the width the next control step would start from - a
        continued call passes it back as `std`; with `log_costs` `Jc`
        [B][steps][iterations][samples], else None.  Of a masked trajectory
        NaN / 0 (`std`: the width given).  No host synchronisation; `events`:
        a (start, stop) pair attached to the one launch.

        Afterwards `z0`, `U` and `Z` are updated in place, the controller
        state is re-armed and records are due, as after `mppi_closed_loop`.

        `objective`: "search" with neither a reference nor per-trajectory
        weights set is the call "shared" makes; with either set both refuse -
        the tracked / weighted trial is not built yet."""
        what = "cem_closed_loop"
        self._need_sample_problem(what)
        if self._one_sampled_objective(what, objective):
            raise _native.NativeError(
                '%s: objective="search" along a reference or under '
                "per-trajectory weights: the tracked / weighted trial is not "
                "built yet" % what)
        B, N, m = self.B, self.N, self.m
        sigma = self._width(what, std)
        sigma0 = None if keep_std else sigma.clone()
        floor = self._action_std(std_min, what)
        masked = active is not None
        p = _native.ptr
        with self._sampled_trial(
                what, steps, samples, iterations, elites, z0, params, x_goal,
                u_goal, disturbance, process_std, obs_std, seed, sample_offset,
                step_offset, active, log_costs) as (T, S, I, out, plant, tail):
            out.J_trace = self._out(masked, B, T, I + 1)
            out.J_m = self._out(masked, B, T, I)
            out.n_elite = self._out(masked, B, T, I, dtype=torch.int32,
                                    fill=0)
            out.plans = self._out(masked, B, T, N, m)
            out.std_steps, out.std = self._out(masked, B, T, N, m), sigma
            work = [self._out(False, B, N, m) for _ in range(4)]
            self._launch(
                events, _native.call, "pddp_cem_trial", self.dtype, self._pp,
                p(self.batch_table), p(plant), B, N, S, int(elites), I, T, 0,
                T, p(self.z0), p(self.U), p(self.Z), *[p(w) for w in work],
                p(self.u_min), p(self.u_max), p(sigma), p(sigma0), p(floor),
                float(smooth), float(mix), int(seed), int(candidate_offset),
                B * S, *tail, p(out.J_trace), p(out.J_m), p(out.n_elite),
                p(out.plans), p(out.std_steps), self._s())
        return out

    @contextlib.contextmanager
    def _sampled_trial(self, what, steps, samples, iterations, elites, z0,
                       params, x_goal, u_goal, disturbance, process_std,
                       obs_std, seed, sample_offset, step_offset, active,
                       log_costs):
        """What `mppi_closed_loop` and `cem_closed_loop` do around their one
        launch.  Before it: the checks of the counts (`elites`: cem's, else
        None) and of `_trial_inputs`, the plant table, the outputs both have
        (`X`, `U`, `J`, `Y`, with `log_costs` `Jc`) and the trial's start.
        Yields (steps, samples, iterations, out, plant, tail); `tail`: the
        native call's arguments from `disturbance` to `Ylog`, the costs'
        buffer - `out.Jc`, or one launch's [B][samples] - among them.  After
        it the plan is a new nominal: the controller state is re-armed and
        records are due at the next round's start."""
        B, n, m = self.B, self.n, self.m
        T, S, I = int(steps), int(samples), int(iterations)
        if S < 1:
            raise _native.NativeError("%s: %d samples" % (what, S))
        if elites is not None and not 1 <= int(elites) <= S:
            raise _native.NativeError(
                "%s: %d elites of %d samples" % (what, int(elites), S))
        if I < 1:
            raise _native.NativeError("%s: %d iterations" % (what, I))
        if T < 1:
            raise _native.NativeError("%s: %d steps" % (what, T))
        step_offset, w_std, v_std, z0, disturbance = self._trial_inputs(
            what, T, z0, disturbance, process_std, obs_std, step_offset,
            active)
        plant = self._plant_table(what, params, x_goal, u_goal)
        masked = active is not None
        out = types.SimpleNamespace(
            X=self._out(masked, B, T + 1, n), U=self._out(masked, B, T, m),
            J=self._out(masked, B), Y=None,
            Jc=self._out(masked, B, T, I, S) if log_costs else None)
        x_true = self._trial_start(T, z0, v_std, seed, sample_offset,
                                   step_offset, active, out)
        Jc = out.Jc if log_costs else self._out(False, B, S)
        p = _native.ptr
        yield T, S, I, out, plant, (
            p(disturbance), p(w_std), p(v_std), int(sample_offset),
            step_offset, p(x_true), p(active), p(Jc), int(bool(log_costs)),
            p(out.X), p(out.U), p(out.J), p(out.Y))
        self.reset_controller_state()
        self._derivs_due = True

    def _plant_table(self, what, params, x_goal, u_goal):
        """[B][BATCH_ROW] plant rows of a trial whose fields are [B][.]: a
        field not given is `batch_table`'s if a table is set, else the shared
        problem's; None when that leaves the controller's own model."""
        if params is None and x_goal is None and u_goal is None:
            return None
        return self._write_fields(what, self._base_table().clone(),
                                  self._row_blocks(params, x_goal, u_goal))

    def _trial_inputs(self, what, T, z0, disturbance, process_std, obs_std,
                      step_offset, active):
        """The checks a trial's entry (`mpc_closed_loop`, `mppi_closed_loop`)
        makes on its start, disturbance, noise levels, step offset and mask:
        (step_offset, w_std, v_std, z0, disturbance) as the launches take
        them."""
        B, n = self.B, self.n
        if isinstance(step_offset, bool) or \
                not isinstance(step_offset, numbers.Integral) or \
                step_offset < 0:
            raise _native.NativeError(
                "%s: step_offset is %r, expected an integer >= 0"
                % (what, step_offset))
        step_offset = int(step_offset)
        w_std = self._noise_std("process_std", process_std, what)
        v_std = self._noise_std("obs_std", obs_std, what)
        opts = dict(dtype=self.dtype, device=self.device)
        if z0 is not None:
            z0 = torch.as_tensor(z0).to(**opts)
            if tuple(z0.shape) != (B, n):
                raise _native.NativeError(
                    "%s: z0 has shape %s, expected (%d, %d)" % (
                        what, tuple(z0.shape), B, n))
        if disturbance is not None:
            disturbance = torch.as_tensor(disturbance).to(**opts).contiguous()
            if tuple(disturbance.shape) != (B, T, n):
                raise _native.NativeError(
                    "%s: disturbance has shape %s, expected "
                    "(%d, %d, %d)" % (what, tuple(disturbance.shape), B, T, n))
        self._check_active(what, active)
        return step_offset, w_std, v_std, z0, disturbance

    def _trial_start(self, T, z0, v_std, seed, sample_offset, step_offset,
                     active, out):
        """The start of a trial: `set_nominal` from the start state - with
        `v_std` from the first observation of the true start, or, continuing
        with z0=None, from the observation held - and `out.Y` with its row 0.
        Returns `x_true` (None without `v_std`), which the solver keeps."""
        B, n = self.B, self.n
        masked = active is not None
        p = _native.ptr
        x_true = None
        if v_std is None:
            self.set_nominal(self.z0 if z0 is None else z0, self.U)
        elif z0 is None and self.x_true is not None:
            # the trial goes on: the plant at x_true, the controller at the
            # observation it holds
            x_true = self.x_true
            self.set_nominal(self.z0, self.U)
        else:
            # the true start, and the first observation under the law of every
            # later one (a skipped trajectory keeps its start)
            x_true = (self.z0 if z0 is None else z0).clone(
                memory_format=torch.contiguous_format)
            y0 = x_true.clone()
            _native.call("pddp_mpc_observe", self.dtype, B, n, p(x_true),
                         p(v_std), int(seed), int(sample_offset), step_offset,
                         p(active), p(y0), self._s())
            self.set_nominal(y0, self.U)
        self.x_true = x_true  # (set_nominal dropped it)
        if x_true is not None:
            out.Y = self._out(masked, B, T + 1, n)
            out.Y[:, 0] = self.z0 if not masked else torch.where(
                active.bool().unsqueeze(1), self.z0, out.Y[:, 0])
        return x_true

    @_on_device
    def mpc_closed_loop(self, steps, rounds_per_step, z0=None, params=None,
                        x_goal=None, u_goal=None, disturbance=None, tol=5e-6,
                        max_reg=1e10, active=None, events=None,
                        process_std=None, obs_std=None, seed=0,
                        sample_offset=0, step_offset=0):
        """A receding-horizon trial of every trajectory on its own plant, on
        the device (the batched `_apply_controller(..., mpc=True)`,
        pddp.py:209-245, around `forward(mpc=True)`, ilqr.py:355-362, with the
        sample models as the plant).  Starts with `set_nominal(z0 or self.z0,
        self.U)`; then `steps` control steps, each

            rounds(rounds_per_step, tol, max_reg, n_iterations=1)
            pddp_mpc_advance_*   (csrc/mpc_advance.hip)

        The rounds are one `step()` of every controller - a trajectory that is
        accepted, has converged or has exhausted its regularisation goes
        inactive, a round with nothing live is a no-op - cut off after
        `rounds_per_step` attempts; the advance applies clamp(U[b][0]) to plant
        b, adds `disturbance[b][t]` ([B][steps][n], optional), logs the trial,
        shifts U by one (the last row repeated), rolls out the new nominal
        from the plant's next state under the controller's model and re-arms
        the controller state.  The controller's model is the solver's as it
        stands, with `batch_table` or without, and the rounds take whatever
        sequence `_plan()` answers.  The step sizes are the solver's own:
        `mpc_alphas` at construction gives the reference's MPC schedule.

        Plant fields `params` ([B][P], dt first), `x_goal` ([B][na]), `u_goal`
        ([B][m]) as in `closed_loop`; a field not given is `batch_table`'s if
        a table is set, else the shared problem's; none given: the plant is
        the controller's model.  The cost of the trial uses the plant row's
        goals.  `active` [B] uint8: trajectories with 0 are neither optimised
        nor advanced, their outputs NaN (`X`, `U`, `J`) and 0.

        Returns an object with `X` [B][steps+1][n], `U` [B][steps][m] (the
        clamped actions applied), `J` [B], `states` [B][steps] (the iLQRState
        each control step's rounds ended in) and `unfinished` [B][steps]
        uint8 (1: the rounds ran out before the step was decided; the nominal
        applied is then the one the last accepted attempt left).  No host
        synchronisation; everything is stream-ordered on the solver's stream,
        `events` a (start, stop) pair recorded around the whole loop.
        Afterwards the solver holds the nominal rolled out from x_T with the
        shifted actions and a re-armed controller state: a second call with
        `z0=None` continues the trial.

        With a reference (`set_reference`) control step t optimises against
        the window that starts at row `ref_start + t`, the advance is
        pddp_mpc_advance_track_* - the stage cost of the trial under that
        row, the terminal cost under the next - and the plant fields supply
        parameters only (`x_goal`, `u_goal` are not read).  Only the integer
        offset changes from step to step; afterwards `ref_start` has advanced
        by `steps`, so that a continued trial continues the reference.

        With per-trajectory cost weights (`set_batch_weights`) the rounds
        inside the trial optimise under each trajectory's weights; the cost
        the trial reports (`J`) is under the shared problem's Q, Q_term, R
        and the plant row's goals - the common yardstick.  The advance kernel
        is unchanged.  With weights AND a reference the rounds run the
        pddp_*_track_weighted_* kernels on the window at `ref_start + t`; the
        advance is the tracked one, unchanged: `J` is under the shared
        matrices along the reference.

        `process_std`, `obs_std` (each a scalar or [n]; None: none of it):
        noise drawn inside the advance (pddp_mpc_advance_noisy_*,
        csrc/mpc_advance_noise.hip, with the reference window when a reference
        is set) - the plant steps to x' + disturbance + process_std (.) w_t,
        and with `obs_std` the controller re-plans from y_t = x_t + obs_std (.)
        v_t instead of the plant's state.  Trial b is rollout `sample_offset`
        + b and control step t step `step_offset` + t of `closed_loop`'s
        generator: `closed_loop(1, process_std=, obs_std=, seed=,
        sample_offset=)` runs the fitted policy under the very normals this
        trial re-plans under, and `closed_loop_draws(1, which, seed,
        sample_offset, steps=)[:, :, 0]` returns them.  With both None the
        launches are those of the call without these keywords.
        With `obs_std`, `z0` (or `self.z0`) is the TRUE start: the solver keeps
        the plant's state in `x_true` [B][n], the first observation y_0 is
        drawn at step `step_offset` (pddp_mpc_observe_*) and is what
        `set_nominal` gets, and the returned object has `Y` [B][steps+1][n],
        the observations (None without `obs_std`); `X` and `J` are the true
        states and their cost.  After such a trial a call with `z0=None` and
        `obs_std` continues it: the plant is at `x_true`, the controller at
        the held `self.z0`, no new first observation is drawn; pass
        `step_offset` = the steps already done.  `set_nominal` from outside,
        or a trial without `obs_std`, drops `x_true`."""
        self._need_sample_problem("mpc_closed_loop")
        B, N, n, m = self.B, self.N, self.n, self.m
        T, R = int(steps), int(rounds_per_step)
        if T < 1 or R < 1:
            raise _native.NativeError(
                "mpc_closed_loop: %d steps of %d rounds" % (T, R))
        step_offset, w_std, v_std, z0, disturbance = self._trial_inputs(
            "mpc_closed_loop", T, z0, disturbance, process_std, obs_std,
            step_offset, active)
        plant = self._plant_table("mpc_closed_loop", params, x_goal, u_goal)
        masked = active is not None
        out = types.SimpleNamespace(
            X=self._out(masked, B, T + 1, n), U=self._out(masked, B, T, m),
            J=self._out(masked, B),
            states=self._out(masked, B, T, dtype=torch.int32, fill=0),
            unfinished=self._out(masked, B, T, dtype=torch.uint8, fill=0),
            Y=None)
        record = _native.lib().pddp_event_record
        if events is not None:
            _native.check(record(events[0], self._s()), "pddp_event_record")
        p = _native.ptr
        x_true = self._trial_start(T, z0, v_std, seed, sample_offset,
                                   step_offset, active, out)
        if masked:  # (the skipped ones take no part in the rounds either)
            self.active.mul_(active)
            self.fresh.mul_(active)
        b = self._buffers()
        nominal = (p(self.z0), b.U, b.Z, b.u_min, b.u_max)
        plants = (p(plant), p(disturbance))
        outputs = (p(active), p(out.X), p(out.U), p(out.J), p(out.states),
                   p(out.unfinished), b.mu, b.delta, b.state, b.iter,
                   b.active, b.fresh, b.n_live)
        tracking = self.reference is not None
        noise = ()
        if w_std is not None or v_std is not None:
            # (one entry point, with a reference window or a NULL one)
            name = "pddp_mpc_advance_noisy"
            noise = (p(w_std), p(v_std), int(seed), int(sample_offset),
                     step_offset, p(x_true), p(out.Y))
        else:
            name = "pddp_mpc_advance_track" if tracking else "pddp_mpc_advance"
        advance = getattr(_native.lib(),
                          name + "_" + _native.suffix(self.dtype))
        for t in range(T):
            self.rounds(R, tol, max_reg, n_iterations=1)
            ref = self._ref_window() if tracking else \
                ((None, 0, 0) if noise else ())
            _native.check(  # (problem, [reference,] shapes, nominal, ...)
                advance(self._pp, p(self.batch_table), *ref, B, N, T, t,
                        *nominal, *plants, *noise, *outputs, self._s()), name)
            # (as set_nominal leaves the host flags: every nominal is new)
            self._derivs_due = True
            if tracking:  # the next step's window; its records are all new
                self.ref_start += 1
        if tracking:
            self._graph = None  # (captured under another window)
        if events is not None:
            _native.check(record(events[1], self._s()), "pddp_event_record")
        return out

    def rounds(self, count, tol=5e-6, max_reg=1e10, n_iterations=50,
               events=None):
        """`count` rounds; in one launch where pddp_round_nominal_f32 applies
        (`events` are then attached to that launch), `count` calls of round()
        otherwise."""
        if count > 1 and self._plan(self.kernel_variant) == ONE_LAUNCH and \
                self.round_nominal(tol, max_reg, n_iterations, events=events,
                                   rounds=count):
            return
        for _ in range(count):
            self.round(tol, max_reg, n_iterations)

    def round(self, tol=5e-6, max_reg=1e10, n_iterations=50, variant=None,
              backward_events=None, always_derivs=False, search_events=None):
        """One attempt of every live trajectory (no host sync): derivative
        records of the trajectories whose nominal is new, backward sweep, and
        - fused into one launch where the problem allows - line search,
        accept / regularisation schedule and the records of the accepted
        nominals (so the first call is a no-op from the second round on)."""
        if variant is None:
            variant = self.kernel_variant
        plan = self._plan(variant, search_events)
        if plan == ONE_LAUNCH and self.round_nominal(
                tol, max_reg, n_iterations, events=backward_events):
            return
        nominal = plan in (ONE_LAUNCH, NOMINAL_FUSED) and \
            self.sweep_nominal(events=backward_events)
        if not nominal:  # on records (derivs() / backward() sync stale ones)
            if self._records_due(always_derivs):
                self.derivs(mask=self.fresh)
            self.backward(active=self.active, variant=variant,
                          events=backward_events)
        # (records evaluated inside the sweep: the fused launch then writes
        # none, and `fresh` stays set until the next sweep has summed the stage
        # costs of the new nominal into J_opt)
        self._derivs_due = False
        if self._search_accept(tol, max_reg, n_iterations,
                               events=search_events, records=not nominal):
            return
        ev = None
        if nominal:
            # nominal+separate (> 16 step sizes); records by derivs from now on
            self._sweep_nominal_done(False)
        elif self.plugin is None and search_events is not None:
            # the separate line search is what gets timed then
            ev, self.last_search_timed = search_events, "line_search"
        self._launch(ev, self.line_search, self.active)
        self.accept(tol, max_reg, n_iterations)
        self._derivs_due = nominal

    def graph_ok(self):
        """A round can be captured: native sample problem, or a plugin whose
        round is all HIP launches and sync-free torch ops (the BNN path)."""
        return self.plugin is None or self.plugin.capture_ok(self)

    _STATE = ("Z", "U", "_rec", "L", "J_opt", "gains", "gains_acc", "Jc",
              "bwd_status", "state", "iter", "mu", "delta", "active", "fresh",
              "n_live")

    @_on_device
    def capture_round(self, tol=5e-6, max_reg=1e10, n_iterations=50):
        """Captures round() - a fixed launch sequence on device-resident state
        - into a hipGraph; `replay_round()` then issues it with one launch.
        For the launch-bound regime: small batches and the receding-horizon
        loop (BASELINE.json configs[4]).

        Native sample problems: one graph (the masked records launch is part
        of it).  Plugin (BNN) rounds: two graphs sharing one memory pool - the
        round with the derivative rollout (every record recomputed, rows
        blended by the `fresh` mask) and the round of retries only (ilqr.py
        :125-139 with a larger mu: nominals, hence records, unchanged); fit()
        picks one per round from the counts it reads back anyway."""
        if not self.graph_ok():
            raise _native.NativeError(
                "graph capture needs a round without host synchronisation: "
                "this plugin runs autograd / torch fallbacks inside a round")
        self._graphs_fresh()
        key = (float(tol), float(max_reg), int(n_iterations),
               self.kernel_variant)
        if self._graph is not None and self._graph[0] == key:
            return self._graph[1]
        if self._per_trajectory():
            self.sync_records()  # (a launch that belongs to no round)
        torch.cuda.synchronize(self.device)
        if self.plugin is None:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                # the masked records launch is always part of the graph (a
                # no-op when no nominal is fresh): a replay after
                # set_nominal() must not sweep the previous nominal's records
                self.round(tol, max_reg, n_iterations, always_derivs=True)
            self._graph = (key, graph, None)
            self._graph_nominal = self._nominal_sweep_applied()
            return graph
        # warm-up outside the capture (noise caches, masks, per-kernel
        # attributes, allocator) on a snapshot of the solver's state
        snap = {k: getattr(self, k).clone() for k in self._STATE}
        self._plugin_round(tol, max_reg, n_iterations, True, False)
        for k, v in snap.items():
            getattr(self, k).copy_(v)
        torch.cuda.synchronize(self.device)
        g_full = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_full):
            self._plugin_round(tol, max_reg, n_iterations, True, True)
        g_retry = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_retry, pool=g_full.pool()):
            self._plugin_round(tol, max_reg, n_iterations, False, True)
        self._graph = (key, g_full, g_retry)
        return g_full

    def _plugin_round(self, tol, max_reg, n_iterations, with_derivs, in_graph):
        if with_derivs:
            self.derivs(mask=self.fresh, in_graph=in_graph)
        self.backward(active=self.active, variant=self.kernel_variant)
        self.line_search(active=self.active)
        self.accept(tol, max_reg, n_iterations)

    @_on_device
    def replay_round(self, with_derivs=True):
        g = self._graph[1] if (with_derivs or self._graph[2] is None) \
            else self._graph[2]
        self._rec_stale |= self._graph_nominal  # (its sweep: no records)
        g.replay()

    def fit(self, n_iterations=50, tol=5e-6, max_reg=1e10, on_round=None,
            max_rounds=None, graph=False, rounds_per_sync=1,
            rounds_per_launch=1):
        """Runs rounds until every trajectory left the fit loop
        (ilqr.py:298-314). Returns the number of rounds.  With `graph=True`
        rounds are hipGraph replays and the host looks at the live count only
        every `rounds_per_sync` rounds (a round with nothing live is a no-op
        on the device, so the result does not depend on it).
        `rounds_per_launch` > 1 (no `on_round`, no graph): that many rounds per
        launch where pddp_round_nominal_f32 applies (`rounds()`), the live
        count read after each launch - the same results, up to
        rounds_per_launch - 1 no-op rounds more."""
        if graph:
            self.capture_round(tol, max_reg, n_iterations)
            if self.plugin is not None:
                rounds_per_sync = 1  # which graph comes next is read back
        rpl = 1 if (graph or on_round is not None) else max(1, rounds_per_launch)
        rounds = 0
        need_derivs = True
        while True:
            if graph:
                self.replay_round(need_derivs)
            elif rpl > 1 and self._one_launch_applied():
                # (only once the one-launch round has applied: a rounds()
                # that loops over round() would run past the last live one)
                c = rpl if max_rounds is None else min(rpl, max_rounds - rounds)
                self.rounds(c, tol, max_reg, n_iterations)
                rounds += c - 1
            else:
                self.round(tol, max_reg, n_iterations)
            rounds += 1
            if on_round is not None:
                on_round(rounds, self)
            if max_rounds is not None and rounds >= max_rounds:
                break
            if not (rpl > 1 and self._one_launch_applied()) and \
                    rounds % rounds_per_sync:
                continue
            # the one host sync: live trajectories, and (plugin graphs) whether
            # any nominal changed
            live, fresh = torch.stack([self.active.sum(),
                                       self.fresh.sum()]).tolist()
            need_derivs = fresh > 0
            if live == 0:
                break
        return rounds
