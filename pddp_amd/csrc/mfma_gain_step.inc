// mfma_gain_step.inc - the scalar gains of one step of a matrix-core sweep with
// m = 1 (every lane the same scalars, ilqr.py:629-657):
// the eig clamp or the regularised Q_uu, the closed-form BoxQP with the
// reference's loop as fall-back, the status precedence.  One text, included by
// the step of riccati_mfma16.hpp, riccati_mfma16_nominal.hpp, riccati_mfma32.hpp
// and (CHOL = false) riccati_mfma32s.hpp - included, not a function: inlined as
// a function it leaves the compiler another instruction order in most kernels.
// Reads  T, BOUNDED, FAST, CHOL; Quu, Quug, Qu, reg, umin, umax, Un, lstep0,
//        ls_tail, lane, n; the includer's macros
//        PDDP_GAIN_ROW  this lane's group holds row n of Q~
//        PDDP_GAIN_COL  this lane's column of Q~
//        PDDP_GAIN_KROW its entry of the row K is made from (Q_uz or Q_uz_reg)
// (undefined again at the end of this text).
// Defines kt, sE; updates kprev (the BoxQP's warm start) and status (the first
// failure stays).
    int st = PDDP_BWD_OK;
    T qp_Q;
    if constexpr (CHOL) {
      qp_Q = Quug;  // Cholesky of Q_uu_reg                          (ilqr.py:595)
      if (!BOUNDED && (!(Quug > T(0)) || !is_finite(Quug))) st = PDDP_BWD_NOT_PD;
    } else {
      if (!is_finite(Quu)) st = PDDP_BWD_NAN;     // eig raises (ilqr.py:631)
      const T e = (Quu < T(0)) ? T(1e-12) : Quu;  // ilqr.py:633
      qp_Q = e + reg;                             // ilqr.py:634
    }
    T kt, sE;
    int stt = st;
    if constexpr (BOUNDED) {
      n4::QpClosed<T, FAST> qc;
      qc.solve(kprev, qp_Q, Qu, umin - Un, umax - Un);
      kt = qc.x;
      bool Kz = !qc.free_, fail = qc.fail;
      if (__builtin_amdgcn_ballot_w64(qc.slow) != 0) {
        const n4::SlowQpOut<T> o = n4::boxqp1_outlined<T, FAST>(
            kprev, qp_Q, Qu, umin - Un, umax - Un, lstep0, ls_tail, lane);
        kt = o.x;
        Kz = (o.result_free & 1) == 0;
        fail = o.result_free < 2;
      }
      // (a NaN Q_uu fails `eig` before the BoxQP is reached, ilqr.py:631)
      if (fail && st == PDDP_BWD_OK) stt = PDDP_BWD_BOXQP_FAILED;
      if constexpr (FAST) sE = Kz ? T(0) : qc.inv;
      else sE = Kz ? T(0) : n4::div_<false>(n4::div_<false>(T(1), qc.U), qc.U);
    } else {
      sE = n4::div_<FAST>(T(1), qp_Q);  // (E / e) E^T               (ilqr.py:636)
      kt = -(sE * Qu);
      // NaN in k or K raises (ilqr.py:639-640)
      const bool nanK = (PDDP_GAIN_ROW) && (PDDP_GAIN_COL < n) &&
                        (sE * PDDP_GAIN_KROW != sE * PDDP_GAIN_KROW);
      if (!CHOL && (kt != kt || __builtin_amdgcn_ballot_w64(nanK) != 0))
        stt = PDDP_BWD_NAN;
    }
    if (status == PDDP_BWD_OK && stt != PDDP_BWD_OK) status = stt;
    kprev = kt;
#undef PDDP_GAIN_ROW
#undef PDDP_GAIN_COL
#undef PDDP_GAIN_KROW
