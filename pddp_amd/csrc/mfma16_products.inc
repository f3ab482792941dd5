// mfma16_products.inc - the two products of a 16x16 step and row n of the
// result (riccati_mfma16.hpp, riccati_mfma16_nominal.hpp).  Reads V, Vz, the
// gathered Fa, La, PDDP_M16_F(r) (f[k] of this lane's row r: the includer's
// gather, undefined again at the end), reg, n and gn, rn, where row n sits
// (defined here under PDDP_M16_ROW_N_HERE).  Defines X, Q and Quu, Qu, rowg,
// Quug.
    T ffrow = T(0);  // (f^T F~)[j]: f^T F_z for j < n, f.f at j = n
    if constexpr (CHOL) {
#pragma unroll
      for (int r = 0; r < 4; ++r) ffrow += PDDP_M16_F(r) * Fa[r];
      ffrow += __shfl_xor(ffrow, 16);
      ffrow += __shfl_xor(ffrow, 32);
    }
    // ---- X = V F~ ; X[:, 15] = V_z (column 15 of F~ is zero)
    Acc X = {Vz[0], Vz[1], Vz[2], Vz[3]};
#pragma unroll
    for (int r = 0; r < 4; ++r) X = TL::mma(V[r], Fa[r], X);
    // ---- Q~ = L~ + F~^T X
    Acc Q = {La[0], La[1], La[2], La[3]};
    Q = TL::mma(Fa[0], X[0], Q);
    Q = TL::mma(Fa[1], X[1], Q);
    Q = TL::mma(Fa[2], X[2], Q);
    Q = TL::mma(Fa[3], X[3], Q);
    // row n (register rn of lane group gn) of Q~ is (Q_uz | Q_uu | Q_u at
    // column 15)
#ifdef PDDP_M16_ROW_N_HERE  // (riccati_mfma16.hpp computes them in its step)
    const int gn = TL::group_of(n), rn = TL::reg_of(n);
#undef PDDP_M16_ROW_N_HERE
#endif
    const T rowv = rn == 0 ? Q[0] : (rn == 1 ? Q[1] : (rn == 2 ? Q[2] : Q[3]));
    const T Quu = TL::read_lane(rowv, gn * 16 + n);
    const T Qu = TL::read_lane(rowv, gn * 16 + 15);
    // the regularised row (Q_uz_reg | Q_uu_reg) of the Cholesky branch
    const T rowg = CHOL ? rowv + reg * ffrow : rowv;
    const T Quug = CHOL ? TL::read_lane(rowg, gn * 16 + n) : Quu;
#undef PDDP_M16_F
