// mfma16_value_update.inc - the value function of a 16x16 step from the
// transpose tile, T[col][row] = Q~[row][col] with Q_uz_reg in row 15
// (riccati_mfma16.hpp, riccati_mfma16_nominal.hpp):
//   V' = sym(Q_zz) + c Q_uz^T Q_uz,  V_z' = Q_z + Q_uz^T w
// Reads tile, Q, n, g, j and kt, sE, c, w, c2, wz; writes V, Vz.
    const T Quz_j = tile[j * 16 + n];  // Q~[n][j]
    const T Qg_j = CHOL ? tile[j * 16 + 15] : T(0);  // Q_uz_reg[j]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = TL::row(g, r);
      const T QT = tile[k * 16 + j];      // Q~[j][k]
      const T Quz_k = tile[k * 16 + n];   // Q~[n][k]
      const T sym = T(0.5) * (Q[r] + QT);
      if constexpr (CHOL) {
        // V' = sym + K^T Quu K + K^T Quz + Quz^T K,  K = -sE Q_uz_reg
        const T Qg_k = tile[k * 16 + 15];
        const T v = sym + c2 * (Qg_k * Qg_j) - sE * (Qg_k * Quz_j + Quz_k * Qg_j);
        // (no masks on V', V_z': their entries outside the n x n block only
        // ever meet zero rows / columns of F~ in the next step's products)
        V[r] = v;
        Vz[r] = (j == 15) ? Q[r] + Quz_k * kt - Qg_k * wz : T(0);
      } else {
        V[r] = n4::fma_(c * Quz_k, Quz_j, sym);
        Vz[r] = (j == 15) ? n4::fma_(Quz_k, w, Q[r]) : T(0);
      }
    }
