// mfma_operand.inc - which word of a record entry (k, j) of the augmented
// matrices reads: PDDP_OPERAND_F for F~ = [F_z | F_u | 0], PDDP_OPERAND_L for
// L~ = [[L_zz, L_uz^T, L_z], [L_uz, L_uu, L_u]] with the first-order terms in
// column PDDP_OPERAND_JZ (the includer's macros: two lvalues and 15 or 31,
// undefined again at the end); word S, the first of the slot's zeroed padding,
// for entries outside the matrices.  Reads lay, n, S, k, j.  Included per entry
// by riccati_mfma16.hpp and riccati_mfma16_nominal.hpp; riccati_mfma32.hpp and
// riccati_mfma32s.hpp keep their own form (see there).
    PDDP_OPERAND_F = (k < n) ? (j < n ? lay.oFz + k * n + j
                                      : (j == n ? lay.oFu + k : S))
                             : S;
    int o = S;
    if (k < n) {
      if (j < n) o = lay.oLzz + k * n + j;
      else if (j == n) o = lay.oLuz + k;  // L_uz^T
      else if (j == PDDP_OPERAND_JZ) o = lay.oLz + k;
    } else if (k == n) {
      if (j < n) o = lay.oLuz + j;
      else if (j == n) o = lay.oLuu;
      else if (j == PDDP_OPERAND_JZ) o = lay.oLu;
    }
    PDDP_OPERAND_L = o;
#undef PDDP_OPERAND_F
#undef PDDP_OPERAND_L
#undef PDDP_OPERAND_JZ
