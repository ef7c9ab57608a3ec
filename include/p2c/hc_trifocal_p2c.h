/*
 * hc_trifocal_p2c.h -- the archived parameter-to-coefficient (P2C) tracker, the
 * first rung of the reference's ablation ladder.
 *
 * Replaces kernel_GPUHC_trifocal_2op1p_30x30_P2C
 * (arxived_GPU_code/gpu-kernels/magmaHC-kernels.hpp, implemented at
 * arxived_GPU_code/gpu-kernels/kernel_GPUHC_trifocal_2op1p_30x30_P2C.cu:56-263
 * with gpu-idx-evals/dev-eval-indxing-trifocal_2op1p_30x30_P2C.cuh:32-118).
 *
 * A header of its own, beside hc_trifocal.h (same rules of the boundary, same
 * hcStatus / hcComplex / hcStream, same workspace): the P2C mode takes other
 * index tables and per-sample coefficient blocks instead of parameters, and no
 * struct of hc_trifocal.h changes for it (the ABI version stays 2).
 *
 * Index tables (the reference's dHdx_indx_P2C.txt / dHdt_indx_P2C.txt, int32):
 *   hx_index  [row][column][term][part]  30 x 30 x 8 x 4, parts (c, k, x_u, x_v)
 *   ht_index  [row][term][part]          30 x 16 x 5,     parts (c, k, x_u, x_v, x_w)
 *   k in 0..37 names a coefficient, x in 0..30 an unknown (x[30] = 1); a padding
 *   term has c = 0.
 * Coefficient blocks, one per sample (hcComplex):
 *   coeffs_hx [sample][k][order]  N x 38 x 3: coefHx_k(t) = C0 + C1 t + (C2 t) t
 *   coeffs_ht [sample][k][order]  N x 38 x 2: coefHt_k(t) = D0 + D1 t
 * Evaluations (complex x float for the interpolation, left to right for a term):
 *   dH/dx[r][c] =   sum_j ((c_j coefHx_k) x_u) x_v
 *   dH/dt[r]    = - sum_j (((c_j coefHt_k) x_u) x_v) x_w
 *   H[r]        =   sum_j (((c_j coefHx_k) x_u) x_v) x_w      (the Hx coefficients)
 */
#ifndef HC_TRIFOCAL_P2C_H
#define HC_TRIFOCAL_P2C_H

#include "../hc_trifocal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HC_P2C_NUM_COEFFS    38     /* Num_of_Coeffs_from_Params + 1 */
#define HC_P2C_HX_INDEX_SIZE 28800  /* 30 x 30 x 8 x 4 */
#define HC_P2C_HT_INDEX_SIZE 2400   /* 30 x 16 x 5 */

/* The P2C launch's own argument block (device pointers). */
typedef struct {
    const int32_t *hx_index;       /* d_Hx_idx_array                               */
    const int32_t *ht_index;       /* d_Ht_idx_array                               */
    const hcComplex *coeffs_hx;    /* d_phc_coeffs_Hx, 114 per sample              */
    const hcComplex *coeffs_ht;    /* d_phc_coeffs_Ht,  76 per sample              */
} hcP2cArgs;                       /* 32 bytes */

/* GPU-HC tracking of 312*N paths with the archived P2C kernel's semantics: the
   archived ..._PH kernel (hc_trifocal_2op1p_30x30_track_ph: explicit RK helpers,
   no path truncation) with the evaluations above, the coefficients interpolated
   where that kernel interpolates its parameters (before the stages 1, 2 and 4 of
   a step; the corrector keeps the fourth stage's), and an initial step of 0.05.
   args: start_sols / tracks (or their pointer arrays), converge, infinity,
   settings and stats as for hc_trifocal_2op1p_30x30_track; start_params,
   target_params, diff_params and unified_index are not read and may be NULL.
   A NULL p2c or a NULL pointer in it returns HC_ERROR_INVALID_VALUE before any
   device work.  No time slicing: a workspace of hc_trifocal_workspace_size()
   bytes is all it uses.  The workspace's tables are rebuilt when the launch
   before it on the same workspace used other tables (of either format). */
hcStatus hc_trifocal_2op1p_30x30_track_p2c(const hcTrackArgs *args, const hcP2cArgs *p2c, void *workspace,
                                           size_t workspace_bytes, hcStream stream);

/* Batched evaluation of dH/dx (row-major 30x30), dH/dt and H of the P2C tables
   at n points: x n x 31, coeffs_hx n x 38 x 3, coeffs_ht n x 38 x 2, t n floats. */
hcStatus hc_trifocal_p2c_eval_batched(int n, const int32_t *hx_index, const int32_t *ht_index, const hcComplex *x,
                                      const hcComplex *coeffs_hx, const hcComplex *coeffs_ht, const float *t,
                                      hcComplex *Hx, hcComplex *Ht, hcComplex *H, void *workspace,
                                      size_t workspace_bytes, hcStream stream);

/* Host: the coefficient blocks of num_samples samples.  coeff_map 38 x 2 ints:
   coefficient k is p_a p_b with p(t) = start + t diff, so with s = start_params
   (34 complex) and d = diff_params (34 per sample)
     C0 = s_a s_b,  C1 = s_a d_b + d_a s_b,  C2 = d_a d_b,  D0 = C1,  D1 = C2 + C2
   in fp32 complex with the products of the arithmetic specification (DESIGN.md
   section 4).  The reference ships no generator: this rounding is the project's.
   Returns HC_ERROR_INVALID_VALUE for a NULL pointer, a negative count or a map
   entry outside 0..33. */
hcStatus hc_p2c_coefficients(int num_samples, const int32_t *coeff_map, const hcComplex *start_params,
                             const hcComplex *diff_params, hcComplex *coeffs_hx, hcComplex *coeffs_ht);

#ifdef __cplusplus
}
#endif
#endif /* HC_TRIFOCAL_P2C_H */
