/*
 * p2c_ref.c -- TEST INFRASTRUCTURE ONLY.
 *
 * CPU restatement of the archived parameter-to-coefficient tracker
 * kernel_GPUHC_trifocal_2op1p_30x30_P2C, the checker of the HIP P2C mode
 * (include/p2c/hc_trifocal_p2c.h).  Restated, with the lines they restate:
 *   arxived_GPU_code/gpu-idx-evals/dev-eval-indxing-trifocal_2op1p_30x30_P2C.cuh
 *     :45-64   coefficient interpolation,  :74-117  dH/dx, dH/dt, H
 *   arxived_GPU_code/gpu-kernels/kernel_GPUHC_trifocal_2op1p_30x30_P2C.cu:56-263
 *     with the explicit Runge-Kutta helpers of magmaHC/dev-get-new-data.cuh:37-71
 * The linear solve is the oracle's orc_cgesv_gpu (oracle/hc_oracle.c, linked).
 * Arithmetic as in the oracle: built with
 * -ffp-contract=off, the only FMAs are the fmaf calls of cmul / cmadd / cmsub.
 * The coefficient generator is the project's (the reference ships none) and is
 * the same arithmetic as hc_p2c_coefficients (csrc/hc_host.cpp).
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef _OPENMP
#include <omp.h>
#endif

#define NV 30
#define NT 312
#define NPP 34
#define NK 38          /* Num_of_Coeffs_from_Params + 1                       (P2C.cu:296) */
#define HX_TERMS 8     /* dHdx_Max_Terms                                      (P2C.cu:292) */
#define HX_PARTS 4     /* dHdx_Max_Parts                                      (P2C.cu:293) */
#define HT_TERMS 16    /* dHdt_Max_Terms                                      (P2C.cu:294) */
#define HT_PARTS 5     /* dHdt_Max_Parts                                      (P2C.cu:295) */
#define HX_ENTRY (HX_TERMS * HX_PARTS)   /* dHdx_Entry_Offset                 (P2C.cu:299) */
#define HX_ROW (NV * HX_ENTRY)           /* dHdx_Row_Offset                   (P2C.cu:300) */
#define HT_ROW (HT_TERMS * HT_PARTS)     /* dHdt_Row_Offset                   (P2C.cu:301) */

void orc_cgesv_gpu(float *A, const float *b, float *x);   /* oracle/hc_oracle.h */

typedef struct { float x, y; } cf;
static inline cf cmk(float x, float y) { cf r; r.x = x; r.y = y; return r; }
static inline cf cadd(cf a, cf b) { return cmk(a.x + b.x, a.y + b.y); }
static inline cf csub(cf a, cf b) { return cmk(a.x - b.x, a.y - b.y); }
static inline cf cscale(cf a, float s) { return cmk(a.x * s, a.y * s); }
static inline cf cdivs(cf a, float s) { return cmk(a.x / s, a.y / s); }
static inline cf cmul(cf a, cf b) { return cmk(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)); }
static inline cf cmadd(cf acc, cf a, cf b) {
    return cmk(fmaf(-a.y, b.y, fmaf(a.x, b.x, acc.x)), fmaf(a.y, b.x, fmaf(a.x, b.y, acc.y)));
}
static inline cf cmsub(cf acc, cf a, cf b) {
    return cmk(fmaf(a.y, b.y, fmaf(-a.x, b.x, acc.x)), fmaf(-a.y, b.x, fmaf(-a.x, b.y, acc.y)));
}
static inline cf ld(const float *p, int i) { return cmk(p[2 * i], p[2 * i + 1]); }
static inline void st(float *p, int i, cf v) { p[2 * i] = v.x; p[2 * i + 1] = v.y; }

/* 1 - 0.05 in C double, the clamp of P2C.cu:122 (the PH kernels write 0.95) */
double p2c_one_minus_005(void) { volatile double a = 1, b = 0.05; return a - b; }

/* The project's generator: C0 = s_a s_b, C1 = s_a d_b + d_a s_b, C2 = d_a d_b, D0 = C1, D1 = C2 + C2 */
void p2c_coefficients(int n, const int *map, const float *sp, const float *dp, float *chx, float *cht) {
    for (int s = 0; s < n; s++) {
        const float *d = dp + (size_t)s * NPP * 2;
        for (int k = 0; k < NK; k++) {
            const int a = map[2 * k], b = map[2 * k + 1];
            const cf c0 = cmul(ld(sp, a), ld(sp, b));
            const cf c1 = cadd(cmul(ld(sp, a), ld(d, b)), cmul(ld(d, a), ld(sp, b)));
            const cf c2 = cmul(ld(d, a), ld(d, b));
            float *hx = chx + ((size_t)s * NK + k) * 3 * 2, *ht = cht + ((size_t)s * NK + k) * 2 * 2;
            st(hx, 0, c0); st(hx, 1, c1); st(hx, 2, c2);
            st(ht, 0, c1); st(ht, 1, cadd(c2, c2));
        }
    }
}

/* eval.cuh:45-64 -- coefHx_k = C0 + C1*t + (C2*t)*t, coefHt_k = D0 + D1*t (complex * float) */
static void interpolate(float t, const float *chx, const float *cht, cf *cHx, cf *cHt) {
    for (int k = 0; k < NK; k++) {
        cHx[k] = cadd(cadd(ld(chx, 3 * k), cscale(ld(chx, 3 * k + 1), t)), cscale(cscale(ld(chx, 3 * k + 2), t), t));
        cHt[k] = cadd(ld(cht, 2 * k), cscale(ld(cht, 2 * k + 1), t));
    }
}

/* eval.cuh:74-83 -- A[r][c] = sum_j ((c*coef[k])*x[u])*x[v]; index j*4 + part + c*32 + r*960.
   Padding terms (c = 0) add exact zeros and are skipped, as in the oracle. */
static inline cf hx_entry(const int *T, int r, int c, const cf *x, const cf *co) {
    cf acc = cmk(0.0f, 0.0f);
    for (int j = 0; j < HX_TERMS; j++) {
        const int *e = T + j * HX_PARTS + c * HX_ENTRY + r * HX_ROW;
        if (e[0] == 0) continue;
        acc = cmadd(acc, cmul(cscale(co[e[1]], (float)e[0]), x[e[2]]), x[e[3]]);
    }
    return acc;
}
/* eval.cuh:93-100 (sub = 1, -=) and :110-117 (sub = 0, +=): (((c*coef[k])*x[u])*x[v])*x[w]; index j*5 + part + r*80 */
static inline cf ht_row(const int *D, int r, const cf *x, const cf *co, int sub) {
    cf acc = cmk(0.0f, 0.0f);
    for (int j = 0; j < HT_TERMS; j++) {
        const int *e = D + j * HT_PARTS + r * HT_ROW;
        if (e[0] == 0) continue;
        const cf P = cmul(cmul(cscale(co[e[1]], (float)e[0]), x[e[2]]), x[e[3]]);
        acc = sub ? cmsub(acc, P, x[e[4]]) : cmadd(acc, P, x[e[4]]);
    }
    return acc;
}

/* dH/dx (row-major 30x30), dH/dt and H (with the Hx coefficients, P2C.cu:197) at n points */
void p2c_eval_batched(int n, const int *hx, const int *ht, const float *xf, const float *chx, const float *cht,
                      const float *t, float *HX, float *HT, float *H) {
    for (int s = 0; s < n; s++) {
        cf x[NV + 1], cHx[NK], cHt[NK];
        for (int i = 0; i <= NV; i++) x[i] = ld(xf + (size_t)s * (NV + 1) * 2, i);
        interpolate(t[s], chx + (size_t)s * NK * 3 * 2, cht + (size_t)s * NK * 2 * 2, cHx, cHt);
        for (int r = 0; r < NV; r++) {
            for (int c = 0; c < NV; c++) st(HX + (size_t)s * NV * NV * 2, r * NV + c, hx_entry(hx, r, c, x, cHx));
            st(HT + (size_t)s * NV * 2, r, ht_row(ht, r, x, cHt, 1));
            st(H + (size_t)s * NV * 2, r, ht_row(ht, r, x, cHx, 0));
        }
    }
}

typedef struct { int max_steps, max_corrections, inc_steps, num_threads; } p2c_settings;
typedef struct { int32_t steps, corrections, inliers21, inliers31; } p2c_path_stats;   /* == hcPathStats */

/* the 32-slot __shfl_down_sync tree of P2C.cu:211-214 (slots 30, 31 read as 0) */
static inline float tree_sum(const float *v) {
    float a[16], b[8], c[4], d[2];
    for (int l = 0; l < 16; l++) a[l] = v[l] + ((l + 16 < NV) ? v[l + 16] : 0.0f);
    for (int l = 0; l < 8; l++) b[l] = a[l] + a[l + 8];
    for (int l = 0; l < 4; l++) c[l] = b[l] + b[l + 4];
    for (int l = 0; l < 2; l++) d[l] = c[l] + c[l + 2];
    return d[0] + d[1];
}

static void solve(const int *hx, const int *ht, const cf *x, const cf *cHx, const cf *cRhs, int sub, cf *kk) {
    float A[NV * NV * 2], B[NV * 2];
    for (int r = 0; r < NV; r++) {
        for (int c = 0; c < NV; c++) st(A, r * NV + c, hx_entry(hx, r, c, x, cHx));
        st(B, r, ht_row(ht, r, x, cRhs, sub));
    }
    orc_cgesv_gpu(A, B, (float *)kk);
}

static void one_path(const p2c_settings *s, int bid, const float *ssf, const int *hx, const int *ht,
                     const float *chx_all, const float *cht_all, float *tracks, uint8_t *conv_o, uint8_t *inf_o,
                     p2c_path_stats *st_o) {
    const int trk = bid % NT, smp = bid / NT;                               /* :60-61 */
    const float *chx = chx_all + (size_t)smp * NK * 3 * 2;                   /* :68 */
    const float *cht = cht_all + (size_t)smp * NK * 2 * 2;                   /* :69 */
    cf x[NV + 1], xl[NV + 1], sols[NV + 1], cHx[NK], cHt[NK], kk[NV];
    float *tr = tracks + (size_t)bid * (NV + 1) * 2;
    for (int i = 0; i < NV; i++) {                                          /* :89-91 */
        sols[i] = ld(ssf + (size_t)trk * (NV + 1) * 2, i);
        x[i] = ld(tr, i);
        xl[i] = x[i];
    }
    sols[NV] = x[NV] = xl[NV] = cmk(1.0f, 0.0f);                            /* :93-95 */
    int succ = 0;                                                           /* :96 */
    float t0 = 0.0f, t_step = 0.0f, delta_t = 0.05f;                        /* :75 */
    int end_zone = 0, isSucc = 0, isInf = 0, nsteps = 0, ncorr = 0;
    float vs[NV], vc[NV];
    const cf one = cmk(1.0f, 0.0f);                                         /* gc = MAGMA_C_ONE */

    for (int step = 0; step <= s->max_steps; step++) {                      /* :108 */
        if (!((double)t0 < 1.0 && (1.0 - (double)t0 > 0.0000001))) break;  /* :109, :254 */
        if (!end_zone && (double)fabsf(1.0f - t0) <= 0.0500001) end_zone = 1;   /* :114 */
        if (end_zone) {                                                     /* :118-124 */
            if (delta_t > fabsf(1.0f - t0)) delta_t = fabsf(1.0f - t0);
        } else if ((double)delta_t > fabs(1 - 0.05 - (double)t0)) {
            delta_t = (float)fabs(1 - 0.05 - (double)t0);
        }
        t_step = t0;                                                        /* :126 */
        const float h2 = (float)(0.5 * (double)delta_t);                    /* :127 */
        nsteps++;
        /* k1 (:133-142) */
        interpolate(t0, chx, cht, cHx, cHt);
        solve(hx, ht, x, cHx, cHt, 1, kk);
        /* create_x_for_k2 (get-new-data:37-45): s += ((k*dt)*gc*1.0)/6; x += k*(h2*gc); t += h2 */
        for (int r = 0; r < NV; r++) {
            sols[r] = cadd(sols[r], cdivs(cscale(cmul(cscale(kk[r], delta_t), one), 1.0f), 6.0f));
            x[r] = cadd(x[r], cmul(kk[r], cmk(h2, 0.0f)));
        }
        t0 += h2;
        /* k2 (:147-156) */
        interpolate(t0, chx, cht, cHx, cHt);
        solve(hx, ht, x, cHx, cHt, 1, kk);
        /* create_x_for_k3 (get-new-data:47-57): s += ((k*dt)*gc*1.0)/3; x = x_last + k*(h2*gc) */
        for (int r = 0; r < NV; r++) {
            sols[r] = cadd(sols[r], cdivs(cscale(cmul(cscale(kk[r], delta_t), one), 1.0f), 3.0f));
            x[r] = cadd(xl[r], cmul(kk[r], cmk(h2, 0.0f)));
        }
        /* k3 (:162-167): no interpolation, the coefficients of k2 (the same t) */
        solve(hx, ht, x, cHx, cHt, 1, kk);
        /* create_x_for_k4 (get-new-data:59-70): s += ((k*dt)*gc*1.0)/3; x = x_last + k*(dt*gc); t += h2 */
        for (int r = 0; r < NV; r++) {
            sols[r] = cadd(sols[r], cdivs(cscale(cmul(cscale(kk[r], delta_t), one), 1.0f), 3.0f));
            x[r] = cadd(xl[r], cmul(kk[r], cmk(delta_t, 0.0f)));
        }
        t0 += h2;
        /* k4 (:172-181) */
        interpolate(t0, chx, cht, cHx, cHt);
        solve(hx, ht, x, cHx, cHt, 1, kk);
        for (int r = 0; r < NV; r++) {                                      /* :184-185 */
            sols[r] = cadd(sols[r], cdivs(cscale(cscale(kk[r], delta_t), 1.0f), 6.0f));
            x[r] = sols[r];
        }
        for (int c = 0; c < s->max_corrections; c++) {                      /* :194-226 */
            solve(hx, ht, x, cHx, cHx, 0, kk);                              /* :196-197: H with the Hx coefficients of k4 */
            ncorr++;
            for (int r = 0; r < NV; r++) {                                  /* :204-208 */
                x[r] = csub(x[r], kk[r]);
                vs[r] = kk[r].x * kk[r].x + kk[r].y * kk[r].y;
                vc[r] = x[r].x * x[r].x + x[r].y * x[r].y;
            }
            const float ns = tree_sum(vs), nc = tree_sum(vc);
            isSucc = (double)ns < 0.000001 * (double)nc;                    /* :217 */
            isInf = (double)nc > 1e14;                                      /* :218 */
            if (isInf) break;
            if (isSucc) break;
        }
        if (isInf) break;                                                   /* :228 */
        if (!isSucc) {                                                      /* :233-241 */
            delta_t = (float)((double)delta_t * 0.5);
            for (int r = 0; r < NV; r++) { x[r] = xl[r]; sols[r] = xl[r]; }
            succ = 0;
            t0 = t_step;
        } else {                                                            /* :242-252 */
            succ++;
            for (int r = 0; r < NV; r++) { xl[r] = x[r]; sols[r] = x[r]; }
            if (succ >= s->inc_steps) { succ = 0; delta_t *= 2.0f; }
        }
    }
    for (int i = 0; i < NV; i++) st(tr, i, x[i]);                           /* :259 */
    conv_o[bid] = ((double)t0 >= 1.0 || (1.0 - (double)t0 <= 0.0000001)) ? 1 : 0;   /* :261 */
    inf_o[bid] = isInf ? 1 : 0;                                             /* :262 */
    if (st_o) { st_o[bid].steps = nsteps; st_o[bid].corrections = ncorr; st_o[bid].inliers21 = 0; st_o[bid].inliers31 = 0; }
}

/* tracks: (312*N) x 31 complex, in/out, path b = sample*312 + track (x[30] is not written) */
void p2c_track(const p2c_settings *s, int num_samples, const float *start_sols, const int *hx, const int *ht,
               const float *chx, const float *cht, float *tracks, uint8_t *conv, uint8_t *inf,
               p2c_path_stats *stats) {
    const int total = num_samples * NT;
#ifdef _OPENMP
    const int nth = s->num_threads > 0 ? s->num_threads : omp_get_max_threads();
#pragma omp parallel for schedule(dynamic) num_threads(nth)
#endif
    for (int b = 0; b < total; b++) one_path(s, b, start_sols, hx, ht, chx, cht, tracks, conv, inf, stats);
}
