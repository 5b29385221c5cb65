/* libwct_hip -- the choice of feature transform: the part of the C ABI behind `--transform`.
 *
 * The reference (MingSun-Tse/Collaborative-Distillation) has one feature transform, whiten_and_color (PytorchWCT/util_wct.py:62-131),
 * and one lighter helper it does not route its cascade through (adaptive instance normalisation, model/model_cd.py:22-40).  This header
 * lets a context choose among three closed-form transforms.  Everything in wct_hip.h holds here too: return codes, wct_last_error, device
 * pointers, one context = one stream, asynchronous calls.
 *
 * The operators (per level)
 *
 * All three are affine maps of the content feature, csF = M cF + b, blended as util_wct.py:219 does:
 *     M = alpha T + (1 - alpha) I,   b = alpha (mu_s - T mu_c)
 * mu_c, cov_c: the unbiased content mean and covariance from the raw moments (n, sum, sumsq).  S, mu_s: what the level's style slot
 * holds (the wct_style_export layout: S = cov_s^(1/2) on the live subspace [C*C], then mu_s [C]) -- so cached, exported, imported,
 * broadcast and blended (wct_style_blend, wct_stylize_interp) statistics serve every transform unchanged.
 *
 *   WCT_TRANSFORM_WCT    T = S cov_c^(-1/2)                       the reference's transform; the default; unchanged bit for bit
 *   WCT_TRANSFORM_OT     T = S B^(-1/2) S,  B = sym(S cov_c S)     the optimal-transport (Monge) map between the two Gaussians (Olkin &
 *                        Pukelsheim 1982; Lu et al., "A Closed-form Solution to Universal Style Transfer", ICCV 2019; Mroueh 2019): T is
 *                        symmetric, reaches the same target covariance as WCT (T cov_c T = cov_s), and among all linear maps that do it
 *                        moves the content features least.  B^(-1/2) is the PSEUDO-inverse square root: eigen-directions of B with
 *                        lambda <= 1e-12 lambda_max contribute exactly zero.  This form needs S and ONE matrix function on the content
 *                        side, like WCT, and never inverts cov_c.  Where B is singular any finite treatment of its null space gives the
 *                        same action on the content's support: B v = 0 means cov_c^(1/2) S v = 0, i.e. (S v) is orthogonal to range(cov_c).
 *   WCT_TRANSFORM_ADAIN  T = diag(sqrt((cov_s_ii + eps) / (cov_c_ii + eps))),  eps = WCT_ADAIN_EPS,  cov_s_ii = SUM_k S_ik^2
 *                        per-channel mean / standard-deviation matching (model_cd.py:22-40); no matrix function on the content side;
 *                        a channel dead on both sides maps with sqrt(eps / eps) = 1.
 *
 * Arithmetic: fp64 on the fp64 matrix cores, fixed summation orders -- results are functions of the inputs alone, reproducible bit
 * for bit across calls and contexts.  The inverse square root of B runs through wct_solve's solver -- coupled Newton-Schulz on the
 * matrix cores, single-CU Jacobi behind it for C <= 128; the deflated iteration for C > 128 -- with an iteration schedule of its own:
 * B's spectrum is the product of two covariances' (condition 1e6 .. 1e9 on real features), so the scaled iteration starts from an
 * assumed lower bound 1e-10 with a budget of 32 steps (17-18 executed whatever the condition up to 1e10).
 *
 * What follows the context's mode
 *
 * The mode is consumed where (M, b) is made: wct_solve -- its style-side moments are turned into S first, as always --, wct_transform,
 * wct_content_solve, wct_style_transfer_level, wct_stylize / _prepared / _u8, wct_synthesize, wct_stylize_color, wct_stylize_smooth,
 * wct_level_sharded / wct_stylize_sharded -- WCT_SHARD_FAST_FOLD is ignored under a non-wct mode: every rank folds (M, b) --, and
 * wct_stylize_interp -- under ot / adain its target is the style whose square-root covariance is the BLENDED slot SUM_k lambda_k S_k
 * (and mean SUM_k lambda_k mu_k); it is no longer the linear mix of the K single-style results, which holds for wct only.
 * The properties of the 16x path hold under every mode: no host synchronisation, no allocation after the first call of a size, capture
 * into a HIP graph.  wct_workspace_bytes / wct_reserve are exact under the mode current at the call (ot adds one buffer of
 * 2 C^2 + C doubles; the wct-mode numbers do not move).
 * Refused with WCT_ERR_INVALID under a non-wct mode, before anything is written: wct_stylize_regions and wct_stylize_blend: their K-slot
 * per-pixel paths use weighted-moment normalisations that are defined for wct only.
 * `--numpy` (+ I on cov_c, wct_set_numpy_variant) is a wct-only variant: wct_set_transform(ot | adain) is WCT_ERR_INVALID while it is on,
 * and switching wct_set_numpy_variant on is WCT_ERR_INVALID under a non-wct mode.
 */
#ifndef WCT_HIP_TRANSFORM_H
#define WCT_HIP_TRANSFORM_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_TRANSFORM_WCT 0
#define WCT_TRANSFORM_OT 1
#define WCT_TRANSFORM_ADAIN 2
#define WCT_ADAIN_EPS 1e-5           /* model_cd.py:22 */

/* The context's transform (default WCT_TRANSFORM_WCT).  A mode outside 0..2 is WCT_ERR_INVALID; so is a non-wct mode while the numpy
 * variant is on.  Prepared style slots stay valid across a change of mode -- except slots rotated by wct_style_diversify
 * (wct_hip_diverse.h), which only the wct transform reads as they are meant: a non-wct mode is WCT_ERR_STATE while one is rotated. */
int wct_set_transform(wct_ctx* ctx, int mode);
int wct_get_transform(const wct_ctx* ctx, int* mode);

/* (M, b) of one transform from raw content moments and a style slot; mode-explicit, the context's mode is neither read nor changed.
 * C even, 2..512, n_c >= 2, like wct_solve.  sum_c [C], sumsq_c [C*C], style_stats [C*C + C] (the wct_style_export layout), M [C*C],
 * b [C]: device fp64.  info (host, may be NULL; reading it synchronises the stream): info[0] = how the content-side matrix function
 * was solved, in wct_solve's coding (1..99: iterations of the matrix-core path; 100 + sweeps: the Jacobi net) -- of B for ot, of cov_c
 * for wct, 0 for adain; info[1] = 0.  Under WCT_TRANSFORM_WCT the numpy variant of the context is NOT applied. */
int wct_transform_solve(wct_ctx* ctx, int mode, int C, double n_c, const double* sum_c, const double* sumsq_c, const double* style_stats,
                        double alpha, double* M, double* b, int* info);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_TRANSFORM_H */
