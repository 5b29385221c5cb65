/* libwct_hip -- attention-weighted style statistics (soft swap) at one cascade level: the part of the C ABI behind
 * `--swap_match attention | attention_whitened`.
 *
 * Between "one set of style statistics for the whole image" (AdaIN / WCT) and "one style patch per pixel" (wct_hip_swap.h): every content
 * position gets its OWN style mean and standard deviation, taken over all style positions and weighted by a softmax of feature similarity
 * (SANet: Park & Lee, CVPR 2019; AdaAttN: Liu et al., ICCV 2021 -- without their learnt 1 x 1 projections, so the shipped encoders and
 * decoders are all it needs).  Everything in wct_hip.h holds here too: return codes, wct_last_error, device pointers, one context = one
 * stream, asynchronous calls.  Every entry returns WCT_ERR_INVALID -- wct_last_error names the entry -- before anything is written when
 * an argument is bad.
 *
 * Definitions
 *
 * Feature maps are NHWC fp32.  Content map cF [h, w, C], Nq = h w queries; style map sF [hs, ws, C], Nk = hs ws keys.  Limits: C a
 * multiple of 4 in 4 .. 512; 2 <= Nq, Nk < 2^31; every pointer a multiple of 16.
 *
 * Standardised map.  X~ = (X - mu_X) / sqrt(v_X + WCT_ADAIN_EPS) per channel, mu_X and v_X the unbiased mean and variance from
 *                    wct_moments; v_X < 0 from round-off counts as 0: wct_apply_labeled with one label, M = diag(1 / sigma_X),
 *                    b = -mu_X / sigma_X (fp64 maps used in fp32).
 * Match domain.      WCT_ATTN_STANDARD: Q = c~F, K = s~F (AdaAttN's domain).  WCT_ATTN_WHITENED: the whitened maps of both sides,
 *                    wct_swap_level's W (X - mu) with the same W = cov^(-1/2) and mu (wct_hip_swap.h: wct_moments +
 *                    wct_transform_solve against (I, 0)).  The patch swap applies (W, -W mu) to the un-centred map in fp32, which is
 *                    1e-6 of the largest unit value from fp64 by itself: nothing to an arg-max, but the size of this header's
 *                    tolerances.  Here the map is centred in fp64 (mu = sum / n), multiplied by W in fp64 in ascending channel order
 *                    and rounded to fp32 once.
 * Unit rows.         q^_p = Q_p / sqrt(|Q_p|^2 + WCT_ATTN_EPS), k^ likewise: |Q_p|^2 an fp64 sum in a fixed order, r = fp32(1 / sqrt(.)),
 *                    q^ = fl(Q r).  Every operand of the score product has magnitude <= 1.
 * Weights.           A(p, k) = softmax_k(tau <q^_p, k^_k>), 0 <= tau <= WCT_ATTN_MAX_TEMP: logits in [-tau, tau]; e^(-2 tau) >= 1.6e-28 is
 *                    a normal fp32 number, so neither a row sum nor a weight underflows in fp32 however the maximum is handled.
 * Values.            V = s~F, the standardised style map, never the raw one (|V| <= sqrt(Nk) for any input).
 *                    m_p = SUM_k A(p, k) V_k     e_p = SUM_k A(p, k) V_k^2     var_p = max(e_p - m_p^2, 0)       per channel
 * Result.            csF_p = alpha (sigma_s (sqrt(var_p) c~F_p + m_p) + mu_s) + (1 - alpha) cF_p,  sigma_s = sqrt(v_s + WCT_ADAIN_EPS).
 * tau = 0: every query has m = 0 and var = (Nk - 1) / Nk  v_s / (v_s + eps): AdaIN with the population variance.  tau -> infinity: the
 * 1 x 1 nearest-feature swap.
 *
 * Arithmetic of wct_attn_stats (csrc/attn.hip)
 *
 * A flash-attention forward on the f16 matrix cores (16x16x32 MFMAs) in the f16x3 split of the convolutions -- x = hi + lo (two f16),
 * products hi.hi + hi.lo + lo.hi, fp32 accumulators -- with every operand brought into the f16 range by a POWER OF TWO, never by a clamp:
 *   scores   q^ and k^ are multiplied by 2^12 before the split (|x| <= 4096; the split's absolute floor 2^-25 is then 2^-37 of a unit
 *            row), the fp32 accumulator by tau 2^-24.  Channels enter in ascending 32-channel steps.
 *   maximum  a RUNNING row maximum over the key tiles (online softmax): P = exp(s - max so far) lies in (0, 1]; at a tile that raises a
 *            row's maximum the row's sum and accumulators are multiplied by exp(old - new) first.
 *   P        is multiplied by 2^15 BEFORE its conversion (P' <= 32768).  P' >= 2^-3, i.e. P >= 2^-18, keeps 22 bits; below that the
 *            conversion rounds to a multiple of 2^-24: a weight moves by at most 2^-40 of the row's largest, so the weight mass a
 *            conversion can drop or add is <= Nk 2^-40 of the row sum (2.4e-7 at Nk = 2^18).  The row sum is the fp32 sum of the
 *            CONVERTED hi + lo, the same numbers that multiply V.
 *   V        enters as it is: the accepted range of an external V is |V| < 65504 (beyond it the conversion gives infinity and the
 *            affected outputs are NaN), which holds every standardised map (|V| <= sqrt(2^31) = 46341).
 *   V^2      fl(V V) is multiplied by 2^(14 - floor(log2 fl(vmax^2))), vmax = max |V| over the whole map (a two-launch maximum that ignores
 *            NaN; the exponent is kept in -60 .. 40), so the largest square lies in [2^14, 2^15] and a square's conversion error is
 *            <= 2^-39 of the largest.  The result is multiplied back by the inverse power.
 *   end      mean = fl(accV / l), e = fl(fl(accW / l) 2^-k), var = fl(e - fl(mean mean)), negative -> 0 (a NaN stays a NaN).
 * No score or weight is ever written to memory.  A workgroup owns WCT_ATTN_QUERY_TILE queries (16 per wave) and walks the keys in
 * ascending index order in tiles of WCT_ATTN_KEY_TILE, whatever the sizes.  For C > 128 the value channels are split into slabs of 128 over the grid and
 * the scores recomputed per slab: equal scores, so the split is exact.  A query's (mean, var) row is a function of its q^ row and the key
 * set (k^, V, in order) alone: not of the query's position, the query tiling, the slab split or the launch split.
 * Bounded launches: at most WCT_ATTN_QUERY_CHUNK QUERIES per launch (queries are independent: the split cannot change a bit and no
 * state crosses launches).  The wct_debug_set key "attn_query_chunk" = n overrides it (n >= 1; 0 restores the default) when the
 * environment has WCT_DEBUG set.  No software barrier, spin wait or atomic anywhere.
 *
 * Range contract.  These kernels clamp nothing and never touch the context's range flag (wct_range_poll).  A non-finite input makes the
 * affected outputs NaN, never a clamped number: a NaN or infinity in V[k, c] -> mean[:, c] and var[:, c] of EVERY query, nothing else; in
 * k^[k, :] -> every output; in q^[p, :] -> mean[p, :] and var[p, :].  Inside wct_attn_level the encoders raise the flag as they always do.
 *
 * wct_attn_apply, fp32, no contraction, correctly rounded square root (sigma32 = fp32(sigma_s), mu32 = fp32(mu_s)):
 *   out = fl(fl(alpha fl(fl(sigma32 fl(fl(fl(sqrt(var)) c_std) + mean)) + mu32)) + fl(fl(1 - alpha) cF))
 *
 * Context memory.  The two encoded features, the standardised and unit maps of both sides, a projection scratch, the transposed whitening matrix, (mean, var), the blended
 * feature and a small block (mu_s, sigma_s, the partial maxima and the scale of V^2) belong to the context: allocated on first use of a
 * size ON TOP of wct_workspace_bytes, scratch in the sense of the "poison" hook, sized and allocated before the first launch of a call
 * (WCT_ERR_NOMEM with nothing enqueued).  The buffers shared with the rest of the library grow as in wct_swap_level.
 */
#ifndef WCT_HIP_ATTN_H
#define WCT_HIP_ATTN_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_ATTN_EPS 1e-12
#define WCT_ATTN_MAX_TEMP 32
#define WCT_ATTN_STANDARD 0
#define WCT_ATTN_WHITENED 1
#define WCT_ATTN_QUERY_TILE 64
#define WCT_ATTN_KEY_TILE 32
/* Queries per launch: 512 workgroups per value slab.  One launch against relu3_1 of a 2048 x 2048 style (262 144 keys, C = 64) costs
 * 9.9e12 f16 flop: 31 ms measured on the MI355X (313 TFLOP/s over the 16 launches of a 3840 x 2160 content; DESIGN.md, "Attention statistics"). */
#define WCT_ATTN_QUERY_CHUNK 32768

/* unit_out [h, w, C] = the unit rows of the map's projection into `domain`; std_out [h, w, C] (may be NULL) = the standardised map.
 * WCT_ERR_INVALID: a NULL feat or unit_out, h w < 2, C not a multiple of 4 in 4 .. 512, domain outside {0, 1}, a misaligned pointer, an
 * output that overlaps feat or the other output. */
int wct_attn_project(wct_ctx* ctx, const float* feat, int h, int w, int C, int domain, float* unit_out, float* std_out /* may be NULL */);
/* mean, var [Nq, C] of the values v [Nk, C] under the weights of qhat [Nq, C] against khat [Nk, C].  WCT_ERR_INVALID: a NULL pointer,
 * Nq or Nk < 2, C as above, tau outside [0, WCT_ATTN_MAX_TEMP] or not finite, a misaligned pointer, an output that overlaps an input or
 * the other output. */
int wct_attn_stats(wct_ctx* ctx, const float* qhat, int Nq, const float* khat, const float* v, int Nk, int C, float tau,
                   float* mean /* [Nq, C] */, float* var /* [Nq, C] */);
/* out [n, C] from (mean, var) of wct_attn_stats, the standardised content c_std, the content cF and the style's mu_s, sigma_s.
 * WCT_ERR_INVALID: a NULL pointer, n < 1, C as above, alpha not finite, a misaligned map, out overlapping any input. */
int wct_attn_apply(wct_ctx* ctx, const float* mean, const float* var, const float* c_std, const float* cF, int n, int C,
                   const double* mu_s, const double* sigma_s /* device fp64 [C] */, float alpha, float* out);
/* wct_encode of both images at `level`, the three calls above, wct_decode: planar 3 x Ho x Wo into out (Ho = h << (level - 1)).
 * WCT_ERR_INVALID: a NULL pointer, level outside 2 .. 5, domain outside {0, 1}, tau outside [0, 32] or not finite, alpha not finite, a
 * feature map of fewer than 2 positions.  On the 16x path it never synchronises the host, allocates nothing after the first call of a
 * size and can be captured into a HIP graph. */
int wct_attn_level(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs, int Ws, int domain, float tau,
                   float alpha, float* out, int* Ho, int* Wo);
/* The 5 -> 1 cascade of wct_stylize, num_run times, with level `attn_level` (2 .. 5) run through wct_attn_level and every other level
 * through wct_style_transfer_level under the context's transform mode: bit-identical to that composition of public calls.  Refusals as
 * for wct_attn_level, and num_run < 1. */
int wct_stylize_attn(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, int attn_level /* 2..5 */,
                     int domain, float tau, float alpha, int num_run, float* out, int* Ho, int* Wo);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_ATTN_H */
