/* libwct_hip -- guided-filter smoothing by the content image: the part of the C ABI behind `--smooth_radius`.
 *
 * The reference (MingSun-Tse/Collaborative-Distillation) stops at the decoder (PytorchWCT/WCT.py:120-128); on photographs its result
 * shows the spatial distortion every WCT cascade has: straight edges wobble, flat regions take on texture.  The remedy that needs no
 * other weights is the smoothing step of Li et al., "A Closed-Form Solution to Photorealistic Image Stylization" (ECCV 2018), in its
 * fast form: the guided image filter of He, Sun and Tang ("Guided Image Filtering", ECCV 2010 / TPAMI 2013) with the content photograph
 * as a COLOUR guide.  It is a post-pass at the image edge, next to wct_luma_merge and the uint8 conversion of save_image (wct_planar_to_u8; WCT.py:128).
 * Everything in wct_hip.h holds here too (wct_hip_color.h is included for the WCT_COLOR_* mask of wct_stylize_smooth): return codes, wct_last_error, device pointers, one context = one stream, asynchronous calls.
 * Both entries run on the context's stream, never synchronise on the 16x path, and return WCT_ERR_INVALID -- wct_last_error names the
 * entry -- before anything is written when an argument is bad.
 *
 * Definition
 *
 * Guide I: planar 3 x Hg x Wg fp32.  Source p: planar 3 x Ho x Wo fp32, Ho <= Hg, Wo <= Wg; the guide's top-left Ho x Wo window is read
 * (the cascade returns 16 floor(H / 16) x 16 floor(W / 16): floor pooling drops trailing rows and columns).  Any 4-byte alignment.
 * Integer radius r >= 1, eps > 0 relative to images in [0, 1].
 *
 * Window.  w(y, x) = [y - r, y + r] x [x - r, x + r] CLIPPED to the Ho x Wo image, and every mean is the window's sum times the fp64
 * reciprocal of its number of in-image pixels: the box filter of He et al.'s reference implementation -- no padding, no reflection.
 * A radius larger than the image is legal (the window is then the image) up to WCT_SMOOTH_MAX_RADIUS.
 *
 *   mean_I (3), mean_p (3), corr_II (3 x 3 symmetric), corr_Ip (3 x 3)     windowed means of I, p, I I^T, I p^T: 21 in all
 *   Sigma  = corr_II - mean_I mean_I^T + eps Id           cov_Ip = corr_Ip - mean_I mean_p^T
 *   a      = Sigma^-1 cov_Ip   (3 x 3: column c maps the guide to output channel c)        b = mean_p - a^T mean_I
 *   q_c(y, x) = SUM_i mean_a[i][c](y, x) I_i(y, x) + mean_b[c](y, x)       mean_a, mean_b: windowed means of a, b: 12 more
 *
 * Arithmetic.  Every window sum is fp64, of exact fp64 products of the fp32 inputs (one fma each).  A box is two separable running
 * sums -- rows, then columns -- that add the entering sample and drop the leaving one, so the cost per pixel does not grow with r; the
 * sums between the two directions are fp64 planes in the context (below).  They are restarted from a directly summed window every
 * clamp(4 r, 128, 2048) rows and every 4096 columns, so no sum is carried across more than about 4096 updates behind the <= 2 r + 1
 * terms of its restart: the window means are within ~1e-12 of the exact ones for values in [-1, 2].  Sigma, the solve -- a CHOLESKY
 * factorisation Sigma = L L^T with three forward and three back substitutions; Sigma is symmetric positive definite with smallest
 * eigenvalue >= eps -- and b are fp64.  a and b ARE stored in fp32 between the two stages (12 planes); that rounding is the larger part
 * of the distance to an all-fp64 evaluation, ~1e-7.  The second-stage sums and the final dot product are fp64, rounded ONCE to fp32.
 * NOT clamped on the planar path.  No floating-point atomics.  The order in which any sum is formed is a function of (Ho, Wo, r)
 * alone -- never of CU count, grid size, addresses, alignment or call history -- so the result is bitwise reproducible across calls,
 * views and contexts.
 *
 * Context memory.  21 fp64 planes + 12 fp32 planes of Ho x Wo (216 bytes per pixel: 1.8 GB at 3840 x 2160) belong to the context:
 * allocated on first use of a size, ON TOP of wct_workspace_bytes, not covered by wct_reserve, like the buffers of wct_stylize_color;
 * scratch in the sense of the "poison" hook.
 */
#ifndef WCT_HIP_SMOOTH_H
#define WCT_HIP_SMOOTH_H

#include "wct_hip_color.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_SMOOTH_MAX_RADIUS 2048   /* a larger radius is WCT_ERR_INVALID: the restart of a running sum adds 2 r + 1 terms in sequence */
#define WCT_SMOOTH_EPS 1e-3          /* the command line's default: a look, not a measurement */

/* q = guided filter of src by guide.  Exactly one of out_planar (fp32, 3 x Ho x Wo) and out_hwc (uint8, Ho x Wo x 3, any alignment) is
 * non-NULL; out_hwc takes the round_mode conversion of wct_planar_to_u8 and is byte-identical to wct_planar_to_u8 of the planar result.
 * out_planar == src is allowed (src is last read before the first output is written).  An output that overlaps the guide is refused:
 * the last kernel reads the guide while it writes.  Also WCT_ERR_INVALID: a NULL image, both or neither output, an empty shape,
 * Ho > Hg or Wo > Wg, radius < 1 or > WCT_SMOOTH_MAX_RADIUS, eps not finite or <= 0, round_mode outside {0, 1}. */
int wct_guided_filter(wct_ctx* ctx, const float* src, int Ho, int Wo, const float* guide, int Hg, int Wg, int radius, double eps,
                      float* out_planar, uint8_t* out_hwc, int round_mode);
/* = wct_stylize, or wct_stylize_color with WCT_COLOR_MATCH when color_mode (0, or the WCT_COLOR_* mask of wct_hip_color.h) has MATCH --
 * the cascade of WCT.py:120-125, num_run times -- then wct_guided_filter of the result with the ORIGINAL content as guide, then
 * wct_luma_merge against the original content if color_mode has WCT_COLOR_LUMA.  Bit-identical to that composition of public calls.
 * On the 16x path it never synchronises, allocates nothing after the first call of a size (wct_debug_get "ws_allocs" does not move)
 * and can be captured into one HIP graph.  Its intermediates -- the filter's planes above, sized for H x W, the matched style and the
 * un-merged result of wct_stylize_color -- are context buffers on top of wct_workspace_bytes, scratch in the sense of the "poison"
 * hook.  The prepared style slot of every level and the f16x3 range flag behave as in the cascade it wraps: afterwards the slots hold
 * the MATCHED style's statistics with WCT_COLOR_MATCH, the given style's otherwise.  out must hold 3*H*W floats and must not overlap
 * the content (it is the guide); color_mode outside 0..3, num_run < 1 and the filter's refusals of radius and eps are WCT_ERR_INVALID. */
int wct_stylize_smooth(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run,
                       int color_mode, int radius, double eps, float* out, int* Ho, int* Wo);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_SMOOTH_H */
