/* libwct_hip -- colour preservation: the part of the C ABI behind `--preserve_color match | luma`.
 *
 * The reference (MingSun-Tse/Collaborative-Distillation) has no colour control: its cascade (PytorchWCT/WCT.py:120-125) hands the
 * style's palette to the result.  The two standard remedies of Gatys et al., "Controlling Perceptual Factors in Neural Style
 * Transfer" (CVPR 2017, section 5), are image-space operations at full resolution and extend what the reference already has:
 *   match   the style image's colours are mapped onto the content's colour distribution BEFORE stylisation.  This is the reference's
 *           own whiten_and_color (PytorchWCT/util_wct.py:62-131) in three channels on pixels instead of C channels on features: fp64
 *           moments, symmetric matrix square roots, one affine map per pixel.
 *   luma    the result keeps the content's chroma and takes only the stylised luminance; a post-pass at the image edge, next to
 *           wct_planar_to_u8 -- save_image, WCT.py:128 -- behind the last level of the cascade of WCT.py:120-125.
 * Everything in wct_hip.h holds here too: return codes, wct_last_error, device pointers, one context = one stream, asynchronous calls.
 * Images are planar 3 x H x W fp32 device buffers of any 4-byte alignment.  Every entry runs on the context's stream, never
 * synchronises on the 16x path, and returns WCT_ERR_INVALID -- wct_last_error names the entry -- before anything is written when an
 * argument is bad (a NULL pointer, an empty shape, and what each entry lists).
 *
 * Definitions
 *
 * Colour moments.  sum[3], sumsq[9] (device f64): the raw sums  SUM_p x_p  and  SUM_p x_p x_p^T  over all H W pixels, row-major,
 * symmetric.  Raw (not centred) so that a sharded run can all-reduce them.  Every accumulator is fp64 and every product of two fp32
 * values is exact in fp64.  The summation tree is a function of (H, W) alone: pixels are dealt to accumulators by their INDEX
 * p = y W + x (groups of four consecutive indices; tiles of 8192 indices; thread t of a tile takes groups t, t + 256, ...), never by
 * address, grid size, CU count or call history; a plane that is not 16-byte aligned is read with 4-byte loads into the same
 * accumulators.  No floating-point atomics.  No accumulator adds more than 4096 terms in sequence before the tree (32 per thread of
 * a tile; ceil(tiles / 256) per thread of the second stage), so the sums are within ~1e-13 relative of the exact ones for values
 * in [0, 1].  That bound is why an image of more than 2^33 pixels (8192 x 256 x 4096) is WCT_ERR_INVALID in every entry that takes
 * moments.  Bitwise reproducible across calls, alignments and contexts.
 *
 * Colour solve.  From (n_c, sum_c, sumsq_c) of the content and (n_s, sum_s, sumsq_s) of the style:
 *   mu    = sum / n
 *   Sigma = (sumsq - n mu mu^T) / (n - 1) + eps I          the unbiased form of util_wct.py:70
 *   A     = Sigma_c^(1/2) Sigma_s^(-1/2)                   symmetric roots by a 3 x 3 fp64 cyclic Jacobi eigen-decomposition on the device
 *   t     = mu_c - A mu_s
 * A[9] (row-major), t[3]: device f64.  eps is an argument; WCT_COLOR_EPS is what wct_color_match and wct_stylize_color use: about
 * the variance of 8-bit quantisation ((1/255)^2 / 12 = 1.3e-6 per channel, times a few), and the value of Gatys' implementation.
 * With it a grey or constant style gives a finite A, ||A||_2 <= sqrt((lambda_max(Sigma_c) + eps) / eps).  No host synchronisation;
 * n < 2 on either side, or an eps that is not finite or not positive, is WCT_ERR_INVALID.
 *
 * Colour apply.  out_p = float(A double(x_p) + t): evaluated in fp64 (row r: fma(A[r][2], x2, fma(A[r][1], x1, fma(A[r][0], x0,
 * t[r])))), rounded ONCE to fp32.  NOT clamped: it is what the encoders are fed.  out == in is allowed.
 *
 * Luma merge.  Y(x) = 0.299 R + 0.587 G + 0.114 B (fp32: fma(0.114, B, fma(0.587, G, 0.299 R))), and for c in {R, G, B}
 *   out_c(y, x) = content_c(y, x) + (Y(stylised)(y, x) - Y(content)(y, x))
 * -- what YIQ and YUV recombination both reduce to: their inverses map (dY, 0, 0) to (dY, dY, dY).  stylised is 3 x Ho x Wo, content
 * is 3 x Hc x Wc with Ho <= Hc, Wo <= Wc; its top-left Ho x Wo window is read (the cascade returns 16 floor(H / 16) x 16 floor(W / 16):
 * floor pooling drops trailing rows and columns).  Exactly one of out_planar (fp32, 3 x Ho x Wo) and out_hwc (uint8, Ho x Wo x 3, any
 * alignment: 4-byte stores where the base allows, single bytes otherwise) is non-NULL, as in wct_resize_u8_filter; out_hwc takes the round_mode conversion of wct_planar_to_u8 and is
 * byte-identical to wct_planar_to_u8 of the planar result.  out_planar == stylised is allowed.
 */
#ifndef WCT_HIP_COLOR_H
#define WCT_HIP_COLOR_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_COLOR_MATCH 1
#define WCT_COLOR_LUMA 2       /* `mode` of wct_stylize_color is a mask: 1, 2 or 3 */
#define WCT_COLOR_EPS 1e-5

/* extends torch.mean + mm(cF, cF.t()) of util_wct.py:68-70 to image pixels.  The stage-1 partials (72 bytes per 8192 pixels) live in
 * the context's workspace, allocated on first use of a size. */
int wct_color_moments(wct_ctx* ctx, const float* planar, int H, int W, double* sum, double* sumsq);
/* extends svd / pow / diag / mm of util_wct.py:74-125 */
int wct_color_solve(wct_ctx* ctx, double n_c, const double* sum_c, const double* sumsq_c, double n_s, const double* sum_s,
                    const double* sumsq_s, double eps, double* A, double* t);
/* extends mm(step2, cF), mm(S, .), + s_mean of util_wct.py:120-126 */
int wct_color_apply(wct_ctx* ctx, const float* in, int H, int W, const double* A, const double* t, float* out);
/* = wct_color_moments(style) + wct_color_moments(content) + wct_color_solve(WCT_COLOR_EPS) + wct_color_apply(style), sums and map in
 * the context's workspace: bit-identical to that chain.  style_out (3 x Hs x Ws) may be `style`.  Hs Ws < 2 or H W < 2 is
 * WCT_ERR_INVALID. */
int wct_color_match(wct_ctx* ctx, const float* style, int Hs, int Ws, const float* content, int H, int W, float* style_out);
int wct_luma_merge(wct_ctx* ctx, const float* stylised, int Ho, int Wo, const float* content, int Hc, int Wc, float* out_planar,
                   uint8_t* out_hwc, int round_mode);
/* extends wct_stylize -- the cascade of WCT.py:120-125, num_run times -- by the colour control `mode`:
 *   WCT_COLOR_MATCH  the style is matched to the ORIGINAL content once (wct_color_match), and wct_stylize runs num_run times on the
 *                    matched style
 *   WCT_COLOR_LUMA   wct_luma_merge against the ORIGINAL content follows the last run
 * Bit-identical to the composition of those public calls.  On the 16x path it never synchronises, allocates nothing after the first
 * call of a size (wct_debug_get "ws_allocs" does not move) and can be captured into one HIP graph.  The matched style (3 Hs Ws
 * floats) and the un-merged result (3 H W floats) belong to the context: allocated on first use of a size, ON TOP of
 * wct_workspace_bytes, not covered by wct_reserve, like the noise buffer of wct_synthesize; scratch in the sense of the "poison"
 * hook.  Afterwards the prepared style slot of every level holds the MATCHED style's statistics (with WCT_COLOR_MATCH; the given
 * style's otherwise): a wct_stylize_prepared that follows runs against them.  The f16x3 range flag behaves as in wct_stylize.
 * out must hold 3*H*W floats; mode outside 1..3 is WCT_ERR_INVALID. */
int wct_stylize_color(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run,
                      int mode, float* out, int* Ho, int* Wo);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_COLOR_H */
