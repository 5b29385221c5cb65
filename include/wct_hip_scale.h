/* libwct_hip -- scale control: a coarse-to-fine cascade on a device image pyramid: the part of the C ABI behind `--level_scale`.
 *
 * Gatys et al., "Controlling Perceptual Factors in Neural Style Transfer" (CVPR 2017), name three controls: spatial (wct_stylize_regions,
 * wct_stylize_blend), colour (wct_hip_color.h) and scale.  This is the third, after section 6 of that paper, carried into the WCT
 * cascade: the deep levels run on a REDUCED image, where one feature pixel sees `divisor` times as much of the content per axis; the
 * result is brought up to the next working size, the content's fine detail is put back, and the shallow levels finish at full size.
 * With a second style on the coarse levels (wct_style_prepare_levels, then style == NULL below) it is the paper's scale mixing.
 * Everything in wct_hip.h holds here too: return codes, wct_last_error, device pointers, one context = one stream, asynchronous calls.
 * Every entry returns WCT_ERR_INVALID -- wct_last_error names the entry -- before anything is written when an argument is bad.
 *
 * Definitions
 *
 * Working sizes.  For a content of H x W and an integer divisor d in 1 .. WCT_SCALE_MAX_DIVISOR:
 *   h_d = 16 floor(H / (16 d))      w_d = 16 floor(W / (16 d))      both >= 32, the five-level cascade refuses less.
 * h_1 x w_1 is the Ho x Wo of wct_stylize; multiples of 16 pass through every level unchanged in size.
 *
 * Resampling R(x -> oh x ow, filter).  Separable, the horizontal pass first, on planar 3 x h x w fp32 of any 4-byte alignment.  Per
 * axis, output sample i of `out` from `in` samples (the rule of Pillow's precompute_coeffs, as wct_resize_u8_filter restates it,
 * WITHOUT its fixed-point step), all in fp64:
 *   scale = in / out      fs = max(scale, 1)      centre = (i + 0.5) scale      support = S fs
 *   S = 1 for WCT_FILTER_BILINEAR (triangle), 2 for WCT_FILTER_BICUBIC (Keys, a = -0.5)
 *   taps t in [ int(centre - support + 0.5), int(centre + support + 0.5) ) clipped to [0, in), int() truncating
 *   v_t = filter((t - centre + 0.5) / fs)      w_t = v_t / SUM_t v_t (summed in ascending t)      rounded ONCE to fp32
 * A sample is acc = fma(w_t, x_t, acc) in fp32 from acc = 0 in ascending tap order, per pass; the horizontally resampled rows are fp32.
 * The order is a function of the four sizes and the filter alone -- never of grid, tile, CU count, alignment or call history -- and
 * there are no floating-point atomics: the result is bitwise reproducible across calls, views and contexts.  Values are NOT clamped
 * (bicubic overshoots, and the cascade takes floats).  Equal sizes are a bit-for-bit copy.  The weights are evaluated on the device
 * per output index by every call; nothing is cached between calls.  An axis may shrink by at most WCT_SCALE_MAX_SHRINK (in <= 32 out).
 *
 * Merge M(a, b, c, g).  a, b: 3 x hc x wc; c: 3 x hf x wf; gain g >= 0:
 *   M = R(a - g b -> hf x wf, bicubic) + g c        as ONE kernel: R( fma(-g, b, a) ), then fma(g, c, .) on every sample
 * (by linearity the two upsamplings collapse into one upsampling of a difference; two coarse maps and one fine map are read, one fine
 * map is written).  With a = the stylised coarse image, b = the content at the coarse size, c = the content at the fine size this is a
 * Laplacian-pyramid step: the fine content plus the low-frequency change the coarse levels made.  g = 0 is exactly R(a): b and c may
 * then be NULL (they are not read), and the result is bit-identical to wct_resample_planar of a with the bicubic filter.
 *
 * Cascade.  div[5] are the divisors of levels 5, 4, 3, 2, 1: each in 1 .. 16, non-increasing from level 5 to level 1, the last one 1.
 *   F_d = R(content -> h_d x w_d, bicubic); for d = 1 with H and W multiples of 16, F_1 is the content itself and no kernel runs
 *   cur = content if div[level 5] == 1, else F_{d5}
 *   for level L = 5 .. 1 with divisor d:   if the previous level's divisor d' != d:  cur = M(cur, F_{d'}, F_d, g)
 *                                          cur = level L of the cascade on cur  (what wct_style_transfer_level computes)
 *   from the second run of num_run > 1 on, when d5 > 1, a run starts with cur = R(cur -> h_{d5} x w_{d5}, bicubic)
 * The style is NOT rescaled: the strokes of the reduced levels grow by the divisor -- that is the control.  All divisors 1 is
 * wct_stylize -- wct_stylize_prepared with style == NULL -- bit for bit, at any size.
 *
 * Context memory.  The F_d of the distinct divisors (3 h_d w_d floats each), one staging image (3 h_1 w_1 floats) and the weight tables
 * of one resampling (4 (2 ceil(support) + 3) bytes per output row and column, rewritten by every call of the three device entries)
 * belong to the context: allocated on first use of a size, ON TOP of wct_workspace_bytes, not covered by wct_reserve, like the buffers
 * of wct_stylize_smooth; scratch in the sense of the "poison" hook.
 */
#ifndef WCT_HIP_SCALE_H
#define WCT_HIP_SCALE_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_SCALE_MAX_DIVISOR 16
#define WCT_SCALE_MAX_SHRINK 32      /* in <= 32 out per axis: 129 bicubic taps at most */
#define WCT_SCALE_DETAIL 1.0         /* the command line's default gain: a look, not a measurement */

/* HOST ONLY.  (h_d, w_d) of a content of H x W.  WCT_ERR_INVALID, with *h and *w untouched: a NULL pointer, H or W < 1, a divisor
 * outside 1 .. WCT_SCALE_MAX_DIVISOR, a working size under 32. */
int wct_scale_shape(int H, int W, int divisor, int* h, int* w);
/* dst (3 x oH x oW) = R(src (3 x H x W) -> oH x oW, filter).  WCT_ERR_INVALID: a NULL image, an empty shape, a filter id other than
 * WCT_FILTER_BILINEAR / WCT_FILTER_BICUBIC, an axis shrinking by more than WCT_SCALE_MAX_SHRINK, dst overlapping src. */
int wct_resample_planar(wct_ctx* ctx, const float* src, int H, int W, float* dst, int oH, int oW, int filter);
/* out (3 x hf x wf) = M(a, b, c, gain).  b and c may be NULL iff gain == 0.  WCT_ERR_INVALID: a NULL a or out, a NULL b or c with
 * gain > 0, an empty shape, gain not finite or < 0, an axis shrinking by more than WCT_SCALE_MAX_SHRINK, out overlapping a, b or c. */
int wct_pyramid_merge(wct_ctx* ctx, const float* a, const float* b, int hc, int wc, const float* c, int hf, int wf, float gain, float* out);
/* The cascade above, num_run times: planar 3 x Ho x Wo into out, Ho x Wo = h_1 x w_1.  Bit-identical to the composition of public calls
 * it is made of: wct_resample_planar, wct_pyramid_merge, wct_style_transfer_level -- under the context's transform mode.
 * style == NULL runs against the statistics already in the context, as wct_synthesize does with a NULL texture:
 * wct_style_prepare_levels of style B with the mask of the coarse levels, then of style A with the rest, in front of it is scale mixing;
 * a level without statistics is WCT_ERR_STATE.  With a style the prepared slots are rewritten as by wct_stylize, the style side running on the
 * side lane; with NULL they survive the call.
 * On the 16x path it never synchronises, allocates nothing after the first call of a size (wct_debug_get "ws_allocs" does not move),
 * can be captured into one HIP graph, and leaves the f16x3 range flag as the cascade it wraps does.  out must hold 3 h_1 w_1 floats.
 * WCT_ERR_INVALID: a NULL content, out or level_div, a divisor outside 1 .. 16, divisors increasing towards level 1, a last divisor
 * other than 1, a working size under 32, detail_gain not finite or < 0, num_run < 1, out overlapping the content (the merges read it). */
int wct_stylize_scaled(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run,
                       const int* level_div /* HOST, [5]: levels 5, 4, 3, 2, 1 */, float detail_gain, float* out, int* Ho, int* Wo);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_SCALE_H */
