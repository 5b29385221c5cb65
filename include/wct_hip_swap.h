/* libwct_hip -- patch-based style swap (style decorator) at one cascade level: the part of the C ABI behind `--swap_level`.
 *
 * Every other transform of the library (wct, ot, adain, regions, interpolation, blend) is an affine map of the content feature.  This one
 * is not: every 3 x 3 content patch is replaced by its best-matching 3 x 3 style patch (Chen & Schmidt, "Fast Patch-based Style Transfer
 * of Arbitrary Style", 2016), in the whitened domains of both features (the style decorator of Avatar-Net: Sheng et al., CVPR 2018) or
 * on the raw features.  Everything in wct_hip.h holds here too: return codes, wct_last_error, device pointers, one context = one stream,
 * asynchronous calls.  Every entry returns WCT_ERR_INVALID -- wct_last_error names the entry -- before anything is written when an
 * argument is bad.
 *
 * Definitions
 *
 * Feature maps are NHWC fp32.  Query map Q [h, w, C], key map Kmap [hs, ws, C], value map V [hs, ws, C].  Patches are 3 x 3, stride 1,
 * valid positions only: Nq = (h - 2)(w - 2) queries, query q = qy (w - 2) + qx covers Q[qy .. qy + 2, qx .. qx + 2, :];
 * Nk = (hs - 2)(ws - 2) keys, indexed the same way.  Limits: h, w, hs, ws >= 3; C a multiple of 4 in 4 .. 512; Nk < 2^31 (and Nq < 2^31).
 * The maps, base and out are read and written in 16-byte pieces along C: their addresses must be multiples of 16.
 *
 * Match.   score(q, k) = <patch_Q(q), patch_K(k)> / sqrt(|patch_K(k)|^2 + WCT_SWAP_EPS)        idx[q] = argmax_k score(q, k)
 * The lowest k wins among equal scores.  The query's own norm does not change the arg-max and is not applied.  A NaN score never wins;
 * a query whose scores are all NaN gets idx 0.
 *
 * Arithmetic of the match.  The inner product is an implicit GEMM [Nq x 9C] . [9C x Nk] on the f16 matrix cores in the f16x3 split
 * arithmetic of the convolutions: x = hi + lo (two f16), products hi.hi + hi.lo + lo.hi, fp32 accumulator (the dropped lo.lo term and the
 * accumulation are < (2^-22 + 9C 2^-24) |patch_Q| |patch_K|).  A value beyond +-65504 (or a NaN) clamps and raises the context's range
 * flag (wct_range_poll).  |patch_K|^2 is an fp64 sum in the fixed order (tap, channel), r = fp32(1 / sqrt(|patch_K|^2 + eps)), and the score is
 * the fp32 product of the accumulator and r.  The score of a (query patch, key patch) pair is a function of the two patches' VALUES alone: the
 * products of one pair enter one accumulator in the order (32-channel chunk, dx, dy, split term) whatever the patches' positions, the
 * map sizes, the tiling or the key chunking, so equal patches give bitwise equal scores and the tie rule decides between them.  No score
 * is written to memory except the optional [Nq] best score.
 *
 * Bounded launches.  Keys are processed in chunks of at most WCT_SWAP_KEY_CHUNK patches per launch (consecutive key indices; the
 * running (score, index) of every query lives in the context between launches and merges by the order-independent rule "greater score,
 * then lower index").  The number of launches depends on the sizes alone.  The wct_debug_set key "swap_key_chunk" = n overrides the chunk
 * (n >= 1; 0 restores the default) when the environment has WCT_DEBUG set, like the other measurement keys.
 *
 * Assemble.   out[y, x, :] = alpha * mean + (1 - alpha) * base[y, x, :]
 * mean = the fp32 average over every query patch (qy, qx) that covers (y, x) of V[ky + (y - qy), kx + (x - qx), :], (ky, kx) = that
 * query's key: 9 patches in the interior, 6 or 4 on edges, 1 in a corner.  Summed in fp32 from 0 in ascending (qy, qx) order, then
 * divided by the count; the blend is fl(fl(alpha * mean) + fl(fl(1 - alpha) * base)) without contraction, fl(alpha * mean) when base is
 * NULL.  An index outside 0 .. Nk - 1 is clamped into that range (never a wild read).
 *
 * Decorator, one level.  Given the content feature cF and the style feature sF of a level:
 *   WCT_SWAP_WHITENED   the match runs on Q = Wc (cF - mu_c), Kmap = Ws (sF - mu_s), W = cov^(-1/2) (pseudo-inverse square root): each
 *                       side is wct_moments + wct_transform_solve [mode WCT_TRANSFORM_WCT, style_stats = (I, 0), alpha = 1], which yields
 *                       (W, -W mu), applied by wct_apply_labeled with one label
 *   WCT_SWAP_RAW        Q = cF, Kmap = sF (Chen & Schmidt)
 * In both modes V = sF and base = cF (colouring the whitened style patches back gives the raw style patches on the style's live
 * subspace, so no colouring step exists), csF = alpha * swapped + (1 - alpha) * cF, and wct_decode of that level turns csF into an image.
 *
 * Context memory.  The two projected maps, the blended feature, the running bests (8 bytes per query), the key norms and a label map
 * belong to the context: allocated on first use of a size ON TOP of wct_workspace_bytes, not covered by wct_reserve, scratch in the
 * sense of the "poison" hook.  These buffers are sized and allocated before the first launch of a call, so a swap whose own buffers do
 * not fit is WCT_ERR_NOMEM with nothing enqueued.  The buffers the swap shares with the rest of the library -- the lanes' activation and
 * moment workspaces of wct_encode / wct_moments / wct_decode, the solver's, and everything the other levels of wct_stylize_swap use --
 * grow on first use of a size as they do in wct_stylize, i.e. possibly after earlier launches of a first call.
 */
#ifndef WCT_HIP_SWAP_H
#define WCT_HIP_SWAP_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_SWAP_EPS 1e-12
#define WCT_SWAP_WHITENED 0
#define WCT_SWAP_RAW 1
/* Keys per launch.  One launch costs Nq * chunk * 9C * 6 f16 flop: 1.46e13 at relu3_1 of a 3840 x 2160 content (5.2e5 queries, C = 64),
 * 15.4 ms measured on the MI355X (938 TFLOP/s over the whole match at that size; DESIGN.md, "Patch swap"). */
#define WCT_SWAP_KEY_CHUNK 8192

/* idx[q] (and best[q] = the winning score, when best is non-NULL) for every query.  WCT_ERR_INVALID: a NULL map or idx, a map smaller
 * than 3 x 3, C not a multiple of 4 in 4 .. 512, Nk >= 2^31, a map that is not 16-byte aligned, an idx or best that
 * overlaps a map or the other output. */
int wct_patch_match(wct_ctx* ctx, const float* q, int h, int w, const float* k, int hs, int ws, int C, int32_t* idx /* [Nq] */,
                    float* best /* [Nq], may be NULL */);
/* out [h, w, C] from the indices of wct_patch_match.  WCT_ERR_INVALID: a NULL idx, v or out, the shape limits above, alpha not finite,
 * base == NULL with alpha != 1, a misaligned v, base or out.  out must not overlap v or idx; out == base is allowed (a pixel's base is read before it is written). */
int wct_patch_assemble(wct_ctx* ctx, const int32_t* idx, int h, int w, const float* v, int hs, int ws, int C,
                       const float* base /* may be NULL iff alpha == 1 */, float alpha, float* out /* [h, w, C] */);
/* wct_encode of both images at `level`, the decorator above, wct_decode: planar 3 x Ho x Wo into out (Ho = h << (level - 1)).
 * WCT_ERR_INVALID: a NULL pointer, level outside 2 .. 5 (a full-resolution 24-channel match is out of scope), match_mode outside
 * {WCT_SWAP_WHITENED, WCT_SWAP_RAW}, alpha not finite, a feature map smaller than 3 x 3.  On the 16x path it never synchronises the
 * host, allocates nothing after the first call of a size and can be captured into a HIP graph. */
int wct_swap_level(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs, int Ws, int match_mode,
                   float alpha, float* out, int* Ho, int* Wo);
/* The 5 -> 1 cascade of wct_stylize, num_run times, with level `swap_level` (2 .. 5) run through wct_swap_level and every other level
 * through wct_style_transfer_level under the context's transform mode: bit-identical to that composition of public calls, each level
 * reading the previous level's result.  Refusals as for wct_swap_level, and num_run < 1. */
int wct_stylize_swap(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, int swap_level /* 2..5 */,
                     int match_mode, float alpha, int num_run, float* out, int* Ho, int* Wo);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_SWAP_H */
