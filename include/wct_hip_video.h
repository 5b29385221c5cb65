/* libwct_hip -- video mode: temporally stable stylisation of a frame sequence: the part of the C ABI behind `--video`.
 *
 * Stylising the frames of a sequence as unrelated stills flickers in two ways.  Globally: the content mean and covariance of every
 * level are re-estimated per frame, so small changes of the frame move the affine map (M, b) of all five levels and the colours and
 * contrast of the whole picture pump.  Locally: where the scene does not move, the decoders still turn sensor noise into different
 * strokes on every frame.  This header holds the two standard flow-free remedies: content statistics tracked over time with a
 * scene-cut reset, and a motion-adaptive recursive blend of the output.  Optical flow is not part of it.
 * Everything in wct_hip.h holds here too: return codes, wct_last_error, device pointers, one context = one stream, asynchronous calls.
 * Every entry returns WCT_ERR_INVALID -- wct_last_error names the entry -- before anything is written when an argument is bad.
 *
 * Definitions
 *
 * Clip.  The state of ONE sequence of H x W frames: an object of its own (wct_clip), not part of the context -- the results of every
 * other entry stay independent of a context's call history.  Ho x Wo = 16 floor(H / 16) x 16 floor(W / 16) is the size of a stylised
 * frame (both >= 32).  With C_L the channels of the level-L encoder and n_L = (Ho >> (L-1)) (Wo >> (L-1)) its pixels, a clip holds in
 * ONE device allocation made by wct_clip_create (wct_clip_bytes(H, W, C) bytes; each part rounded up to 256 bytes):
 *   running sums   rs_L[C_L], rss_L[C_L * C_L]   fp64, levels 5, 4, 3, 2, 1 in this order      8 SUM_L (C_L + C_L^2) bytes
 *   pending sums   the same layout: what the frame in flight has tracked and not yet committed  8 SUM_L (C_L + C_L^2) bytes
 *   flags          int frames (commits since creation / the last reset), int cut (the last decision)            256 bytes
 *   three images   the previous content crop, the previous output, the cascade's un-blended result         3 * 12 Ho Wo bytes
 * all zero after wct_clip_create.  n_L is fixed by the clip's size, so an exponential average of raw sums is one of moments.
 *
 * Tracking T(level, decide, c) of incoming raw sums c = (sum[C], sumsq[C * C]) against the running r = (rs, rss), n = n_level:
 *   decision, only when decide != 0 (the cascade: at level 5, whose input is the raw content frame):
 *     mu_c = sum / n     mu_r = rs / n     var_r[k] = rss[k,k] / n - mu_r[k]^2
 *     D = SUM_k (mu_c[k] - mu_r[k])^2 / max(SUM_k var_r[k], DBL_MIN)
 *     cut = frames == 0 || !(D <= params.cut)          a NaN therefore counts as a cut; params.cut = +inf: only the first frame does
 *     both sums over k run over 512 slots (k >= C adds 0) as a pairwise tree in fp64: an order that is a function of nothing at all.
 *     The flag goes to the clip's device memory; decide == 0 reads the stored one.  Nothing is read back to the host.
 *   update, per element of sum and sumsq:
 *     cut, or rate == 1:   r' = c           exactly ((c - r) + r would round)
 *     else:     r' = r + rate * (c - r)     three separately rounded fp64 operations, no contraction: numpy reproduces it bit for bit,
 *                                           and c == r gives exactly r
 *     sum / sumsq are overwritten with r'; r' also goes to the pending sums.
 *   commit: pending -> running and frames += 1, on the device.  wct_stylize_clip commits once, as the frame's last step;
 *     a standalone wct_moments_track commits its level at once.
 *   One launch per level for any C in 1 .. 512 (a deciding launch is a single workgroup: it reads all of `sum` before it rewrites it).
 *   Test key: "clip_channels" = C (through wct_debug_set) makes the clips created afterwards hold C channels at every level instead of the loaded
 *   encoders' (0: off) -- tracking on its own at widths no loadable encoder has; wct_stylize_clip refuses such a clip (WCT_ERR_STATE).
 *
 * Blend B(cur, prev, s, p).  c = the top-left Ho x Wo of cur_content (3 x Hc x Wc, the convention of wct_luma_merge), q = prev_content
 * (3 x Ho x Wo), s = stylised, p = prev_out, radius r:
 *   e(y,x) = SUM_ch (c - q)^2
 *   d(y,x) = SUM of e over the (2r+1)^2 window clipped to the image / the clipped window's pixel count
 *   w      = cut ? 0 : blend * expf(-d / (2 sigma^2))
 *   out    = cut ? s : s + w (p - s)          per channel; p == s therefore gives s
 * all in fp32; the window sum is separable and direct: per row the 2r+1 terms in ascending x, then the 2r+1 row sums in ascending y --
 * never a running sum, whose error would grow along the row.  ONE kernel, tiled through LDS with a halo of r; it reads four images
 * and writes one.  On a cut only `stylised` is read.  With out_hwc it also writes the uint8 H x W x 3 image, bit-identical to
 * wct_planar_to_u8 of out_planar with that round_mode.  The result is a function of the arguments alone: bitwise reproducible.
 *
 * Frame.  wct_stylize_clip = the cascade of wct_stylize_prepared with num_run = 1 against the context's prepared style under the context's
 * transform mode, with ONE change: between a level's moments and its solve the content sums go through T(level, level == 5, .); then
 * out = B(content, previous content crop, cascade result, previous output) with the stored cut flag; then content crop and out are
 * stored for the next frame and the sums are committed.  It follows that
 *   the first frame, the frame after wct_clip_reset and every frame with params.cut == 0 are wct_stylize_prepared bit for bit;
 *   so is every frame with rate == 1 and blend == 0; and a frame fed again and again is reproduced bit for bit under any parameters.
 */
#ifndef WCT_HIP_VIDEO_H
#define WCT_HIP_VIDEO_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_CLIP_MAX_RADIUS 8
/* the command line's defaults: a look, not a measurement */
#define WCT_CLIP_RATE 0.25
#define WCT_CLIP_CUT 0.5
#define WCT_CLIP_BLEND 0.6
#define WCT_CLIP_SIGMA 0.05
#define WCT_CLIP_RADIUS 2

typedef struct wct_clip wct_clip;
/* rate in (0, 1]; cut >= 0 or +inf; blend in [0, 1); sigma > 0 and finite; radius 0 .. WCT_CLIP_MAX_RADIUS */
typedef struct { double rate; double cut; float blend; float sigma; int radius; } wct_clip_params;

/* HOST ONLY.  The bytes of a clip's single device allocation (Definitions).  C: HOST, [5], the channels of levels 5, 4, 3, 2, 1.
 * WCT_ERR_INVALID, with *bytes untouched: a NULL pointer, H or W < 32, a C outside 1 .. 512. */
int wct_clip_bytes(int H, int W, const int* C, size_t* bytes);
/* A clip for H x W frames of this context's loaded model: allocates everything, once, and zeroes it (synchronises).  WCT_ERR_STATE: an
 * encoder of levels 1 .. 5 is not loaded.  WCT_ERR_INVALID: a NULL pointer, H or W < 32, parameters outside the ranges above. */
int wct_clip_create(wct_ctx* ctx, int H, int W, const wct_clip_params* params, wct_clip** clip);
/* Waits for the context's streams, then frees.  A NULL clip is ignored.  ctx == NULL (the context is gone already): frees without waiting. */
void wct_clip_destroy(wct_ctx* ctx, wct_clip* clip);
/* Asynchronous: frames = 0 in stream order -- the next frame is a first frame (a cut).  Can be captured. */
int wct_clip_reset(wct_ctx* ctx, wct_clip* clip);
/* The running sums of `level` and the flags, device to device in stream order.  sum [C], sumsq [C * C], flags [2] (frames, cut): DEVICE
 * pointers, each may be NULL. */
int wct_clip_export(wct_ctx* ctx, wct_clip* clip, int level, double* sum, double* sumsq, int* flags);
/* T(level, decide, (sum, sumsq)) in place, then the commit of that level.  sum [C_level], sumsq [C_level^2]: DEVICE. */
int wct_moments_track(wct_ctx* ctx, wct_clip* clip, int level, int decide, double* sum, double* sumsq);
/* out = B(...).  cut_flag_dev: a DEVICE int, NULL = 0.  out_hwc may be NULL.  WCT_ERR_INVALID: a NULL image or out_planar, an empty
 * shape, Ho > Hc or Wo > Wc, blend outside [0, 1), sigma not finite or <= 0, radius outside 0 .. WCT_CLIP_MAX_RADIUS, round_mode other
 * than 0 / 1, out_planar or out_hwc overlapping an input or each other (the kernel reads a halo: nothing may alias). */
int wct_temporal_blend(wct_ctx* ctx, const float* cur_content, int Hc, int Wc, const float* prev_content /* 3 x Ho x Wo */,
                       const float* stylised, const float* prev_out, int Ho, int Wo, float blend, float sigma, int radius,
                       const int* cut_flag_dev, float* out_planar, uint8_t* out_hwc, int round_mode);
/* One frame (Definitions).  out_planar: 3 Ho Wo floats; out_hwc (may be NULL): Ho x Wo x 3 bytes.  It never synchronises, allocates
 * nothing after the first frame of a size (wct_debug_get "ws_allocs" does not move), leaves the f16x3 range flag as the cascade does,
 * and can be captured into ONE HIP graph that is replayed for successive frames: the previous-frame buffers are rewritten by a kernel
 * inside the call, there is no host-side ping-pong.
 * WCT_ERR_INVALID: a NULL pointer, a frame of another size than the clip's, a clip of another context, round_mode other than 0 / 1,
 * an output overlapping the content or the other output.  WCT_ERR_STATE: a level without style statistics (wct_style_prepare /
 * wct_style_import); a wide model (an encoder wider than 128 channels, --mode original): its deferred solves may run the cascade
 * twice, which would track the frame twice -- not supported. */
int wct_stylize_clip(wct_ctx* ctx, wct_clip* clip, const float* content, int H, int W, float alpha, float* out_planar, uint8_t* out_hwc,
                     int round_mode, int* Ho, int* Wo);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_VIDEO_H */
