/* libwct_hip -- motion compensation for video mode: a block-matched integer vector field between consecutive content frames, and the
 * temporal blend of wct_hip_video.h against the DISPLACED previous content and previous output: the part of the C ABI behind `--motion`.
 *
 * The blend of video mode weighs the previous output by w = blend exp(-d / 2 sigma^2), d a windowed difference of the current and the
 * previous content AT THE SAME PIXEL.  Where the camera pans or an object moves d is large, w falls to 0 and those pixels are stylised as
 * unrelated stills again -- where an unstable stylisation shows most.  With a motion field the previous frame is fetched from where the
 * pixel came from, and d measures what compensation could not explain.
 * Everything in wct_hip.h and wct_hip_video.h holds here too: return codes, wct_last_error, device pointers, one context = one stream,
 * asynchronous calls.  Every entry returns WCT_ERR_INVALID -- wct_last_error names the entry -- before anything is written when an
 * argument is bad.  All integer steps below are exact: a result is a function of the arguments alone, bitwise reproducible.
 *
 * Definitions
 *
 * Luma.  Of a planar fp32 pixel (r, g, b):  t = (0.299f r + 0.587f g) + 0.114f b  -- three products and two sums, each rounded to fp32 on
 * its own, in this order, never contracted into an fma -- then the library's uint8 conversion with rounding: x = t * 255, x = x + 0.5,
 * x = min(max(x, 0), 255) with NaN -> 0, truncation.  numpy float32 arithmetic reproduces it bit for bit.
 *
 * Pyramid.  Level 0 is the luma of the top-left Ho x Wo of the image, H_0 x W_0 = Ho x Wo.  Level k + 1 is (a + b + c + d + 2) >> 2 over
 * the 2 x 2 cells of level k, of size floor(H_k / 2) x floor(W_k / 2) (an odd last row / column is dropped).  `levels` levels,
 * 1 .. WCT_MOTION_MAX_LEVELS; Ho and Wo must be >= 2^(levels - 1), so that every level has a pixel.
 *
 * Blocks.  WCT_MOTION_BLOCK x WCT_MOTION_BLOCK = 8 x 8 pixels.  The grid of level k is nby_k x nbx_k = ceil(H_k / 8) x ceil(W_k / 8); the
 * blocks of the last row / column are clipped to the image.  The parent of block (by, bx) of level k is block
 * (min(by >> 1, nby_(k+1) - 1), min(bx >> 1, nbx_(k+1) - 1)) of level k + 1.
 *
 * Vector.  (vy, vx) of a block says cur(y, x) ~ prev(y + vy, x + vx) for the block's pixels.  A candidate is ADMISSIBLE when the clipped
 * block displaced by it lies wholly inside the previous image of that level; the zero vector always is.
 *
 * Candidates, in this order -- the position in the order is the candidate's index:
 *   top level (levels - 1):  (0, 0), then every (dy, dx) of [-range, range]^2, dy ascending and dx ascending inside it
 *                            (range 0 .. WCT_MOTION_MAX_RANGE; (0, 0) therefore appears twice, the first wins);
 *   every finer level:       (0, 0), then 2 v_parent + (dy, dx) over [-1, 1]^2 in the same order.
 *
 * Cost.  SAD of the clipped block + penalty (|vy| + |vx|), penalty 0 .. 255, the vector in that level's pixels.  The admissible candidate
 * with the smallest (cost, index) wins.  A cost stays below 2^16 (64 * 255 + 255 * 2 * 63) and an index below 2^8 (1 + 15^2), so ONE
 * 32-bit key  cost << 8 | index  and an integer minimum decide it: no floating point, no dependence on the order of evaluation.
 *
 * Result.  The field of level 0:  int16_t mv[nby][nbx][2] = (vy, vx),  nby x nbx = wct_motion_shape(Ho, Wo).
 *
 * Compensated blend.  With the vector (vy, vx) of block (y >> 3, x >> 3):
 *   q'(ch, y, x) = q(ch, clamp(y + vy, 0, Ho - 1), clamp(x + vx, 0, Wo - 1))          and p' of p likewise;
 *   the result is B of wct_hip_video.h applied to (c, q', s, p'): the same fp32 operations in the same order.
 * The clamp never acts on a field the estimator made (its vectors are admissible); it is there so that NO field, however wrong, makes the
 * kernel read outside its images.  Two identities follow: a zero field gives the blend of video mode bit for bit, and any field gives
 * the blend of video mode applied to host-gathered q' and p' bit for bit.
 *
 * Frame.  A clip with motion attached (wct_motion_attach) runs, all on the device with nothing read back:
 *   1. the cascade with tracking, as wct_hip_video.h says;
 *   2. the field estimated from (the content's crop, the previous content's crop);
 *   3. the compensated blend with the stored cut flag;
 *   4. the store, as wct_hip_video.h says, and the current pyramid becomes the previous one.
 * On a cut the kernels leave the field all zero and the output is the cascade's result; the launches are issued regardless, so a
 * captured graph stays valid.  It follows that the first frame, a cut, and rate == 1 with blend == 0 remain wct_stylize_prepared bit for
 * bit, and that a frame fed again gives an all-zero field and, bit for bit, the output of the same clip without motion.
 */
#ifndef WCT_HIP_MOTION_H
#define WCT_HIP_MOTION_H

#include "wct_hip_video.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_MOTION_BLOCK 8
#define WCT_MOTION_MAX_LEVELS 4
#define WCT_MOTION_MAX_RANGE 7
/* the command line's defaults: a look, not a measurement */
#define WCT_MOTION_LEVELS 4
#define WCT_MOTION_RANGE 4
#define WCT_MOTION_PENALTY 4

/* levels 1 .. WCT_MOTION_MAX_LEVELS; range 0 .. WCT_MOTION_MAX_RANGE; penalty 0 .. 255 */
typedef struct { int levels; int range; int penalty; } wct_motion_params;

/* HOST ONLY.  The block grid of an Ho x Wo image: ceil(Ho / 8) x ceil(Wo / 8).  WCT_ERR_INVALID, with *nby and *nbx untouched: a NULL
 * pointer, Ho or Wo < 1. */
int wct_motion_shape(int Ho, int Wo, int* nby, int* nbx);
/* The luma pyramid of the top-left Ho x Wo of planar (3 x Hc x Wc): out = level 0 (Ho * Wo bytes), level 1, ..., each dense, row-major,
 * one behind the other.  WCT_ERR_INVALID: a NULL pointer, an empty shape, Ho > Hc or Wo > Wc, levels outside 1 .. WCT_MOTION_MAX_LEVELS,
 * Ho or Wo < 2^(levels - 1), out overlapping planar. */
int wct_motion_luma(wct_ctx* ctx, const float* planar, int Hc, int Wc, int Ho, int Wo, int levels, uint8_t* out);
/* mv = the field between the top-left Ho x Wo of cur (3 x Hc x Wc) and prev (3 x Ho x Wo).  Any Ho, Wo >= 2^(levels - 1).  The scratch
 * (two pyramids, the coarser fields) is the context's workspace.  WCT_ERR_INVALID: as wct_motion_luma, and NULL params, a parameter
 * outside its range, mv overlapping an image. */
int wct_motion_estimate(wct_ctx* ctx, const float* cur, int Hc, int Wc, const float* prev /* 3 x Ho x Wo */, int Ho, int Wo,
                        const wct_motion_params* params, int16_t* mv);
/* The compensated blend: the arguments of the blend entry of wct_hip_video.h, and the field.  mv: DEVICE, wct_motion_shape(Ho, Wo)
 * vectors; NULL = the zero field.  WCT_ERR_INVALID: what the blend entry of wct_hip_video.h refuses, and an output overlapping mv. */
int wct_motion_blend(wct_ctx* ctx, const float* cur_content, int Hc, int Wc, const float* prev_content /* 3 x Ho x Wo */,
                     const float* stylised, const float* prev_out, int Ho, int Wo, float blend, float sigma, int radius,
                     const int* cut_flag_dev, float* out_planar, uint8_t* out_hwc, int round_mode, const int16_t* mv);
/* Attaches motion compensation to a clip: wct_stylize_clip, its signature unchanged, then runs the Frame above.  Allocates the
 * clip's motion block -- two pyramids and the fields of every level, ONE allocation -- once, zeroes it, and synchronises; no frame
 * allocates afterwards (wct_debug_get "ws_allocs" does not move).  The next frame is a first frame (a cut), as after wct_clip_reset: the
 * previous pyramid a field is estimated against is the clip's own state.  params == NULL detaches (and frees the block); attaching
 * again replaces the parameters.  wct_clip_destroy frees the block.  A clip without motion attached behaves exactly as wct_hip_video.h
 * says.  WCT_ERR_INVALID: a NULL clip, a clip of another context, a parameter outside its range. */
int wct_motion_attach(wct_ctx* ctx, wct_clip* clip, const wct_motion_params* params);
/* The field of the last frame (all zero after a cut), device to device in stream order.  mv_dev: wct_motion_shape(Ho, Wo) vectors of the
 * clip's Ho x Wo.  WCT_ERR_INVALID: a NULL pointer, a clip of another context; WCT_ERR_STATE: no motion attached. */
int wct_motion_export(wct_ctx* ctx, wct_clip* clip, int16_t* mv_dev);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_MOTION_H */
