/* libwct_hip -- proxy mode: stylise a reduced copy, apply the result at full size through a bilateral grid of local affine colour
 * maps: the part of the C ABI behind `--proxy_scale`.
 *
 * The method is Chen, Adams, Wadhwa and Hasinoff, "Bilateral Guided Upsampling" (SIGGRAPH Asia 2016): from the pair (reduced input,
 * reduced output) of an image operator, fit a field of 3 x 4 affine colour maps that is coarse in x, y and luminance, and apply that
 * field to the full-resolution input.  It is also the output model of HDRnet and of Xia et al., "Joint Bilateral Learning for
 * Real-time Universal Photorealistic Style Transfer" (ECCV 2020).  The operator here is the cascade (wct_stylize).  Every output pixel
 * is an affine function of the content pixel under it: the result has the content's edges and the content's exact H x W, and what is
 * paid at full size is one memory-bound pass.  It transfers colour and tone, locally -- by construction no strokes or texture.
 * Everything in wct_hip.h holds here too: return codes, wct_last_error, device pointers, one context = one stream, asynchronous calls.
 * The device entries run on the context's stream, never synchronise on the 16x path, and return WCT_ERR_INVALID -- wct_last_error
 * names the entry -- before anything is written when an argument is bad.
 *
 * Definition
 *
 * Images: planar 3 x h x w fp32, any 4-byte alignment.  cl: the reduced content, h x w; sl: its stylisation, h x w; c: the full
 * content, H x W.
 *
 * Guide.  g = clamp(0.299 R + 0.587 G + 0.114 B, 0, 1), the coefficients of wct_luma_merge, evaluated in fp64.
 *
 * Grid.  gz x gh x gw vertices, gh and gw in 1 .. WCT_BGRID_MAX_XY, gz in 1 .. WCT_BGRID_MAX_Z.  Vertex (k, j, i) holds a 3 x 4 affine
 * map: A[((k gh + j) gw + i) 12 + 4 ch + a], fp32; a = 0 .. 2 multiplies R, G, B of the content, a = 3 is the offset of channel ch.
 *
 * Coordinates are normalised, so the reduced and the full image address the same grid.  Sample x of an axis with n samples and G
 * vertices: u = (x + 0.5) / n * (G - 1), i0 = min(floor(u), max(G - 2, 0)), f = u - i0; weight 1 - f on vertex i0 and f on vertex
 * min(i0 + 1, G - 1); G = 1 gives weight 1 on vertex 0.  z: u = g (gz - 1), the same rule.  A pixel's weight on a vertex is the
 * product of the three tent weights: 8 vertices, summing to 1.
 *
 * Fit, from (cl, sl), eps > 0 and smooth in 0 .. WCT_BGRID_MAX_SMOOTH, with v = (R, G, B, 1) of cl and s the pixel of sl:
 *   1. per vertex     Gv = SUM_p w_v(p) v v^T  (4 x 4 symmetric: 10 distinct sums)      Rv = SUM_p w_v(p) v s_p^T  (4 x 3: 12 sums)
 *   2. smooth times   a [1 2 1] / 4 pass along z, then y, then x over all the sums, the edge vertex repeated at the borders (this
 *                     preserves the totals)
 *   3. Gg, Rg = the totals over all vertices;  lambda = eps h w / (gz gh gw);  Ag = (Gg + lambda I)^-1 Rg
 *   4. A_v = (Gv + lambda I)^-1 (Rv + lambda Ag): a local least-squares fit regularised towards the global one.  A vertex no pixel
 *      reaches (its weight sum is exactly 0) gets Ag.  The matrix is symmetric positive definite with smallest eigenvalue >= lambda:
 *      CHOLESKY, four forward and four back substitutions per output channel.
 * Everything is fp64 and rounded ONCE to fp32 into A.
 *
 * Slice.  For every pixel of c: the 12 coefficients interpolated from its 8 vertices with the weights above (guide from c itself),
 * then out_ch = A_ch . (R, G, B, 1).  THE SLICE INTERPOLATES IN FP64: guide, weights, the 8-vertex sums (in the order k, j, i, one fma
 * each) and the final dot product are fp64 of the fp32 grid and content, rounded once to fp32.  Planar fp32 is NOT clamped; on the
 * uint8 path the round_mode conversion of wct_planar_to_u8 is fused in, byte-identical to wct_planar_to_u8 of the planar result.
 *
 * Arithmetic.  No floating-point atomics.  The order of every sum is a function of the shapes and parameters alone -- never of CU
 * count, launch geometry, alignment or call history: a vertex's sums are gathered from the reduced pixels within one cell of it in
 * row chunks of WCT_BGRID_FIT_ROWS rows of its support (64 lanes striding the chunk in row-major order, folded 32, 16, .. 1 lanes
 * apart), the chunks added in ascending order; the totals over slabs of 256 vertices likewise.  Both entries are bitwise reproducible
 * across calls, views and contexts, as wct_guided_filter is.  The slice reads a tile's vertices from LDS where they fit and from
 * global memory where they do not (a grid finer than the pixels), with identical bits on both paths.
 *
 * Context memory.  The fit's sums -- (2 + chunks) x 22 fp64 per vertex, chunks = ceil(tallest support / WCT_BGRID_FIT_ROWS) when
 * that is above 1, else 0 -- and, for wct_stylize_proxy, cl, sl and the grid belong to the context: allocated on first use of a size,
 * ON TOP of wct_workspace_bytes, not covered by wct_reserve, like the buffers of wct_stylize_smooth; scratch in the sense of the
 * "poison" hook.
 */
#ifndef WCT_HIP_BGRID_H
#define WCT_HIP_BGRID_H

#include "wct_hip_scale.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_BGRID_MAX_XY 256
#define WCT_BGRID_MAX_Z 32
#define WCT_BGRID_MAX_SMOOTH 4
#define WCT_BGRID_FIT_ROWS 64        /* rows of a vertex's support per partial sum of the fit */
#define WCT_BGRID_TILE_W 128         /* the slice's tile of full-resolution pixels per workgroup */
#define WCT_BGRID_TILE_H 8
#define WCT_BGRID_LDS_VERTICES 320   /* a tile whose footprint has more vertices (15 KB) reads the grid from global memory */
/* the command line's defaults: a look, not a measurement */
#define WCT_BGRID_CELL 16
#define WCT_BGRID_BINS 8
#define WCT_BGRID_EPS 1e-2
#define WCT_BGRID_SMOOTH 1

/* Host only.  gh = ceil(h / cell) + 1, gw = ceil(w / cell) + 1: one vertex per `cell` reduced pixels and one to close the axis.
 * WCT_ERR_INVALID (no context: no message) for a NULL result, h, w or cell < 1, or a result outside 1 .. WCT_BGRID_MAX_XY. */
int wct_bgrid_shape(int h, int w, int cell, int* gh, int* gw);
/* grid (gz gh gw 12 floats) = the fit of (cl, sl) above.  WCT_ERR_INVALID: a NULL image or grid, h or w < 1, a grid axis outside its
 * range, eps not finite or <= 0, smooth outside 0 .. WCT_BGRID_MAX_SMOOTH, a grid that overlaps cl or sl. */
int wct_bgrid_fit(wct_ctx* ctx, const float* cl, const float* sl, int h, int w, int gz, int gh, int gw, double eps, int smooth, float* grid);
/* The slice above.  Exactly one of out_planar (fp32, 3 x H x W) and out_hwc (uint8, H x W x 3, any alignment) is non-NULL.
 * out_planar == content is ALLOWED (a thread reads its pixels before it writes them and no other thread reads them); every other
 * overlap of the output with the content, and any with the grid, is refused.  Also WCT_ERR_INVALID: a NULL grid or content, H or
 * W < 1, a grid axis outside its range, round_mode outside {0, 1}. */
int wct_bgrid_slice(wct_ctx* ctx, const float* grid, int gz, int gh, int gw, const float* content, int H, int W, float* out_planar, uint8_t* out_hwc,
                    int round_mode);
/* Six public calls in one.  (h, w) = wct_scale_shape of (H, W, divisor); cl = wct_resample_planar of the content to h x w with
 * WCT_FILTER_BICUBIC; sl = wct_stylize of (cl, style, alpha, num_run) -- style == NULL: wct_stylize_prepared, against the statistics in
 * the context, as wct_stylize_scaled allows; (gh, gw) = wct_bgrid_shape of (h, w, cell); wct_bgrid_fit of (cl, sl) with (gz, gh, gw,
 * eps, smooth); wct_bgrid_slice of the full content.
 * Bit-identical to that composition of public calls; follows the context's transform (wct_set_transform).  On the 16x path it never
 * synchronises, allocates nothing after the first call of a size (wct_debug_get "ws_allocs" does not move) and can be captured into
 * one HIP graph.  The result is H x W: exactly one of out_planar and out_hwc, as in wct_bgrid_slice, out_planar == content allowed.
 * WCT_ERR_INVALID: a NULL content, both or neither output, num_run < 1, bad shapes, divisor outside 1 .. WCT_SCALE_MAX_DIVISOR or a
 * working size under 32, cell < 1 or a grid outside its range, the fit's refusals of gz, eps and smooth, round_mode outside {0, 1},
 * an output overlapping the content (other than out_planar == content); WCT_ERR_STATE: style == NULL without prepared statistics. */
int wct_stylize_proxy(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run, int divisor,
                      int cell, int gz, double eps, int smooth, float* out_planar, uint8_t* out_hwc, int round_mode);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_BGRID_H */
