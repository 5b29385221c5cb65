/* libwct_hip -- region-to-region transfer: style label maps and k-means feature regions.
 *
 * wct_stylize_regions of wct_hip.h gives every content region its own style IMAGE, whole.  The paired form of spatial control -- Gatys et
 * al., "Controlling Perceptual Factors in Neural Style Transfer" (CVPR 2017), section 4; the mask-guided front ends of WCT and PhotoWCT --
 * also labels the STYLE: the style's sky goes on the content's sky, from one style image with its own label map (wct_stylize_guided).
 * Where no segmentation exists the label maps are made by clustering the style's features and giving every content feature pixel the
 * nearest cluster -- Zhang et al., "Multimodal Style Transfer via Graph Cuts" (ICCV 2019), without the graph cut -- wct_feature_regions,
 * on top of wct_kmeans_seed / wct_kmeans_assign.
 * Everything in wct_hip.h holds here too: return codes, wct_last_error, device pointers unless marked HOST, one context = one stream.
 * Every entry returns WCT_ERR_INVALID -- wct_last_error names the entry -- before anything is written when an argument is bad.
 *
 * Definitions
 *
 * Guided transfer.  Region k of the content (label k of the H x W uint8 map; 255 = unstyled) is exactly wct_stylize_regions' region k:
 * at level L its pixels are those of lab_L[i][j] = labels[i s + s/2][j s + s/2], s = 2^(L-1).  It is transformed against style image
 * region_style[k].  If that style has a label map, only its feature pixels with label k enter the style mean and covariance of the level;
 * the style's level map follows the same rule in the style's own coordinates: lab_s,L[i][j] = style_labels[i s + s/2][j s + s/2] over the
 * floor(Hs / s) x floor(Ws / s) feature map of the (uncropped) style.  A NULL map means the whole image, as in wct_stylize_regions.  A region
 * keeps its content features at a level where it has fewer than 2 content pixels OR fewer than 2 style pixels.
 *
 * Standardised space.  z_c = (x_c - sh_c) * sc_c per channel of an NHWC fp32 map: sh and sc are fp64 arrays rounded to fp32, the
 * subtraction comes first, then the product -- two fp32 roundings, never a fused step, so numpy reproduces z bit for bit.
 * Distance.  d_k = SUM_c (z_c - m_kc)^2, the direct difference form, in fp32 in a channel order that is a function of C alone; m = the
 * fp64 centroids rounded to fp32.  The label is the arg-min, the LOWEST k among equal distances.
 * Farthest-first start.  centre 0 = the pixel with the largest |z|^2, centre j = the pixel with the largest min_{i<j} d(z, centre_i),
 * each the lowest pixel index among equals; K passes over the map.
 *
 * Nothing here clamps to the f16x3 range; no floating-point atomics: every result is bitwise reproducible across calls and contexts.
 * The k-means workspaces and the style side's label maps and moments live in the context on top of wct_workspace_bytes, allocated on
 * first use of a size, scratch in the sense of the "poison" hook.
 */
#ifndef WCT_HIP_GUIDED_H
#define WCT_HIP_GUIDED_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_GUIDED_MAX_REGIONS 8     /* K */
#define WCT_GUIDED_MAX_STYLES 8      /* S */
#define WCT_KMEANS_MAX_K 8
#define WCT_KMEANS_MAX_ITERS 64
#define WCT_KMEANS_DEAD_VARIANCE 1e-12   /* wct_feature_regions: a channel at or under this share of the largest variance gets sc = 0 */

/* The five-level cascade with content regions AND style regions, num_run times: planar 3 x Ho x Wo into out (Ho x Wo as wct_stylize).
 * labels: H x W uint8 on the device.  styles, Hs, Ws, style_labels: HOST arrays of S entries -- device pointers to planar 3 x Hs[s] x Ws[s]
 * images and to their Hs[s] x Ws[s] uint8 maps, a NULL map = unmapped.  region_style (K ints in [0, S)) and alpha (K floats): HOST.
 * Style side: each distinct mapped style that a region names is encoded once per level on the side lane, its per-label moments taken
 * over its level map, and one matrix square root solved per region naming it; an unmapped style goes through the same style side as in
 * wct_stylize_regions, once per region naming it.  With every map NULL, S == K and region_style[k] == k the call IS wct_stylize_regions:
 * the same code path, bit for bit.
 * Like wct_stylize_regions the call synchronises the caller's stream ONCE -- the level maps and label histograms of the content and of
 * every mapped style are made in one pre-pass and read back together: the solvers take the pixel counts on the host, and the labels are
 * checked before anything is written to out -- so it cannot be captured into a HIP graph.  Prepared style slots survive the call.
 * WCT_ERR_INVALID: a NULL argument or style image, K outside 1 .. 8, S outside 1 .. 8, region_style[k] outside [0, S), a non-finite
 * alpha, num_run < 1, a content under 32 x 32, a mapped style under 32 x 32, a content or style label other than 0 .. K-1 and 255, a
 * transform mode other than wct (wct_hip_transform.h). */
int wct_stylize_guided(wct_ctx* ctx, const float* content, int H, int W, const uint8_t* labels, int K, int S, const float* const* styles,
                       const int* Hs, const int* Ws, const uint8_t* const* style_labels, const int* region_style, const float* alpha,
                       int num_run, float* out, int* Ho, int* Wo);

/* One Lloyd step in one pass over feat (NHWC fp32, h x w x C, 16-byte aligned; C a multiple of 4 in 4 .. 512; 1 <= K <= 8).
 * shift, scale: C fp64; centroids: K x C fp64 (standardised space).  labels: h x w uint8 or NULL.  n[K], sum[K x C], cost[1]: fp64 --
 * the pixels of each label, the totals of the fp32 z over each label, SUM of the minimal distances.  The totals are taken in fp64 per
 * workgroup and reduced in a fixed order: a function of the input alone.  next (K x C fp64, or NULL; may be `centroids` itself):
 * sum_k / n_k where n_k > 0, else centroids_k -- an empty cluster stays where it was -- made on the device, nothing is read back. */
int wct_kmeans_assign(wct_ctx* ctx, const float* feat, int C, int h, int w, const double* shift, const double* scale, const double* centroids,
                      int K, uint8_t* labels, double* n, double* sum, double* cost, double* next);
/* The farthest-first start: centroids (K x C fp64: the chosen pixels' z) and idx (K int32: their pixel indices i * w + j).  K passes,
 * nothing is read back. */
int wct_kmeans_seed(wct_ctx* ctx, const float* feat, int C, int h, int w, const double* shift, const double* scale, int K, double* centroids,
                    int* idx);
/* Label maps for wct_stylize_guided from the features of `level` (2 .. 5): both images are encoded; each is standardised with its OWN
 * sh = mean, sc = 1 / sqrt(population variance) from wct_moments -- sc = 0 where the variance is <= WCT_KMEANS_DEAD_VARIANCE of the
 * largest: dead channels behind a ReLU; seed on the STYLE map, `iters` (1 .. 64) Lloyd steps on the style map alone, one final assign
 * of each map against the final centroids; label(y, x) = lab[min(y / s, h - 1)][min(x / s, w - 1)], s = 2^(level-1).  labels_c: H x W,
 * labels_s: Hs x Ws uint8, every value in 0 .. K-1; centroids_out: K x C fp64 or NULL.  No synchronisation inside; the outputs go
 * straight into wct_stylize_guided with S = 1 and region_style[k] = 0. */
int wct_feature_regions(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs, int Ws, int K, int iters,
                        uint8_t* labels_c, uint8_t* labels_s, double* centroids_out);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_GUIDED_H */
