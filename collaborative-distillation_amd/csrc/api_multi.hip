// Several styles in one call behind the C ABI: regions and weighted moments / interpolation / blend (include/wct_hip.h), region-to-region
// transfer and k-means feature regions (wct_hip_guided.h).  Host orchestration only; the kernels are in regions.hip / cluster.hip / blend.hip.
#include "../../include/wct_hip_guided.h"
#include "wct_ctx.h"

using namespace wct_host;

namespace wct_host {

int apply_labeled_impl(wct_ctx* ctx, const float* feat, int C, long npix, const uint8_t* lab, int K, const double* M, const double* b, float* out) {
  if (int rc = ensure(ctx, ctx->wsRegApply, apply_labeled_workspace_bytes(C, K))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "apply_labeled", 2.0 * C * C * npix, 8.0 * C * npix + npix);
  HIPCHK(ctx, launch_apply_labeled(feat, C, npix, lab, K, M, b, out, ctx->wsRegApply.p, ctx->wsRegApply.cap, ctx->main.stream));
  return WCT_OK;
}

}  // namespace wct_host

// =====================================================================================================
// Spatial control: K styles over the regions of a uint8 label map (regions.hip).  Per region, the level's transform is the
// reference's whiten_and_color (util_wct.py:62-131) on that region's feature columns; everything else in the cascade is local.
namespace {
constexpr int REG_MAX = 8;

int labeled_args(wct_ctx* ctx, const char* what, int C, int h, int w, int K) {
  if (C < 4 || (C & 3) || C > 512) return fail(ctx, WCT_ERR_INVALID, "%s: C=%d must be a multiple of 4 in [4,512]", what, C);
  if (h < 1 || w < 1) return fail(ctx, WCT_ERR_INVALID, "%s: bad map %dx%d", what, h, w);
  if (K < 1 || K > REG_MAX) return fail(ctx, WCT_ERR_INVALID, "%s: K=%d outside [1, %d]", what, K, REG_MAX);
  return WCT_OK;
}

int moments_labeled_impl(wct_ctx* ctx, Lane& ln, const float* feat, int C, int h, int w, const uint8_t* lab, int K, double* n, double* sum,
                         double* sumsq) {
  const long npix = (long)h * w;
  if (int rc = ensure(ctx, ctx->wsRegMom, moments_labeled_workspace_bytes(C, npix, K))) return rc;
  ProfScope ps(ctx, ln.stream, "moments_labeled", 2.0 * C * C * npix, 4.0 * C * npix + (double)K * npix);
  HIPCHK(ctx, launch_moments_labeled(feat, C, npix, lab, K, n, sum, sumsq, ctx->wsRegMom.p, ctx->wsRegMom.cap, ln.stream, mom32_on(ctx, npix)));
  return WCT_OK;
}

// the K style sides of one level, slot by slot (they share featS and the side lane's sums: one after the other)
int style_side_slots(wct_ctx* ctx, int level, int K, const float* const* styles, const int* Hs, const int* Ws) {
  for (int k = 0; k < K; ++k)
    if (int rc = style_side(ctx, level, styles[k], Hs[k], Ws[k], k)) return rc;
  return WCT_OK;
}

// geometry of a K-style call: level L's feature map is h[L] x w[L] in every run (the cascade crops to multiples of 16 at level 5 and
// keeps that size); what the call keeps per level (label map, K pooled weight maps) lives at element off[L] of its buffer
struct LevelGeom {
  int h[6], w[6];
  size_t off[6];
};

// g for an H x W content with per_pixel elements per feature pixel, every level's block padded to a multiple of `align` elements (a
// power of two); returns the elements of all five
size_t level_geom(LevelGeom& g, int H, int W, size_t per_pixel, size_t align) {
  size_t total = 0;
  for (int level = 5; level >= 1; --level) {
    g.h[level] = (H >> 4) << (5 - level);
    g.w[level] = (W >> 4) << (5 - level);
    g.off[level] = total;
    total += (per_pixel * g.h[level] * g.w[level] + align - 1) & ~(align - 1);
  }
  return total;
}

// a regions call: the level label maps in regLab (bytes); cnt[L][v] = pixels of lab_L with label v (host, read back once)
struct RegionPlan : LevelGeom {
  unsigned cnt[6][256];
};

// One level of a K-style cascade on the main lane: encoder (fp32 NHWC) -> K sets of content moments -> one content solve per active
// slot k, against style slot k -> (M, b) per slot, the identity for the idle ones -> apply -> the decoder with its unfolded first conv.
// What the regions and the weights cascades do differently comes in as callables:
//   moments(fC, C, h, w, n, sum, sumsq): the K moment sets into regSums = [n K (only with n_head) |] sum K*C | sumsq K*C*C
//   slot_n(k): the samples behind slot k's moments, as the solver is to count them; below 2 the slot is idle
//   apply(fC, C, npix, M, b, fO): the K maps on the feature
// `what` names the cascade in the refusal.
template <typename MOMENTS, typename SLOTN, typename APPLY>
int multi_style_level(wct_ctx* ctx, const char* what, int level, const float* img, int H, int W, const LevelGeom& g, int K, const float* alpha,
                      bool n_head, float* dst, int* ho, int* wo, MOMENTS&& moments, SLOTN&& slot_n, APPLY&& apply) {
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  const int C = me.layers.back().d.cout;
  int h, w;
  level_dims(level, H, W, h, w);
  if (h != g.h[level] || w != g.w[level]) return fail(ctx, WCT_ERR_INVALID, "%s: level %d map %dx%d, planned %dx%d", what, level, h, w, g.h[level], g.w[level]);
  Lane& ln = ctx->main;
  const size_t fbytes = (size_t)h * w * C * sizeof(float), cc = (size_t)C * C;
  if (int rc = ensure(ctx, ctx->featC, fbytes)) return rc;
  if (int rc = ensure(ctx, ctx->regFeat, fbytes)) return rc;
  if (int rc = ensure(ctx, ctx->regSums, (size_t)K * ((n_head ? 1 : 0) + C + cc) * sizeof(double))) return rc;
  if (int rc = ensure(ctx, ctx->regMb, (size_t)K * (cc + C) * sizeof(double))) return rc;
  SumsView sv;
  if (int rc = sums_view(ctx, ln, sv)) return rc;
  float* fC = reinterpret_cast<float*>(ctx->featC.p);
  float* fO = reinterpret_cast<float*>(ctx->regFeat.p);
  double* n = reinterpret_cast<double*>(ctx->regSums.p);
  double* sum = n + (n_head ? K : 0);
  double* sumsq = sum + (size_t)K * C;
  double* M = reinterpret_cast<double*>(ctx->regMb.p);
  double* b = M + (size_t)K * cc;
  if (int rc = encode_impl(ctx, ln, level, img, H, W, fC, nullptr, nullptr)) return rc;
  if (int rc = moments(fC, C, h, w, n, sum, sumsq)) return rc;
  unsigned ident = 0;
  for (int k = 0; k < K; ++k) {
    const double nk = slot_n(k);
    if (nk < 2) { ident |= 1u << k; continue; }
    if (int rc = eig_impl(ctx, ln, C, nk, sum + (size_t)k * C, sumsq + k * cc, 1, ctx->eigCR[k], sv.info)) return rc;
  }
  HIPCHK(ctx, hipStreamWaitEvent(ln.stream, ctx->ev_style[level], 0));
  for (int k = 0; k < K; ++k)
    if (!(ident >> k & 1u))
      if (int rc = assemble_impl(ctx, C, ctx->eigCR[k], ctx->eigR[k][level], alpha[k], M + k * cc, b + (size_t)k * C)) return rc;
  HIPCHK(ctx, launch_mb_identity(M, b, C, K, ident, ln.stream));
  if (int rc = apply(fC, C, (long)h * w, M, b, fO)) return rc;
  if (int rc = decode_impl(ctx, level, fO, h, w, nullptr, dst)) return rc;
  *ho = h << (level - 1);
  *wo = w << (level - 1);
  return WCT_OK;
}

// The style half of the guidance (include/wct_hip_guided.h): which style image region k is transformed against, and for a style with a
// label map its level maps (gdLab, element lab_off[s] + off[L]) and per-(level, label) pixel counts.  wct_stylize_regions is the case
// without maps and with region_style[k] = k.
struct StyleMapPlan {
  int h[6], w[6];
  size_t off[6];
  unsigned cnt[6][256];
};

struct GuidedStyles {
  int S = 0;
  const float* const* styles = nullptr;
  const int *Hs = nullptr, *Ws = nullptr;
  const uint8_t* const* maps = nullptr;     // null: no style has a map
  const int* region_style = nullptr;        // null: region k against style k
  bool any_mapped = false;
  std::vector<StyleMapPlan> plan;           // [S], filled for the mapped styles
  size_t lab_off[REG_MAX] = {};
  int style_of(int k) const { return region_style ? region_style[k] : k; }
  bool mapped(int s) const { return maps && maps[s]; }
  // style pixels behind region k at `level`: the whole image (always >= 2 where its encoder runs) or its label k
  double style_n(int level, int k) const {
    const int s = style_of(k);
    return mapped(s) ? (double)plan[s].cnt[level][k] : 2.0;
  }
};

// one level of the regions cascade: per-label moments, a region with fewer than 2 content or style pixels keeps its features, per-label apply
int regions_level(wct_ctx* ctx, int level, const float* img, int H, int W, const RegionPlan& pl, const GuidedStyles& g, int K, const float* alpha,
                  float* dst, int* ho, int* wo) {
  const uint8_t* lab = reinterpret_cast<const uint8_t*>(ctx->regLab.p) + pl.off[level];
  return multi_style_level(
      ctx, "regions", level, img, H, W, pl, K, alpha, true, dst, ho, wo,
      [&](const float* fC, int C, int h, int w, double* n, double* sum, double* sumsq) {
        return moments_labeled_impl(ctx, ctx->main, fC, C, h, w, lab, K, n, sum, sumsq);
      },
      [&](int k) -> double { return g.style_n(level, k) < 2 ? 0.0 : (double)pl.cnt[level][k]; },
      [&](const float* fC, int C, long npix, const double* M, const double* b, float* fO) { return apply_labeled_impl(ctx, fC, C, npix, lab, K, M, b, fO); });
}

// The style side of one level of a regions / guided call.  Unmapped styles: style_side into slot k, region by region, as ever.  A mapped
// style that a region names: encoded ONCE into featS (fp32 NHWC at every level: the fused level-1 moments keep no feature map), its
// per-label moments over its level map into gdSums with the side lane's OWN workspace (the main lane's moments_labeled_impl is using
// regSums / wsRegMom meanwhile), then one matrix square root per region naming it, with that region's style pixel count.
int guided_style_side(wct_ctx* ctx, int level, int K, const GuidedStyles& g) {
  for (int k = 0; k < K; ++k) {
    const int s = g.style_of(k);
    if (!g.mapped(s))
      if (int rc = style_side(ctx, level, g.styles[s], g.Hs[s], g.Ws[s], k)) return rc;
  }
  if (!g.any_mapped) return WCT_OK;
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  const int C = me.layers.back().d.cout;
  const size_t cc = (size_t)C * C;
  Lane& ln = ctx->overlap ? ctx->side : ctx->main;
  for (int s = 0; s < g.S; ++s) {
    if (!g.mapped(s)) continue;
    bool named = false;
    for (int k = 0; k < K; ++k) named = named || g.style_of(k) == s;
    if (!named) continue;
    const StyleMapPlan& sp = g.plan[s];
    const int hs = sp.h[level], ws = sp.w[level];
    const long npix = (long)hs * ws;
    if (int rc = ensure(ctx, ctx->featS, (size_t)npix * C * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->gdSums, (size_t)K * (1 + C + cc) * sizeof(double))) return rc;
    if (int rc = ensure(ctx, ctx->wsGdMom, moments_labeled_workspace_bytes(C, npix, K))) return rc;
    SumsView sv;
    if (int rc = sums_view(ctx, ln, sv)) return rc;
    float* fS = reinterpret_cast<float*>(ctx->featS.p);
    double* n = reinterpret_cast<double*>(ctx->gdSums.p);
    double* sum = n + K;
    double* sumsq = sum + (size_t)K * C;
    const uint8_t* lab = reinterpret_cast<const uint8_t*>(ctx->gdLab.p) + g.lab_off[s] + sp.off[level];
    if (int rc = encode_impl(ctx, ln, level, g.styles[s], g.Hs[s], g.Ws[s], fS, nullptr, nullptr)) return rc;
    {
      ProfScope ps(ctx, ln.stream, "moments_labeled", 2.0 * C * C * npix, 4.0 * C * npix + (double)K * npix);
      HIPCHK(ctx, launch_moments_labeled(fS, C, npix, lab, K, n, sum, sumsq, ctx->wsGdMom.p, ctx->wsGdMom.cap, ln.stream, mom32_on(ctx, npix)));
    }
    for (int k = 0; k < K; ++k)
      if (g.style_of(k) == s && sp.cnt[level][k] >= 2)
        if (int rc = eig_impl(ctx, ln, C, (double)sp.cnt[level][k], sum + (size_t)k * C, sumsq + k * cc, 0, ctx->eigR[k][level], sv.info + 1)) return rc;
  }
  HIPCHK(ctx, hipEventRecord(ctx->ev_style[level], ln.stream));
  return WCT_OK;
}

// wct_stylize_regions and wct_stylize_guided: ONE path.  `what` names the entry in a refusal.
int regions_cascade(wct_ctx* ctx, const char* what, const float* content, int H, int W, const uint8_t* labels, int K, GuidedStyles& g,
                    const float* alpha, int num_run, float* out, int* Ho, int* Wo) {
  for (int level = 1; level <= 5; ++level)
    if (!ctx->mod[WCT_KIND_ENC][level].loaded || !ctx->mod[WCT_KIND_DEC][level].loaded) return fail(ctx, WCT_ERR_STATE, "%s: level %d not loaded", what, level);
  if (H < 32 || W < 32) return fail(ctx, WCT_ERR_INVALID, "%s: content %dx%d too small for level 5", what, H, W);
  // label maps of the five levels + their histograms, read back ONCE: the solvers take each region's pixel count on the host, and the
  // labels are checked before anything is written to `out`
  RegionPlan pl{};
  const size_t total = level_geom(pl, H, W, 1, 256);
  if (int rc = ensure(ctx, ctx->regLab, total)) return rc;
  if (int rc = ensure(ctx, ctx->regHist, 6 * 256 * sizeof(unsigned))) return rc;
  if (!ctx->reg_hist_host) HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->reg_hist_host), 6 * 256 * sizeof(unsigned), hipHostMallocDefault));
  // the mapped styles' geometry: the style is not cropped, level L's map is floor(Hs / 2^(L-1)) x floor(Ws / 2^(L-1)) (level_dims)
  size_t stotal = 0;
  if (g.any_mapped) {
    g.plan.assign(g.S, StyleMapPlan{});
    for (int s = 0; s < g.S; ++s) {
      if (!g.mapped(s)) continue;
      if (g.Hs[s] < 32 || g.Ws[s] < 32) return fail(ctx, WCT_ERR_INVALID, "%s: mapped style %d is %dx%d, too small for level 5", what, s, g.Hs[s], g.Ws[s]);
      g.lab_off[s] = stotal;
      size_t off = 0;
      for (int level = 5; level >= 1; --level) {
        level_dims(level, g.Hs[s], g.Ws[s], g.plan[s].h[level], g.plan[s].w[level]);
        g.plan[s].off[level] = off;
        off += ((size_t)g.plan[s].h[level] * g.plan[s].w[level] + 255) & ~(size_t)255;
      }
      stotal += off;
    }
    if (int rc = ensure(ctx, ctx->gdLab, stotal)) return rc;
    if (int rc = ensure(ctx, ctx->gdHist, (size_t)REG_MAX * 6 * 256 * sizeof(unsigned))) return rc;
    if (!ctx->gd_hist_host)
      HIPCHK(ctx, hipHostMalloc(reinterpret_cast<void**>(&ctx->gd_hist_host), (size_t)REG_MAX * 6 * 256 * sizeof(unsigned), hipHostMallocDefault));
  }
  uint8_t* maps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int level = 1; level <= 5; ++level) maps[level] = reinterpret_cast<uint8_t*>(ctx->regLab.p) + pl.off[level];
  unsigned* hist = reinterpret_cast<unsigned*>(ctx->regHist.p);
  {
    ProfScope ps(ctx, ctx->main.stream, "labels_levels", 0, (double)H * W + 2.0 * total);
    HIPCHK(ctx, launch_labels_levels(labels, H, W, pl.h, pl.w, maps, hist, ctx->main.stream));
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->reg_hist_host, hist, 6 * 256 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->main.stream));
  if (g.any_mapped) {
    for (int s = 0; s < g.S; ++s) {
      if (!g.mapped(s)) continue;
      uint8_t* smaps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
      for (int level = 1; level <= 5; ++level) smaps[level] = reinterpret_cast<uint8_t*>(ctx->gdLab.p) + g.lab_off[s] + g.plan[s].off[level];
      unsigned* shist = reinterpret_cast<unsigned*>(ctx->gdHist.p) + (size_t)s * 6 * 256;
      ProfScope ps(ctx, ctx->main.stream, "labels_levels", 0, (double)g.Hs[s] * g.Ws[s]);
      HIPCHK(ctx, launch_labels_levels(g.maps[s], g.Hs[s], g.Ws[s], g.plan[s].h, g.plan[s].w, smaps, shist, ctx->main.stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->gd_hist_host, ctx->gdHist.p, (size_t)g.S * 6 * 256 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->main.stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  memcpy(pl.cnt, ctx->reg_hist_host, sizeof pl.cnt);
  for (int v = K; v < 255; ++v)
    if (pl.cnt[0][v])
      return fail(ctx, WCT_ERR_INVALID, "%s: label value %d (%u pixels) is neither a region 0..%d nor 255 (unstyled)", what, v, pl.cnt[0][v], K - 1);
  for (int s = 0; s < g.S && g.any_mapped; ++s) {
    if (!g.mapped(s)) continue;
    memcpy(g.plan[s].cnt, ctx->gd_hist_host + (size_t)s * 6 * 256, sizeof g.plan[s].cnt);
    for (int v = K; v < 255; ++v)
      if (g.plan[s].cnt[0][v])
        return fail(ctx, WCT_ERR_INVALID, "%s: style %d label value %d (%u pixels) is neither a region 0..%d nor 255 (unused)", what, s, v,
                    g.plan[s].cnt[0][v], K - 1);
  }
  if (int rc = with_deferred_solves(ctx, false, [&]() -> int {
        if (int rc = fork_side(ctx)) return rc;
        if (int rc = guided_style_side(ctx, 5, K, g)) return rc;
        return run_cascade(
            ctx, content, H, W, num_run, out, Ho, Wo,
            [&](int level, const float* cur, int h, int w, float* dst, int* ho, int* wo) { return regions_level(ctx, level, cur, h, w, pl, g, K, alpha, dst, ho, wo); },
            [&](int level) { return guided_style_side(ctx, level - 1, K, g); });
      })) return rc;
  return range_readback(ctx);
}
}  // namespace

extern "C" {

int wct_moments_labeled(wct_ctx* ctx, const float* feat, int C, int h, int w, const uint8_t* lab, int K, double* n, double* sum,
                        double* sumsq) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !lab || !n || !sum || !sumsq) return fail(ctx, WCT_ERR_INVALID, "moments_labeled: NULL pointer");
  if (int rc = labeled_args(ctx, "moments_labeled", C, h, w, K)) return rc;
  return moments_labeled_impl(ctx, ctx->main, feat, C, h, w, lab, K, n, sum, sumsq);
}

int wct_apply_labeled(wct_ctx* ctx, const float* feat, int C, int h, int w, int layout, const uint8_t* lab, int K, const double* M,
                      const double* b, float* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !lab || !M || !b || !out) return fail(ctx, WCT_ERR_INVALID, "apply_labeled: NULL pointer");
  if (int rc = labeled_args(ctx, "apply_labeled", C, h, w, K)) return rc;
  const long npix = (long)h * w;
  if (layout == WCT_LAYOUT_NHWC) return apply_labeled_impl(ctx, feat, C, npix, lab, K, M, b, out);
  if (layout != WCT_LAYOUT_NCHW) return fail(ctx, WCT_ERR_INVALID, "apply_labeled: bad layout %d", layout);
  return apply_nchw(ctx, feat, C, npix, out, [&](const float* in, float* res) { return apply_labeled_impl(ctx, in, C, npix, lab, K, M, b, res); });
}

int wct_stylize_regions(wct_ctx* ctx, const float* content, int H, int W, const uint8_t* labels, int K, const float* const* styles,
                        const int* Hs, const int* Ws, const float* alpha, int num_run, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (ctx->transform != WCT_TRANSFORM_WCT) return fail(ctx, WCT_ERR_INVALID, "stylize_regions: defined for the wct transform only (wct_set_transform)");
  if (!content || !labels || !styles || !Hs || !Ws || !alpha || !out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "stylize_regions: bad arguments");
  if (K < 1 || K > REG_MAX) return fail(ctx, WCT_ERR_INVALID, "stylize_regions: K=%d outside [1, %d]", K, REG_MAX);
  for (int k = 0; k < K; ++k) {
    if (!styles[k]) return fail(ctx, WCT_ERR_INVALID, "stylize_regions: style %d is NULL", k);
    if (!std::isfinite(alpha[k])) return fail(ctx, WCT_ERR_INVALID, "stylize_regions: alpha[%d] is not finite", k);
  }
  GuidedStyles g;
  g.S = K; g.styles = styles; g.Hs = Hs; g.Ws = Ws;
  return regions_cascade(ctx, "stylize_regions", content, H, W, labels, K, g, alpha, num_run, out, Ho, Wo);
}

int wct_stylize_guided(wct_ctx* ctx, const float* content, int H, int W, const uint8_t* labels, int K, int S, const float* const* styles,
                       const int* Hs, const int* Ws, const uint8_t* const* style_labels, const int* region_style, const float* alpha,
                       int num_run, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (ctx->transform != WCT_TRANSFORM_WCT) return fail(ctx, WCT_ERR_INVALID, "stylize_guided: defined for the wct transform only (wct_set_transform)");
  if (!content || !labels || !styles || !Hs || !Ws || !style_labels || !region_style || !alpha || !out || num_run < 1)
    return fail(ctx, WCT_ERR_INVALID, "stylize_guided: bad arguments");
  if (K < 1 || K > WCT_GUIDED_MAX_REGIONS) return fail(ctx, WCT_ERR_INVALID, "stylize_guided: K=%d outside [1, %d]", K, WCT_GUIDED_MAX_REGIONS);
  if (S < 1 || S > WCT_GUIDED_MAX_STYLES) return fail(ctx, WCT_ERR_INVALID, "stylize_guided: S=%d outside [1, %d]", S, WCT_GUIDED_MAX_STYLES);
  GuidedStyles g;
  g.S = S; g.styles = styles; g.Hs = Hs; g.Ws = Ws; g.maps = style_labels; g.region_style = region_style;
  for (int s = 0; s < S; ++s) {
    if (!styles[s]) return fail(ctx, WCT_ERR_INVALID, "stylize_guided: style %d is NULL", s);
    g.any_mapped = g.any_mapped || style_labels[s] != nullptr;
  }
  for (int k = 0; k < K; ++k) {
    if (region_style[k] < 0 || region_style[k] >= S) return fail(ctx, WCT_ERR_INVALID, "stylize_guided: region_style[%d]=%d outside [0, %d)", k, region_style[k], S);
    if (!std::isfinite(alpha[k])) return fail(ctx, WCT_ERR_INVALID, "stylize_guided: alpha[%d] is not finite", k);
  }
  return regions_cascade(ctx, "stylize_guided", content, H, W, labels, K, g, alpha, num_run, out, Ho, Wo);
}

}  // extern "C"

// ---- k-means on feature maps (include/wct_hip_guided.h; kernels in cluster.hip) ---------------------------------------------------------
namespace {
int kmeans_args(wct_ctx* ctx, const char* what, int C, int h, int w, int K) {
  if (C < 4 || (C & 3) || C > 512) return fail(ctx, WCT_ERR_INVALID, "%s: C=%d must be a multiple of 4 in [4,512]", what, C);
  if (h < 1 || w < 1 || (long)h * w >= (1L << 31)) return fail(ctx, WCT_ERR_INVALID, "%s: bad map %dx%d", what, h, w);
  if (K < 1 || K > WCT_KMEANS_MAX_K) return fail(ctx, WCT_ERR_INVALID, "%s: K=%d outside [1, %d]", what, K, WCT_KMEANS_MAX_K);
  return WCT_OK;
}

int kmeans_assign_impl(wct_ctx* ctx, const float* feat, int C, long npix, const double* shift, const double* scale, const double* cent, int K,
                       uint8_t* labels, double* n, double* sum, double* cost, double* next) {
  if (int rc = ensure(ctx, ctx->kmWs, kmeans_assign_workspace_bytes(C, npix, K))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "kmeans_assign", 3.0 * K * C * npix, 4.0 * C * npix);
  HIPCHK(ctx, launch_kmeans_assign(feat, C, npix, shift, scale, cent, K, labels, n, sum, cost, next, ctx->kmWs.p, ctx->kmWs.cap, ctx->main.stream));
  return WCT_OK;
}

int kmeans_seed_impl(wct_ctx* ctx, const float* feat, int C, long npix, const double* shift, const double* scale, int K, double* cent, int* idx) {
  if (int rc = ensure(ctx, ctx->kmWs, kmeans_seed_workspace_bytes(npix))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "kmeans_seed", 3.0 * K * C * npix, 4.0 * K * C * npix);
  HIPCHK(ctx, launch_kmeans_seed(feat, C, npix, shift, scale, K, cent, idx, ctx->kmWs.p, ctx->kmWs.cap, ctx->main.stream));
  return WCT_OK;
}
}  // namespace

extern "C" {

int wct_kmeans_assign(wct_ctx* ctx, const float* feat, int C, int h, int w, const double* shift, const double* scale, const double* centroids,
                      int K, uint8_t* labels, double* n, double* sum, double* cost, double* next) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !shift || !scale || !centroids || !n || !sum || !cost) return fail(ctx, WCT_ERR_INVALID, "kmeans_assign: NULL pointer");
  if (reinterpret_cast<uintptr_t>(feat) & 15) return fail(ctx, WCT_ERR_INVALID, "kmeans_assign: the map must be 16-byte aligned");
  if (int rc = kmeans_args(ctx, "kmeans_assign", C, h, w, K)) return rc;
  return kmeans_assign_impl(ctx, feat, C, (long)h * w, shift, scale, centroids, K, labels, n, sum, cost, next);
}

int wct_kmeans_seed(wct_ctx* ctx, const float* feat, int C, int h, int w, const double* shift, const double* scale, int K, double* centroids,
                    int* idx) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !shift || !scale || !centroids || !idx) return fail(ctx, WCT_ERR_INVALID, "kmeans_seed: NULL pointer");
  if (reinterpret_cast<uintptr_t>(feat) & 15) return fail(ctx, WCT_ERR_INVALID, "kmeans_seed: the map must be 16-byte aligned");
  if (int rc = kmeans_args(ctx, "kmeans_seed", C, h, w, K)) return rc;
  return kmeans_seed_impl(ctx, feat, C, (long)h * w, shift, scale, K, centroids, idx);
}

int wct_feature_regions(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs, int Ws, int K, int iters,
                        uint8_t* labels_c, uint8_t* labels_s, double* centroids_out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || !style || !labels_c || !labels_s) return fail(ctx, WCT_ERR_INVALID, "feature_regions: NULL pointer");
  if (level < 2 || level > 5) return fail(ctx, WCT_ERR_INVALID, "feature_regions: level %d outside 2..5", level);
  if (iters < 1 || iters > WCT_KMEANS_MAX_ITERS) return fail(ctx, WCT_ERR_INVALID, "feature_regions: iters=%d outside [1, %d]", iters, WCT_KMEANS_MAX_ITERS);
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "feature_regions: encoder %d not loaded", level);
  const int C = me.layers.back().d.cout;
  const int smin = 2 << (level - 1);
  if (H < smin || W < smin || Hs < smin || Ws < smin)
    return fail(ctx, WCT_ERR_INVALID, "feature_regions: images %dx%d / %dx%d too small for level %d", H, W, Hs, Ws, level);
  int h, w, hs, ws;
  level_dims(level, H, W, h, w);
  level_dims(level, Hs, Ws, hs, ws);
  if (int rc = kmeans_args(ctx, "feature_regions", C, h, w, K)) return rc;
  if (int rc = kmeans_args(ctx, "feature_regions", C, hs, ws, K)) return rc;
  Lane& ln = ctx->main;
  const long np = (long)h * w, nps = (long)hs * ws;
  const size_t kc = (size_t)K * C;
  if (int rc = ensure(ctx, ctx->kmFeatC, (size_t)np * C * sizeof(float))) return rc;
  if (int rc = ensure(ctx, ctx->kmFeatS, (size_t)nps * C * sizeof(float))) return rc;
  // [sh_c C | sc_c C | sh_s C | sc_s C | centroids 2 K C | n K | sum K C | cost 1] fp64, then idx K int32 (padded), lab_c, lab_s
  const size_t nd = 4 * (size_t)C + 2 * kc + K + kc + 1, idx_off = nd * sizeof(double), labc_off = idx_off + 64, labs_off = labc_off + (((size_t)np + 255) & ~(size_t)255);
  if (int rc = ensure(ctx, ctx->kmStat, labs_off + (size_t)nps)) return rc;
  if (int rc = ensure(ctx, ctx->kmWs, std::max({kmeans_seed_workspace_bytes(nps), kmeans_assign_workspace_bytes(C, nps, K), kmeans_assign_workspace_bytes(C, np, K)})))
    return rc;   // once for the whole call: a growing workspace would synchronise between the passes
  SumsView sv;
  if (int rc = sums_view(ctx, ln, sv)) return rc;
  float* fC = reinterpret_cast<float*>(ctx->kmFeatC.p);
  float* fS = reinterpret_cast<float*>(ctx->kmFeatS.p);
  double* st = reinterpret_cast<double*>(ctx->kmStat.p);
  double *sh_c = st, *sc_c = st + C, *sh_s = st + 2 * C, *sc_s = st + 3 * C, *cent = st + 4 * C;
  double *n = cent + 2 * kc, *sum = n + K, *cost = sum + kc;
  int* idx = reinterpret_cast<int*>(reinterpret_cast<char*>(ctx->kmStat.p) + idx_off);
  uint8_t* lab_c = reinterpret_cast<uint8_t*>(ctx->kmStat.p) + labc_off;
  uint8_t* lab_s = reinterpret_cast<uint8_t*>(ctx->kmStat.p) + labs_off;
  if (int rc = encode_impl(ctx, ln, level, content, H, W, fC, nullptr, nullptr)) return rc;
  if (int rc = moments_impl(ctx, ln, fC, C, h, w, 0, w, sv.sum, sv.sumsq)) return rc;
  HIPCHK(ctx, launch_kmeans_standardise(sv.sum, sv.sumsq, C, (double)np, sh_c, sc_c, ln.stream));
  if (int rc = encode_impl(ctx, ln, level, style, Hs, Ws, fS, nullptr, nullptr)) return rc;
  if (int rc = moments_impl(ctx, ln, fS, C, hs, ws, 0, ws, sv.sum, sv.sumsq)) return rc;
  HIPCHK(ctx, launch_kmeans_standardise(sv.sum, sv.sumsq, C, (double)nps, sh_s, sc_s, ln.stream));
  if (int rc = kmeans_seed_impl(ctx, fS, C, nps, sh_s, sc_s, K, cent, idx)) return rc;
  for (int it = 0; it < iters; ++it)
    if (int rc = kmeans_assign_impl(ctx, fS, C, nps, sh_s, sc_s, cent + (it & 1) * kc, K, nullptr, n, sum, cost, cent + ((it + 1) & 1) * kc)) return rc;
  const double* fin = cent + (iters & 1) * kc;
  if (int rc = kmeans_assign_impl(ctx, fS, C, nps, sh_s, sc_s, fin, K, lab_s, n, sum, cost, nullptr)) return rc;
  if (int rc = kmeans_assign_impl(ctx, fC, C, np, sh_c, sc_c, fin, K, lab_c, n, sum, cost, nullptr)) return rc;
  HIPCHK(ctx, launch_kmeans_expand(lab_s, hs, ws, level, labels_s, Hs, Ws, ln.stream));
  HIPCHK(ctx, launch_kmeans_expand(lab_c, h, w, level, labels_c, H, W, ln.stream));
  if (centroids_out) HIPCHK(ctx, hipMemcpyAsync(centroids_out, fin, kc * sizeof(double), hipMemcpyDeviceToDevice, ln.stream));
  return range_readback(ctx);
}

}  // extern "C"

// =====================================================================================================
// Style interpolation (uniform weights) and per-pixel style weights (blend.hip).  The reference's whiten_and_color (util_wct.py:62-131)
// is linear in the style statistics: sum_k lambda_k WCT(fc, fs_k) is the single-style transform against ONE blended style slot
// (sum_k lambda_k cov_s,k^(1/2), sum_k lambda_k mu_s,k).  Weight maps generalise regions: per level, reliability-weighted content
// moments per style and out_p = x_p + sum_k w_k(p) alpha_k (target_k(x_p) - x_p).
namespace {
int moments_weighted_impl(wct_ctx* ctx, Lane& ln, const float* feat, int C, int h, int w, const float* wts, int K, double* sum, double* sumsq) {
  const long npix = (long)h * w;
  if (int rc = ensure(ctx, ctx->wsRegMom, moments_weighted_workspace_bytes(C, npix, K))) return rc;
  ProfScope ps(ctx, ln.stream, "moments_weighted", 2.0 * C * C * npix * K, 4.0 * C * npix + 4.0 * K * npix);
  HIPCHK(ctx, launch_moments_weighted(feat, C, npix, wts, K, sum, sumsq, ctx->wsRegMom.p, ctx->wsRegMom.cap, ln.stream, mom32_on(ctx, npix)));
  return WCT_OK;
}

int apply_mixed_impl(wct_ctx* ctx, const float* feat, int C, long npix, const float* wts, int K, const double* M, const double* b, float* out) {
  if (int rc = ensure(ctx, ctx->wsBlendApply, apply_mixed_workspace_bytes(C, K))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "apply_mixed", 2.0 * C * C * npix, 8.0 * C * npix + 4.0 * K * npix);
  HIPCHK(ctx, launch_apply_mixed(feat, C, npix, wts, K, M, b, out, ctx->wsBlendApply.p, ctx->wsBlendApply.cap, ctx->main.stream));
  return WCT_OK;
}

// lambda (host, K values): finite, >= 0, sum > 0 -> lambda / sum (as -styleInterpWeights)
int normalised_lambda(wct_ctx* ctx, const char* what, int K, const float* lambda, double* out) {
  if (!lambda) return fail(ctx, WCT_ERR_INVALID, "%s: NULL weights", what);
  double sum = 0.;
  for (int k = 0; k < K; ++k) {
    if (!std::isfinite(lambda[k]) || lambda[k] < 0.f) return fail(ctx, WCT_ERR_INVALID, "%s: weight %d (%g) must be finite and >= 0", what, k, (double)lambda[k]);
    sum += lambda[k];
  }
  if (!(sum > 0.)) return fail(ctx, WCT_ERR_INVALID, "%s: the weights sum to 0", what);
  for (int k = 0; k < K; ++k) out[k] = lambda[k] / sum;
  return WCT_OK;
}

// F = sum_k lam[k] F_k, mu = sum_k lam[k] mu_k into eigS[level] on `st`, then the style-side fold and ev_style[level] (what content_side
// waits for).  F[k] / mu[k]: device pointers.
int blend_into_style(wct_ctx* ctx, int level, int K, const double* const* F, const double* const* mu, const double* lam, hipStream_t st) {
  const size_t C = ctx->mod[WCT_KIND_ENC][level].layers.back().d.cout, cc = C * C;
  if (int rc = ensure(ctx, ctx->eigS[level], eig_result_bytes((int)C))) return rc;
  double* res = reinterpret_cast<double*>(ctx->eigS[level].p);
  {
    ProfScope ps(ctx, st, "stats_blend", 2.0 * K * (cc + C), 8.0 * (K + 1) * (cc + C));
    HIPCHK(ctx, launch_stats_blend((int)C, K, F, mu, lam, res + eig_result_F_offset(C), res + cc + C, st));
  }
  if (int rc = style_fold(ctx, level, st)) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev_style[level], st));
  return WCT_OK;
}

// style side of one level of wct_stylize_interp: the K style sides into eigR[k][level], then their blend into eigS[level] (side lane)
int interp_style_side(wct_ctx* ctx, int level, int K, const float* const* styles, const int* Hs, const int* Ws, const double* lam) {
  if (int rc = style_side_slots(ctx, level, K, styles, Hs, Ws)) return rc;
  const size_t C = ctx->mod[WCT_KIND_ENC][level].layers.back().d.cout, cc = C * C;
  const double* F[REG_MAX];
  const double* mu[REG_MAX];
  for (int k = 0; k < K; ++k) {
    const double* r = reinterpret_cast<const double*>(ctx->eigR[k][level].p);
    F[k] = r + eig_result_F_offset(C);
    mu[k] = r + cc + C;
  }
  Lane& ln = ctx->overlap ? ctx->side : ctx->main;
  return blend_into_style(ctx, level, K, F, mu, lam, ln.stream);
}

int multi_style_args(wct_ctx* ctx, const char* what, const float* content, int H, int W, int K, const float* const* styles, const int* Hs,
                     const int* Ws, int num_run, const float* out) {
  if (!content || !styles || !Hs || !Ws || !out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "%s: bad arguments", what);
  if (K < 1 || K > REG_MAX) return fail(ctx, WCT_ERR_INVALID, "%s: K=%d outside [1, %d]", what, K, REG_MAX);
  for (int k = 0; k < K; ++k)
    if (!styles[k]) return fail(ctx, WCT_ERR_INVALID, "%s: style %d is NULL", what, k);
  for (int level = 1; level <= 5; ++level)
    if (!ctx->mod[WCT_KIND_ENC][level].loaded || !ctx->mod[WCT_KIND_DEC][level].loaded) return fail(ctx, WCT_ERR_STATE, "%s: level %d not loaded", what, level);
  if (H < 32 || W < 32) return fail(ctx, WCT_ERR_INVALID, "%s: content %dx%d too small for level 5", what, H, W);
  return WCT_OK;
}

// a weights call: the K pooled weight maps of every level in blendW (floats); V1[L][k], V2[L][k] read back once
struct BlendPlan : LevelGeom {
  double V1[6][REG_MAX], V2[6][REG_MAX];
};
constexpr size_t BLEND_STAT_BYTES = 6 * REG_MAX * 2 * sizeof(double) + 4 * sizeof(unsigned);

// one level of the weights cascade: weighted moments, n_eff = V1^2 / V2 samples per active style with its sums scaled by V1 / V2 (the
// solver's (sumsq - n mu mu^T) / (n - 1) is then the reliability-weighted covariance), mixed apply
int blend_level(wct_ctx* ctx, int level, const float* img, int H, int W, const BlendPlan& pl, int K, const float* alpha, float* dst, int* ho, int* wo) {
  const float* wl = reinterpret_cast<const float*>(ctx->blendW.p) + pl.off[level];
  auto n_eff = [&](int k) -> double {
    const double v1 = pl.V1[level][k], v2 = pl.V2[level][k];
    return v1 > 0. && v2 > 0. && v1 * v1 / v2 >= 2. ? v1 * v1 / v2 : 0.;
  };
  return multi_style_level(
      ctx, "stylize_blend", level, img, H, W, pl, K, alpha, false, dst, ho, wo,
      [&](const float* fC, int C, int h, int w, double*, double* sum, double* sumsq) -> int {
        if (int rc = moments_weighted_impl(ctx, ctx->main, fC, C, h, w, wl, K, sum, sumsq)) return rc;
        double f[REG_MAX];
        for (int k = 0; k < K; ++k) f[k] = n_eff(k) > 0. ? pl.V1[level][k] / pl.V2[level][k] : 1.;
        HIPCHK(ctx, launch_scale_sums(sum, sumsq, C, K, f, ctx->main.stream));
        return WCT_OK;
      },
      n_eff, [&](const float* fC, int C, long npix, const double* M, const double* b, float* fO) { return apply_mixed_impl(ctx, fC, C, npix, wl, K, M, b, fO); });
}
}  // namespace

extern "C" {

int wct_moments_weighted(wct_ctx* ctx, const float* feat, int C, int h, int w, const float* weights, int K, double* sum, double* sumsq) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !weights || !sum || !sumsq) return fail(ctx, WCT_ERR_INVALID, "moments_weighted: NULL pointer");
  if (int rc = labeled_args(ctx, "moments_weighted", C, h, w, K)) return rc;
  return moments_weighted_impl(ctx, ctx->main, feat, C, h, w, weights, K, sum, sumsq);
}

int wct_apply_mixed(wct_ctx* ctx, const float* feat, int C, int h, int w, int layout, const float* weights, int K, const double* M,
                    const double* b, float* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !weights || !M || !b || !out) return fail(ctx, WCT_ERR_INVALID, "apply_mixed: NULL pointer");
  if (int rc = labeled_args(ctx, "apply_mixed", C, h, w, K)) return rc;
  const long npix = (long)h * w;
  if (layout == WCT_LAYOUT_NHWC) return apply_mixed_impl(ctx, feat, C, npix, weights, K, M, b, out);
  if (layout != WCT_LAYOUT_NCHW) return fail(ctx, WCT_ERR_INVALID, "apply_mixed: bad layout %d", layout);
  return apply_nchw(ctx, feat, C, npix, out, [&](const float* in, float* res) { return apply_mixed_impl(ctx, in, C, npix, weights, K, M, b, res); });
}

int wct_style_blend(wct_ctx* ctx, int level, int K, const double* stats, const float* lambda) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !stats) return fail(ctx, WCT_ERR_INVALID, "style_blend: bad arguments");
  if (K < 1 || K > REG_MAX) return fail(ctx, WCT_ERR_INVALID, "style_blend: K=%d outside [1, %d]", K, REG_MAX);
  double lam[REG_MAX];
  if (int rc = normalised_lambda(ctx, "style_blend", K, lambda, lam)) return rc;
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  const size_t C = me.layers.back().d.cout, cc = C * C;
  const double* F[REG_MAX];
  const double* mu[REG_MAX];
  for (int k = 0; k < K; ++k) {
    F[k] = stats + (size_t)k * (cc + C);
    mu[k] = F[k] + cc;
  }
  return blend_into_style(ctx, level, K, F, mu, lam, ctx->main.stream);
}

int wct_stylize_interp(wct_ctx* ctx, const float* content, int H, int W, int K, const float* const* styles, const int* Hs, const int* Ws,
                       const float* lambda, float alpha, int num_run, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = multi_style_args(ctx, "stylize_interp", content, H, W, K, styles, Hs, Ws, num_run, out)) return rc;
  if (!std::isfinite(alpha)) return fail(ctx, WCT_ERR_INVALID, "stylize_interp: alpha is not finite");
  double lam[REG_MAX];
  if (int rc = normalised_lambda(ctx, "stylize_interp", K, lambda, lam)) return rc;
  if (int rc = with_deferred_solves(ctx, false, [&]() -> int {
        if (int rc = fork_side(ctx)) return rc;
        if (int rc = interp_style_side(ctx, 5, K, styles, Hs, Ws, lam)) return rc;
        return run_cascade(
            ctx, content, H, W, num_run, out, Ho, Wo,
            [&](int level, const float* cur, int h, int w, float* dst, int* ho, int* wo) { return content_side(ctx, level, cur, h, w, alpha, dst, ho, wo); },
            [&](int level) { return interp_style_side(ctx, level - 1, K, styles, Hs, Ws, lam); });
      })) return rc;
  return range_readback(ctx);
}

int wct_stylize_blend(wct_ctx* ctx, const float* content, int H, int W, const float* weights, int K, const float* const* styles, const int* Hs,
                      const int* Ws, const float* alpha, int num_run, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (ctx->transform != WCT_TRANSFORM_WCT) return fail(ctx, WCT_ERR_INVALID, "stylize_blend: defined for the wct transform only (wct_set_transform)");
  if (!weights || !alpha) return fail(ctx, WCT_ERR_INVALID, "stylize_blend: bad arguments");
  if (int rc = multi_style_args(ctx, "stylize_blend", content, H, W, K, styles, Hs, Ws, num_run, out)) return rc;
  for (int k = 0; k < K; ++k)
    if (!std::isfinite(alpha[k])) return fail(ctx, WCT_ERR_INVALID, "stylize_blend: alpha[%d] is not finite", k);
  // the pooled weight maps of the five levels, their (V1, V2) and the weight check, read back ONCE: the solvers take each style's
  // n_eff on the host, and the weights are checked before anything is written to `out`
  BlendPlan pl{};
  const size_t total = level_geom(pl, H, W, K, 64);
  if (int rc = ensure(ctx, ctx->blendW, total * sizeof(float))) return rc;
  if (int rc = ensure(ctx, ctx->blendStat, BLEND_STAT_BYTES)) return rc;
  if (int rc = ensure(ctx, ctx->wsBlendPool, weights_levels_workspace_bytes(H, W))) return rc;
  if (!ctx->blend_host) HIPCHK(ctx, hipHostMalloc(&ctx->blend_host, BLEND_STAT_BYTES, hipHostMallocDefault));
  float* maps[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int level = 1; level <= 5; ++level) maps[level] = reinterpret_cast<float*>(ctx->blendW.p) + pl.off[level];
  double* vv = reinterpret_cast<double*>(ctx->blendStat.p);
  unsigned* cnt = reinterpret_cast<unsigned*>(vv + 6 * REG_MAX * 2);
  {
    ProfScope ps(ctx, ctx->main.stream, "weights_levels", 0, 4.0 * K * H * W * 6 + 4.0 * total);
    HIPCHK(ctx, launch_weights_levels(weights, H, W, K, pl.h, pl.w, maps, vv, cnt, ctx->wsBlendPool.p, ctx->wsBlendPool.cap, ctx->main.stream));
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->blend_host, ctx->blendStat.p, BLEND_STAT_BYTES, hipMemcpyDeviceToHost, ctx->main.stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  const double* hv = reinterpret_cast<const double*>(ctx->blend_host);
  const unsigned* hc = reinterpret_cast<const unsigned*>(hv + 6 * REG_MAX * 2);
  if (hc[0]) return fail(ctx, WCT_ERR_INVALID, "stylize_blend: %u weight value(s) are not finite", hc[0]);
  if (hc[1]) return fail(ctx, WCT_ERR_INVALID, "stylize_blend: %u weight value(s) lie outside [0, 1]", hc[1]);
  if (hc[2]) return fail(ctx, WCT_ERR_INVALID, "stylize_blend: at %u pixel(s) the weights sum to more than 1", hc[2]);
  for (int level = 1; level <= 5; ++level)
    for (int k = 0; k < K; ++k) {
      pl.V1[level][k] = hv[((size_t)level * REG_MAX + k) * 2];
      pl.V2[level][k] = hv[((size_t)level * REG_MAX + k) * 2 + 1];
    }
  if (int rc = with_deferred_solves(ctx, false, [&]() -> int {
        if (int rc = fork_side(ctx)) return rc;
        if (int rc = style_side_slots(ctx, 5, K, styles, Hs, Ws)) return rc;
        return run_cascade(
            ctx, content, H, W, num_run, out, Ho, Wo,
            [&](int level, const float* cur, int h, int w, float* dst, int* ho, int* wo) { return blend_level(ctx, level, cur, h, w, pl, K, alpha, dst, ho, wo); },
            [&](int level) { return style_side_slots(ctx, level - 1, K, styles, Hs, Ws); });
      })) return rc;
  return range_readback(ctx);
}

}  // extern "C"
