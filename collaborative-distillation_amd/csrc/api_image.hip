// Image-space entry points of the C ABI: uint8 conversion and resize (include/wct_hip.h), colour preservation (wct_hip_color.h),
// guided-filter smoothing (wct_hip_smooth.h) and scale control (wct_hip_scale.h).  Host orchestration only; the kernels are in
// misc.hip / resize.hip / color.hip / smooth.hip / scale.hip.
#include "../../include/wct_hip_color.h"
#include "../../include/wct_hip_scale.h"
#include "../../include/wct_hip_smooth.h"
#include "wct_ctx.h"

using namespace wct_host;

// ---- colour preservation (include/wct_hip_color.h; kernels in color.hip) ------------------------------------------------------------
namespace {
constexpr size_t COLOR_WS_HEAD = 64;   // doubles in front of the stage-1 partials: the two sides' sums and (A, t) of wct_color_match

int color_ws(wct_ctx* ctx, long npix) { return ensure(ctx, ctx->colWs, COLOR_WS_HEAD * sizeof(double) + color_moments_workspace_bytes(npix)); }

int color_moments_impl(wct_ctx* ctx, const float* planar, int H, int W, double* sum, double* sumsq) {
  const long npix = (long)H * W;
  if (int rc = color_ws(ctx, npix)) return rc;
  ProfScope ps(ctx, ctx->main.stream, "color_moments", 18.0 * npix, 12.0 * npix);
  HIPCHK(ctx, launch_color_moments(planar, npix, sum, sumsq, reinterpret_cast<double*>(ctx->colWs.p) + COLOR_WS_HEAD,
                                   ctx->colWs.cap - COLOR_WS_HEAD * sizeof(double), ctx->main.stream));
  return WCT_OK;
}

int color_solve_impl(wct_ctx* ctx, double n_c, const double* sum_c, const double* sumsq_c, double n_s, const double* sum_s, const double* sumsq_s,
                     double eps, double* A, double* t) {
  ProfScope ps(ctx, ctx->main.stream, "color_solve", 0, 36 * sizeof(double));
  HIPCHK(ctx, launch_color_solve(n_c, sum_c, sumsq_c, n_s, sum_s, sumsq_s, eps, A, t, ctx->main.stream));
  return WCT_OK;
}

int color_apply_impl(wct_ctx* ctx, const float* in, int H, int W, const double* A, const double* t, float* out) {
  const long npix = (long)H * W;
  ProfScope ps(ctx, ctx->main.stream, "color_apply", 18.0 * npix, 24.0 * npix);
  HIPCHK(ctx, launch_color_apply(in, npix, A, t, out, ctx->main.stream));
  return WCT_OK;
}

int color_match_impl(wct_ctx* ctx, const float* style, int Hs, int Ws, const float* content, int H, int W, float* style_out) {
  const long ns = (long)Hs * Ws, nc = (long)H * W;
  if (int rc = color_ws(ctx, ns > nc ? ns : nc)) return rc;   // both sides' partials fit BEFORE the first sums are written: the head never moves
  double* hd = reinterpret_cast<double*>(ctx->colWs.p);
  double *sum_s = hd, *sumsq_s = hd + 3, *sum_c = hd + 12, *sumsq_c = hd + 15, *A = hd + 24, *t = hd + 33;
  if (int rc = color_moments_impl(ctx, style, Hs, Ws, sum_s, sumsq_s)) return rc;
  if (int rc = color_moments_impl(ctx, content, H, W, sum_c, sumsq_c)) return rc;
  if (int rc = color_solve_impl(ctx, (double)nc, sum_c, sumsq_c, (double)ns, sum_s, sumsq_s, WCT_COLOR_EPS, A, t)) return rc;
  return color_apply_impl(ctx, style, Hs, Ws, A, t, style_out);
}

int luma_merge_impl(wct_ctx* ctx, const float* stylised, int Ho, int Wo, const float* content, int Hc, int Wc, float* out_planar, uint8_t* out_hwc,
                    int round_mode) {
  ProfScope ps(ctx, ctx->main.stream, "luma_merge", 14.0 * Ho * Wo, (out_planar ? 36.0 : 27.0) * Ho * Wo);
  HIPCHK(ctx, launch_luma_merge(stylised, Ho, Wo, content, Hc, Wc, out_planar, out_hwc, round_mode, ctx->main.stream));
  return WCT_OK;
}
}  // namespace

extern "C" {

int wct_color_moments(wct_ctx* ctx, const float* planar, int H, int W, double* sum, double* sumsq) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!planar || !sum || !sumsq || H < 1 || W < 1)
    return fail(ctx, WCT_ERR_INVALID, "wct_color_moments: bad arguments (%dx%d, planar %s, sum %s, sumsq %s)", H, W, planar ? "given" : "NULL",
                sum ? "given" : "NULL", sumsq ? "given" : "NULL");
  if ((long)H * W > color_moments_max_pixels())
    return fail(ctx, WCT_ERR_INVALID, "wct_color_moments: %dx%d exceeds the %ld pixels the summation contract covers", H, W, color_moments_max_pixels());
  return color_moments_impl(ctx, planar, H, W, sum, sumsq);
}

int wct_color_solve(wct_ctx* ctx, double n_c, const double* sum_c, const double* sumsq_c, double n_s, const double* sum_s, const double* sumsq_s,
                    double eps, double* A, double* t) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!sum_c || !sumsq_c || !sum_s || !sumsq_s || !A || !t) return fail(ctx, WCT_ERR_INVALID, "wct_color_solve: NULL argument");
  if (!(n_c >= 2.0) || !(n_s >= 2.0) || !std::isfinite(n_c) || !std::isfinite(n_s))
    return fail(ctx, WCT_ERR_INVALID, "wct_color_solve: at least 2 pixels on either side expected, got n_c = %g, n_s = %g", n_c, n_s);
  if (!std::isfinite(eps) || !(eps > 0.0)) return fail(ctx, WCT_ERR_INVALID, "wct_color_solve: eps must be finite and positive, got %g", eps);
  return color_solve_impl(ctx, n_c, sum_c, sumsq_c, n_s, sum_s, sumsq_s, eps, A, t);
}

int wct_color_apply(wct_ctx* ctx, const float* in, int H, int W, const double* A, const double* t, float* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!in || !A || !t || !out || H < 1 || W < 1) return fail(ctx, WCT_ERR_INVALID, "wct_color_apply: bad arguments (%dx%d, or a NULL pointer)", H, W);
  return color_apply_impl(ctx, in, H, W, A, t, out);
}

int wct_color_match(wct_ctx* ctx, const float* style, int Hs, int Ws, const float* content, int H, int W, float* style_out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!style || !content || !style_out) return fail(ctx, WCT_ERR_INVALID, "wct_color_match: NULL argument");
  if (Hs < 1 || Ws < 1 || H < 1 || W < 1 || (long)Hs * Ws < 2 || (long)H * W < 2)
    return fail(ctx, WCT_ERR_INVALID, "wct_color_match: at least 2 pixels on either side expected, got style %dx%d, content %dx%d", Hs, Ws, H, W);
  if ((long)Hs * Ws > color_moments_max_pixels() || (long)H * W > color_moments_max_pixels())
    return fail(ctx, WCT_ERR_INVALID, "wct_color_match: style %dx%d or content %dx%d exceeds the %ld pixels the summation contract covers", Hs, Ws, H, W,
                color_moments_max_pixels());
  return color_match_impl(ctx, style, Hs, Ws, content, H, W, style_out);
}

int wct_luma_merge(wct_ctx* ctx, const float* stylised, int Ho, int Wo, const float* content, int Hc, int Wc, float* out_planar, uint8_t* out_hwc,
                   int round_mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!stylised || !content) return fail(ctx, WCT_ERR_INVALID, "wct_luma_merge: NULL image");
  if ((out_planar != nullptr) == (out_hwc != nullptr))
    return fail(ctx, WCT_ERR_INVALID, "wct_luma_merge: exactly one of out_planar and out_hwc expected, got %s", out_planar ? "both" : "neither");
  if (Ho < 1 || Wo < 1 || Ho > Hc || Wo > Wc)
    return fail(ctx, WCT_ERR_INVALID, "wct_luma_merge: result %dx%d must be non-empty and no larger than the content %dx%d", Ho, Wo, Hc, Wc);
  if (round_mode != 0 && round_mode != 1) return fail(ctx, WCT_ERR_INVALID, "wct_luma_merge: round_mode 0 or 1 expected, got %d", round_mode);
  return luma_merge_impl(ctx, stylised, Ho, Wo, content, Hc, Wc, out_planar, out_hwc, round_mode);
}

}  // extern "C"

// ---- guided-filter smoothing (include/wct_hip_smooth.h; kernels in smooth.hip) -------------------------------------------------------
namespace {
int smooth_bufs(wct_ctx* ctx, long npix) {
  if (int rc = ensure(ctx, ctx->smSums, smooth_sums_bytes(npix))) return rc;
  return ensure(ctx, ctx->smAB, smooth_ab_bytes(npix));
}

int guided_filter_impl(wct_ctx* ctx, const float* src, int Ho, int Wo, const float* guide, int Hg, int Wg, int radius, double eps, float* out_planar,
                       uint8_t* out_hwc, int round_mode) {
  const long npix = (long)Ho * Wo;
  if (int rc = smooth_bufs(ctx, npix)) return rc;
  ProfScope ps(ctx, ctx->main.stream, "guided_filter", 600.0 * npix, (24.0 + 168.0 * 2 + 48.0 * 2 + 96.0 * 2 + 12.0 + (out_planar ? 12.0 : 3.0)) * npix);
  HIPCHK(ctx, launch_guided_filter(src, Ho, Wo, guide, Hg, Wg, radius, eps, out_planar, out_hwc, round_mode, reinterpret_cast<double*>(ctx->smSums.p),
                                   ctx->smSums.cap, reinterpret_cast<float*>(ctx->smAB.p), ctx->smAB.cap, ctx->main.stream));
  return WCT_OK;
}

// the refusals both entries share; `who` names the entry
int smooth_check(wct_ctx* ctx, const char* who, int radius, double eps) {
  if (radius < 1 || radius > WCT_SMOOTH_MAX_RADIUS)
    return fail(ctx, WCT_ERR_INVALID, "%s: radius 1 .. %d expected, got %d", who, WCT_SMOOTH_MAX_RADIUS, radius);
  if (!std::isfinite(eps) || !(eps > 0.0)) return fail(ctx, WCT_ERR_INVALID, "%s: eps must be finite and positive, got %g", who, eps);
  return WCT_OK;
}

// body of wct_stylize_color and wct_stylize_smooth (`who`): colour match -> stylize -> [guided filter by the content] -> [luma merge].
// `smooth`: the filter runs, (radius, eps) are checked, and mode 0 (no colour preservation) is allowed.
int stylize_color_impl(wct_ctx* ctx, const char* who, bool smooth, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha,
                       int num_run, int mode, int radius, double eps, float* out, int* Ho, int* Wo) {
  if (!content || !style || !out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "%s: bad arguments (a NULL pointer, or num_run < 1)", who);
  if (mode < (smooth ? 0 : 1) || mode > 3)
    return fail(ctx, WCT_ERR_INVALID, "%s: %s %d is not %sWCT_COLOR_MATCH (1), WCT_COLOR_LUMA (2) or both (3)", who, smooth ? "color_mode" : "mode", mode,
                smooth ? "0, " : "");
  const bool match = mode & WCT_COLOR_MATCH, luma = mode & WCT_COLOR_LUMA;
  if (H < 1 || W < 1 || Hs < 1 || Ws < 1 || (match && ((long)Hs * Ws < 2 || (long)H * W < 2)))
    return fail(ctx, WCT_ERR_INVALID, "%s: bad shapes (content %dx%d, style %dx%d)", who, H, W, Hs, Ws);
  if (match && ((long)Hs * Ws > color_moments_max_pixels() || (long)H * W > color_moments_max_pixels()))
    return fail(ctx, WCT_ERR_INVALID, "%s: style %dx%d or content %dx%d exceeds the %ld pixels the summation contract covers", who, Hs, Ws, H, W,
                color_moments_max_pixels());
  if (smooth) {
    if (int rc = smooth_check(ctx, who, radius, eps)) return rc;
    if (ranges_overlap(out, (size_t)3 * H * W * sizeof(float), content, (size_t)3 * H * W * sizeof(float)))
      return fail(ctx, WCT_ERR_INVALID, "%s: out overlaps the content, which is the filter's guide", who);
  }
  // every buffer first: a growing one synchronises, and nothing enqueued below may find its source moved
  if (match)
    if (int rc = ensure(ctx, ctx->colStyle, (size_t)3 * Hs * Ws * sizeof(float))) return rc;
  if (luma)
    if (int rc = ensure(ctx, ctx->colOut, (size_t)3 * H * W * sizeof(float))) return rc;
  if (smooth)
    if (int rc = smooth_bufs(ctx, (long)H * W)) return rc;   // the result is no larger than the content
  const float* st = style;
  if (match) {
    float* matched = reinterpret_cast<float*>(ctx->colStyle.p);
    if (int rc = color_match_impl(ctx, style, Hs, Ws, content, H, W, matched)) return rc;
    st = matched;   // the side lane reads it behind fork_side's event, and the cascade's last level has waited for the side lane
  }
  float* dst = luma ? reinterpret_cast<float*>(ctx->colOut.p) : out;
  int ho = 0, wo = 0;
  if (int rc = stylize_impl(ctx, content, H, W, st, Hs, Ws, alpha, num_run, dst, &ho, &wo)) return rc;
  if (smooth)
    if (int rc = guided_filter_impl(ctx, dst, ho, wo, content, H, W, radius, eps, dst, nullptr, 0)) return rc;   // in place
  if (luma)
    if (int rc = luma_merge_impl(ctx, dst, ho, wo, content, H, W, out, nullptr, 0)) return rc;
  if (Ho) *Ho = ho;
  if (Wo) *Wo = wo;
  return WCT_OK;
}
}  // namespace

extern "C" {

int wct_guided_filter(wct_ctx* ctx, const float* src, int Ho, int Wo, const float* guide, int Hg, int Wg, int radius, double eps, float* out_planar,
                      uint8_t* out_hwc, int round_mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!src || !guide) return fail(ctx, WCT_ERR_INVALID, "wct_guided_filter: NULL image");
  if ((out_planar != nullptr) == (out_hwc != nullptr))
    return fail(ctx, WCT_ERR_INVALID, "wct_guided_filter: exactly one of out_planar and out_hwc expected, got %s", out_planar ? "both" : "neither");
  if (Ho < 1 || Wo < 1 || Ho > Hg || Wo > Wg)
    return fail(ctx, WCT_ERR_INVALID, "wct_guided_filter: source %dx%d must be non-empty and no larger than the guide %dx%d", Ho, Wo, Hg, Wg);
  if (int rc = smooth_check(ctx, "wct_guided_filter", radius, eps)) return rc;
  if (round_mode != 0 && round_mode != 1) return fail(ctx, WCT_ERR_INVALID, "wct_guided_filter: round_mode 0 or 1 expected, got %d", round_mode);
  const size_t out_bytes = (size_t)3 * Ho * Wo * (out_planar ? sizeof(float) : 1);
  if (ranges_overlap(out_planar ? static_cast<const void*>(out_planar) : static_cast<const void*>(out_hwc), out_bytes, guide,
                     (size_t)3 * Hg * Wg * sizeof(float)))
    return fail(ctx, WCT_ERR_INVALID, "wct_guided_filter: the output overlaps the guide, which the last kernel still reads");
  return guided_filter_impl(ctx, src, Ho, Wo, guide, Hg, Wg, radius, eps, out_planar, out_hwc, round_mode);
}

// (include/wct_hip_color.h; here because it shares its body with wct_stylize_smooth)
int wct_stylize_color(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run, int mode,
                      float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  return stylize_color_impl(ctx, "wct_stylize_color", false, content, H, W, style, Hs, Ws, alpha, num_run, mode, 0, 0., out, Ho, Wo);
}

int wct_stylize_smooth(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run, int color_mode,
                       int radius, double eps, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  return stylize_color_impl(ctx, "wct_stylize_smooth", true, content, H, W, style, Hs, Ws, alpha, num_run, color_mode, radius, eps, out, Ho, Wo);
}

int wct_u8_to_planar(wct_ctx* ctx, const uint8_t* hwc, int H, int W, float* planar) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!hwc || !planar || H < 1 || W < 1) return fail(ctx, WCT_ERR_INVALID, "u8_to_planar: bad arguments");
  ProfScope ps(ctx, ctx->main.stream, "u8_to_planar", 0, 15.0 * H * W);
  HIPCHK(ctx, launch_u8_to_planar(hwc, (long)H * W, planar, ctx->main.stream));
  return WCT_OK;
}

int wct_planar_to_u8(wct_ctx* ctx, const float* planar, int H, int W, uint8_t* hwc, int round_mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!hwc || !planar || H < 1 || W < 1 || (round_mode != 0 && round_mode != 1)) return fail(ctx, WCT_ERR_INVALID, "planar_to_u8: bad arguments");
  ProfScope ps(ctx, ctx->main.stream, "planar_to_u8", 0, 15.0 * H * W);
  HIPCHK(ctx, launch_planar_to_u8(planar, (long)H * W, hwc, round_mode, ctx->main.stream));
  return WCT_OK;
}

int wct_stylize_u8(wct_ctx* ctx, const uint8_t* content_hwc, int H, int W, const uint8_t* style_hwc, int Hs, int Ws,
                   float alpha, int num_run, uint8_t* out_hwc, int* Ho, int* Wo, int round_mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content_hwc || !style_hwc || !out_hwc) return fail(ctx, WCT_ERR_INVALID, "stylize_u8: bad arguments");
  if (int rc = ensure(ctx, ctx->u8c, (size_t)3 * H * W * sizeof(float))) return rc;
  if (int rc = ensure(ctx, ctx->u8s, (size_t)3 * Hs * Ws * sizeof(float))) return rc;
  if (int rc = ensure(ctx, ctx->u8o, (size_t)3 * H * W * sizeof(float))) return rc;
  float* c = reinterpret_cast<float*>(ctx->u8c.p);
  float* s = reinterpret_cast<float*>(ctx->u8s.p);
  float* o = reinterpret_cast<float*>(ctx->u8o.p);
  if (int rc = wct_u8_to_planar(ctx, style_hwc, Hs, Ws, s)) return rc;
  if (int rc = wct_u8_to_planar(ctx, content_hwc, H, W, c)) return rc;
  int ho = 0, wo = 0;
  if (int rc = wct_stylize(ctx, c, H, W, s, Hs, Ws, alpha, num_run, o, &ho, &wo)) return rc;
  if (int rc = wct_planar_to_u8(ctx, o, ho, wo, out_hwc, round_mode)) return rc;
  if (Ho) *Ho = ho;
  if (Wo) *Wo = wo;
  return WCT_OK;
}

int wct_resize_shape(int H, int W, int size, int* oH, int* oW) {
  if (H < 1 || W < 1 || size < 0 || !oH || !oW) return WCT_ERR_INVALID;
  *oH = H; *oW = W;
  if (size == 0 || (W <= H && W == size) || (H <= W && H == size)) return WCT_OK;
  // torchvision 0.2.1 functional.resize(img, int): the smaller edge becomes `size`, the other int(size * long / short)
  // (Python float division of ints, then truncation)
  if (W < H) { *oW = size; *oH = (int)((double)size * H / W); }
  else { *oH = size; *oW = (int)((double)size * W / H); }
  return (*oH >= 1 && *oW >= 1) ? WCT_OK : WCT_ERR_INVALID;
}

}  // extern "C"

namespace {
int resize_axis(wct_ctx* ctx, int in_size, int out_size, int filter, const ResizeAxis** out) {
  for (ResizeAxis& a : ctx->rsz_axes)
    if (a.in_size == in_size && a.out_size == out_size && a.filter == filter) { a.used = ++ctx->rsz_clock; *out = &a; return WCT_OK; }
  if (ctx->rsz_axes.size() >= 16) {   // a bounded cache: evict the least recently used entry (hipFree waits for kernels still reading it)
    size_t lru = 0;
    for (size_t i = 1; i < ctx->rsz_axes.size(); ++i)
      if (ctx->rsz_axes[i].used < ctx->rsz_axes[lru].used) lru = i;
    (void)hipFree(ctx->rsz_axes[lru].bounds);
    ctx->rsz_axes.erase(ctx->rsz_axes.begin() + (long)lru);
  }
  std::vector<int> bounds, kk;
  ResizeAxis a;
  a.in_size = in_size; a.out_size = out_size; a.filter = filter;
  resize_axis_tables(in_size, out_size, filter, a.ksize, bounds, kk);
  a.first = bounds[0];
  a.last = bounds[2 * (size_t)(out_size - 1)] + bounds[2 * (size_t)(out_size - 1) + 1];
  // bounds | shifted bounds | kk in ONE allocation and ONE copy: nothing to leak when a call fails part-way
  std::vector<int> tab(2 * bounds.size() + kk.size());
  std::copy(bounds.begin(), bounds.end(), tab.begin());
  std::copy(bounds.begin(), bounds.end(), tab.begin() + (long)bounds.size());
  for (int i = 0; i < out_size; ++i) tab[bounds.size() + 2 * (size_t)i] -= a.first;
  std::copy(kk.begin(), kk.end(), tab.begin() + 2 * (long)bounds.size());
  int* dev = nullptr;
  HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&dev), tab.size() * sizeof(int)));
  if (hipError_t e = hipMemcpy(dev, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice); e != hipSuccess) {
    (void)hipFree(dev);
    return fail(ctx, WCT_ERR_HIP, "resize tables: %s", hipGetErrorString(e));
  }
  a.bounds = dev; a.bounds_shifted = dev + bounds.size(); a.kk = dev + 2 * bounds.size();
  a.used = ++ctx->rsz_clock;
  ctx->rsz_axes.push_back(a);
  *out = &ctx->rsz_axes.back();
  return WCT_OK;
}

int resize_impl(wct_ctx* ctx, const uint8_t* src, int H, int W, int oH, int oW, uint8_t* dst, float* planar, int filter = RESIZE_BILINEAR) {
  if (!src || (!dst && !planar) || H < 1 || W < 1 || oH < 1 || oW < 1 || H > 65535 || oH > 65535)
    return fail(ctx, WCT_ERR_INVALID, "resize_u8: bad arguments (%dx%d -> %dx%d)", H, W, oH, oW);
  const ResizeAxis *ax = nullptr, *ay = nullptr;
  // the vector may reallocate (or evict) when the second axis is added: look the first one up again afterwards
  if (int rc = resize_axis(ctx, W, oW, filter, &ax)) return rc;
  if (int rc = resize_axis(ctx, H, oH, filter, &ay)) return rc;
  if (int rc = resize_axis(ctx, W, oW, filter, &ax)) return rc;
  if (int rc = resize_axis(ctx, H, oH, filter, &ay)) return rc;
  const bool need_h = oW != W, need_v = oH != H;
  const int row0 = need_v ? ay->first : 0, rows = need_v ? ay->last - ay->first : H;
  if (need_h && (need_v || planar))
    if (int rc = ensure(ctx, ctx->rsz_tmp, (size_t)rows * oW * 3)) return rc;
  ProfScope ps(ctx, ctx->main.stream, filter == RESIZE_BICUBIC ? "resize_u8<bicubic>" : "resize_u8", 0, 3.0 * H * W + 3.0 * oH * oW * (planar ? 4 : 1));
  HIPCHK(ctx, launch_resize_u8(src, H, W, oH, oW, ax->bounds, ax->kk, ax->ksize, ay->bounds_shifted, ay->kk, ay->ksize, row0, rows,
                               reinterpret_cast<uint8_t*>(ctx->rsz_tmp.p), dst, planar, ctx->main.stream));
  return WCT_OK;
}
}  // namespace

extern "C" {

int wct_resize_u8(wct_ctx* ctx, const uint8_t* src_hwc, int H, int W, uint8_t* dst_hwc, int oH, int oW) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!dst_hwc) return fail(ctx, WCT_ERR_INVALID, "resize_u8: bad arguments");
  return resize_impl(ctx, src_hwc, H, W, oH, oW, dst_hwc, nullptr);
}

int wct_resize_u8_to_planar(wct_ctx* ctx, const uint8_t* src_hwc, int H, int W, float* planar, int oH, int oW) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!planar) return fail(ctx, WCT_ERR_INVALID, "resize_u8_to_planar: bad arguments");
  return resize_impl(ctx, src_hwc, H, W, oH, oW, nullptr, planar);
}

int wct_resize_u8_filter(wct_ctx* ctx, const uint8_t* src_hwc, int H, int W, uint8_t* dst_hwc, float* planar, int oH, int oW, int filter) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if ((dst_hwc == nullptr) == (planar == nullptr)) return fail(ctx, WCT_ERR_INVALID, "resize_u8_filter: exactly one of dst_hwc / planar must be given");
  if (filter != WCT_FILTER_BILINEAR && filter != WCT_FILTER_BICUBIC)
    return fail(ctx, WCT_ERR_INVALID, "resize_u8_filter: unknown filter %d (WCT_FILTER_BILINEAR = 0, WCT_FILTER_BICUBIC = 1)", filter);
  return resize_impl(ctx, src_hwc, H, W, oH, oW, dst_hwc, planar, filter);
}

}  // extern "C"

// ---- scale control (include/wct_hip_scale.h; kernel in scale.hip) --------------------------------------------------------------------
namespace {
// the shapes both image calls accept; `who` names the entry
int scale_shapes_check(wct_ctx* ctx, const char* who, int H, int W, int oH, int oW) {
  if (H < 1 || W < 1 || oH < 1 || oW < 1) return fail(ctx, WCT_ERR_INVALID, "%s: empty shape (%dx%d -> %dx%d)", who, H, W, oH, oW);
  if ((long)H > (long)WCT_SCALE_MAX_SHRINK * oH || (long)W > (long)WCT_SCALE_MAX_SHRINK * oW)
    return fail(ctx, WCT_ERR_INVALID, "%s: %dx%d -> %dx%d shrinks an axis by more than %d", who, H, W, oH, oW, WCT_SCALE_MAX_SHRINK);
  return WCT_OK;
}

// algorithmic products of R: every output sample of a pass takes its taps once
double resample_flops(int H, int W, int oH, int oW, int filter) {
  const double S = filter == WCT_FILTER_BICUBIC ? 2.0 : 1.0;
  const double tx = 2.0 * S * std::max((double)W / oW, 1.0), ty = 2.0 * S * std::max((double)H / oH, 1.0);
  return 2.0 * 3.0 * ((double)H * oW * tx + (double)oH * oW * ty);
}

int resample_impl(wct_ctx* ctx, const float* src, int H, int W, float* dst, int oH, int oW, int filter) {
  if (H == oH && W == oW) {   // equal sizes: a bit-for-bit copy
    ProfScope ps(ctx, ctx->main.stream, "resample<copy>", 0, 24.0 * H * W);
    HIPCHK(ctx, hipMemcpyAsync(dst, src, (size_t)3 * H * W * sizeof(float), hipMemcpyDeviceToDevice, ctx->main.stream));
    return WCT_OK;
  }
  if (int rc = ensure(ctx, ctx->scTab, scale_table_bytes(H, W, oH, oW, filter))) return rc;
  char name[48];
  snprintf(name, sizeof name, "resample<%s,%s>", filter == WCT_FILTER_BICUBIC ? "bicubic" : "bilinear", (double)oH * oW < (double)H * W ? "down" : "up");
  ProfScope ps(ctx, ctx->main.stream, name, resample_flops(H, W, oH, oW, filter), 12.0 * ((double)H * W + (double)oH * oW));
  HIPCHK(ctx, launch_scale(src, nullptr, nullptr, 0.f, H, W, dst, oH, oW, filter, ctx->scTab.p, ctx->scTab.cap, ctx->main.stream));
  return WCT_OK;
}

int merge_impl(wct_ctx* ctx, const float* a, const float* b, int hc, int wc, const float* c, int hf, int wf, float gain, float* out) {
  if (gain == 0.f) return resample_impl(ctx, a, hc, wc, out, hf, wf, WCT_FILTER_BICUBIC);   // exactly R(a): b and c are not read
  if (int rc = ensure(ctx, ctx->scTab, scale_table_bytes(hc, wc, hf, wf, WCT_FILTER_BICUBIC))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "pyramid_merge", resample_flops(hc, wc, hf, wf, WCT_FILTER_BICUBIC) + 12.0 * ((double)hc * wc + (double)hf * wf),
               12.0 * (2.0 * hc * wc + 2.0 * hf * wf));
  HIPCHK(ctx, launch_scale(a, b, c, gain, hc, wc, out, hf, wf, WCT_FILTER_BICUBIC, ctx->scTab.p, ctx->scTab.cap, ctx->main.stream));
  return WCT_OK;
}
}  // namespace

extern "C" {

int wct_scale_shape(int H, int W, int divisor, int* h, int* w) {
  if (!h || !w || H < 1 || W < 1 || divisor < 1 || divisor > WCT_SCALE_MAX_DIVISOR) return WCT_ERR_INVALID;
  const int hd = 16 * (H / (16 * divisor)), wd = 16 * (W / (16 * divisor));
  if (hd < 32 || wd < 32) return WCT_ERR_INVALID;
  *h = hd; *w = wd;
  return WCT_OK;
}

int wct_resample_planar(wct_ctx* ctx, const float* src, int H, int W, float* dst, int oH, int oW, int filter) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!src || !dst) return fail(ctx, WCT_ERR_INVALID, "wct_resample_planar: NULL image");
  if (int rc = scale_shapes_check(ctx, "wct_resample_planar", H, W, oH, oW)) return rc;
  if (filter != WCT_FILTER_BILINEAR && filter != WCT_FILTER_BICUBIC)
    return fail(ctx, WCT_ERR_INVALID, "wct_resample_planar: filter %d is neither WCT_FILTER_BILINEAR (0) nor WCT_FILTER_BICUBIC (1)", filter);
  if (ranges_overlap(dst, (size_t)3 * oH * oW * sizeof(float), src, (size_t)3 * H * W * sizeof(float)))
    return fail(ctx, WCT_ERR_INVALID, "wct_resample_planar: dst overlaps src, which is read while it is written");
  return resample_impl(ctx, src, H, W, dst, oH, oW, filter);
}

int wct_pyramid_merge(wct_ctx* ctx, const float* a, const float* b, int hc, int wc, const float* c, int hf, int wf, float gain, float* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!a || !out) return fail(ctx, WCT_ERR_INVALID, "wct_pyramid_merge: NULL a or out");
  if (!std::isfinite(gain) || gain < 0.f) return fail(ctx, WCT_ERR_INVALID, "wct_pyramid_merge: gain must be finite and >= 0, got %g", (double)gain);
  if (gain > 0.f && (!b || !c)) return fail(ctx, WCT_ERR_INVALID, "wct_pyramid_merge: b and c may be NULL only when gain == 0 (got %g)", (double)gain);
  if (int rc = scale_shapes_check(ctx, "wct_pyramid_merge", hc, wc, hf, wf)) return rc;
  const size_t cb = (size_t)3 * hc * wc * sizeof(float), fb = (size_t)3 * hf * wf * sizeof(float);
  if (ranges_overlap(out, fb, a, cb) || (gain > 0.f && (ranges_overlap(out, fb, b, cb) || ranges_overlap(out, fb, c, fb))))
    return fail(ctx, WCT_ERR_INVALID, "wct_pyramid_merge: out overlaps a, b or c, which are read while it is written");
  return merge_impl(ctx, a, b, hc, wc, c, hf, wf, gain, out);
}

int wct_stylize_scaled(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run,
                       const int* level_div, float detail_gain, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || !out || !level_div || num_run < 1)
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_scaled: bad arguments (a NULL content, out or level_div, or num_run < 1)");
  if (!std::isfinite(detail_gain) || detail_gain < 0.f)
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_scaled: detail_gain must be finite and >= 0, got %g", (double)detail_gain);
  if (H < 1 || W < 1 || (style && (Hs < 1 || Ws < 1)))
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_scaled: bad shapes (content %dx%d, style %dx%d)", H, W, Hs, Ws);
  int hd[5], wd[5];   // working size of levels 5, 4, 3, 2, 1
  for (int i = 0; i < 5; ++i) {
    const int d = level_div[i];
    if (d < 1 || d > WCT_SCALE_MAX_DIVISOR)
      return fail(ctx, WCT_ERR_INVALID, "wct_stylize_scaled: divisor %d of level %d is outside 1 .. %d", d, 5 - i, WCT_SCALE_MAX_DIVISOR);
    if (i > 0 && d > level_div[i - 1])
      return fail(ctx, WCT_ERR_INVALID, "wct_stylize_scaled: divisors must not increase towards level 1 (level %d has %d, level %d has %d)", 6 - i,
                  level_div[i - 1], 5 - i, d);
    if (wct_scale_shape(H, W, d, &hd[i], &wd[i]))
      return fail(ctx, WCT_ERR_INVALID, "wct_stylize_scaled: content %dx%d at divisor %d is under the 32x32 the five-level cascade needs", H, W, d);
  }
  if (level_div[4] != 1) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_scaled: the divisor of level 1 must be 1, got %d", level_div[4]);
  if (ranges_overlap(out, (size_t)3 * hd[4] * wd[4] * sizeof(float), content, (size_t)3 * H * W * sizeof(float)))
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_scaled: out overlaps the content, which the merges still read");
  if (!style)
    for (int level = 5; level >= 1; --level)
      if (!ctx->eigS[level].p)
        return fail(ctx, WCT_ERR_STATE, "wct_stylize_scaled: no style statistics for level %d (wct_style_prepare / wct_style_import)", level);
  if (level_div[0] == 1)   // every divisor is 1: the plain cascade, bit for bit
    return style ? stylize_impl(ctx, content, H, W, style, Hs, Ws, alpha, num_run, out, Ho, Wo)
                 : stylize_prepared_impl(ctx, "wct_stylize_scaled", content, H, W, alpha, num_run, out, Ho, Wo);

  // every buffer first: a growing one synchronises, and nothing enqueued below may find its source moved
  const float* F[5];   // F_d of every level's divisor; equal divisors share one
  for (int i = 0, slot = 0; i < 5; ++i) {
    if (i > 0 && level_div[i] == level_div[i - 1]) { F[i] = F[i - 1]; continue; }
    if (level_div[i] == 1 && hd[i] == H && wd[i] == W) { F[i] = content; continue; }
    if (int rc = ensure(ctx, ctx->scF[slot], (size_t)3 * hd[i] * wd[i] * sizeof(float))) return rc;
    F[i] = reinterpret_cast<const float*>(ctx->scF[slot++].p);
  }
  if (int rc = ensure(ctx, ctx->scStage, (size_t)3 * hd[4] * wd[4] * sizeof(float))) return rc;
  {
    size_t tab = scale_table_bytes(hd[4], wd[4], hd[0], wd[0], WCT_FILTER_BICUBIC);   // the reduction in front of a later run
    for (int i = 0; i < 5; ++i) {
      tab = std::max(tab, scale_table_bytes(H, W, hd[i], wd[i], WCT_FILTER_BICUBIC));                                // F_d
      if (i > 0) tab = std::max(tab, scale_table_bytes(hd[i - 1], wd[i - 1], hd[i], wd[i], WCT_FILTER_BICUBIC));     // the merges
    }
    if (int rc = ensure(ctx, ctx->scTab, tab)) return rc;
  }
  for (int i = 0; i < 5; ++i)
    if (F[i] != content && (i == 0 || F[i] != F[i - 1]))
      if (int rc = resample_impl(ctx, content, H, W, const_cast<float*>(F[i]), hd[i], wd[i], WCT_FILTER_BICUBIC)) return rc;

  int transitions = 0;
  for (int i = 1; i < 5; ++i) transitions += level_div[i] != level_div[i - 1];
  const int n_ops = num_run * (5 + transitions) + (num_run - 1);   // levels and merges of every run, and the reduction in front of every later run
  float* bufs[2] = {out, reinterpret_cast<float*>(ctx->scStage.p)};
  const bool interleaved = style && ctx->interleave && ctx->overlap;
  if (int rc = with_deferred_solves(ctx, false, [&]() -> int {
        if (style) {   // the style side as in wct_stylize: on the side lane, level L - 1 behind the content side of level L of the first run
          if (int rc = fork_side(ctx)) return rc;
          for (int level = 5; level >= (interleaved ? 5 : 1); --level)
            if (int rc = style_side(ctx, level, style, Hs, Ws)) return rc;
        }
        int op = 0;   // operation `op` of n_ops writes bufs[(n_ops - 1 - op) & 1]: each reads what the one before wrote, the last writes `out`
        const float* cur = F[0];
        int h = hd[0], w = wd[0];
        for (int run = 0; run < num_run; ++run) {
          if (run > 0) {
            float* dst = bufs[(n_ops - 1 - op++) & 1];
            if (int rc = resample_impl(ctx, cur, h, w, dst, hd[0], wd[0], WCT_FILTER_BICUBIC)) return rc;
            cur = dst; h = hd[0]; w = wd[0];
          }
          for (int i = 0; i < 5; ++i) {
            const int level = 5 - i;
            if (i > 0 && level_div[i] != level_div[i - 1]) {
              float* dst = bufs[(n_ops - 1 - op++) & 1];
              if (int rc = merge_impl(ctx, cur, F[i - 1], h, w, F[i], hd[i], wd[i], detail_gain, dst)) return rc;
              cur = dst; h = hd[i]; w = wd[i];
            }
            float* dst = bufs[(n_ops - 1 - op++) & 1];
            int ho = 0, wo = 0;
            if (int rc = content_side(ctx, level, cur, h, w, alpha, dst, &ho, &wo)) return rc;
            cur = dst; h = ho; w = wo;
            if (interleaved && run == 0 && level > 1)
              if (int rc = style_side(ctx, level - 1, style, Hs, Ws)) return rc;
          }
        }
        return WCT_OK;
      })) return rc;
  if (Ho) *Ho = hd[4];
  if (Wo) *Wo = wd[4];
  return range_readback(ctx);
}

}  // extern "C"
