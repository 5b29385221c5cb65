// Proxy mode's entry points of the C ABI (include/wct_hip_bgrid.h): the bilateral grid's fit and slice, and wct_stylize_proxy, which is the
// composition of PUBLIC calls it documents.  Host orchestration only; the kernels are in bgrid.hip.
#include "../../include/wct_hip_bgrid.h"
#include "wct_ctx.h"

using namespace wct_host;

namespace {
// the refusals the entries share; `who` names the entry
int grid_check(wct_ctx* ctx, const char* who, int gz, int gh, int gw) {
  if (gz < 1 || gz > WCT_BGRID_MAX_Z || gh < 1 || gh > WCT_BGRID_MAX_XY || gw < 1 || gw > WCT_BGRID_MAX_XY)
    return fail(ctx, WCT_ERR_INVALID, "%s: grid %d x %d x %d (z, y, x) is outside 1 .. %d x 1 .. %d x 1 .. %d", who, gz, gh, gw, WCT_BGRID_MAX_Z,
                WCT_BGRID_MAX_XY, WCT_BGRID_MAX_XY);
  return WCT_OK;
}

int fit_check(wct_ctx* ctx, const char* who, double eps, int smooth) {
  if (!std::isfinite(eps) || !(eps > 0.0)) return fail(ctx, WCT_ERR_INVALID, "%s: eps must be finite and positive, got %g", who, eps);
  if (smooth < 0 || smooth > WCT_BGRID_MAX_SMOOTH)
    return fail(ctx, WCT_ERR_INVALID, "%s: smooth 0 .. %d expected, got %d", who, WCT_BGRID_MAX_SMOOTH, smooth);
  return WCT_OK;
}

// exactly one output, a round_mode of wct_planar_to_u8, and no overlap with the content other than out_planar == content
int out_check(wct_ctx* ctx, const char* who, const float* content, int H, int W, const float* out_planar, const uint8_t* out_hwc, int round_mode) {
  if ((out_planar != nullptr) == (out_hwc != nullptr))
    return fail(ctx, WCT_ERR_INVALID, "%s: exactly one of out_planar and out_hwc expected, got %s", who, out_planar ? "both" : "neither");
  if (round_mode != 0 && round_mode != 1) return fail(ctx, WCT_ERR_INVALID, "%s: round_mode 0 or 1 expected, got %d", who, round_mode);
  const size_t cb = (size_t)3 * H * W * sizeof(float);
  if (out_planar ? out_planar != content && ranges_overlap(out_planar, cb, content, cb) : ranges_overlap(out_hwc, (size_t)3 * H * W, content, cb))
    return fail(ctx, WCT_ERR_INVALID, "%s: the output overlaps the content, which is still read (only out_planar == content is allowed)", who);
  return WCT_OK;
}

size_t grid_bytes(int gz, int gh, int gw) { return (size_t)gz * gh * gw * 12 * sizeof(float); }
}  // namespace

extern "C" {

int wct_bgrid_shape(int h, int w, int cell, int* gh, int* gw) {
  if (!gh || !gw || h < 1 || w < 1 || cell < 1) return WCT_ERR_INVALID;
  const long a = ((long)h + cell - 1) / cell + 1, b = ((long)w + cell - 1) / cell + 1;
  if (a > WCT_BGRID_MAX_XY || b > WCT_BGRID_MAX_XY) return WCT_ERR_INVALID;
  *gh = (int)a; *gw = (int)b;
  return WCT_OK;
}

int wct_bgrid_fit(wct_ctx* ctx, const float* cl, const float* sl, int h, int w, int gz, int gh, int gw, double eps, int smooth, float* grid) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!cl || !sl || !grid) return fail(ctx, WCT_ERR_INVALID, "wct_bgrid_fit: NULL image or grid");
  if (h < 1 || w < 1) return fail(ctx, WCT_ERR_INVALID, "wct_bgrid_fit: empty shape %dx%d", h, w);
  if (int rc = grid_check(ctx, "wct_bgrid_fit", gz, gh, gw)) return rc;
  if (int rc = fit_check(ctx, "wct_bgrid_fit", eps, smooth)) return rc;
  if (bgrid_fit_chunks(h, gh) > 65535) return fail(ctx, WCT_ERR_INVALID, "wct_bgrid_fit: %d rows are more than a launch of row chunks covers", h);
  const size_t ib = (size_t)3 * h * w * sizeof(float);
  if (ranges_overlap(grid, grid_bytes(gz, gh, gw), cl, ib) || ranges_overlap(grid, grid_bytes(gz, gh, gw), sl, ib))
    return fail(ctx, WCT_ERR_INVALID, "wct_bgrid_fit: the grid overlaps an image, which is read while it is written");
  if (int rc = ensure(ctx, ctx->bgWs, bgrid_fit_workspace_bytes(h, gz, gh, gw))) return rc;
  const double nv = (double)gz * gh * gw;
  ProfScope ps(ctx, ctx->main.stream, "bgrid_fit", 2.0 * 44.0 * 8.0 * h * w, 24.0 * h * w + nv * (22.0 * 8.0 * (2 + 6 * smooth) + 48.0));
  HIPCHK(ctx, launch_bgrid_fit(cl, sl, h, w, gz, gh, gw, eps, smooth, grid, reinterpret_cast<double*>(ctx->bgWs.p), ctx->bgWs.cap, ctx->main.stream));
  return WCT_OK;
}

int wct_bgrid_slice(wct_ctx* ctx, const float* grid, int gz, int gh, int gw, const float* content, int H, int W, float* out_planar, uint8_t* out_hwc,
                    int round_mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!grid || !content) return fail(ctx, WCT_ERR_INVALID, "wct_bgrid_slice: NULL grid or content");
  if (H < 1 || W < 1) return fail(ctx, WCT_ERR_INVALID, "wct_bgrid_slice: empty shape %dx%d", H, W);
  if (int rc = grid_check(ctx, "wct_bgrid_slice", gz, gh, gw)) return rc;
  if (int rc = out_check(ctx, "wct_bgrid_slice", content, H, W, out_planar, out_hwc, round_mode)) return rc;
  const size_t ob = (size_t)3 * H * W * (out_planar ? sizeof(float) : 1);
  if (ranges_overlap(out_planar ? static_cast<const void*>(out_planar) : static_cast<const void*>(out_hwc), ob, grid, grid_bytes(gz, gh, gw)))
    return fail(ctx, WCT_ERR_INVALID, "wct_bgrid_slice: the output overlaps the grid, which is read while it is written");
  ProfScope ps(ctx, ctx->main.stream, out_planar ? "bgrid_slice" : "bgrid_slice<u8>", 2.0 * 120.0 * H * W, (out_planar ? 24.0 : 15.0) * H * W);
  HIPCHK(ctx, launch_bgrid_slice(grid, gz, gh, gw, content, H, W, out_planar, out_hwc, round_mode, ctx->bgrid_lds != 0, ctx->main.stream));
  return WCT_OK;
}

int wct_stylize_proxy(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run, int divisor,
                      int cell, int gz, double eps, int smooth, float* out_planar, uint8_t* out_hwc, int round_mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_proxy: bad arguments (a NULL content, or num_run < 1)");
  if (H < 1 || W < 1 || (style && (Hs < 1 || Ws < 1)))
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_proxy: bad shapes (content %dx%d, style %dx%d)", H, W, Hs, Ws);
  if (divisor < 1 || divisor > WCT_SCALE_MAX_DIVISOR)
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_proxy: divisor %d is outside 1 .. %d", divisor, WCT_SCALE_MAX_DIVISOR);
  int h = 0, w = 0, gh = 0, gw = 0;
  if (wct_scale_shape(H, W, divisor, &h, &w))
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_proxy: content %dx%d at divisor %d is under the 32x32 the five-level cascade needs", H, W, divisor);
  if (cell < 1 || wct_bgrid_shape(h, w, cell, &gh, &gw))
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_proxy: cell %d on the %dx%d working size gives a grid outside 1 .. %d vertices per axis", cell, h, w,
                WCT_BGRID_MAX_XY);
  if (int rc = grid_check(ctx, "wct_stylize_proxy", gz, gh, gw)) return rc;
  if (int rc = fit_check(ctx, "wct_stylize_proxy", eps, smooth)) return rc;
  if (int rc = out_check(ctx, "wct_stylize_proxy", content, H, W, out_planar, out_hwc, round_mode)) return rc;
  if (!style)
    for (int level = 5; level >= 1; --level)
      if (!ctx->eigS[level].p)
        return fail(ctx, WCT_ERR_STATE, "wct_stylize_proxy: no style statistics for level %d (wct_style_prepare / wct_style_import)", level);
  // every buffer of this call first: a growing one synchronises, and nothing enqueued below may find its source moved
  const size_t lb = (size_t)3 * h * w * sizeof(float);
  if (int rc = ensure(ctx, ctx->pxCl, lb)) return rc;
  if (int rc = ensure(ctx, ctx->pxSl, lb)) return rc;
  if (int rc = ensure(ctx, ctx->bgGrid, grid_bytes(gz, gh, gw))) return rc;
  if (int rc = ensure(ctx, ctx->bgWs, bgrid_fit_workspace_bytes(h, gz, gh, gw))) return rc;
  float *cl = reinterpret_cast<float*>(ctx->pxCl.p), *sl = reinterpret_cast<float*>(ctx->pxSl.p), *grid = reinterpret_cast<float*>(ctx->bgGrid.p);
  // the composition, through the public entries themselves (a failure below carries the message of the entry that refused)
  if (int rc = wct_resample_planar(ctx, content, H, W, cl, h, w, WCT_FILTER_BICUBIC)) return rc;
  int ho = 0, wo = 0;
  if (int rc = style ? wct_stylize(ctx, cl, h, w, style, Hs, Ws, alpha, num_run, sl, &ho, &wo)
                     : wct_stylize_prepared(ctx, cl, h, w, alpha, num_run, sl, &ho, &wo)) return rc;
  if (ho != h || wo != w) return fail(ctx, WCT_ERR_STATE, "wct_stylize_proxy: the cascade returned %dx%d for a working size of %dx%d", ho, wo, h, w);
  if (int rc = wct_bgrid_fit(ctx, cl, sl, h, w, gz, gh, gw, eps, smooth, grid)) return rc;
  return wct_bgrid_slice(ctx, grid, gz, gh, gw, content, H, W, out_planar, out_hwc, round_mode);
}

}  // extern "C"
