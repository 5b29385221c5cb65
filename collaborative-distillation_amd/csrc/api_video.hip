// Video mode of the C ABI (include/wct_hip_video.h): the clip object, the tracking step, the temporal blend and the one-call frame entry.
// Host orchestration only; the kernels are in video.hip.
#include "../../include/wct_hip_video.h"
#include "wct_clip.h"

using namespace wct_host;

namespace {
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

struct ClipLayout { size_t sums, flags, image, total; };

// C: levels 5, 4, 3, 2, 1
bool clip_layout(int H, int W, const int* C, ClipLayout& l) {
  if (!C || H < 32 || W < 32) return false;
  size_t nd = 0;
  for (int i = 0; i < 5; ++i) {
    if (C[i] < 1 || C[i] > 512) return false;
    nd += (size_t)C[i] + (size_t)C[i] * C[i];
  }
  const size_t Ho = (size_t)(H / 16) * 16, Wo = (size_t)(W / 16) * 16;
  l.sums = up256(nd * sizeof(double));
  l.flags = 256;
  l.image = up256(3 * Ho * Wo * sizeof(float));
  l.total = 2 * l.sums + l.flags + 3 * l.image;
  return true;
}

int params_check(wct_ctx* ctx, const char* who, double rate, double cut, float blend, float sigma, int radius) {
  if (!(rate > 0.0 && rate <= 1.0)) return fail(ctx, WCT_ERR_INVALID, "%s: rate in (0, 1] expected, got %g", who, rate);
  if (!(cut >= 0.0)) return fail(ctx, WCT_ERR_INVALID, "%s: cut >= 0 (or +inf) expected, got %g", who, cut);
  if (!(blend >= 0.f && blend < 1.f)) return fail(ctx, WCT_ERR_INVALID, "%s: blend in [0, 1) expected, got %g", who, (double)blend);
  if (!std::isfinite(sigma) || !(sigma > 0.f)) return fail(ctx, WCT_ERR_INVALID, "%s: sigma must be finite and positive, got %g", who, (double)sigma);
  if (radius < 0 || radius > WCT_CLIP_MAX_RADIUS) return fail(ctx, WCT_ERR_INVALID, "%s: radius 0 .. %d expected, got %d", who, WCT_CLIP_MAX_RADIUS, radius);
  return WCT_OK;
}

// mv == NULL: video mode's blend; else the compensated one (include/wct_hip_motion.h), profiled under a name of its own
int blend_impl(wct_ctx* ctx, const float* cur, int Hc, int Wc, const float* prev, const float* sty, const float* pout, int Ho, int Wo, float blend,
               float sigma, int radius, const int* cut_flag, float* out_planar, uint8_t* out_hwc, int round_mode, const int16_t* mv = nullptr) {
  const double px = (double)Ho * Wo;
  ProfScope ps(ctx, ctx->main.stream, mv ? "motion_blend" : "temporal_blend", (9.0 + 4.0 * (2 * radius + 1) + 12.0) * px, (60.0 + (out_hwc ? 3.0 : 0.0)) * px);
  if (mv)
    HIPCHK(ctx, launch_motion_blend(cur, Hc, Wc, prev, sty, pout, Ho, Wo, blend, sigma, radius, cut_flag, out_planar, out_hwc, round_mode, mv,
                                    (Wo + WCT_MOTION_BLOCK - 1) / WCT_MOTION_BLOCK, ctx->main.stream));
  else
    HIPCHK(ctx, launch_temporal_blend(cur, Hc, Wc, prev, sty, pout, Ho, Wo, blend, sigma, radius, cut_flag, out_planar, out_hwc, round_mode, ctx->main.stream));
  return WCT_OK;
}

// ctx->track for the duration of one frame, whatever way the frame ends
struct TrackScope {
  wct_ctx* ctx;
  TrackScope(wct_ctx* c, wct_clip* clip) : ctx(c) { ctx->track = clip; }
  ~TrackScope() { ctx->track = nullptr; }
};
}  // namespace

namespace wct_host {
int clip_check(wct_ctx* ctx, const char* who, const wct_clip* clip) {
  if (!clip) return fail(ctx, WCT_ERR_INVALID, "%s: NULL clip", who);
  if (clip->owner != ctx) return fail(ctx, WCT_ERR_INVALID, "%s: the clip belongs to another context", who);
  return WCT_OK;
}

int blend_entry(wct_ctx* ctx, const char* who, const float* cur_content, int Hc, int Wc, const float* prev_content, const float* stylised,
                const float* prev_out, int Ho, int Wo, float blend, float sigma, int radius, const int* cut_flag_dev, float* out_planar, uint8_t* out_hwc,
                int round_mode, const int16_t* mv) {
  if (!cur_content || !prev_content || !stylised || !prev_out || !out_planar) return fail(ctx, WCT_ERR_INVALID, "%s: NULL image", who);
  if (Ho < 1 || Wo < 1 || Ho > Hc || Wo > Wc)
    return fail(ctx, WCT_ERR_INVALID, "%s: result %dx%d must be non-empty and no larger than the content %dx%d", who, Ho, Wo, Hc, Wc);
  if (int rc = params_check(ctx, who, 1.0, 0.0, blend, sigma, radius)) return rc;
  if (round_mode != 0 && round_mode != 1) return fail(ctx, WCT_ERR_INVALID, "%s: round_mode 0 or 1 expected, got %d", who, round_mode);
  const size_t img = (size_t)3 * Ho * Wo * sizeof(float), cimg = (size_t)3 * Hc * Wc * sizeof(float), u8 = (size_t)3 * Ho * Wo;
  const size_t field = mv ? (size_t)((Ho + WCT_MOTION_BLOCK - 1) / WCT_MOTION_BLOCK) * ((Wo + WCT_MOTION_BLOCK - 1) / WCT_MOTION_BLOCK) * 2 * sizeof(int16_t) : 0;
  const void* ins[5] = {cur_content, prev_content, stylised, prev_out, mv};
  const size_t in_bytes[5] = {cimg, img, img, img, field};
  for (int i = 0; i < (mv ? 5 : 4); ++i)
    if (ranges_overlap(out_planar, img, ins[i], in_bytes[i]) || (out_hwc && ranges_overlap(out_hwc, u8, ins[i], in_bytes[i])))
      return fail(ctx, WCT_ERR_INVALID, "%s: an output overlaps an input (the kernel reads a halo: nothing may alias)", who);
  if (out_hwc && ranges_overlap(out_hwc, u8, out_planar, img)) return fail(ctx, WCT_ERR_INVALID, "%s: out_hwc overlaps out_planar", who);
  return blend_impl(ctx, cur_content, Hc, Wc, prev_content, stylised, prev_out, Ho, Wo, blend, sigma, radius, cut_flag_dev, out_planar, out_hwc, round_mode, mv);
}

int clip_track_level(wct_ctx* ctx, wct_clip* clip, int level, int C, double* sum, double* sumsq) {
  if (C != clip->C[level]) return fail(ctx, WCT_ERR_STATE, "clip: level %d has %d channels, the clip was made for %d (a module was reloaded)", level, C, clip->C[level]);
  const double nel = (double)C + (double)C * C;
  ProfScope ps(ctx, ctx->main.stream, "clip_track", 3.0 * nel, 32.0 * nel);
  HIPCHK(ctx, launch_clip_track(C, clip->n[level], level == 5 ? 1 : 0, clip->p.rate, clip->p.cut, clip->run + clip->off[level], clip->pend + clip->off[level], sum,
                                sumsq, clip->flags, ctx->main.stream));
  return WCT_OK;
}
}  // namespace wct_host

extern "C" {

int wct_clip_bytes(int H, int W, const int* C, size_t* bytes) {
  ClipLayout l;
  if (!bytes || !clip_layout(H, W, C, l)) return WCT_ERR_INVALID;
  *bytes = l.total;
  return WCT_OK;
}

int wct_clip_create(wct_ctx* ctx, int H, int W, const wct_clip_params* params, wct_clip** out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!params || !out) return fail(ctx, WCT_ERR_INVALID, "wct_clip_create: NULL argument");
  *out = nullptr;
  if (H < 32 || W < 32) return fail(ctx, WCT_ERR_INVALID, "wct_clip_create: frames of %dx%d are too small for the five-level cascade (32x32 at least)", H, W);
  if (int rc = params_check(ctx, "wct_clip_create", params->rate, params->cut, params->blend, params->sigma, params->radius)) return rc;
  int C[5];
  for (int level = 5; level >= 1; --level) {
    const Module& me = ctx->mod[WCT_KIND_ENC][level];
    if (ctx->clip_channels) { C[5 - level] = ctx->clip_channels; continue; }   // test key: a clip for standalone tracking
    if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "wct_clip_create: encoder %d not loaded", level);
    C[5 - level] = me.layers.back().d.cout;
  }
  ClipLayout l;
  if (!clip_layout(H, W, C, l)) return fail(ctx, WCT_ERR_INVALID, "wct_clip_create: a level has more than 512 channels");
  wct_clip* c = new (std::nothrow) wct_clip();
  if (!c) return fail(ctx, WCT_ERR_NOMEM, "wct_clip_create: out of host memory");
  c->owner = ctx; c->H = H; c->W = W; c->Ho = H / 16 * 16; c->Wo = W / 16 * 16; c->p = *params;
  size_t nd = 0;
  for (int level = 5; level >= 1; --level) {
    const int Cl = C[5 - level];
    c->C[level] = Cl;
    c->n[level] = (double)(c->Ho >> (level - 1)) * (c->Wo >> (level - 1));
    c->off[level] = nd;
    nd += (size_t)Cl + (size_t)Cl * Cl;
  }
  c->nd = nd;
  hipError_t e = hipMalloc(&c->base, l.total);
  if (e == hipSuccess) e = hipMemset(c->base, 0, l.total);
  if (e != hipSuccess) {
    if (c->base) (void)hipFree(c->base);
    delete c;
    return fail(ctx, e == hipErrorOutOfMemory ? WCT_ERR_NOMEM : WCT_ERR_HIP, "wct_clip_create: %zu bytes: %s", l.total, hipGetErrorString(e));
  }
  char* b = reinterpret_cast<char*>(c->base);
  c->run = reinterpret_cast<double*>(b);
  c->pend = reinterpret_cast<double*>(b + l.sums);
  c->flags = reinterpret_cast<int*>(b + 2 * l.sums);
  c->prev_content = reinterpret_cast<float*>(b + 2 * l.sums + l.flags);
  c->prev_out = reinterpret_cast<float*>(b + 2 * l.sums + l.flags + l.image);
  c->stylised = reinterpret_cast<float*>(b + 2 * l.sums + l.flags + 2 * l.image);
  *out = c;
  return WCT_OK;
}

void wct_clip_destroy(wct_ctx* ctx, wct_clip* clip) {
  if (!clip) return;
  {
    WCT_GUARD(ctx);
    if (ctx) {
      (void)hipStreamSynchronize(ctx->main.stream);
      (void)hipStreamSynchronize(ctx->side.stream);
      if (ctx->track == clip) ctx->track = nullptr;
    }
    motion_release(clip);
    if (clip->base) (void)hipFree(clip->base);
  }
  delete clip;
}

int wct_clip_reset(wct_ctx* ctx, wct_clip* clip) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = clip_check(ctx, "wct_clip_reset", clip)) return rc;
  HIPCHK(ctx, hipMemsetAsync(clip->flags, 0, sizeof(int), ctx->main.stream));
  return WCT_OK;
}

int wct_clip_export(wct_ctx* ctx, wct_clip* clip, int level, double* sum, double* sumsq, int* flags) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = clip_check(ctx, "wct_clip_export", clip)) return rc;
  if (!valid_level(level)) return fail(ctx, WCT_ERR_INVALID, "wct_clip_export: level %d outside 1 .. 5", level);
  const size_t C = (size_t)clip->C[level];
  const double* r = clip->run + clip->off[level];
  hipStream_t st = ctx->main.stream;
  if (sum) HIPCHK(ctx, hipMemcpyAsync(sum, r, C * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (sumsq) HIPCHK(ctx, hipMemcpyAsync(sumsq, r + C, C * C * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (flags) HIPCHK(ctx, hipMemcpyAsync(flags, clip->flags, 2 * sizeof(int), hipMemcpyDeviceToDevice, st));
  return WCT_OK;
}

int wct_moments_track(wct_ctx* ctx, wct_clip* clip, int level, int decide, double* sum, double* sumsq) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = clip_check(ctx, "wct_moments_track", clip)) return rc;
  if (!valid_level(level) || !sum || !sumsq) return fail(ctx, WCT_ERR_INVALID, "wct_moments_track: bad arguments (level %d, or a NULL pointer)", level);
  const int C = clip->C[level];
  const size_t nel = (size_t)C + (size_t)C * C;
  double *run = clip->run + clip->off[level], *pend = clip->pend + clip->off[level];
  if (ranges_overlap(sum, C * sizeof(double), sumsq, (size_t)C * C * sizeof(double)) || ranges_overlap(sum, C * sizeof(double), clip->base, 2 * up256(clip->nd * sizeof(double))) ||
      ranges_overlap(sumsq, (size_t)C * C * sizeof(double), clip->base, 2 * up256(clip->nd * sizeof(double))))
    return fail(ctx, WCT_ERR_INVALID, "wct_moments_track: sum and sumsq must not overlap each other or the clip");
  hipStream_t st = ctx->main.stream;
  {
    ProfScope ps(ctx, st, "clip_track", 3.0 * nel, 32.0 * nel);
    HIPCHK(ctx, launch_clip_track(C, clip->n[level], decide ? 1 : 0, clip->p.rate, clip->p.cut, run, pend, sum, sumsq, clip->flags, st));
  }
  ProfScope ps(ctx, st, "clip_store", 0, 16.0 * nel);
  HIPCHK(ctx, launch_clip_store(nullptr, 0, 0, nullptr, 0, 0, nullptr, nullptr, pend, run, nel, clip->flags, st));
  return WCT_OK;
}

int wct_temporal_blend(wct_ctx* ctx, const float* cur_content, int Hc, int Wc, const float* prev_content, const float* stylised, const float* prev_out,
                       int Ho, int Wo, float blend, float sigma, int radius, const int* cut_flag_dev, float* out_planar, uint8_t* out_hwc, int round_mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  return blend_entry(ctx, "wct_temporal_blend", cur_content, Hc, Wc, prev_content, stylised, prev_out, Ho, Wo, blend, sigma, radius, cut_flag_dev, out_planar,
                     out_hwc, round_mode, nullptr);
}

int wct_stylize_clip(wct_ctx* ctx, wct_clip* clip, const float* content, int H, int W, float alpha, float* out_planar, uint8_t* out_hwc, int round_mode,
                     int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = clip_check(ctx, "wct_stylize_clip", clip)) return rc;
  if (!content || !out_planar) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_clip: NULL %s", content ? "out_planar" : "content");
  if (H != clip->H || W != clip->W) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_clip: frame %dx%d, the clip was created for %dx%d", H, W, clip->H, clip->W);
  if (round_mode != 0 && round_mode != 1) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_clip: round_mode 0 or 1 expected, got %d", round_mode);
  const int ho = clip->Ho, wo = clip->Wo;
  const size_t img = (size_t)3 * ho * wo * sizeof(float), cimg = (size_t)3 * H * W * sizeof(float), u8 = (size_t)3 * ho * wo;
  if (ranges_overlap(out_planar, img, content, cimg) || (out_hwc && ranges_overlap(out_hwc, u8, content, cimg)))
    return fail(ctx, WCT_ERR_INVALID, "wct_stylize_clip: an output overlaps the content (the blend and the next frame read it)");
  if (out_hwc && ranges_overlap(out_hwc, u8, out_planar, img)) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_clip: out_hwc overlaps out_planar");
  // with_deferred_solves may run a wide model's cascade twice, and the second pass would track the frame a second time
  if (ctx->wide_model) return fail(ctx, WCT_ERR_STATE, "wct_stylize_clip: wide models (an encoder wider than 128 channels, --mode original) are not supported");
  for (int level = 5; level >= 1; --level) {
    const Module& me = ctx->mod[WCT_KIND_ENC][level];
    if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "wct_stylize_clip: encoder %d not loaded", level);
    if (me.layers.back().d.cout != clip->C[level])
      return fail(ctx, WCT_ERR_STATE, "wct_stylize_clip: level %d has %d channels, the clip was created for %d", level, me.layers.back().d.cout, clip->C[level]);
    if (!ctx->eigS[level].p) return fail(ctx, WCT_ERR_STATE, "wct_stylize_clip: no style statistics for level %d (wct_style_prepare / wct_style_import)", level);
  }
  int h2 = 0, w2 = 0;
  {
    TrackScope ts(ctx, clip);
    if (int rc = stylize_prepared_impl(ctx, "wct_stylize_clip", content, H, W, alpha, 1, clip->stylised, &h2, &w2)) return rc;
  }
  if (h2 != ho || w2 != wo) return fail(ctx, WCT_ERR_STATE, "wct_stylize_clip: the cascade returned %dx%d, the clip holds %dx%d", h2, w2, ho, wo);
  const wct_clip_motion* mo = clip->motion;
  if (mo)
    if (int rc = motion_frame_estimate(ctx, clip, content, H, W)) return rc;
  if (int rc = blend_impl(ctx, content, H, W, clip->prev_content, clip->stylised, clip->prev_out, ho, wo, clip->p.blend, clip->p.sigma, clip->p.radius,
                          clip->flags + 1, out_planar, out_hwc, round_mode, mo ? mo->mv + mo->lay.lv[0].mv_off : nullptr)) return rc;
  if (mo)
    if (int rc = motion_frame_store(ctx, clip)) return rc;
  {
    ProfScope ps(ctx, ctx->main.stream, "clip_store", 0, 48.0 * ho * wo + 16.0 * clip->nd);
    HIPCHK(ctx, launch_clip_store(content, H, W, out_planar, ho, wo, clip->prev_content, clip->prev_out, clip->pend, clip->run, clip->nd, clip->flags,
                                  ctx->main.stream));
  }
  if (Ho) *Ho = ho;
  if (Wo) *Wo = wo;
  return WCT_OK;
}

}  // extern "C"
