// Motion compensation of the C ABI (include/wct_hip_motion.h): the standalone pyramid / estimate / blend entries on the context's workspace,
// the clip's motion block, and the two steps wct_stylize_clip adds to a frame.  Host orchestration only; the kernels are in motion.hip
// (pyramid, search) and video.hip (the blend with a field).
#include "../../include/wct_hip_motion.h"
#include "wct_clip.h"

using namespace wct_host;

namespace {
size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int params_check(wct_ctx* ctx, const char* who, const wct_motion_params* p) {
  if (!p) return fail(ctx, WCT_ERR_INVALID, "%s: NULL params", who);
  if (p->levels < 1 || p->levels > WCT_MOTION_MAX_LEVELS) return fail(ctx, WCT_ERR_INVALID, "%s: levels 1 .. %d expected, got %d", who, WCT_MOTION_MAX_LEVELS, p->levels);
  if (p->range < 0 || p->range > WCT_MOTION_MAX_RANGE) return fail(ctx, WCT_ERR_INVALID, "%s: range 0 .. %d expected, got %d", who, WCT_MOTION_MAX_RANGE, p->range);
  if (p->penalty < 0 || p->penalty > 255) return fail(ctx, WCT_ERR_INVALID, "%s: penalty 0 .. 255 expected, got %d", who, p->penalty);
  return WCT_OK;
}

int shape_check(wct_ctx* ctx, const char* who, int Hc, int Wc, int Ho, int Wo, int levels, MotionLayout& l) {
  if (Ho < 1 || Wo < 1 || Ho > Hc || Wo > Wc)
    return fail(ctx, WCT_ERR_INVALID, "%s: the window %dx%d must be non-empty and no larger than the image %dx%d", who, Ho, Wo, Hc, Wc);
  if (levels < 1 || levels > WCT_MOTION_MAX_LEVELS) return fail(ctx, WCT_ERR_INVALID, "%s: levels 1 .. %d expected, got %d", who, WCT_MOTION_MAX_LEVELS, levels);
  if (!motion_layout(Ho, Wo, levels, l))
    return fail(ctx, WCT_ERR_INVALID, "%s: a %dx%d image has no pyramid of %d levels (%d pixels at least in each direction)", who, Ho, Wo, levels, 1 << (levels - 1));
  return WCT_OK;
}

// every level of the search, top first: level k's field into fields + lv[k].mv_off, level 0's into mv0
int search_all(wct_ctx* ctx, const MotionLayout& l, const wct_motion_params& p, const uint8_t* pyr_cur, const uint8_t* pyr_prev, int16_t* fields, int16_t* mv0,
               const int* cut_flag) {
  hipStream_t st = ctx->main.stream;
  const int16_t* parent = nullptr;
  for (int k = l.levels - 1; k >= 0; --k) {
    int16_t* out = k == 0 ? mv0 : fields + l.lv[k].mv_off;
    const double blocks = (double)l.lv[k].nby * l.lv[k].nbx;
    const double window = k == l.levels - 1 ? (8.0 + 2 * p.range) * (8.0 + 2 * p.range) : 164.0;   // finer: 10 x 10 and the co-located block
    char name[24];
    snprintf(name, sizeof name, "motion_search%d", k);
    ProfScope ps(ctx, st, name, 0, blocks * (64.0 + window + 4.0));
    HIPCHK(ctx, launch_motion_search(pyr_cur, pyr_prev, l, k, p.range, p.penalty, parent, out, cut_flag, st));
    parent = out;
  }
  return WCT_OK;
}
}  // namespace

namespace wct_host {
int motion_frame_estimate(wct_ctx* ctx, wct_clip* clip, const float* content, int H, int W) {
  wct_clip_motion* m = clip->motion;
  hipStream_t st = ctx->main.stream;
  {
    ProfScope ps(ctx, st, "motion_pyramid", 8.0 * clip->Ho * clip->Wo, (12.0 + 4.0 / 3.0) * clip->Ho * clip->Wo);
    HIPCHK(ctx, launch_motion_pyramid(content, H, W, m->lay, m->pyr_cur, st));
  }
  return search_all(ctx, m->lay, m->p, m->pyr_cur, m->pyr_prev, m->mv, m->mv + m->lay.lv[0].mv_off, clip->flags + 1);
}

int motion_frame_store(wct_ctx* ctx, wct_clip* clip) {
  wct_clip_motion* m = clip->motion;
  ProfScope ps(ctx, ctx->main.stream, "motion_store", 0, 2.0 * m->lay.pyr_bytes);
  HIPCHK(ctx, hipMemcpyAsync(m->pyr_prev, m->pyr_cur, m->lay.pyr_bytes, hipMemcpyDeviceToDevice, ctx->main.stream));
  return WCT_OK;
}

void motion_release(wct_clip* clip) {
  if (!clip->motion) return;
  if (clip->motion->base) (void)hipFree(clip->motion->base);
  delete clip->motion;
  clip->motion = nullptr;
}
}  // namespace wct_host

extern "C" {

int wct_motion_shape(int Ho, int Wo, int* nby, int* nbx) {
  if (!nby || !nbx || Ho < 1 || Wo < 1) return WCT_ERR_INVALID;
  *nby = (Ho + WCT_MOTION_BLOCK - 1) / WCT_MOTION_BLOCK;
  *nbx = (Wo + WCT_MOTION_BLOCK - 1) / WCT_MOTION_BLOCK;
  return WCT_OK;
}

int wct_motion_luma(wct_ctx* ctx, const float* planar, int Hc, int Wc, int Ho, int Wo, int levels, uint8_t* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!planar || !out) return fail(ctx, WCT_ERR_INVALID, "wct_motion_luma: NULL %s", planar ? "out" : "planar");
  MotionLayout l;
  if (int rc = shape_check(ctx, "wct_motion_luma", Hc, Wc, Ho, Wo, levels, l)) return rc;
  size_t dense = 0;
  for (int k = 0; k < levels; ++k) dense += (size_t)l.lv[k].H * l.lv[k].W;
  if (ranges_overlap(out, dense, planar, (size_t)3 * Hc * Wc * sizeof(float))) return fail(ctx, WCT_ERR_INVALID, "wct_motion_luma: out overlaps planar");
  if (int rc = ensure(ctx, ctx->motionWs, l.pyr_bytes)) return rc;
  uint8_t* pyr = reinterpret_cast<uint8_t*>(ctx->motionWs.p);
  hipStream_t st = ctx->main.stream;
  ProfScope ps(ctx, st, "motion_pyramid", 8.0 * Ho * Wo, (12.0 + 4.0) * Ho * Wo);
  HIPCHK(ctx, launch_motion_pyramid(planar, Hc, Wc, l, pyr, st));
  HIPCHK(ctx, launch_motion_unpad(pyr, l, out, st));
  return WCT_OK;
}

int wct_motion_estimate(wct_ctx* ctx, const float* cur, int Hc, int Wc, const float* prev, int Ho, int Wo, const wct_motion_params* params, int16_t* mv) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!cur || !prev || !mv) return fail(ctx, WCT_ERR_INVALID, "wct_motion_estimate: NULL %s", !cur ? "cur" : !prev ? "prev" : "mv");
  if (int rc = params_check(ctx, "wct_motion_estimate", params)) return rc;
  MotionLayout l;
  if (int rc = shape_check(ctx, "wct_motion_estimate", Hc, Wc, Ho, Wo, params->levels, l)) return rc;
  const size_t field = (size_t)l.lv[0].nby * l.lv[0].nbx * 2 * sizeof(int16_t);
  if (ranges_overlap(mv, field, cur, (size_t)3 * Hc * Wc * sizeof(float)) || ranges_overlap(mv, field, prev, (size_t)3 * Ho * Wo * sizeof(float)))
    return fail(ctx, WCT_ERR_INVALID, "wct_motion_estimate: mv overlaps an image");
  if (int rc = ensure(ctx, ctx->motionWs, 2 * l.pyr_bytes + up256(l.mv_count * sizeof(int16_t)))) return rc;
  uint8_t* pyr_cur = reinterpret_cast<uint8_t*>(ctx->motionWs.p);
  uint8_t* pyr_prev = pyr_cur + l.pyr_bytes;
  int16_t* fields = reinterpret_cast<int16_t*>(pyr_prev + l.pyr_bytes);
  hipStream_t st = ctx->main.stream;
  {
    ProfScope ps(ctx, st, "motion_pyramid", 16.0 * Ho * Wo, 2 * (12.0 + 4.0 / 3.0) * Ho * Wo);
    HIPCHK(ctx, launch_motion_pyramid(cur, Hc, Wc, l, pyr_cur, st));
    HIPCHK(ctx, launch_motion_pyramid(prev, Ho, Wo, l, pyr_prev, st));
  }
  return search_all(ctx, l, *params, pyr_cur, pyr_prev, fields, mv, nullptr);
}

int wct_motion_blend(wct_ctx* ctx, const float* cur_content, int Hc, int Wc, const float* prev_content, const float* stylised, const float* prev_out, int Ho,
                     int Wo, float blend, float sigma, int radius, const int* cut_flag_dev, float* out_planar, uint8_t* out_hwc, int round_mode,
                     const int16_t* mv) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  return blend_entry(ctx, "wct_motion_blend", cur_content, Hc, Wc, prev_content, stylised, prev_out, Ho, Wo, blend, sigma, radius, cut_flag_dev, out_planar,
                     out_hwc, round_mode, mv);
}

int wct_motion_attach(wct_ctx* ctx, wct_clip* clip, const wct_motion_params* params) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = clip_check(ctx, "wct_motion_attach", clip)) return rc;
  MotionLayout l;
  if (params) {
    if (int rc = params_check(ctx, "wct_motion_attach", params)) return rc;
    if (int rc = shape_check(ctx, "wct_motion_attach", clip->Ho, clip->Wo, clip->Ho, clip->Wo, params->levels, l)) return rc;
  }
  // frames in flight may read the block that goes, and the flag is written behind them
  HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  motion_release(clip);
  HIPCHK(ctx, hipMemsetAsync(clip->flags, 0, sizeof(int), ctx->main.stream));     // the next frame is a first frame, with or without motion
  if (!params) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    return WCT_OK;
  }
  wct_clip_motion* m = new (std::nothrow) wct_clip_motion();
  if (!m) return fail(ctx, WCT_ERR_NOMEM, "wct_motion_attach: out of host memory");
  m->p = *params;
  m->lay = l;
  const size_t total = 2 * l.pyr_bytes + up256(l.mv_count * sizeof(int16_t));
  hipError_t e = hipMalloc(&m->base, total);
  if (e == hipSuccess) e = hipMemsetAsync(m->base, 0, total, ctx->main.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->main.stream);
  if (e != hipSuccess) {
    if (m->base) (void)hipFree(m->base);
    delete m;
    return fail(ctx, e == hipErrorOutOfMemory ? WCT_ERR_NOMEM : WCT_ERR_HIP, "wct_motion_attach: %zu bytes: %s", total, hipGetErrorString(e));
  }
  m->pyr_cur = reinterpret_cast<uint8_t*>(m->base);
  m->pyr_prev = m->pyr_cur + l.pyr_bytes;
  m->mv = reinterpret_cast<int16_t*>(m->pyr_prev + l.pyr_bytes);
  clip->motion = m;
  return WCT_OK;
}

int wct_motion_export(wct_ctx* ctx, wct_clip* clip, int16_t* mv_dev) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = clip_check(ctx, "wct_motion_export", clip)) return rc;
  if (!mv_dev) return fail(ctx, WCT_ERR_INVALID, "wct_motion_export: NULL mv_dev");
  const wct_clip_motion* m = clip->motion;
  if (!m) return fail(ctx, WCT_ERR_STATE, "wct_motion_export: no motion attached to the clip (wct_motion_attach)");
  const size_t field = (size_t)m->lay.lv[0].nby * m->lay.lv[0].nbx * 2 * sizeof(int16_t);
  HIPCHK(ctx, hipMemcpyAsync(mv_dev, m->mv + m->lay.lv[0].mv_off, field, hipMemcpyDeviceToDevice, ctx->main.stream));
  return WCT_OK;
}

}  // extern "C"
