// Seeded style variations (include/wct_hip_diverse.h; kernels in rotate.hip) behind the C ABI.
#include "../../include/wct_hip_diverse.h"
#include "wct_ctx.h"

using namespace wct_host;

namespace {
int strength_check(wct_ctx* ctx, const char* who, double strength) {
  if (!(strength >= 0.0 && strength <= (double)WCT_DIVERSE_MAX_STRENGTH))
    return fail(ctx, WCT_ERR_INVALID, "%s: strength=%g outside [0, %d]", who, strength, WCT_DIVERSE_MAX_STRENGTH);
  return WCT_OK;
}

// what of wct_style_diversify's arguments can be judged without looking at the slots
int diversify_args_check(wct_ctx* ctx, const char* who, unsigned level_mask, double strength) {
  if (ctx->transform != WCT_TRANSFORM_WCT) return fail(ctx, WCT_ERR_INVALID, "%s: defined for the wct transform only (wct_set_transform)", who);
  if (!level_mask || (level_mask & ~0x3eu)) return fail(ctx, WCT_ERR_INVALID, "%s: level mask 0x%x is empty or has a bit outside levels 1..5", who, level_mask);
  return strength_check(ctx, who, strength);
}

// Z(C, seed, stream_id, tag, strength) into Z (and A into skew, may be null) on the caller's stream
int rotation_impl(wct_ctx* ctx, int C, uint64_t seed, uint32_t stream_id, unsigned tag, double strength, double* Z, double* skew) {
  if (strength > 0.0)
    if (int rc = ensure(ctx, ctx->dvWs, rotation_workspace_bytes(C))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "rotation_make", 0, 0);
  HIPCHK(ctx, launch_rotation_make(C, seed, stream_id, tag, strength, Z, skew, ctx->dvWs.p, ctx->dvWs.cap, ctx->main.stream));
  return WCT_OK;
}
}  // namespace

extern "C" {

int wct_rotation_make(wct_ctx* ctx, int C, uint64_t seed, uint32_t stream_id, unsigned tag, double strength, double* Z, double* skew) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!Z) return fail(ctx, WCT_ERR_INVALID, "rotation_make: NULL Z");
  if (C < 2 || (C & 1) || C > 512) return fail(ctx, WCT_ERR_INVALID, "rotation_make: C=%d must be even and in [2, 512]", C);
  if (tag > 255u) return fail(ctx, WCT_ERR_INVALID, "rotation_make: tag=%u outside 0..255", tag);
  if (int rc = strength_check(ctx, "rotation_make", strength)) return rc;
  const size_t nb = (size_t)C * C * sizeof(double);
  if (skew && ranges_overlap(Z, nb, skew, nb)) return fail(ctx, WCT_ERR_INVALID, "rotation_make: Z overlaps skew");
  return rotation_impl(ctx, C, seed, stream_id, tag, strength, Z, skew);
}

int wct_style_diversify(wct_ctx* ctx, unsigned level_mask, double strength, uint64_t seed, uint32_t stream_id) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = diversify_args_check(ctx, "style_diversify", level_mask, strength)) return rc;
  for (int level = 5; level >= 1; --level)
    if ((level_mask >> level & 1u) && (!ctx->mod[WCT_KIND_ENC][level].loaded || !ctx->eigS[level].p))
      return fail(ctx, WCT_ERR_STATE, "style_diversify: no style statistics for level %d (wct_style_prepare / wct_style_import)", level);
  if (strength == 0.0) return WCT_OK;     // Z = I: the slots stay as they are, bit for bit
  hipStream_t st = ctx->main.stream;
  int cmax = 0;
  for (int level = 5; level >= 1; --level) {
    if (!(level_mask >> level & 1u)) continue;
    const int C = ctx->mod[WCT_KIND_ENC][level].layers.back().d.cout;
    if (C < 2 || (C & 1) || C > 512) return fail(ctx, WCT_ERR_INVALID, "style_diversify: level %d has C=%d, which must be even and in [2, 512]", level, C);
    if (ctx->eigS[level].cap < eig_result_bytes(C))     // an encoder of another width was loaded behind the slot's back
      return fail(ctx, WCT_ERR_STATE, "style_diversify: the style statistics of level %d were prepared for a narrower encoder; prepare them again", level);
    cmax = std::max(cmax, C);
  }
  // both buffers at the widest masked level's size before the first slot is touched
  if (int rc = ensure(ctx, ctx->dvWs, rotation_workspace_bytes(cmax))) return rc;
  if (int rc = ensure(ctx, ctx->dvZ, 2 * (size_t)cmax * cmax * sizeof(double))) return rc;
  for (int level = 5; level >= 1; --level) {
    if (!(level_mask >> level & 1u)) continue;
    const int C = ctx->mod[WCT_KIND_ENC][level].layers.back().d.cout;
    const size_t cc = (size_t)C * C;
    double* Z = reinterpret_cast<double*>(ctx->dvZ.p);
    double* F0 = Z + cc;
    double* F = reinterpret_cast<double*>(ctx->eigS[level].p) + eig_result_F_offset((size_t)C);
    if (int rc = rotation_impl(ctx, C, seed, stream_id, (unsigned)level, strength, Z, nullptr)) return rc;
    HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_style[level], 0));
    HIPCHK(ctx, hipMemcpyAsync(F0, F, cc * sizeof(double), hipMemcpyDeviceToDevice, st));
    {
      ProfScope ps(ctx, st, "rotation_apply", 2.0 * C * cc, 24.0 * cc);
      HIPCHK(ctx, launch_rotation_apply(C, F0, Z, F, st));
    }
    if (int rc = style_fold(ctx, level, st)) return rc;
    ctx->rotated[level] = true;
    HIPCHK(ctx, hipEventRecord(ctx->ev_style[level], st));   // what content_side / wct_content_solve wait for
  }
  return WCT_OK;
}

int wct_stylize_diverse(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, unsigned level_mask, double strength,
                        uint64_t seed, uint32_t stream_id, float alpha, int num_run, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  {
    WCT_GUARD(ctx);
    if (!content || !style || !out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "stylize_diverse: bad arguments (a NULL pointer, or num_run < 1)");
    if (int rc = diversify_args_check(ctx, "stylize_diverse", level_mask, strength)) return rc;
  }
  if (int rc = wct_style_prepare(ctx, style, Hs, Ws)) return rc;
  if (int rc = wct_style_diversify(ctx, level_mask, strength, seed, stream_id)) return rc;
  return wct_stylize_prepared(ctx, content, H, W, alpha, num_run, out, Ho, Wo);
}

}  // extern "C"
