// Patch swap (include/wct_hip_swap.h; kernels in swap.hip) and the entry points of include/wct_hip_transform.h behind the C ABI.
#include "../../include/wct_hip_swap.h"
#include "wct_ctx.h"

using namespace wct_host;

namespace {
// (M, b) of the transform `mode` from raw content moments against a style slot given as device doubles in the wct_style_export layout
// (cov_s^(1/2) [C*C] | mu_s [C]); style_stats == nullptr: the identity slot [I, 0].  The slot becomes an EigResult in eigS[0] (wct_solve's
// style buffer; no level uses it); mode-explicit, so the numpy variant (+ I on cov_c) is off for the call.  The ONE body behind
// wct_transform_solve and the patch swap's whitening.
int solve_against_slot(wct_ctx* ctx, int mode, int C, double n_c, const double* sum_c, const double* sumsq_c, const double* style_stats, double alpha,
                       double* M, double* b, int* info_dev) {
  hipStream_t st = ctx->main.stream;
  const size_t cc = (size_t)C * C;
  if (int rc = ensure(ctx, ctx->eigS[0], eig_result_bytes(C))) return rc;
  double* es = reinterpret_cast<double*>(ctx->eigS[0].p);
  if (style_stats) {
    HIPCHK(ctx, hipMemcpyAsync(es + eig_result_F_offset(C), style_stats, cc * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(es + cc + C, style_stats + cc, (size_t)C * sizeof(double), hipMemcpyDeviceToDevice, st));
  } else {
    HIPCHK(ctx, launch_mb_identity(es + eig_result_F_offset(C), es + cc + C, C, 1, 1u, st));
  }
  HIPCHK(ctx, hipMemsetAsync(info_dev, 0, 2 * sizeof(int), st));
  const int numpy = ctx->numpy_variant;
  ctx->numpy_variant = 0;     // mode-explicit: T as the header defines it
  const int rc = transform_mb(ctx, mode, C, n_c, sum_c, sumsq_c, ctx->eigS[0], alpha, M, b, info_dev, nullptr);
  ctx->numpy_variant = numpy;
  return rc;
}
}  // namespace

extern "C" {

int wct_set_transform(wct_ctx* ctx, int mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (mode != WCT_TRANSFORM_WCT && mode != WCT_TRANSFORM_OT && mode != WCT_TRANSFORM_ADAIN) return fail(ctx, WCT_ERR_INVALID, "set_transform: mode %d outside 0..2", mode);
  if (mode != WCT_TRANSFORM_WCT && ctx->numpy_variant) return fail(ctx, WCT_ERR_INVALID, "set_transform: the numpy variant (+ I on cov_c) is defined for the wct transform only");
  if (mode != WCT_TRANSFORM_WCT)
    for (int level = 1; level <= 5; ++level)
      if (ctx->rotated[level])
        return fail(ctx, WCT_ERR_STATE, "set_transform: the style slot of level %d is rotated (wct_style_diversify), which the wct transform alone reads as it is meant; "
                    "prepare or import the style again first", level);
  ctx->transform = mode;
  return WCT_OK;
}

int wct_get_transform(const wct_ctx* ctx, int* mode) {
  if (!ctx || !mode) return WCT_ERR_INVALID;
  *mode = ctx->transform;
  return WCT_OK;
}

int wct_transform_solve(wct_ctx* ctx, int mode, int C, double n_c, const double* sum_c, const double* sumsq_c, const double* style_stats, double alpha,
                        double* M, double* b, int* info) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!sum_c || !sumsq_c || !style_stats || !M || !b) return fail(ctx, WCT_ERR_INVALID, "transform_solve: NULL pointer");
  if (mode != WCT_TRANSFORM_WCT && mode != WCT_TRANSFORM_OT && mode != WCT_TRANSFORM_ADAIN) return fail(ctx, WCT_ERR_INVALID, "transform_solve: mode %d outside 0..2", mode);
  if (C < 2 || (C & 1) || C > 512) return fail(ctx, WCT_ERR_INVALID, "transform_solve: C=%d must be even and <= 512", C);
  if (!(n_c >= 2)) return fail(ctx, WCT_ERR_INVALID, "transform_solve: unbiased covariance needs >= 2 pixels (n=%g)", n_c);
  SumsView sv;
  if (int rc = sums_view(ctx, ctx->main, sv)) return rc;
  hipStream_t st = ctx->main.stream;
  if (int rc = solve_against_slot(ctx, mode, C, n_c, sum_c, sumsq_c, style_stats, alpha, M, b, sv.info)) return rc;
  if (info) {
    HIPCHK(ctx, hipMemcpyAsync(info, sv.info, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  return WCT_OK;
}

}  // extern "C"

// ---- patch swap (include/wct_hip_swap.h; kernels in swap.hip) -----------------------------------------------------------------------
namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the shape limits every entry shares; `who` names the entry
int swap_shape_check(wct_ctx* ctx, const char* who, int h, int w, int hs, int ws, int C) {
  if (h < 3 || w < 3 || hs < 3 || ws < 3) return fail(ctx, WCT_ERR_INVALID, "%s: maps %dx%d and %dx%d must be at least 3x3 (patches are 3x3)", who, h, w, hs, ws);
  if (C < 4 || (C & 3) || C > 512) return fail(ctx, WCT_ERR_INVALID, "%s: C=%d must be a multiple of 4 in [4,512]", who, C);
  if ((long)(hs - 2) * (ws - 2) > 2147483647L) return fail(ctx, WCT_ERR_INVALID, "%s: %ld keys do not fit a 32-bit index", who, (long)(hs - 2) * (ws - 2));
  if ((long)(h - 2) * (w - 2) > 2147483647L) return fail(ctx, WCT_ERR_INVALID, "%s: %ld queries exceed 2^31 - 1", who, (long)(h - 2) * (w - 2));
  return WCT_OK;
}

int swap_mode_check(wct_ctx* ctx, const char* who, int level, int match_mode, float alpha) {
  if (level < 2 || level > 5) return fail(ctx, WCT_ERR_INVALID, "%s: swap level %d outside 2..5 (level 1 is a full-resolution match: out of scope)", who, level);
  if (match_mode != WCT_SWAP_WHITENED && match_mode != WCT_SWAP_RAW)
    return fail(ctx, WCT_ERR_INVALID, "%s: match_mode %d is not WCT_SWAP_WHITENED (0) or WCT_SWAP_RAW (1)", who, match_mode);
  if (!std::isfinite(alpha)) return fail(ctx, WCT_ERR_INVALID, "%s: alpha must be finite", who);
  return WCT_OK;
}

int patch_match_impl(wct_ctx* ctx, const float* q, int h, int w, const float* k, int hs, int ws, int C, int32_t* idx, float* best) {
  const long nq = (long)(h - 2) * (w - 2), nk = (long)(hs - 2) * (ws - 2);
  if (int rc = ensure(ctx, ctx->swRun, swap_run_bytes(nq))) return rc;
  if (int rc = ensure(ctx, ctx->swNorm, swap_norm_bytes(nk))) return rc;
  const int chunk = ctx->swap_key_chunk > 0 ? ctx->swap_key_chunk : WCT_SWAP_KEY_CHUNK;
  ProfScope ps(ctx, ctx->main.stream, "patch_match<f16x3>", 6.0 * 9 * C * (double)nq * (double)nk, 4.0 * C * ((double)h * w + (double)hs * ws));
  HIPCHK(ctx, launch_patch_match(q, h, w, k, hs, ws, C, chunk, idx, best, ctx->swRun.p, ctx->swRun.cap, reinterpret_cast<float*>(ctx->swNorm.p),
                                 ctx->swNorm.cap, ctx->sat_dev, ctx->main.stream));
  return WCT_OK;
}

int patch_assemble_impl(wct_ctx* ctx, const int32_t* idx, int h, int w, const float* v, int hs, int ws, int C, const float* base, float alpha, float* out) {
  ProfScope ps(ctx, ctx->main.stream, "patch_assemble", 10.0 * C * h * w, (10.0 + (base ? 2 : 1)) * 4.0 * C * h * w);
  HIPCHK(ctx, launch_patch_assemble(idx, h, w, v, hs, ws, C, base, alpha, out, ctx->main.stream));
  return WCT_OK;
}

// every context buffer one wct_swap_level of these feature sizes touches, before anything is enqueued
int swap_bufs(wct_ctx* ctx, int C, int h, int w, int hs, int ws, bool whitened) {
  const size_t fc = (size_t)h * w * C * sizeof(float), fs = (size_t)hs * ws * C * sizeof(float);
  if (int rc = ensure(ctx, ctx->swFc, fc)) return rc;
  if (int rc = ensure(ctx, ctx->swFs, fs)) return rc;
  if (int rc = ensure(ctx, ctx->swOut, fc)) return rc;
  if (int rc = ensure(ctx, ctx->swIdx, (size_t)(h - 2) * (w - 2) * sizeof(int32_t))) return rc;
  if (int rc = ensure(ctx, ctx->swRun, swap_run_bytes((long)(h - 2) * (w - 2)))) return rc;
  if (int rc = ensure(ctx, ctx->swNorm, swap_norm_bytes((long)(hs - 2) * (ws - 2)))) return rc;
  if (!whitened) return WCT_OK;
  if (int rc = ensure(ctx, ctx->swQ, fc)) return rc;
  if (int rc = ensure(ctx, ctx->swK, fs)) return rc;
  if (int rc = ensure(ctx, ctx->swLab, std::max((size_t)h * w, (size_t)hs * ws))) return rc;
  if (int rc = ensure(ctx, ctx->eigS[0], eig_result_bytes(C))) return rc;
  if (int rc = ensure(ctx, ctx->wsRegApply, apply_labeled_workspace_bytes(C, 1))) return rc;
  return WCT_OK;
}

}  // namespace

// (W, -W mu) of a map, W = cov^(-1/2) of the map itself, into the context's (M, b), and its raw moments into the main lane's sums:
// wct_moments + wct_transform_solve(WCT_TRANSFORM_WCT, [I, 0], alpha = 1).  Shared with the attention statistics' whitened domain (api_attn.hip).
int wct_host::whiten_solve(wct_ctx* ctx, const float* feat, int C, int h, int w, SumsView& sv, double** M, double** b) {
  Lane& ln = ctx->main;
  if (int rc = sums_view(ctx, ln, sv)) return rc;
  if (int rc = mb_view(ctx, M, b)) return rc;
  if (int rc = moments_impl(ctx, ln, feat, C, h, w, 0, w, sv.sum, sv.sumsq)) return rc;
  return solve_against_slot(ctx, WCT_TRANSFORM_WCT, C, (double)h * w, sv.sum, sv.sumsq, nullptr, 1.0, *M, *b, sv.info);
}

namespace {
// dst = W (feat - mu): whiten_solve + wct_apply_labeled with one label
int swap_whiten(wct_ctx* ctx, const float* feat, int C, int h, int w, float* dst) {
  SumsView sv;
  double *M, *b;
  if (int rc = whiten_solve(ctx, feat, C, h, w, sv, &M, &b)) return rc;
  const long npix = (long)h * w;
  HIPCHK(ctx, hipMemsetAsync(ctx->swLab.p, 0, (size_t)npix, ctx->main.stream));
  return apply_labeled_impl(ctx, feat, C, npix, reinterpret_cast<const uint8_t*>(ctx->swLab.p), 1, M, b, dst);
}

// the feature sizes of a level, checked: WCT_OK or the refusal
int swap_level_dims(wct_ctx* ctx, const char* who, int level, int H, int W, int Hs, int Ws, int& C, int& h, int& w, int& hs, int& ws) {
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded || !ctx->mod[WCT_KIND_DEC][level].loaded) return fail(ctx, WCT_ERR_STATE, "%s: encoder / decoder %d not loaded", who, level);
  if (H < 1 || W < 1 || Hs < 1 || Ws < 1) return fail(ctx, WCT_ERR_INVALID, "%s: bad shapes (content %dx%d, style %dx%d)", who, H, W, Hs, Ws);
  C = me.layers.back().d.cout;
  level_dims(level, H, W, h, w);
  level_dims(level, Hs, Ws, hs, ws);
  return swap_shape_check(ctx, who, h, w, hs, ws, C);
}

// body of wct_swap_level behind its checks and swap_bufs
int swap_level_impl(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs, int Ws, int C, int h, int w, int hs, int ws,
                    int match_mode, float alpha, float* out) {
  Lane& ln = ctx->main;
  float* fC = reinterpret_cast<float*>(ctx->swFc.p);
  float* fS = reinterpret_cast<float*>(ctx->swFs.p);
  if (int rc = encode_impl(ctx, ln, level, content, H, W, fC, nullptr, nullptr)) return rc;
  if (int rc = encode_impl(ctx, ln, level, style, Hs, Ws, fS, nullptr, nullptr)) return rc;
  const float *qm = fC, *km = fS;
  if (match_mode == WCT_SWAP_WHITENED) {
    if (int rc = swap_whiten(ctx, fC, C, h, w, reinterpret_cast<float*>(ctx->swQ.p))) return rc;
    if (int rc = swap_whiten(ctx, fS, C, hs, ws, reinterpret_cast<float*>(ctx->swK.p))) return rc;
    qm = reinterpret_cast<float*>(ctx->swQ.p);
    km = reinterpret_cast<float*>(ctx->swK.p);
  }
  int32_t* idx = reinterpret_cast<int32_t*>(ctx->swIdx.p);
  float* csF = reinterpret_cast<float*>(ctx->swOut.p);
  if (int rc = patch_match_impl(ctx, qm, h, w, km, hs, ws, C, idx, nullptr)) return rc;
  if (int rc = patch_assemble_impl(ctx, idx, h, w, fS, hs, ws, C, fC, alpha, csF)) return rc;
  return decode_impl(ctx, level, csF, h, w, nullptr, out);
}
}  // namespace

extern "C" {

int wct_patch_match(wct_ctx* ctx, const float* q, int h, int w, const float* k, int hs, int ws, int C, int32_t* idx, float* best) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!q || !k || !idx) return fail(ctx, WCT_ERR_INVALID, "wct_patch_match: NULL map or idx");
  if (int rc = swap_shape_check(ctx, "wct_patch_match", h, w, hs, ws, C)) return rc;
  if (!aligned16(q) || !aligned16(k)) return fail(ctx, WCT_ERR_INVALID, "wct_patch_match: the maps must be 16-byte aligned");
  {
    const size_t nq = (size_t)(h - 2) * (w - 2), qb = (size_t)h * w * C * sizeof(float), kb = (size_t)hs * ws * C * sizeof(float);
    if (ranges_overlap(idx, nq * sizeof(int32_t), q, qb) || ranges_overlap(idx, nq * sizeof(int32_t), k, kb) ||
        (best && (ranges_overlap(best, nq * sizeof(float), q, qb) || ranges_overlap(best, nq * sizeof(float), k, kb) ||
                  ranges_overlap(best, nq * sizeof(float), idx, nq * sizeof(int32_t)))))
      return fail(ctx, WCT_ERR_INVALID, "wct_patch_match: idx or best overlaps a map (read by every launch) or each other");
  }
  if (int rc = patch_match_impl(ctx, q, h, w, k, hs, ws, C, idx, best)) return rc;
  return range_readback(ctx);
}

int wct_patch_assemble(wct_ctx* ctx, const int32_t* idx, int h, int w, const float* v, int hs, int ws, int C, const float* base, float alpha, float* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!idx || !v || !out) return fail(ctx, WCT_ERR_INVALID, "wct_patch_assemble: NULL idx, v or out");
  if (int rc = swap_shape_check(ctx, "wct_patch_assemble", h, w, hs, ws, C)) return rc;
  if (!std::isfinite(alpha)) return fail(ctx, WCT_ERR_INVALID, "wct_patch_assemble: alpha must be finite");
  if (!base && alpha != 1.f) return fail(ctx, WCT_ERR_INVALID, "wct_patch_assemble: base may be NULL only when alpha == 1 (got %g)", (double)alpha);
  if (!aligned16(v) || !aligned16(out) || !aligned16(base)) return fail(ctx, WCT_ERR_INVALID, "wct_patch_assemble: v, base and out must be 16-byte aligned");
  const size_t ob = (size_t)h * w * C * sizeof(float);
  if (ranges_overlap(out, ob, v, (size_t)hs * ws * C * sizeof(float)) || ranges_overlap(out, ob, idx, (size_t)(h - 2) * (w - 2) * sizeof(int32_t)))
    return fail(ctx, WCT_ERR_INVALID, "wct_patch_assemble: out overlaps v or idx, which are read while it is written");
  return patch_assemble_impl(ctx, idx, h, w, v, hs, ws, C, base, alpha, out);
}

int wct_swap_level(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs, int Ws, int match_mode, float alpha,
                   float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || !style || !out) return fail(ctx, WCT_ERR_INVALID, "wct_swap_level: NULL pointer");
  if (int rc = swap_mode_check(ctx, "wct_swap_level", level, match_mode, alpha)) return rc;
  int C, h, w, hs, ws;
  if (int rc = swap_level_dims(ctx, "wct_swap_level", level, H, W, Hs, Ws, C, h, w, hs, ws)) return rc;
  if (int rc = swap_bufs(ctx, C, h, w, hs, ws, match_mode == WCT_SWAP_WHITENED)) return rc;
  if (int rc = swap_level_impl(ctx, level, content, H, W, style, Hs, Ws, C, h, w, hs, ws, match_mode, alpha, out)) return rc;
  if (Ho) *Ho = h << (level - 1);
  if (Wo) *Wo = w << (level - 1);
  return range_readback(ctx);
}

int wct_stylize_swap(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, int swap_level, int match_mode, float alpha,
                     int num_run, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || !style || !out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_swap: bad arguments (a NULL pointer, or num_run < 1)");
  if (int rc = swap_mode_check(ctx, "wct_stylize_swap", swap_level, match_mode, alpha)) return rc;
  if (H < 16 || W < 16) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_swap: content %dx%d is smaller than 16x16", H, W);
  // the swap level's input is the result of the levels above it: 16 floor(H / 16) x 16 floor(W / 16) from level 5 on, in every run
  const int Hl = swap_level == 5 ? H : (H / 16) * 16, Wl = swap_level == 5 ? W : (W / 16) * 16;
  int C, h, w, hs, ws;
  if (int rc = swap_level_dims(ctx, "wct_stylize_swap", swap_level, Hl, Wl, Hs, Ws, C, h, w, hs, ws)) return rc;
  // every buffer of the swap first (level 5 of a first run sees the un-cropped content; its feature map is the cropped one's)
  if (int rc = swap_bufs(ctx, C, h, w, hs, ws, match_mode == WCT_SWAP_WHITENED)) return rc;
  return run_cascade(
      ctx, content, H, W, num_run, out, Ho, Wo,
      [&](int level, const float* cur, int ch, int cw, float* dst, int* ho, int* wo) -> int {
        if (level == swap_level) {
          int lc, lh, lw, lhs, lws;
          if (int rc = swap_level_dims(ctx, "wct_stylize_swap", level, ch, cw, Hs, Ws, lc, lh, lw, lhs, lws)) return rc;
          if (int rc = swap_level_impl(ctx, level, cur, ch, cw, style, Hs, Ws, lc, lh, lw, lhs, lws, match_mode, alpha, dst)) return rc;
          *ho = lh << (level - 1); *wo = lw << (level - 1);
        } else {
          if (int rc = with_deferred_solves(ctx, false, [&]() -> int {
                if (int rc = fork_side(ctx)) return rc;
                if (int rc = style_side(ctx, level, style, Hs, Ws)) return rc;
                return content_side(ctx, level, cur, ch, cw, alpha, dst, ho, wo);
              })) return rc;
        }
        return range_readback(ctx);   // per level: the call ends without one of its own
      },
      [](int) { return (int)WCT_OK; });
}

}  // extern "C"
