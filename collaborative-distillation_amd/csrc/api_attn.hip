// Attention-weighted style statistics (include/wct_hip_attn.h; kernels in attn.hip) behind the C ABI.
#include "../../include/wct_hip_attn.h"
#include "wct_ctx.h"

using namespace wct_host;

namespace {
bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int attn_c_check(wct_ctx* ctx, const char* who, int C) {
  if (C < 4 || (C & 3) || C > 512) return fail(ctx, WCT_ERR_INVALID, "%s: C=%d must be a multiple of 4 in [4,512]", who, C);
  return WCT_OK;
}

int attn_mode_check(wct_ctx* ctx, const char* who, int level, int domain, float tau, float alpha) {
  if (level < 2 || level > 5) return fail(ctx, WCT_ERR_INVALID, "%s: level %d outside 2..5", who, level);
  if (domain != WCT_ATTN_STANDARD && domain != WCT_ATTN_WHITENED)
    return fail(ctx, WCT_ERR_INVALID, "%s: domain %d is not WCT_ATTN_STANDARD (0) or WCT_ATTN_WHITENED (1)", who, domain);
  if (!(tau >= 0.f && tau <= (float)WCT_ATTN_MAX_TEMP)) return fail(ctx, WCT_ERR_INVALID, "%s: tau=%g outside [0, %d]", who, (double)tau, WCT_ATTN_MAX_TEMP);
  if (!std::isfinite(alpha)) return fail(ctx, WCT_ERR_INVALID, "%s: alpha must be finite", who);
  return WCT_OK;
}

// the f16 products one wct_attn_stats issues: per (query, key) pair 3 terms over the 32-channel steps of the scores (once per value slab) and
// 2 x 3 terms over the 16-channel tiles of the values
double attn_stats_flops(int C, double nq, double nk) {
  const int slabs = (C + 127) / 128;
  double per_pair = 0;
  for (int s = 0; s < slabs; ++s) {
    const int sc = std::min(C - 128 * s, 128);
    per_pair += 3.0 * ((C + 31) / 32 * 32) + 6.0 * ((sc + 15) / 16 * 16);
  }
  return 2.0 * per_pair * nq * nk;
}

// every context buffer the projection of an h x w map touches that this file sizes itself
int project_bufs(wct_ctx* ctx, int C, long npix, bool whitened, bool need_scratch) {
  if (int rc = ensure(ctx, ctx->swLab, (size_t)npix)) return rc;
  if (int rc = ensure(ctx, ctx->wsRegApply, apply_labeled_workspace_bytes(C, 1))) return rc;
  if (whitened) {
    if (int rc = ensure(ctx, ctx->eigS[0], eig_result_bytes(C))) return rc;
    if (int rc = ensure(ctx, ctx->atMt, (size_t)C * C * sizeof(double))) return rc;
  }
  if (need_scratch)
    if (int rc = ensure(ctx, ctx->atProj, (size_t)npix * C * sizeof(float))) return rc;
  SumsView sv;
  if (int rc = sums_view(ctx, ctx->main, sv)) return rc;
  double *M, *b;
  return mb_view(ctx, &M, &b);
}

// unit_out, std_out (may be null: then the standardised map is made only where the domain needs it, in atProj), (mu, sigma) (may be null)
int project_impl(wct_ctx* ctx, const float* feat, int h, int w, int C, int domain, float* unit_out, float* std_out, double* mu_out, double* sigma_out) {
  Lane& ln = ctx->main;
  const long npix = (long)h * w;
  const bool need_std = std_out || domain == WCT_ATTN_STANDARD;
  float* sd = std_out ? std_out : reinterpret_cast<float*>(ctx->atProj.p);
  if (need_std || mu_out) {
    SumsView sv;
    if (int rc = sums_view(ctx, ln, sv)) return rc;
    double *M, *b;
    if (int rc = mb_view(ctx, &M, &b)) return rc;
    if (int rc = moments_impl(ctx, ln, feat, C, h, w, 0, w, sv.sum, sv.sumsq)) return rc;
    HIPCHK(ctx, launch_attn_diag(C, (double)npix, WCT_ADAIN_EPS, sv.sum, sv.sumsq, M, b, mu_out, sigma_out, ln.stream));
    if (need_std) {
      HIPCHK(ctx, hipMemsetAsync(ctx->swLab.p, 0, (size_t)npix, ln.stream));
      if (int rc = apply_labeled_impl(ctx, feat, C, npix, reinterpret_cast<const uint8_t*>(ctx->swLab.p), 1, M, b, sd)) return rc;
    }
  }
  const float* proj = sd;
  if (domain == WCT_ATTN_WHITENED) {
    // the patch swap's whitening matrix (whiten_solve), applied to the centred map in fp64: the swap's own fp32 application of (W, -W mu)
    // to the un-centred map is 1e-6 of the largest unit value from fp64 by itself, which an arg-max does not feel and a softmax weight does
    SumsView sv;
    double *M, *b;
    if (int rc = whiten_solve(ctx, feat, C, h, w, sv, &M, &b)) return rc;
    {
      ProfScope pw(ctx, ln.stream, "attn_whiten", 2.0 * C * C * npix, 8.0 * C * npix);
      HIPCHK(ctx, launch_attn_whiten(feat, npix, C, sv.sum, M, reinterpret_cast<double*>(ctx->atMt.p), reinterpret_cast<float*>(ctx->atProj.p), ln.stream));
    }
    proj = reinterpret_cast<float*>(ctx->atProj.p);
  }
  ProfScope ps(ctx, ln.stream, "attn_unit", 3.0 * C * npix, 8.0 * C * npix);
  HIPCHK(ctx, launch_attn_unit(proj, npix, C, unit_out, ln.stream));
  return WCT_OK;
}

float* stat_scratch(wct_ctx* ctx, int C) { return reinterpret_cast<float*>(reinterpret_cast<double*>(ctx->atStat.p) + 2 * (size_t)C); }

int stats_impl(wct_ctx* ctx, const float* qhat, int Nq, const float* khat, const float* v, int Nk, int C, float tau, float* mean, float* var) {
  const int chunk = ctx->attn_query_chunk > 0 ? ctx->attn_query_chunk : WCT_ATTN_QUERY_CHUNK;
  ProfScope ps(ctx, ctx->main.stream, "attn_stats<f16x3>", attn_stats_flops(C, Nq, Nk), 4.0 * C * (3.0 * Nq + 2.0 * Nk));
  HIPCHK(ctx, launch_attn_stats(qhat, Nq, khat, v, Nk, C, tau, chunk, mean, var, stat_scratch(ctx, C), ctx->main.stream));
  return WCT_OK;
}

int apply_impl(wct_ctx* ctx, const float* mean, const float* var, const float* c_std, const float* cF, long n, int C, const double* mu_s,
               const double* sigma_s, float alpha, float* out) {
  ProfScope ps(ctx, ctx->main.stream, "attn_apply", 8.0 * C * n, 20.0 * C * n);
  HIPCHK(ctx, launch_attn_apply(mean, var, c_std, cF, n, C, mu_s, sigma_s, alpha, out, ctx->main.stream));
  return WCT_OK;
}

// every context buffer one wct_attn_level of these feature sizes touches, before anything is enqueued
int attn_bufs(wct_ctx* ctx, int C, int h, int w, int hs, int ws, bool whitened) {
  const long nq = (long)h * w, nk = (long)hs * ws;
  const size_t fc = (size_t)nq * C * sizeof(float), fs = (size_t)nk * C * sizeof(float);
  for (DevBuf* b : {&ctx->atFc, &ctx->atCs, &ctx->atQ, &ctx->atMean, &ctx->atVar, &ctx->atOut})
    if (int rc = ensure(ctx, *b, fc)) return rc;
  for (DevBuf* b : {&ctx->atFs, &ctx->atSs, &ctx->atK})
    if (int rc = ensure(ctx, *b, fs)) return rc;
  if (int rc = ensure(ctx, ctx->atStat, attn_stat_bytes(C))) return rc;
  if (int rc = project_bufs(ctx, C, std::max(nq, nk), whitened, false)) return rc;
  if (whitened)
    if (int rc = ensure(ctx, ctx->atProj, std::max(fc, fs))) return rc;
  return WCT_OK;
}

// the feature sizes of a level, checked: WCT_OK or the refusal
int attn_level_dims(wct_ctx* ctx, const char* who, int level, int H, int W, int Hs, int Ws, int& C, int& h, int& w, int& hs, int& ws) {
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded || !ctx->mod[WCT_KIND_DEC][level].loaded) return fail(ctx, WCT_ERR_STATE, "%s: encoder / decoder %d not loaded", who, level);
  if (H < 1 || W < 1 || Hs < 1 || Ws < 1) return fail(ctx, WCT_ERR_INVALID, "%s: bad shapes (content %dx%d, style %dx%d)", who, H, W, Hs, Ws);
  C = me.layers.back().d.cout;
  level_dims(level, H, W, h, w);
  level_dims(level, Hs, Ws, hs, ws);
  if ((long)h * w < 2 || (long)hs * ws < 2)
    return fail(ctx, WCT_ERR_INVALID, "%s: feature maps %dx%d and %dx%d need at least 2 positions each (the variance is unbiased)", who, h, w, hs, ws);
  if ((long)h * w > 2147483647L || (long)hs * ws > 2147483647L) return fail(ctx, WCT_ERR_INVALID, "%s: more than 2^31 - 1 positions", who);
  return attn_c_check(ctx, who, C);
}

// body of wct_attn_level behind its checks and attn_bufs
int attn_level_impl(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs, int Ws, int C, int h, int w, int hs, int ws,
                    int domain, float tau, float alpha, float* out) {
  Lane& ln = ctx->main;
  float* fC = reinterpret_cast<float*>(ctx->atFc.p);
  float* fS = reinterpret_cast<float*>(ctx->atFs.p);
  float* cS = reinterpret_cast<float*>(ctx->atCs.p);
  float* sS = reinterpret_cast<float*>(ctx->atSs.p);
  float* qh = reinterpret_cast<float*>(ctx->atQ.p);
  float* kh = reinterpret_cast<float*>(ctx->atK.p);
  float* mean = reinterpret_cast<float*>(ctx->atMean.p);
  float* var = reinterpret_cast<float*>(ctx->atVar.p);
  float* csF = reinterpret_cast<float*>(ctx->atOut.p);
  double* mu = reinterpret_cast<double*>(ctx->atStat.p);
  double* sigma = mu + C;
  if (int rc = encode_impl(ctx, ln, level, content, H, W, fC, nullptr, nullptr)) return rc;
  if (int rc = encode_impl(ctx, ln, level, style, Hs, Ws, fS, nullptr, nullptr)) return rc;
  if (int rc = project_impl(ctx, fS, hs, ws, C, domain, kh, sS, mu, sigma)) return rc;
  if (int rc = project_impl(ctx, fC, h, w, C, domain, qh, cS, nullptr, nullptr)) return rc;
  if (int rc = stats_impl(ctx, qh, h * w, kh, sS, hs * ws, C, tau, mean, var)) return rc;
  if (int rc = apply_impl(ctx, mean, var, cS, fC, (long)h * w, C, mu, sigma, alpha, csF)) return rc;
  return decode_impl(ctx, level, csF, h, w, nullptr, out);
}
}  // namespace

extern "C" {

int wct_attn_project(wct_ctx* ctx, const float* feat, int h, int w, int C, int domain, float* unit_out, float* std_out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !unit_out) return fail(ctx, WCT_ERR_INVALID, "wct_attn_project: NULL feat or unit_out");
  if (int rc = attn_c_check(ctx, "wct_attn_project", C)) return rc;
  if (h < 1 || w < 1 || (long)h * w < 2 || (long)h * w > 2147483647L)
    return fail(ctx, WCT_ERR_INVALID, "wct_attn_project: a map of %dx%d: 2 .. 2^31 - 1 positions expected (the variance is unbiased)", h, w);
  if (domain != WCT_ATTN_STANDARD && domain != WCT_ATTN_WHITENED)
    return fail(ctx, WCT_ERR_INVALID, "wct_attn_project: domain %d is not WCT_ATTN_STANDARD (0) or WCT_ATTN_WHITENED (1)", domain);
  if (!al16(feat) || !al16(unit_out) || !al16(std_out)) return fail(ctx, WCT_ERR_INVALID, "wct_attn_project: the maps must be 16-byte aligned");
  const size_t nb = (size_t)h * w * C * sizeof(float);
  if (ranges_overlap(unit_out, nb, feat, nb) || (std_out && (ranges_overlap(std_out, nb, feat, nb) || ranges_overlap(std_out, nb, unit_out, nb))))
    return fail(ctx, WCT_ERR_INVALID, "wct_attn_project: an output overlaps feat or the other output");
  const bool whitened = domain == WCT_ATTN_WHITENED;
  if (int rc = project_bufs(ctx, C, (long)h * w, whitened, whitened || !std_out)) return rc;
  return project_impl(ctx, feat, h, w, C, domain, unit_out, std_out, nullptr, nullptr);
}

int wct_attn_stats(wct_ctx* ctx, const float* qhat, int Nq, const float* khat, const float* v, int Nk, int C, float tau, float* mean, float* var) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!qhat || !khat || !v || !mean || !var) return fail(ctx, WCT_ERR_INVALID, "wct_attn_stats: NULL pointer");
  if (int rc = attn_c_check(ctx, "wct_attn_stats", C)) return rc;
  if (Nq < 2 || Nk < 2) return fail(ctx, WCT_ERR_INVALID, "wct_attn_stats: Nq=%d, Nk=%d: at least 2 each expected", Nq, Nk);
  if (!(tau >= 0.f && tau <= (float)WCT_ATTN_MAX_TEMP)) return fail(ctx, WCT_ERR_INVALID, "wct_attn_stats: tau=%g outside [0, %d]", (double)tau, WCT_ATTN_MAX_TEMP);
  if (!al16(qhat) || !al16(khat) || !al16(v) || !al16(mean) || !al16(var)) return fail(ctx, WCT_ERR_INVALID, "wct_attn_stats: every pointer must be 16-byte aligned");
  const size_t qb = (size_t)Nq * C * sizeof(float), kb = (size_t)Nk * C * sizeof(float);
  for (const float* o : {mean, var})
    if (ranges_overlap(o, qb, qhat, qb) || ranges_overlap(o, qb, khat, kb) || ranges_overlap(o, qb, v, kb))
      return fail(ctx, WCT_ERR_INVALID, "wct_attn_stats: an output overlaps an input (every launch reads them)");
  if (ranges_overlap(mean, qb, var, qb)) return fail(ctx, WCT_ERR_INVALID, "wct_attn_stats: mean overlaps var");
  if (int rc = ensure(ctx, ctx->atStat, attn_stat_bytes(C))) return rc;
  return stats_impl(ctx, qhat, Nq, khat, v, Nk, C, tau, mean, var);
}

int wct_attn_apply(wct_ctx* ctx, const float* mean, const float* var, const float* c_std, const float* cF, int n, int C, const double* mu_s,
                   const double* sigma_s, float alpha, float* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!mean || !var || !c_std || !cF || !mu_s || !sigma_s || !out) return fail(ctx, WCT_ERR_INVALID, "wct_attn_apply: NULL pointer");
  if (int rc = attn_c_check(ctx, "wct_attn_apply", C)) return rc;
  if (n < 1) return fail(ctx, WCT_ERR_INVALID, "wct_attn_apply: n=%d positions", n);
  if (!std::isfinite(alpha)) return fail(ctx, WCT_ERR_INVALID, "wct_attn_apply: alpha must be finite");
  if (!al16(mean) || !al16(var) || !al16(c_std) || !al16(cF) || !al16(out)) return fail(ctx, WCT_ERR_INVALID, "wct_attn_apply: the maps must be 16-byte aligned");
  const size_t nb = (size_t)n * C * sizeof(float), sb = (size_t)C * sizeof(double);
  for (const float* in : {mean, var, c_std, cF})
    if (ranges_overlap(out, nb, in, nb)) return fail(ctx, WCT_ERR_INVALID, "wct_attn_apply: out overlaps an input map");
  if (ranges_overlap(out, nb, mu_s, sb) || ranges_overlap(out, nb, sigma_s, sb)) return fail(ctx, WCT_ERR_INVALID, "wct_attn_apply: out overlaps mu_s or sigma_s");
  return apply_impl(ctx, mean, var, c_std, cF, n, C, mu_s, sigma_s, alpha, out);
}

int wct_attn_level(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs, int Ws, int domain, float tau, float alpha,
                   float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || !style || !out) return fail(ctx, WCT_ERR_INVALID, "wct_attn_level: NULL pointer");
  if (int rc = attn_mode_check(ctx, "wct_attn_level", level, domain, tau, alpha)) return rc;
  int C, h, w, hs, ws;
  if (int rc = attn_level_dims(ctx, "wct_attn_level", level, H, W, Hs, Ws, C, h, w, hs, ws)) return rc;
  if (int rc = attn_bufs(ctx, C, h, w, hs, ws, domain == WCT_ATTN_WHITENED)) return rc;
  if (int rc = attn_level_impl(ctx, level, content, H, W, style, Hs, Ws, C, h, w, hs, ws, domain, tau, alpha, out)) return rc;
  if (Ho) *Ho = h << (level - 1);
  if (Wo) *Wo = w << (level - 1);
  return range_readback(ctx);
}

int wct_stylize_attn(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, int attn_level, int domain, float tau,
                     float alpha, int num_run, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || !style || !out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_attn: bad arguments (a NULL pointer, or num_run < 1)");
  if (int rc = attn_mode_check(ctx, "wct_stylize_attn", attn_level, domain, tau, alpha)) return rc;
  if (H < 16 || W < 16) return fail(ctx, WCT_ERR_INVALID, "wct_stylize_attn: content %dx%d is smaller than 16x16", H, W);
  // the attention level's input is the result of the levels above it: 16 floor(H / 16) x 16 floor(W / 16) from level 5 on, in every run
  const int Hl = attn_level == 5 ? H : (H / 16) * 16, Wl = attn_level == 5 ? W : (W / 16) * 16;
  int C, h, w, hs, ws;
  if (int rc = attn_level_dims(ctx, "wct_stylize_attn", attn_level, Hl, Wl, Hs, Ws, C, h, w, hs, ws)) return rc;
  if (int rc = attn_bufs(ctx, C, h, w, hs, ws, domain == WCT_ATTN_WHITENED)) return rc;
  return run_cascade(
      ctx, content, H, W, num_run, out, Ho, Wo,
      [&](int level, const float* cur, int ch, int cw, float* dst, int* ho, int* wo) -> int {
        if (level == attn_level) {
          int lc, lh, lw, lhs, lws;
          if (int rc = attn_level_dims(ctx, "wct_stylize_attn", level, ch, cw, Hs, Ws, lc, lh, lw, lhs, lws)) return rc;
          if (int rc = attn_level_impl(ctx, level, cur, ch, cw, style, Hs, Ws, lc, lh, lw, lhs, lws, domain, tau, alpha, dst)) return rc;
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
