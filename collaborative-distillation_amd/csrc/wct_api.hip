// C ABI of libwct_hip (see include/wct_hip.h): the context, the per-level pipeline and the 5-level cascade, and the
// definitions of the internals the feature files share (wct_ctx.h; module loading is api_model.hip, the sharded cascade
// api_sharded.hip, the image / multi-style / swap entry points api_image.hip / api_multi.hip / api_swap.hip).  Host-side
// C++ only orchestrates launches on the context's HIP stream; all arithmetic is in the kernels.
#include "wct_ctx.h"

using namespace wct_host;

__thread LaunchForm wct_launch_form = {0, 0, false, {0}};   // wct_common.h

// Internals: what another host file also calls is declared in wct_ctx.h and has external linkage here; the rest is in anonymous namespaces.
namespace wct_host {

int fail(wct_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

constexpr int SAT_SIDE_WORD = 4;

void range_host_set(wct_ctx* ctx, unsigned n) {    // both lanes idle (the callers have synchronised them)
  if (ctx->sat_host) ctx->sat_host[0] = ctx->sat_host[SAT_SIDE_WORD] = n;
}

namespace {
// An entry point whose clamping kernels ran on the SIDE lane and that does not join the caller's stream to it (wct_style_prepare*: the
// style side is meant to overlap whatever the caller enqueues next) mirrors the counter on that lane, behind those kernels in stream
// order -- the caller's stream neither waits for the side lane nor does the host
int range_readback_side(wct_ctx* ctx, Lane& ln) {
  if (ctx->quiet_readback || &ln == &ctx->main) return WCT_OK;
  if (ctx->sat_host) HIPCHK(ctx, hipMemcpyAsync(ctx->sat_host + SAT_SIDE_WORD, ctx->sat_dev, sizeof(unsigned), hipMemcpyDeviceToHost, ln.stream));
  return WCT_OK;
}
}  // namespace

// the saturation counter follows every compute entry point to pinned host memory on the caller's stream (4 bytes, no sync):
// wct_range_poll then reports a clamp of any COMPLETED call without stalling the pipeline
int range_readback(wct_ctx* ctx) {
  if (ctx->quiet_readback) return WCT_OK;   // inside wct_stylize_sharded: the split-level entries it calls do not each mirror the counters, the call does once
  // 16 bytes: the saturation counter, its snapshot, and the two lanes' aborted single-launch solves (coop_health reads those)
  if (ctx->sat_host) HIPCHK(ctx, hipMemcpyAsync(ctx->sat_host, ctx->sat_dev, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->main.stream));
  return WCT_OK;
}

int ensure(wct_ctx* ctx, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes) return WCT_OK;
  if (b.p) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
    HIPCHK(ctx, hipFree(b.p));
    b.p = nullptr; b.cap = 0;
  }
  const size_t want = (bytes + 255) & ~(size_t)255;
  HIPCHK(ctx, hipMalloc(&b.p, want));
  b.cap = want;
  ++ctx->ws_allocs;
  if (ctx->poison >= 0) {   // debug hook "poison": a fresh allocation is usually zero pages -- it must not escape the fill
    HIPCHK(ctx, hipMemsetAsync(b.p, ctx->poison, want, ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));   // whichever lane writes the buffer first finds the fill finished
  }
  return WCT_OK;
}

namespace {
// debug hook "poison": fill every allocated SCRATCH buffer (wct_ctx::each_buf) with `byte`, each on the lane that owns it, between
// two synchronisations of both lanes
int poison_scratch(wct_ctx* ctx, int byte) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  hipError_t e = hipSuccess;
  ctx->each_buf([&](DevBuf& b, Lane* ln, bool scratch) {
    if (scratch && b.p && e == hipSuccess) e = hipMemsetAsync(b.p, byte, b.cap, ln->stream);
  });
  HIPCHK(ctx, e);
  HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  return WCT_OK;
}

void release(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr; b.cap = 0;
}
}  // namespace

int pad_cout(int c) {
  if (c <= 16) return 16;
  if (c <= 32) return 32;
  if (c <= 64) return 64;
  return (c + 127) / 128 * 128;
}

namespace {
void prof_collect(wct_ctx* ctx) {
  if (ctx->recs.empty()) return;
  (void)hipStreamSynchronize(ctx->main.stream);
  (void)hipStreamSynchronize(ctx->side.stream);
  // WCT_TIMELINE=<file>: every record as "name lane start_ms end_ms" relative to the first one (tools/experiments/lane_timeline.py:
  // what the two lanes do in an OVERLAPPED step -- event timestamps are device time, comparable across streams)
  FILE* tl = nullptr;
  if (const char* path = wct_debug_env("WCT_TIMELINE")) tl = fopen(path, "a");
  if (tl) fprintf(tl, "# collect %zu records\n", ctx->recs.size());
  for (auto& r : ctx->recs) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.e0, r.e1);
    if (tl) {
      float t0 = 0.f;
      (void)hipEventElapsedTime(&t0, ctx->recs.front().e0, r.e0);
      fprintf(tl, "%s %s %.4f %.4f\n", r.name.c_str(), r.side ? "side" : "main", t0, t0 + ms);
    }
    auto& e = ctx->prof_acc[r.name];
    if (e.launches == 0) { memset(&e, 0, sizeof e); snprintf(e.name, sizeof e.name, "%s", r.name.c_str()); }
    e.ms += ms; e.flops += r.flops; e.bytes += r.bytes; e.launches += 1;
  }
  for (auto& r : ctx->recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  if (tl) fclose(tl);
  ctx->recs.clear();
}

// ---- one conv launch, with algorithmic work accounting ---------------------------------------------
bool conv_runs_f16(const wct_ctx* ctx, const ConvDesc& d) {
  return ctx->conv_mode == 1 && d.wpk16 && !(d.flags & CONV_IN_NCHW3) && !(d.cin & 7);
}

int run_conv(wct_ctx* ctx, Lane& ln, const ConvDesc& d, const float* in, float* out, int H, int W) {
  char name[48];
  const bool f16 = conv_runs_f16(ctx, d);
  const bool spk = f16 && (d.flags & CONV_IN_SP16) && conv_sp_supported(d);   // DMA-staged persistent kernel
  if (!f16 && ((d.flags & CONV_IN_SP16) || ((d.flags & CONV_OUT_SP16) && !(d.flags & CONV_IN_NCHW3))))
    return fail(ctx, WCT_ERR_INVALID, "SP16 activations need the f16x3 path");
  // the layers behind an upsample get their own family: they issue 4/9 of the operator's products, so their algorithmic rate must not be
  // averaged into the nine-tap family's roofline figure
  snprintf(name, sizeof name, "conv3x3%s<co=%d%s%s%s%s%s>", f16 ? "_f16x3" : "_f32", d.cout_pad > 128 ? 128 : d.cout_pad,
           (d.flags & CONV_IN_NCHW3) ? ",in3" : "", (d.flags & CONV_POOL_OUT) ? ",pool" : "", (d.flags & CONV_OUT_NCHW3) ? ",out3" : "",
           spk ? ",dma" : "", (spk && conv_sp_up_form(d, H, W)) ? ",up" : "");
  static const bool shapes = getenv("WCT_PROF_SHAPES") != nullptr;   // one profile row per layer shape instead of per family
  if (shapes) { const size_t n = strlen(name); snprintf(name + n, sizeof name - n, "@%dx%dx%d", H, W, d.cin); }
  const double px = (double)H * W;
  const double in_px = (d.flags & CONV_UP_IN) ? px / 4 : px, out_px = (d.flags & CONV_POOL_OUT) ? px / 4 : px;
  const double flops = 2.0 * 9 * d.cin * d.cout * px;
  const double bytes = 4.0 * (in_px * d.cin + out_px * d.cout + 9.0 * d.cin * d.cout);
  ProfScope ps(ctx, ln.stream, name, flops, bytes);
  if (spk) HIPCHK(ctx, launch_conv3x3_sp(d, in, out, H, W, ln.stream));
  else if (f16) HIPCHK(ctx, launch_conv3x3_f16(d, in, out, H, W, ln.stream));
  else HIPCHK(ctx, launch_conv3x3(d, in, out, H, W, ln.stream));
  return WCT_OK;
}

size_t max_act_bytes(const Module& m, int H, int W, bool enc) {
  // largest intermediate activation of a module run on an H x W image (enc) / h x w feature (dec).  Per pixel: whole 16-channel chunks --
  // an SP16 tensor (conv_f16_dev.h) is ceil(cout / 16) planes of 64-byte records, more than the cout * 4 bytes of fp32 NHWC wherever cout
  // is no multiple of 16 (8, 24, 40, ...): sized by cout * 4, a layer's SP16 output ran past the buffer
  // (the last layer writes fp32 into the caller's buffer, never SP16)
  auto px_bytes = [&](size_t i) {
    const int cout = m.layers[i].d.cout;
    return (size_t)(i + 1 < m.layers.size() ? (cout + 15) / 16 * 16 : cout) * sizeof(float);
  };
  size_t best = 0;
  int h = H, w = W;
  for (size_t i = 0; i < m.layers.size(); ++i) {
    const auto& l = m.layers[i];
    if (enc) {
      int oh = h, ow = w;
      if (l.pool_after) { oh = h / 2; ow = w / 2; }
      best = std::max(best, (size_t)oh * ow * px_bytes(i));
      h = oh; w = ow;
    } else {
      if (i > 0 && m.layers[i - 1].up_after) { h *= 2; w *= 2; }
      best = std::max(best, (size_t)h * w * px_bytes(i));
    }
  }
  return best;
}
}  // namespace

int encode_impl(wct_ctx* ctx, Lane& ln, int level, const float* img, int H, int W, float* feat_nhwc, int* ho, int* wo) {
  Module& m = ctx->mod[WCT_KIND_ENC][level];
  if (!m.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  if (H < (2 << (level - 1)) || W < (2 << (level - 1)))
    return fail(ctx, WCT_ERR_INVALID, "image %dx%d too small for level %d (reflect padding needs >= 2 samples at every scale)", H, W, level);
  const size_t need = max_act_bytes(m, H, W, true);
  if (int rc = ensure(ctx, ln.actA, need)) return rc;
  if (int rc = ensure(ctx, ln.actB, need)) return rc;
  const float* cur = img;
  int h = H, w = W;
  size_t i0 = 0;
  // SP16 between f16x3 layers: a layer writes SP16 when it is not the last one and its consumer runs in f16x3
  const bool sp = ctx->conv_mode == 1 && ctx->sp;
  bool cur_sp = false;
  auto wants_sp = [&](size_t i) {   // may layer i's output be SP16?
    return sp && i + 1 < m.layers.size() && (m.layers[i].d.cout % 8) == 0 && conv_runs_f16(ctx, m.layers[i + 1].d);
  };
  if (ctx->conv_mode == 1 && ctx->fuse && m.layers.size() >= 2 && conv_fusable_head(m.layers[0].d, m.layers[1].d)) {
    // conv11 + conv12 + pool in one kernel: the 64 B/px intermediate never leaves LDS
    const bool last = m.layers.size() == 2;
    float* dst = last ? feat_nhwc : reinterpret_cast<float*>(ln.actB.p);
    const double px = (double)h * w;
    ConvDesc d1 = m.layers[1].d;
    cur_sp = wants_sp(1);
    if (cur_sp) d1.flags |= CONV_OUT_SP16;
    ProfScope ps(ctx, ln.stream, "enc_head_fused<3-16-16,pool>", 2.0 * 9 * (3 * 16 + 16 * 16) * px, 4.0 * (3 * px + 16 * px / 4));
    HIPCHK(ctx, launch_enc_head(m.layers[0].d, d1, cur, dst, h, w, ln.stream));
    h /= 2; w /= 2;
    cur = dst;
    i0 = 2;
  }
  if (i0 == 0 && ctx->conv_mode == 1 && ctx->fuse && ctx->l1fuse && m.layers.size() == 1 && l1_capable(m.layers[0].d)) {
    // the level-1 encoder on its own (API): same conv11 arithmetic as the fused level-1 kernels
    const ConvDesc& d = m.layers[0].d;
    const double px = (double)h * w;
    ProfScope ps(ctx, ln.stream, "l1_encode<3-24>", 2.0 * 27.0 * d.cout * px, 4.0 * (3 + d.cout) * px);
    HIPCHK(ctx, launch_l1_encode(d, cur, feat_nhwc, h, w, ln.stream));
    i0 = 1;
  }
  for (size_t i = i0; i < m.layers.size(); ++i) {
    const auto& l = m.layers[i];
    const bool last = i + 1 == m.layers.size();
    float* dst = last ? feat_nhwc : reinterpret_cast<float*>((i & 1) ? ln.actB.p : ln.actA.p);
    ConvDesc d = l.d;
    // the image-input conv runs on the fp32 MFMA kernel; it can hand SP16 to an f16x3 consumer all the same
    const bool img_in = (d.flags & CONV_IN_NCHW3) && !(d.flags & CONV_POOL_OUT) && (d.cout & 15) == 0;
    const bool out_sp = (conv_runs_f16(ctx, d) || img_in) && wants_sp(i);
    if (cur_sp) d.flags |= CONV_IN_SP16;
    if (out_sp) d.flags |= CONV_OUT_SP16;
    if (i == 0 && ctx->conv_mode == 1 && ctx->fuse && ctx->in3wide && in3_wide_capable(d)) {
      // 3 -> 64 first conv of the un-pruned encoders: four cout tiles per operand read, exact-fp32 products (default) or f16x3
      const double px = (double)h * w;
      ProfScope ps(ctx, ln.stream, ctx->in3wide == 2 ? "conv3x3_fp32<co=64,in3>" : "conv3x3_f16x3<co=64,in3>", 2.0 * 27.0 * 64 * px, 4.0 * (3 + 64) * px);
      HIPCHK(ctx, launch_in3_wide(d, cur, dst, h, w, out_sp, ctx->in3wide == 2, ln.stream));
      cur = dst;
      cur_sp = out_sp;
      continue;
    }
    if (int rc = run_conv(ctx, ln, d, cur, dst, h, w)) return rc;
    if (l.pool_after) { h /= 2; w /= 2; }
    cur = dst;
    cur_sp = out_sp;
  }
  if (ho) *ho = h;
  if (wo) *wo = w;
  return WCT_OK;
}

// feat NHWC [h*w][C] -> planar image 3 x Ho x Wo.  `first` optionally overrides layer 0 (folded affine).
int decode_impl(wct_ctx* ctx, int level, const float* feat, int h, int w, const ConvDesc* first, float* img) {
  Module& m = ctx->mod[WCT_KIND_DEC][level];
  if (!m.loaded) return fail(ctx, WCT_ERR_STATE, "decoder %d not loaded", level);
  if (h < 2 || w < 2) return fail(ctx, WCT_ERR_INVALID, "feature %dx%d too small (reflect padding needs >= 2 samples)", h, w);
  Lane& ln = ctx->main;
  const size_t need = max_act_bytes(m, h, w, false);
  if (int rc = ensure(ctx, ln.actA, need)) return rc;
  if (int rc = ensure(ctx, ln.actB, need)) return rc;
  const float* cur = feat;
  int ch = h, cw = w;
  const size_t n = m.layers.size();
  const bool sp = ctx->conv_mode == 1 && ctx->sp;
  bool cur_sp = false;
  for (size_t i = 0; i < n; ++i) {
    const auto& l = m.layers[i];
    const bool last = i + 1 == n;
    ConvDesc d = (i == 0 && first) ? *first : l.d;
    if (!ctx->upconv) d.wup16 = nullptr;     // nine-tap form behind the upsamples
    if (i > 0 && m.layers[i - 1].up_after) { ch *= 2; cw *= 2; }
    if (cur_sp) d.flags |= CONV_IN_SP16;
    if (ctx->conv_mode == 1 && ctx->fuse && i + 2 == n && conv_fusable_tail(d, m.layers[i + 1].d)) {
      // conv12 + conv11 in one kernel: the 64 B/px intermediate never leaves LDS
      const double px = (double)ch * cw;
      const double in_px = (d.flags & CONV_UP_IN) ? px / 4 : px;
      ProfScope ps(ctx, ln.stream, "dec_tail_fused<16-16-3>", 2.0 * 9 * (16 * 16 + 16 * 3) * px, 4.0 * (16 * in_px + 3 * px));
      HIPCHK(ctx, launch_dec_tail(d, m.layers[i + 1].d, cur, img, ch, cw, ln.stream));
      break;
    }
    const bool out_sp = sp && !last && conv_runs_f16(ctx, d) && (d.cout % 8) == 0 && conv_runs_f16(ctx, m.layers[i + 1].d);
    if (out_sp) d.flags |= CONV_OUT_SP16;
    float* dst = last ? img : reinterpret_cast<float*>((i & 1) ? ln.actB.p : ln.actA.p);
    if (int rc = run_conv(ctx, ln, d, cur, dst, ch, cw)) return rc;
    cur = dst;
    cur_sp = out_sp;
  }
  return WCT_OK;
}

// ctx->small (doubles): M[512*512] | b[512]     lane.sums (doubles): sum[512] | sumsq[512*512] | info (2 ints)
constexpr size_t SMALL_BYTES = (512 * 512 + 512) * sizeof(double);
constexpr size_t SUMS_BYTES = (512 * 512 + 512) * sizeof(double) + 64;

int sums_view(wct_ctx* ctx, Lane& ln, SumsView& v) {
  if (int rc = ensure(ctx, ln.sums, SUMS_BYTES)) return rc;
  double* p = reinterpret_cast<double*>(ln.sums.p);
  v.sum = p; v.sumsq = p + 512; v.info = reinterpret_cast<int*>(p + 512 + 512 * 512);
  return WCT_OK;
}

int mb_view(wct_ctx* ctx, double** M, double** b) {
  if (int rc = ensure(ctx, ctx->small, SMALL_BYTES)) return rc;
  *M = reinterpret_cast<double*>(ctx->small.p);
  *b = *M + 512 * 512;
  return WCT_OK;
}

// fp32-product moments only where the fp64 sum over blocks averages the blocks' fp32 rounding down far enough: maps of at least this many
// pixels (>= 1024 blocks of 64: relative error of a raw second moment <= ~3e-8).  Smaller maps are cheap in fp64 and are the deep,
// worst-conditioned levels.
constexpr long MOM32_MIN_PIXELS = 65536;
bool mom32_on(const wct_ctx* ctx, long npix) { return ctx->mom32 == 2 || (ctx->mom32 == 1 && npix >= MOM32_MIN_PIXELS); }

int moments_impl(wct_ctx* ctx, Lane& ln, const float* feat, int C, int h, int w, int x0, int x1, double* sum, double* sumsq) {
  if (C < 4 || (C & 3) || C > 512) return fail(ctx, WCT_ERR_INVALID, "moments: C=%d must be a multiple of 4 in [4,512]", C);
  if (h < 1 || x0 < 0 || x1 > w || x1 <= x0) return fail(ctx, WCT_ERR_INVALID, "moments: bad window h=%d w=%d [%d,%d)", h, w, x0, x1);
  const long npix = (long)h * (x1 - x0);
  const size_t wsb = moments_workspace_bytes(C, npix);
  if (int rc = ensure(ctx, ln.wsMom, wsb)) return rc;
  ProfScope ps(ctx, ln.stream, "moments", 2.0 * C * C * npix, 4.0 * C * npix);
  // the arithmetic is chosen on the WHOLE map's pixel count, not the window's: every window of one map shares one arithmetic
  HIPCHK(ctx, launch_moments(feat, C, h, w, x0, x1, sum, sumsq, ln.wsMom.p, ln.wsMom.cap, ln.stream, mom32_on(ctx, (long)h * w)));
  return WCT_OK;
}

namespace {
// May this lane still use the single-launch C = 128 solve?  An aborted solve is correct (the Jacobi net behind every solve repairs it) but costs
// the watchdog's 5 ms plus ~2 ms, silently; the device counts aborts per lane (sat_dev[2 + lane], solve.hip coop_abort), every compute entry
// point mirrors the count to pinned host memory without synchronising, and a lane on which at least three solves and at least a quarter of
// all of them have aborted goes back to the multi-launch schedule for good.  Readable through wct_debug_get ("nscoop_aborts", "nscoop_off").
bool coop_usable(wct_ctx* ctx, Lane& ln) {
  if (ln.coop_off) return false;
  const unsigned seen = ctx->sat_host ? reinterpret_cast<volatile unsigned*>(ctx->sat_host)[2 + (&ln == &ctx->side ? 1 : 0)] : 0u;
  if (seen >= 3u && 4u * seen >= ln.coop_solves) ln.coop_off = true;
  return !ln.coop_off;
}

// The iteration schedule for the inverse square root of the ot transform's B = sym(S cov_c S) (C <= 128; the deflated iteration of wider
// matrices needs none).  B's spectrum is the product of two covariances': on the live block of real 16x features its condition is
// 6.5e5 .. 8.8e8, where the covariance schedule (assumed lower bound 1e-5, 16 scaled / 26 plain steps) runs out of budget
// and every solve would fall into the Jacobi net.  Scaled from an assumed lower bound 1e-10 the iteration takes 17-18 steps for any
// condition up to 1e10 (numpy prototype); a wrong guess costs iterations, never correctness.  32 = the single-launch kernel's limit.
constexpr int OT_MAXIT = 32;
constexpr double OT_GUESS = 1e-10;
}  // namespace

// (n, sum, sumsq) of one feature map -> EigResult in `res` (covariance, Jacobi eigen-decomposition)
// ot_sched: the matrix is the ot transform's B = S cov_c S entering as pseudo-moments (transform_mb) -- its own iteration schedule, never + I
int eig_impl(wct_ctx* ctx, Lane& ln, int C, double n, const double* sum, const double* sumsq, int inverse, DevBuf& res, int* info_dev, bool ot_sched) {
  if (C < 2 || (C & 1) || C > 512) return fail(ctx, WCT_ERR_INVALID, "solve: C=%d must be even and <= 512", C);
  if (n < 2) return fail(ctx, WCT_ERR_INVALID, "solve: unbiased covariance needs >= 2 pixels (n=%g)", n);
  if (int rc = ensure(ctx, res, eig_result_bytes(C))) return rc;
  if (int rc = ensure(ctx, ln.wsEig, eig_workspace_bytes(C))) return rc;
  // timing experiment (debug key "eig_skip" = N): after N solves the launches are left out and `res` keeps what the last solve
  // of this lane / level left there -- on repeated identical frames the same numbers, so the step's wall time minus the matrix
  // functions' exposed time can be read off (tools/experiments/ab_eig_skip.sh)
  if (ctx->eig_skip > 0 && ++ctx->eig_calls > ctx->eig_skip) return WCT_OK;
  ProfScope ps(ctx, ln.stream, inverse ? "matfun_invsqrt" : "matfun_sqrt", 0, 0);
  int* defer = nullptr;
  if (ctx->defer_big && eig_is_big(C, ctx->wide_model) && ctx->ok_n < OK_SLOTS) defer = ctx->ok_log + ctx->ok_n++;
  const bool coop_ok = ctx->nscoop && coop_usable(ctx, ln);
  bool coop_used = false;
  HIPCHK(ctx, launch_eig(C, n, sum, sumsq, inverse, reinterpret_cast<double*>(res.p), info_dev, ln.wsEig.p, ln.wsEig.cap, ln.stream,
                         (inverse && ctx->numpy_variant && !ot_sched) ? 1.0 : 0.0, ctx->wide_model, defer, coop_ok ? (ln.xcd | (ctx->nscoop == 2 ? 16 : 0)) : -1, ln.coop, &ln.coop_epoch,
                         ctx->sat_dev + 2 + (&ln == &ctx->side ? 1 : 0), &coop_used, ot_sched ? OT_MAXIT : 0, ot_sched ? OT_GUESS : -1.0));
  if (coop_used) ++ln.coop_solves;
  return WCT_OK;
}

int assemble_impl(wct_ctx* ctx, int C, const DevBuf& eig_c, const DevBuf& eig_s, double alpha, double* M, double* b) {
  if (int rc = ensure(ctx, ctx->wsAsm, assemble_workspace_bytes(C))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "assemble_Mb", 0, 0);
  HIPCHK(ctx, launch_assemble(C, reinterpret_cast<const double*>(eig_c.p), reinterpret_cast<const double*>(eig_s.p), alpha, 1e-10,
                              M, b, ctx->wsAsm.p, ctx->wsAsm.cap, ctx->main.stream));
  return WCT_OK;
}

// Content moments + a style EigResult (F = cov_s^(1/2), mu_s) -> (M, b) of the transform `mode` (include/wct_hip_transform.h), on the
// main lane: THE place where a level's map is made.  info_dev[0] = how the content-side matrix function was solved.  style_ready (may
// be null): the event behind which eig_s is complete; waited for as late as the mode allows -- wct solves the content side first.
int transform_mb(wct_ctx* ctx, int mode, int C, double n, const double* sum, const double* sumsq, const DevBuf& eig_s, double alpha, double* M,
                 double* b, int* info_dev, hipEvent_t style_ready) {
  Lane& ln = ctx->main;
  if (mode == WCT_TRANSFORM_WCT) {
    if (int rc = eig_impl(ctx, ln, C, n, sum, sumsq, 1, ctx->eigC, info_dev)) return rc;
    if (style_ready) HIPCHK(ctx, hipStreamWaitEvent(ln.stream, style_ready, 0));
    return assemble_impl(ctx, C, ctx->eigC, eig_s, alpha, M, b);
  }
  if (mode != WCT_TRANSFORM_OT && mode != WCT_TRANSFORM_ADAIN) return fail(ctx, WCT_ERR_INVALID, "transform: mode %d outside 0..2", mode);
  if (C < 2 || (C & 1) || C > 512) return fail(ctx, WCT_ERR_INVALID, "solve: C=%d must be even and <= 512", C);
  if (n < 2) return fail(ctx, WCT_ERR_INVALID, "solve: unbiased covariance needs >= 2 pixels (n=%g)", n);
  if (style_ready) HIPCHK(ctx, hipStreamWaitEvent(ln.stream, style_ready, 0));
  const size_t cc = (size_t)C * C;
  const double* es = reinterpret_cast<const double*>(eig_s.p);
  const double *S = es + eig_result_F_offset(C), *mu_s = es + cc + C;
  if (mode == WCT_TRANSFORM_ADAIN) {
    ProfScope ps(ctx, ln.stream, "adain_assemble", 0, 0);
    HIPCHK(ctx, launch_adain_assemble(C, alpha, WCT_ADAIN_EPS, S, mu_s, n, sum, sumsq, M, b, info_dev, ln.stream));
    return WCT_OK;
  }
  if (int rc = ensure(ctx, ctx->trBuf, ot_workspace_bytes(C))) return rc;
  double* B = reinterpret_cast<double*>(ctx->trBuf.p);
  double *tmp = B + cc, *zeros = tmp + cc;
  {
    ProfScope ps(ctx, ln.stream, "ot_sandwich", 8.0 * C * cc, 0);
    HIPCHK(ctx, launch_ot_sandwich(C, n, sum, sumsq, S, B, zeros, tmp, ln.stream));
  }
  // B^(-1/2) into eigC's F: the pseudo-moments n = 2, sum = 0, sumsq = B give cov = (B - 2 * 0 * 0) / (2 - 1) = B exactly
  if (int rc = eig_impl(ctx, ln, C, 2.0, zeros, B, 1, ctx->eigC, info_dev, true)) return rc;
  ProfScope ps(ctx, ln.stream, "ot_assemble", 4.0 * C * cc, 0);
  HIPCHK(ctx, launch_ot_assemble(C, alpha, S, mu_s, reinterpret_cast<const double*>(ctx->eigC.p) + eig_result_F_offset(C), n, sum, tmp, M, b, ln.stream));
  return WCT_OK;
}

namespace {
int fold_impl(wct_ctx* ctx, int level, const double* M, const double* b, ConvDesc& out) {
  Module& m = ctx->mod[WCT_KIND_DEC][level];
  if (!m.loaded) return fail(ctx, WCT_ERR_STATE, "decoder %d not loaded", level);
  const LayerDev& l = m.layers[0];
  hipStream_t st = ctx->main.stream;
  const size_t wbytes = (size_t)l.d.cin_chunks * 36 * l.d.cout_pad * 4 * sizeof(float);
  if (int rc = ensure(ctx, ctx->foldW, wbytes + l.d.cout_pad * sizeof(float))) return rc;
  float* wpk = reinterpret_cast<float*>(ctx->foldW.p);
  float* bias = wpk + wbytes / sizeof(float);
  ProfScope ps(ctx, st, "fold_affine", 0, 0);
  out = l.d;
  out.wpk = wpk;
  out.bias = bias;
  out.wpk16 = nullptr;
  out.wph16 = nullptr;
  out.inv_scale_ptr = nullptr;
  if (ctx->conv_mode == 1) {
    const int taps = l.d.cout_pad == 16 ? 10 : 9;
    const size_t b16 = conv_f16_weight_bytes(l.d.cin, l.d.cout_pad, taps);
    // a single-conv decoder (level 1: 24 -> 3) is also needed block-packed, for l1_decode_kernel
    const bool phase = (l.d.flags & CONV_OUT_NCHW3) && l.d.cout_pad == 16 && l.d.cout == 3;
    const size_t bph = phase ? conv_phase_weight_bytes(l.d.cin) : 0;
    if (int rc = ensure(ctx, ctx->foldW16, b16 + 64 + bph)) return rc;
    char* base = reinterpret_cast<char*>(ctx->foldW16.p);
    float* inv = reinterpret_cast<float*>(base + b16);
    unsigned* maxbits = reinterpret_cast<unsigned*>(base + b16 + 16);
    if (l.fold_rows && ctx->foldgemm) HIPCHK(ctx, launch_fold_gemm(l.fold_rows, l.bias_raw, l.d.cout, l.d.cin, l.d.cout_pad, M, b, wpk, bias, maxbits, st));
    else HIPCHK(ctx, launch_fold_affine(l.w_oihw, l.bias_raw, l.d.cout, l.d.cin, l.d.cout_pad, M, b, wpk, bias, maxbits, st));
    HIPCHK(ctx, launch_split_pack(wpk, l.d.cin, l.d.cout_pad, taps, maxbits, base, inv, st, true));
    out.wpk16 = base;
    out.inv_scale_ptr = inv;
    out.wph16 = nullptr;
    if (phase) {
      HIPCHK(ctx, launch_split_pack_phase(wpk, l.d.cin, maxbits, base + b16 + 64, st));
      out.wph16 = base + b16 + 64;
    }
  } else {
    if (l.fold_rows && ctx->foldgemm) HIPCHK(ctx, launch_fold_gemm(l.fold_rows, l.bias_raw, l.d.cout, l.d.cin, l.d.cout_pad, M, b, wpk, bias, nullptr, st));
    else HIPCHK(ctx, launch_fold_affine(l.w_oihw, l.bias_raw, l.d.cout, l.d.cin, l.d.cout_pad, M, b, wpk, bias, nullptr, st));
  }
  return WCT_OK;
}
}  // namespace

bool fast_fold_level(const wct_ctx* ctx, int level) {
  const Module& m = ctx->mod[WCT_KIND_DEC][level];
  return ctx->fastfold && m.loaded && m.layers[0].w_oihw && fold_fast_capable(m.layers[0].d.cin);
}

// the style-side part of the fast fold for `level`, on `st`, from the style EigResult in ctx->eigS[level] (F = cov_s^(1/2), mu_s)
// Everything that rewrites a slot ends here, so this is also where the slot stops counting as rotated (wct_style_diversify sets the mark
// again behind its own call).
int style_fold(wct_ctx* ctx, int level, hipStream_t st) {
  ctx->fold_ready[level] = false;
  ctx->rotated[level] = false;
  if (!fast_fold_level(ctx, level)) return WCT_OK;
  const LayerDev& l = ctx->mod[WCT_KIND_DEC][level].layers[0];
  const size_t C = l.d.cin, cc = C * C;
  if (int rc = ensure(ctx, ctx->foldS[level], fold_style_doubles(l.d.cout, l.d.cin) * sizeof(double))) return rc;
  const double* res = reinterpret_cast<const double*>(ctx->eigS[level].p);
  ProfScope ps(ctx, st, "fold_style", 0, 0);
  HIPCHK(ctx, launch_fold_style(l.w_oihw, l.d.cout, l.d.cin, res + eig_result_F_offset(C), res + cc + C, reinterpret_cast<double*>(ctx->foldS[level].p), st));
  ctx->fold_ready[level] = true;
  return WCT_OK;
}

// content side: cov_c^(-1/2) and mu_c (ctx->eigC) + the level's style-side part -> the folded first decoder conv, no M / b
int fold_fast_impl(wct_ctx* ctx, int level, double alpha, ConvDesc& out) {
  Module& m = ctx->mod[WCT_KIND_DEC][level];
  const LayerDev& l = m.layers[0];
  hipStream_t st = ctx->main.stream;
  const size_t C = l.d.cin, cc = C * C;
  const size_t wbytes = (size_t)l.d.cin_chunks * 36 * l.d.cout_pad * 4 * sizeof(float);
  if (int rc = ensure(ctx, ctx->foldW, wbytes + l.d.cout_pad * sizeof(float))) return rc;
  float* wpk = reinterpret_cast<float*>(ctx->foldW.p);
  float* bias = wpk + wbytes / sizeof(float);
  const int taps = l.d.cout_pad == 16 ? 10 : 9;
  const size_t b16 = conv_f16_weight_bytes(l.d.cin, l.d.cout_pad, taps);
  const bool phase = (l.d.flags & CONV_OUT_NCHW3) && l.d.cout_pad == 16 && l.d.cout == 3;
  const size_t bph = phase ? conv_phase_weight_bytes(l.d.cin) : 0;
  if (int rc = ensure(ctx, ctx->foldW16, b16 + 64 + bph + 512 * sizeof(unsigned))) return rc;
  char* base = reinterpret_cast<char*>(ctx->foldW16.p);
  float* inv = reinterpret_cast<float*>(base + b16);
  unsigned* rowmax = reinterpret_cast<unsigned*>(base + b16 + 64 + bph);
  const double* resc = reinterpret_cast<const double*>(ctx->eigC.p);
  out = l.d;
  out.wpk = wpk; out.bias = bias; out.wph16 = nullptr;
  {
    ProfScope ps(ctx, st, "fold_affine", 0, 0);
    HIPCHK(ctx, launch_fold_fast(l.w_oihw, l.bias_raw, l.d.cout, l.d.cin, l.d.cout_pad, reinterpret_cast<const double*>(ctx->foldS[level].p),
                                 resc + eig_result_F_offset(C), resc + cc + C, alpha, wpk, bias, rowmax, st));
    HIPCHK(ctx, launch_split_pack(wpk, l.d.cin, l.d.cout_pad, taps, rowmax, base, inv, st, true, l.d.cout_pad));
    out.wpk16 = base;
    out.inv_scale_ptr = inv;
    if (phase) {
      HIPCHK(ctx, launch_split_pack_phase(wpk, l.d.cin, rowmax, base + b16 + 64, st, l.d.cout_pad));
      out.wph16 = base + b16 + 64;
    }
  }
  return WCT_OK;
}

void level_dims(int level, int H, int W, int& h, int& w) {
  h = H; w = W;
  for (int i = 1; i < level; ++i) { h /= 2; w /= 2; }
}

// level 1 of the 16x cascade without relu1_1 in HBM: single-conv encoder (3 -> 17..24) and single-conv decoder (-> 3).  Wider level-1
// encoders (25..32) take the layer-wise path: the fused moments and decoder kernels cover 24 channels only (l1_fusable)
bool l1_fused(const wct_ctx* ctx, int level) {
  if (ctx->conv_mode != 1 || !ctx->fuse || !ctx->l1fuse) return false;
  const Module& me = ctx->mod[WCT_KIND_ENC][level];
  const Module& md = ctx->mod[WCT_KIND_DEC][level];
  if (!me.loaded || !md.loaded || me.layers.size() != 1 || md.layers.size() != 1) return false;
  const ConvDesc& e = me.layers[0].d;
  const ConvDesc& d = md.layers[0].d;
  return l1_fusable(e) && d.cin == e.cout && d.cout == 3 && d.cout_pad == 16 && d.cin_chunks == 2 && (d.flags & CONV_OUT_NCHW3);
}

int l1_moments_impl(wct_ctx* ctx, Lane& ln, int level, const float* img, int H, int W, int x0, int x1, double* sum, double* sumsq) {
  const ConvDesc& e = ctx->mod[WCT_KIND_ENC][level].layers[0].d;
  if (H < 2 || W < 2 || x0 < 0 || x1 > W || x1 <= x0) return fail(ctx, WCT_ERR_INVALID, "moments: bad window %dx%d [%d,%d)", H, W, x0, x1);
  if (int rc = ensure(ctx, ln.wsMom, l1_moments_workspace_bytes())) return rc;
  const double px = (double)H * W;
  ProfScope ps(ctx, ln.stream, "l1_moments_fused<3-24>", 2.0 * (27.0 * e.cout + (double)e.cout * e.cout) * px, 12.0 * px);
  HIPCHK(ctx, launch_l1_moments(e, img, H, W, x0, x1, sum, sumsq, ln.wsMom.p, ln.wsMom.cap, ln.stream, mom32_on(ctx, (long)H * W)));
  return WCT_OK;
}

int l1_decode_impl(wct_ctx* ctx, int level, const float* img, int H, int W, const ConvDesc& first, float* out) {
  const ConvDesc& e = ctx->mod[WCT_KIND_ENC][level].layers[0].d;
  const double px = (double)H * W;
  ProfScope ps(ctx, ctx->main.stream, "l1_decode_fused<3-24-3>", 2.0 * 27.0 * e.cout * px * 2, 24.0 * px);
  HIPCHK(ctx, launch_l1_decode(e, first, img, out, H, W, ctx->main.stream));
  return WCT_OK;
}

// style side of one level on the SIDE lane: sF = encoder(styleImg) (WCT.py:100), its moments and eigen-decomposition.
// Independent of the content, so it is enqueued first and overlaps the content side.  Leaves eigS[level] + ev_style[level].
// slot k >= 0 (the K-style calls): into eigR[k][level], and no fold -- their maps are applied to the features or blended into eigS
// first, not folded into the decoder from here.
int style_side(wct_ctx* ctx, int level, const float* style, int Hs, int Ws, int slot) {
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  const int C = me.layers.back().d.cout;
  int hs, ws;
  level_dims(level, Hs, Ws, hs, ws);
  Lane& ln = ctx->overlap ? ctx->side : ctx->main;
  if (int rc = ensure(ctx, ctx->featS, (size_t)hs * ws * C * sizeof(float))) return rc;
  SumsView sv;
  if (int rc = sums_view(ctx, ln, sv)) return rc;
  float* fS = reinterpret_cast<float*>(ctx->featS.p);
  if (l1_fused(ctx, level)) {
    if (int rc = l1_moments_impl(ctx, ln, level, style, Hs, Ws, 0, Ws, sv.sum, sv.sumsq)) return rc;
  } else {
    if (int rc = encode_impl(ctx, ln, level, style, Hs, Ws, fS, nullptr, nullptr)) return rc;
    if (int rc = moments_impl(ctx, ln, fS, C, hs, ws, 0, ws, sv.sum, sv.sumsq)) return rc;
  }
  DevBuf& res = slot < 0 ? ctx->eigS[level] : ctx->eigR[slot][level];
  if (int rc = eig_impl(ctx, ln, C, (double)hs * ws, sv.sum, sv.sumsq, 0, res, sv.info + 1)) return rc;
  if (slot < 0)
    if (int rc = style_fold(ctx, level, ln.stream)) return rc;    // (W Ss), off the content side's critical path
  HIPCHK(ctx, hipEventRecord(ctx->ev_style[level], ln.stream));
  return WCT_OK;
}

// the side lane may start once everything already enqueued on the caller's stream (e.g. the producer of the
// style image) has run
int fork_side(wct_ctx* ctx) {
  HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ctx->main.stream));
  HIPCHK(ctx, hipStreamWaitEvent(ctx->side.stream, ctx->ev_fork, 0));
  return WCT_OK;
}

// content side of one level on the MAIN lane; expects style_side(level) to have been enqueued
int content_side(wct_ctx* ctx, int level, const float* content, int H, int W, float alpha, float* out, int* Ho, int* Wo) {
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  const int C = me.layers.back().d.cout;
  int h, w;
  level_dims(level, H, W, h, w);
  Lane& ln = ctx->main;
  if (int rc = ensure(ctx, ctx->featC, (size_t)h * w * C * sizeof(float))) return rc;
  SumsView sv;
  if (int rc = sums_view(ctx, ln, sv)) return rc;
  double *M, *b;
  if (int rc = mb_view(ctx, &M, &b)) return rc;
  float* fC = reinterpret_cast<float*>(ctx->featC.p);
  // cF = encoder(contentImg)                                  (WCT.py:101)
  const bool l1 = l1_fused(ctx, level);
  if (l1) {
    if (int rc = l1_moments_impl(ctx, ln, level, content, H, W, 0, W, sv.sum, sv.sumsq)) return rc;
  } else {
    if (int rc = encode_impl(ctx, ln, level, content, H, W, fC, nullptr, nullptr)) return rc;
    if (int rc = moments_impl(ctx, ln, fC, C, h, w, 0, w, sv.sum, sv.sumsq)) return rc;
  }
  // video mode: the sums of this frame become the sums tracked over the clip's frames, in place, before either solve below sees them
  if (ctx->track)
    if (int rc = clip_track_level(ctx, ctx->track, level, C, sv.sum, sv.sumsq)) return rc;
  // csF = wct.transform(cF, sF, csF, alpha)                  (WCT.py:104) -- as an affine map
  // Img = decoder(csF)                                       (WCT.py:105) -- M, b folded into the first conv
  ConvDesc first;
  if (ctx->transform == WCT_TRANSFORM_WCT && ctx->conv_mode == 1 && ctx->fold_ready[level] && fast_fold_level(ctx, level)) {
    if (int rc = eig_impl(ctx, ln, C, (double)h * w, sv.sum, sv.sumsq, 1, ctx->eigC, sv.info)) return rc;
    HIPCHK(ctx, hipStreamWaitEvent(ln.stream, ctx->ev_style[level], 0));
    if (int rc = fold_fast_impl(ctx, level, alpha, first)) return rc;      // straight from cov_c^(-1/2): no T, M, b on the critical path
  } else {
    if (int rc = transform_mb(ctx, ctx->transform, C, (double)h * w, sv.sum, sv.sumsq, ctx->eigS[level], alpha, M, b, sv.info, ctx->ev_style[level])) return rc;
    if (int rc = fold_impl(ctx, level, M, b, first)) return rc;
  }
  if (l1) {
    if (int rc = l1_decode_impl(ctx, level, content, H, W, first, out)) return rc;
  } else {
    if (int rc = decode_impl(ctx, level, fC, h, w, &first, out)) return rc;
  }
  if (Ho) *Ho = h << (level - 1);
  if (Wo) *Wo = w << (level - 1);
  return WCT_OK;
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace wct_host

// =====================================================================================================
extern "C" {

int wct_version(void) { return 1; }

int wct_create(int device, wct_ctx** out) {
  if (!out) return WCT_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return WCT_ERR_HIP;
  wct_ctx* c = new (std::nothrow) wct_ctx();
  if (!c) return WCT_ERR_NOMEM;
  c->device = device;
  WCT_GUARD(c);
  if (const char* m = wct_debug_env("WCT_CONV_MODE")) c->conv_mode = (m[0] == '0' || !strcmp(m, "fp32")) ? 0 : 1;
  if (const char* m = wct_debug_env("WCT_OVERLAP")) c->overlap = m[0] != '0';
  if (const char* m = wct_debug_env("WCT_FUSE")) c->fuse = m[0] != '0';
  if (const char* m = wct_debug_env("WCT_SP")) c->sp = m[0] != '0';
  if (const char* m = wct_debug_env("WCT_L1FUSE")) c->l1fuse = m[0] != '0';
  static std::atomic<int> next_xcd{0};
  c->main.xcd = next_xcd.fetch_add(2) & 7;
  c->side.xcd = (c->main.xcd + 1) & 7;
  bool ok = hipStreamCreateWithFlags(&c->side.stream, hipStreamNonBlocking) == hipSuccess;
  for (Lane* ln : {&c->main, &c->side})
    ok = ok && hipMalloc(reinterpret_cast<void**>(&ln->coop), 64) == hipSuccess && hipMemset(ln->coop, 0, 64) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming) == hipSuccess;
  for (int l = 1; l <= 5 && ok; ++l)
    ok = hipEventCreateWithFlags(&c->ev_style[l], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&c->ev_smom[l], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->ev_sar[l], hipEventDisableTiming) == hipSuccess;
  ok = ok && hipMalloc(reinterpret_cast<void**>(&c->sat_dev), 256) == hipSuccess && hipMemset(c->sat_dev, 0, 256) == hipSuccess;
  ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->sat_host), 64, hipHostMallocDefault) == hipSuccess;
  ok = ok && hipMalloc(reinterpret_cast<void**>(&c->ok_log), 64 * sizeof(int)) == hipSuccess;
  ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->ok_host), 64 * sizeof(int), hipHostMallocDefault) == hipSuccess;
  if (ok) memset(c->sat_host, 0, 64);     // all 16 words: [2 + lane] are the single-launch solves' abort counts coop_usable() reads
  if (!ok) { wct_destroy(c); return WCT_ERR_HIP; }
  *out = c;
  return WCT_OK;
}

void wct_destroy(wct_ctx* ctx) {
  if (!ctx) return;
  {
  WCT_GUARD(ctx);
  (void)hipStreamSynchronize(ctx->main.stream);
  (void)hipStreamSynchronize(ctx->side.stream);
  prof_collect(ctx);
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < 6; ++l) free_module(ctx->mod[k][l]);
  ctx->each_buf([](DevBuf& b, Lane*, bool) { release(b); });
  for (Lane* ln : {&ctx->main, &ctx->side}) {
    if (ln->coop) (void)hipFree(ln->coop);
    ln->coop = nullptr;
  }
  for (ResizeAxis& a : ctx->rsz_axes) (void)hipFree(a.bounds);
  ctx->rsz_axes.clear();
  for (int l = 0; l < 6; ++l) {
    if (ctx->ev_style[l]) (void)hipEventDestroy(ctx->ev_style[l]);
    if (ctx->ev_smom[l]) (void)hipEventDestroy(ctx->ev_smom[l]);
    if (ctx->ev_sar[l]) (void)hipEventDestroy(ctx->ev_sar[l]);
  }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->ev_switch) (void)hipEventDestroy(ctx->ev_switch);
  if (ctx->reg_hist_host) (void)hipHostFree(ctx->reg_hist_host);
  if (ctx->blend_host) (void)hipHostFree(ctx->blend_host);
  if (ctx->gd_hist_host) (void)hipHostFree(ctx->gd_hist_host);

  if (ctx->side.stream) (void)hipStreamDestroy(ctx->side.stream);
  if (ctx->sat_dev) (void)hipFree(ctx->sat_dev);
  release_comm(ctx);
  if (ctx->sat_host) (void)hipHostFree(ctx->sat_host);
  if (ctx->ok_log) (void)hipFree(ctx->ok_log);
  if (ctx->ok_host) (void)hipHostFree(ctx->ok_host);
  }
  delete ctx;
}

const char* wct_last_error(const wct_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int wct_set_stream(wct_ctx* ctx, void* s) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  hipStream_t ns = reinterpret_cast<hipStream_t>(s);
  if (ns == ctx->main.stream) return WCT_OK;
  // Calls issued under two streams share every workspace of the context: the new stream waits for whatever the context has enqueued
  // on the old one (the side lane orders itself: it is one stream, and forks from / joins the caller's stream by events).  The old
  // stream must still exist; if it cannot take the event the switch goes ahead unordered, as it always did.
  // A stream that is being captured into a graph takes no dependency on work outside the capture (the caller synchronised before it began).
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(ns, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
  if (cap == hipStreamCaptureStatusNone) {
    if (ctx->ev_switch && hipEventRecord(ctx->ev_switch, ctx->main.stream) == hipSuccess) HIPCHK(ctx, hipStreamWaitEvent(ns, ctx->ev_switch, 0));
    else (void)hipGetLastError();
  }
  ctx->main.stream = ns;
  return WCT_OK;
}

int wct_sync(wct_ctx* ctx) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  unsigned n = 0;
  HIPCHK(ctx, hipMemcpy(&n, ctx->sat_dev, sizeof n, hipMemcpyDeviceToHost));
  if (n) {
    // reported ONCE and cleared: a later WCT_ERR_RANGE then means a later clamp, not a stale flag (the total stays readable
    // through wct_saturation_count until this point only)
    HIPCHK(ctx, hipMemset(ctx->sat_dev, 0, sizeof n));
    range_host_set(ctx, 0u);
    return fail(ctx, WCT_ERR_RANGE, "%u thread(s) clamped an activation to the f16x3 range (|x| > 65504, or NaN) since the last report: results "
                "deviate from the fp32 reference; use conv mode 0 (exact fp32) for these weights / inputs.  The flag is now cleared", n);
  }
  return WCT_OK;
}

int wct_saturation_count(wct_ctx* ctx, int reset, unsigned long long* count) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  unsigned n = 0;
  HIPCHK(ctx, hipMemcpy(&n, ctx->sat_dev, sizeof n, hipMemcpyDeviceToHost));
  if (reset && n) HIPCHK(ctx, hipMemset(ctx->sat_dev, 0, sizeof n));
  range_host_set(ctx, reset ? 0u : n);
  if (count) *count = n;
  return WCT_OK;
}

int wct_range_poll(wct_ctx* ctx, unsigned long long* count) {
  if (!ctx || !count) return WCT_ERR_INVALID;
  const volatile unsigned* m = reinterpret_cast<volatile unsigned*>(ctx->sat_host);
  *count = m ? std::max(m[0], m[SAT_SIDE_WORD]) : 0u;     // the caller's stream's mirror and the side lane's (range_readback_side)
  return WCT_OK;
}

int wct_range_flag_f64(wct_ctx* ctx, double* flag_dev) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!flag_dev) return fail(ctx, WCT_ERR_INVALID, "range_flag_f64: NULL pointer");
  HIPCHK(ctx, launch_counter_to_f64(ctx->sat_dev, flag_dev, ctx->main.stream));
  return WCT_OK;
}

int wct_debug_set(wct_ctx* ctx, const char* key, double value) {
  if (!ctx || !key) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  const int v = value != 0.0;
  if (!strcmp(key, "fuse")) ctx->fuse = v;
  else if (!strcmp(key, "sp")) ctx->sp = v;
  else if (!strcmp(key, "l1fuse")) ctx->l1fuse = v;
  else if (!strcmp(key, "u8fuse")) ctx->u8fuse = v;
  else if (!strcmp(key, "upconv")) ctx->upconv = v;
  else if (!strcmp(key, "fastfold")) ctx->fastfold = v;
  else if (!strcmp(key, "interleave")) ctx->interleave = v;
  else if (!strcmp(key, "foldgemm")) ctx->foldgemm = v;
  else if (!strcmp(key, "prof_forms")) ctx->prof_forms = v;
  else if (!strcmp(key, "bgrid_lds")) ctx->bgrid_lds = v;       // 0: wct_bgrid_slice reads the grid from global memory in every tile (same bits)
  else if (!strcmp(key, "nscoop")) ctx->nscoop = (int)value;      // 0: multi-launch, 1: single launch, 2: single launch with an injected placement fault
  else if (!strcmp(key, "mom32")) ctx->mom32 = (int)value;       // 0 / 1 / 2, see wct_ctx
  else if (!strcmp(key, "in3wide")) ctx->in3wide = (int)value;   // 2 / 1 / 0, see wct_ctx
  else if (!strcmp(key, "poison")) {
    // -1: off; 0..255: fill every allocated scratch buffer with this byte NOW (both lanes synchronised) and every later ensure()
    // allocation too, until turned off.  State survives (wct_ctx::each_buf).
    if (value < 0) { ctx->poison = -1; return WCT_OK; }
    if (value > 255 || value != (double)(int)value) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'poison' takes a byte 0..255, or -1 for off");
    ctx->poison = (int)value;
    return poison_scratch(ctx, ctx->poison);
  }
  else if (!strcmp(key, "eig_skip")) {
    // MEASUREMENT ONLY: solves are left out and stale results reused -- wrong pictures by design; refused outside a debug run
    if (!getenv("WCT_DEBUG")) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'eig_skip' produces wrong results by design (timing experiment); set WCT_DEBUG to allow it");
    ctx->eig_skip = (int)value; ctx->eig_calls = 0;
  }
  else if (!strcmp(key, "swap_key_chunk")) {
    // keys per launch of wct_patch_match (0: the default WCT_SWAP_KEY_CHUNK).  Results do not depend on it; a tiny chunk makes a match of a
    // large map thousands of launches, so it is a test / measurement key
    if (!getenv("WCT_DEBUG")) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'swap_key_chunk' is a test / measurement key; set WCT_DEBUG to allow it");
    if (value < 0 || value > 2147483647.0 || value != (double)(long)value) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'swap_key_chunk' takes a key count >= 1, or 0 for the default");
    ctx->swap_key_chunk = (int)value;
    return WCT_OK;
  }
  else if (!strcmp(key, "attn_query_chunk")) {
    // queries per launch of wct_attn_stats (0: the default WCT_ATTN_QUERY_CHUNK).  Results do not depend on it: a test / measurement key
    if (!getenv("WCT_DEBUG")) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'attn_query_chunk' is a test / measurement key; set WCT_DEBUG to allow it");
    if (value < 0 || value > 2147483647.0 || value != (double)(long)value) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'attn_query_chunk' takes a query count >= 1, or 0 for the default");
    ctx->attn_query_chunk = (int)value;
    return WCT_OK;
  }
  else if (!strcmp(key, "clip_channels")) {
    // TEST KEY (include/wct_hip_video.h): clips created from now on hold `value` channels at every level instead of the loaded encoders'
    // (0: off) -- the tracking step on its own at widths no loadable encoder has; wct_stylize_clip refuses such a clip
    if (value < 0 || value > 512 || value != (double)(int)value) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'clip_channels' takes 1 .. 512, or 0 for off");
    ctx->clip_channels = (int)value;
    return WCT_OK;
  }
  else if (!strcmp(key, "shard_emulate")) {
    // MEASUREMENT ONLY (bench.py passes.cfg4_rank_sim): this context, holding a ONE-rank communicator, runs wct_stylize_sharded with the
    // geometry of rank (value % 100) of a (value / 100)-rank job; every peer is itself (a received margin is the equally wide block it
    // sends the other way), the all-reduces see its own sums only -- what ONE rank of the job executes, with other numbers.  0: off.
    if (!getenv("WCT_DEBUG")) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'shard_emulate' produces wrong results by design (timing experiment); set WCT_DEBUG to allow it");
    const int v = (int)value, world = v / 100, rank = v % 100;
    if (v == 0) { if (ctx->shard_emulate) { ctx->shard_emulate = false; ctx->comm_ranks = 1; ctx->comm_rank = 0; } return WCT_OK; }
    if (!ctx->coll_set || (ctx->comm_ranks != 1 && !ctx->shard_emulate)) return fail(ctx, WCT_ERR_STATE, "debug_set: 'shard_emulate' needs a ONE-rank communicator on the context");
    if (world < 2 || rank >= world) return fail(ctx, WCT_ERR_INVALID, "debug_set: 'shard_emulate' = 100 * ranks + rank");
    ctx->shard_emulate = true; ctx->comm_ranks = world; ctx->comm_rank = rank;
    return WCT_OK;
  }
  else if (!strcmp(key, "side_priority")) {
    // priority of the style-side stream relative to the default: 0 = default, 1 = lowest (style kernels only fill the
    // content cascade's gaps), -1 = highest
    int lo = 0, hi = 0;
    HIPCHK(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));   // lo = least priority (numerically largest)
    HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
    hipStream_t ns = nullptr;
    HIPCHK(ctx, hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, value > 0 ? lo : (value < 0 ? hi : 0)));
    (void)hipStreamDestroy(ctx->side.stream);
    ctx->side.stream = ns;
    return WCT_OK;
  }
  else return fail(ctx, WCT_ERR_INVALID, "debug_set: unknown key '%s' (fuse, sp, l1fuse, u8fuse, upconv, fastfold, interleave, foldgemm, nscoop, in3wide, mom32, eig_skip, side_priority, poison, prof_forms, swap_key_chunk, attn_query_chunk, clip_channels, bgrid_lds)", key);
  HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  return WCT_OK;
}

int wct_debug_get(wct_ctx* ctx, const char* key, double* value) {
  if (!ctx || !key || !value) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!strcmp(key, "nscoop_aborts") || !strcmp(key, "nscoop_solves") || !strcmp(key, "nscoop_off")) {
    if (!strcmp(key, "nscoop_solves")) { *value = (double)ctx->main.coop_solves + (double)ctx->side.coop_solves; return WCT_OK; }
    if (!strcmp(key, "nscoop_off")) { (void)coop_usable(ctx, ctx->main); (void)coop_usable(ctx, ctx->side); *value = (ctx->main.coop_off ? 1 : 0) + (ctx->side.coop_off ? 2 : 0); return WCT_OK; }
    HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
    unsigned n[2] = {0u, 0u};
    HIPCHK(ctx, hipMemcpy(n, ctx->sat_dev + 2, sizeof n, hipMemcpyDeviceToHost));
    if (ctx->sat_host) { reinterpret_cast<volatile unsigned*>(ctx->sat_host)[2] = n[0]; reinterpret_cast<volatile unsigned*>(ctx->sat_host)[3] = n[1]; }
    *value = (double)n[0] + (double)n[1];
    return WCT_OK;
  }
  if (!strcmp(key, "ws_allocs")) { *value = (double)ctx->ws_allocs; return WCT_OK; }
  if (!strcmp(key, "ws_bytes")) {
    size_t total = 0;
    ctx->each_buf([&](DevBuf& b, Lane*, bool) { total += b.cap; });
    *value = (double)total;
    return WCT_OK;
  }
  return fail(ctx, WCT_ERR_INVALID, "debug_get: unknown key '%s' (nscoop_aborts, nscoop_solves, nscoop_off, ws_allocs, ws_bytes)", key);
}

int wct_encode(wct_ctx* ctx, int level, const float* img, int H, int W, float* feat, int layout) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !img || !feat || H < 1 || W < 1) return fail(ctx, WCT_ERR_INVALID, "encode: bad arguments");
  if (layout == WCT_LAYOUT_NHWC) {
    if (int rc = encode_impl(ctx, ctx->main, level, img, H, W, feat, nullptr, nullptr)) return rc;
    return range_readback(ctx);
  }
  if (layout != WCT_LAYOUT_NCHW) return fail(ctx, WCT_ERR_INVALID, "encode: bad layout %d", layout);
  int C, h, w;
  if (int rc = wct_feature_shape(ctx, level, H, W, &C, &h, &w)) return fail(ctx, rc, "encoder %d not loaded", level);
  if (int rc = ensure(ctx, ctx->tmpT, (size_t)h * w * C * sizeof(float))) return rc;
  if (int rc = encode_impl(ctx, ctx->main, level, img, H, W, reinterpret_cast<float*>(ctx->tmpT.p), nullptr, nullptr)) return rc;
  HIPCHK(ctx, launch_nhwc_to_nchw(reinterpret_cast<float*>(ctx->tmpT.p), feat, C, h * w, ctx->main.stream));
  return range_readback(ctx);
}

int wct_decode(wct_ctx* ctx, int level, const float* feat, int h, int w, int layout, float* img) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !img || !feat || h < 1 || w < 1) return fail(ctx, WCT_ERR_INVALID, "decode: bad arguments");
  Module& m = ctx->mod[WCT_KIND_DEC][level];
  if (!m.loaded) return fail(ctx, WCT_ERR_STATE, "decoder %d not loaded", level);
  const float* f = feat;
  if (layout == WCT_LAYOUT_NCHW) {
    const int C = m.layers[0].d.cin;
    if (int rc = ensure(ctx, ctx->tmpT, (size_t)h * w * C * sizeof(float))) return rc;
    HIPCHK(ctx, launch_nchw_to_nhwc(feat, reinterpret_cast<float*>(ctx->tmpT.p), C, h * w, ctx->main.stream));
    f = reinterpret_cast<float*>(ctx->tmpT.p);
  } else if (layout != WCT_LAYOUT_NHWC) {
    return fail(ctx, WCT_ERR_INVALID, "decode: bad layout %d", layout);
  }
  if (int rc = decode_impl(ctx, level, f, h, w, nullptr, img)) return rc;
  return range_readback(ctx);
}

int wct_moments(wct_ctx* ctx, const float* feat, int C, int h, int w, int x0, int x1, double* sum, double* sumsq) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !sum || !sumsq) return fail(ctx, WCT_ERR_INVALID, "moments: NULL pointer");
  return moments_impl(ctx, ctx->main, feat, C, h, w, x0, x1, sum, sumsq);
}

int wct_solve(wct_ctx* ctx, int C, double n_c, const double* sum_c, const double* sumsq_c, double n_s,
              const double* sum_s, const double* sumsq_s, double alpha, double* M, double* b, int* info) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!sum_c || !sumsq_c || !sum_s || !sumsq_s || !M || !b) return fail(ctx, WCT_ERR_INVALID, "solve: NULL pointer");
  SumsView sv;
  if (int rc = sums_view(ctx, ctx->main, sv)) return rc;
  // the style side first: ot and adain read cov_s^(1/2) while they work on the content side (the order does not touch a result)
  if (int rc = eig_impl(ctx, ctx->main, C, n_s, sum_s, sumsq_s, 0, ctx->eigS[0], sv.info + 1)) return rc;
  if (int rc = transform_mb(ctx, ctx->transform, C, n_c, sum_c, sumsq_c, ctx->eigS[0], alpha, M, b, sv.info, nullptr)) return rc;
  if (info) {
    HIPCHK(ctx, hipMemcpyAsync(info, sv.info, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->main.stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  }
  return WCT_OK;
}

int wct_apply(wct_ctx* ctx, const float* feat, int C, int h, int w, int layout, const double* M, const double* b, float* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!feat || !M || !b || !out || h < 2 || w < 2 || C < 4 || (C & 3) || C > 512) return fail(ctx, WCT_ERR_INVALID, "apply: bad arguments");
  const int cp = pad_cout(C), chunks = (C + 15) / 16;
  const size_t wfl = (size_t)chunks * 36 * cp * 4;
  if (int rc = ensure(ctx, ctx->foldW, (wfl + cp) * sizeof(float))) return rc;
  float* wpk = reinterpret_cast<float*>(ctx->foldW.p);
  float* bias = wpk + wfl;
  HIPCHK(ctx, launch_pack_center_tap(M, b, C, cp, wpk, bias, ctx->main.stream));
  ConvDesc d{};
  d.cin = C; d.cout = C; d.cin_chunks = chunks; d.cout_pad = cp; d.flags = CONV_NO_RELU; d.wpk = wpk; d.bias = bias;
  if (layout == WCT_LAYOUT_NHWC) return run_conv(ctx, ctx->main, d, feat, out, h, w);
  if (layout != WCT_LAYOUT_NCHW) return fail(ctx, WCT_ERR_INVALID, "apply: bad layout %d", layout);
  return apply_nchw(ctx, feat, C, (long)h * w, out, [&](const float* in, float* res) { return run_conv(ctx, ctx->main, d, in, res, h, w); });
}

int wct_transform(wct_ctx* ctx, const float* cF, int C, int h, int w, const float* sF, int hs, int ws, float alpha,
                  int layout, float* out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!cF || !sF || !out || h < 1 || w < 1 || hs < 1 || ws < 1) return fail(ctx, WCT_ERR_INVALID, "transform: bad arguments");
  if (layout != WCT_LAYOUT_NHWC && layout != WCT_LAYOUT_NCHW) return fail(ctx, WCT_ERR_INVALID, "transform: bad layout %d", layout);
  if (h < 2 || w < 2) return fail(ctx, WCT_ERR_INVALID, "transform: feature %dx%d too small", h, w);
  Lane& ln = ctx->main;
  SumsView sv;
  if (int rc = sums_view(ctx, ln, sv)) return rc;
  double *M, *b;
  if (int rc = mb_view(ctx, &M, &b)) return rc;
  const float *c = cF, *s = sF;
  if (layout == WCT_LAYOUT_NCHW) {
    if (int rc = ensure(ctx, ctx->featC, (size_t)h * w * C * sizeof(float))) return rc;
    if (int rc = ensure(ctx, ctx->featS, (size_t)hs * ws * C * sizeof(float))) return rc;
    HIPCHK(ctx, launch_nchw_to_nhwc(cF, reinterpret_cast<float*>(ctx->featC.p), C, h * w, ln.stream));
    HIPCHK(ctx, launch_nchw_to_nhwc(sF, reinterpret_cast<float*>(ctx->featS.p), C, hs * ws, ln.stream));
    c = reinterpret_cast<float*>(ctx->featC.p);
    s = reinterpret_cast<float*>(ctx->featS.p);
  }
  // the style side first: its moments share the lane's buffer with the content's, which ot and adain read next to cov_s^(1/2)
  if (int rc = moments_impl(ctx, ln, s, C, hs, ws, 0, ws, sv.sum, sv.sumsq)) return rc;
  if (int rc = eig_impl(ctx, ln, C, (double)hs * ws, sv.sum, sv.sumsq, 0, ctx->eigS[0], sv.info + 1)) return rc;
  if (int rc = moments_impl(ctx, ln, c, C, h, w, 0, w, sv.sum, sv.sumsq)) return rc;
  if (int rc = transform_mb(ctx, ctx->transform, C, (double)h * w, sv.sum, sv.sumsq, ctx->eigS[0], alpha, M, b, sv.info, nullptr)) return rc;
  return wct_apply(ctx, cF, C, h, w, layout, M, b, out);
}

int wct_decode_affine(wct_ctx* ctx, int level, const float* feat, int h, int w, const double* M, const double* b, float* img) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !feat || !M || !b || !img) return fail(ctx, WCT_ERR_INVALID, "decode_affine: bad arguments");
  ConvDesc first;
  if (int rc = fold_impl(ctx, level, M, b, first)) return rc;
  if (int rc = decode_impl(ctx, level, feat, h, w, &first, img)) return rc;
  return range_readback(ctx);
}

int wct_style_transfer_level(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style, int Hs,
                             int Ws, float alpha, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !content || !style || !out) return fail(ctx, WCT_ERR_INVALID, "style_transfer_level: bad arguments");
  if (int rc = with_deferred_solves(ctx, false, [&]() -> int {
        if (int rc = fork_side(ctx)) return rc;
        if (int rc = style_side(ctx, level, style, Hs, Ws)) return rc;
        return content_side(ctx, level, content, H, W, alpha, out, Ho, Wo);
      })) return rc;
  return range_readback(ctx);
}

// ---- split form of a level, for content-sharded runs (wct_hip/sharded.py): the caller all-reduces the moments
//      between wct_content_encode and wct_content_solve and may broadcast (M, b) before wct_content_decode.
int wct_style_prepare_levels(wct_ctx* ctx, const float* style, int Hs, int Ws, unsigned level_mask) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!style) return fail(ctx, WCT_ERR_INVALID, "style_prepare: NULL style");
  if (int rc = with_deferred_solves(ctx, true, [&]() -> int {
        if (int rc = fork_side(ctx)) return rc;
        for (int level = 5; level >= 1; --level)
          if ((level_mask >> level & 1u) && ctx->mod[WCT_KIND_ENC][level].loaded)
            if (int rc = style_side(ctx, level, style, Hs, Ws)) return rc;
        return WCT_OK;
      })) return rc;
  // the encoders ran on the side lane (with overlap on): the mirror goes behind them on that lane, so that the caller's stream stays
  // free to overlap the style side; with overlap off everything ran on the caller's stream
  if (int rc = range_readback_side(ctx, ctx->overlap ? ctx->side : ctx->main)) return rc;
  return range_readback(ctx);
}

int wct_style_prepare(wct_ctx* ctx, const float* style, int Hs, int Ws) { return wct_style_prepare_levels(ctx, style, Hs, Ws, 0x3eu); }

int wct_style_stats_count(const wct_ctx* ctx, int level, size_t* n_doubles) {
  if (!ctx || !valid_level(level) || !n_doubles) return WCT_ERR_INVALID;
  const Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return WCT_ERR_STATE;
  const size_t C = me.layers.back().d.cout;
  *n_doubles = C * C + C;
  return WCT_OK;
}

// stats = cov_s^(1/2) [C*C] | mu_s [C]  (the two parts of the EigResult that launch_assemble consumes)
int wct_style_export(wct_ctx* ctx, int level, double* stats) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !stats) return fail(ctx, WCT_ERR_INVALID, "style_export: bad arguments");
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded || !ctx->eigS[level].p) return fail(ctx, WCT_ERR_STATE, "style_export: wct_style_prepare has not run for level %d", level);
  const size_t C = me.layers.back().d.cout, cc = C * C;
  const double* res = reinterpret_cast<const double*>(ctx->eigS[level].p);
  hipStream_t st = ctx->main.stream;
  HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_style[level], 0));
  HIPCHK(ctx, hipMemcpyAsync(stats, res + eig_result_F_offset(C), cc * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(stats + cc, res + cc + C, C * sizeof(double), hipMemcpyDeviceToDevice, st));
  return WCT_OK;
}

int wct_style_import(wct_ctx* ctx, int level, const double* stats) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !stats) return fail(ctx, WCT_ERR_INVALID, "style_import: bad arguments");
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  const size_t C = me.layers.back().d.cout, cc = C * C;
  if (int rc = ensure(ctx, ctx->eigS[level], eig_result_bytes((int)C))) return rc;
  double* res = reinterpret_cast<double*>(ctx->eigS[level].p);
  hipStream_t st = ctx->main.stream;
  HIPCHK(ctx, hipMemcpyAsync(res + eig_result_F_offset(C), stats, cc * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(res + cc + C, stats + cc, C * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (int rc = style_fold(ctx, level, st)) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev_style[level], st));   // what content_side / wct_content_solve wait for
  return WCT_OK;
}

int wct_content_encode(wct_ctx* ctx, int level, const float* content, int H, int W, int x0, int x1, double* sum,
                       double* sumsq, int* h_out, int* w_out) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !content || !sum || !sumsq) return fail(ctx, WCT_ERR_INVALID, "content_encode: bad arguments");
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  const int C = me.layers.back().d.cout;
  int h, w;
  level_dims(level, H, W, h, w);
  if (x1 < 0) x1 = w;
  if (l1_fused(ctx, level)) {
    // relu1_1 is never materialised: keep a copy of the image for wct_content_decode (12 B/px, device to device)
    const size_t ib = (size_t)3 * H * W * sizeof(float);
    if (int rc = ensure(ctx, ctx->l1img, ib)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(ctx->l1img.p, content, ib, hipMemcpyDeviceToDevice, ctx->main.stream));
    if (int rc = l1_moments_impl(ctx, ctx->main, level, content, H, W, x0, x1, sum, sumsq)) return rc;
  } else {
    if (int rc = ensure(ctx, ctx->featC, (size_t)h * w * C * sizeof(float))) return rc;
    float* fC = reinterpret_cast<float*>(ctx->featC.p);
    if (int rc = encode_impl(ctx, ctx->main, level, content, H, W, fC, nullptr, nullptr)) return rc;
    if (int rc = moments_impl(ctx, ctx->main, fC, C, h, w, x0, x1, sum, sumsq)) return rc;
  }
  ctx->cur_level = level; ctx->cur_h = h; ctx->cur_w = w; ctx->cur_H = H; ctx->cur_W = W;
  ctx->pair_open = true;
  if (h_out) *h_out = h;
  if (w_out) *w_out = w;
  return range_readback(ctx);
}

int wct_content_solve(wct_ctx* ctx, int level, double n_c, const double* sum_c, const double* sumsq_c, float alpha, double* M,
                      double* b) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !sum_c || !sumsq_c || !M || !b) return fail(ctx, WCT_ERR_INVALID, "content_solve: bad arguments");
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  if (!ctx->eigS[level].p) return fail(ctx, WCT_ERR_STATE, "content_solve: wct_style_prepare has not run for level %d", level);
  const int C = me.layers.back().d.cout;
  SumsView sv;
  if (int rc = sums_view(ctx, ctx->main, sv)) return rc;
  return transform_mb(ctx, ctx->transform, C, n_c, sum_c, sumsq_c, ctx->eigS[level], alpha, M, b, sv.info, ctx->ev_style[level]);
}

int wct_content_decode(wct_ctx* ctx, int level, const double* M, const double* b, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!valid_level(level) || !M || !b || !out) return fail(ctx, WCT_ERR_INVALID, "content_decode: bad arguments");
  if (ctx->cur_level != level) return fail(ctx, WCT_ERR_STATE, "content_decode: wct_content_encode(level %d) has not run", level);
  ConvDesc first;
  if (int rc = fold_impl(ctx, level, M, b, first)) return rc;
  if (l1_fused(ctx, level)) {
    if (int rc = l1_decode_impl(ctx, level, reinterpret_cast<const float*>(ctx->l1img.p), ctx->cur_H, ctx->cur_W, first, out)) return rc;
  } else {
    if (int rc = decode_impl(ctx, level, reinterpret_cast<float*>(ctx->featC.p), ctx->cur_h, ctx->cur_w, &first, out)) return rc;
  }
  if (Ho) *Ho = ctx->cur_h << (level - 1);
  if (Wo) *Wo = ctx->cur_w << (level - 1);
  ctx->pair_open = false;
  return range_readback(ctx);
}

}  // extern "C"

namespace {
// the content cascade of WCT.py:120-125 against the style statistics already in the context
// `style` (wct_stylize): the style side of level L - 1 is enqueued behind the content side of level L of the first run
int cascade(wct_ctx* ctx, const float* content, int H, int W, float alpha, int num_run, float* out, int* Ho, int* Wo,
            const float* style = nullptr, int Hs = 0, int Ws = 0) {
  if (int rc = run_cascade(ctx, content, H, W, num_run, out, Ho, Wo,
        [&](int level, const float* cur, int h, int w, float* dst, int* ho, int* wo) { return content_side(ctx, level, cur, h, w, alpha, dst, ho, wo); },
        [&](int level) { return style ? style_side(ctx, level - 1, style, Hs, Ws) : (int)WCT_OK; })) return rc;
  return range_readback(ctx);
}

int noise_impl(wct_ctx* ctx, uint64_t seed, uint32_t stream_id, int H, int W, float* planar) {
  ProfScope ps(ctx, ctx->main.stream, "noise_uniform<philox4x32-10>", 0, 12.0 * H * W);
  HIPCHK(ctx, launch_noise_uniform(seed, stream_id, H, W, planar, ctx->main.stream));
  return WCT_OK;
}
}  // namespace

namespace wct_host {

// the bodies of wct_stylize / wct_stylize_prepared behind their argument checks; wct_synthesize runs them on its noise image
int stylize_impl(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run, float* out,
                 int* Ho, int* Wo) {
  // style side of all five levels first, on the side lane: it only depends on the style image (the SAME image at
  // every level and every run, WCT.py:121-125), so it is computed once and overlaps the content cascade
  return with_deferred_solves(ctx, false, [&]() -> int {
    if (int rc = fork_side(ctx)) return rc;
    if (!ctx->interleave || !ctx->overlap) {   // (one lane: its moments buffer holds ONE level's sums at a time -- nothing to interleave)
      for (int level = 5; level >= 1; --level)
        if (int rc = style_side(ctx, level, style, Hs, Ws)) return rc;
      return cascade(ctx, content, H, W, alpha, num_run, out, Ho, Wo);
    }
    // Host order: S5, C5, S4, C4, ... -- on the GPU the lanes run exactly as if everything were queued (the host is ~10x ahead of
    // the kernels), but the FIRST content kernel of a cold call no longer waits for ~400 style-side launches to be enqueued
    // (tools/experiments/lane_timeline.py: the content lane of a lone 4K call started 0.53 ms late, of a lone --mode original
    // call 1.5 ms).  What was also tried here and measured slower on every box: GATING the style side of level L - 1 on the
    // content lane's progress (start it when the content moments of level L are done, or when its matrix function is) so
    // that content-lane matrix functions never share the GPU with a style encoder -- config 2 +0.2 ms, config 3 +0..0.8 ms:
    // two big kernels that overlap finish sooner than the same two in sequence, and the gates trade that overlap away.
    if (int rc = style_side(ctx, 5, style, Hs, Ws)) return rc;
    return cascade(ctx, content, H, W, alpha, num_run, out, Ho, Wo, style, Hs, Ws);
  });
}

int stylize_prepared_impl(wct_ctx* ctx, const char* what, const float* content, int H, int W, float alpha, int num_run, float* out, int* Ho, int* Wo) {
  for (int level = 5; level >= 1; --level)
    if (!ctx->eigS[level].p) return fail(ctx, WCT_ERR_STATE, "%s: no style statistics for level %d (wct_style_prepare / wct_style_import)", what, level);
  return with_deferred_solves(ctx, false, [&]() -> int { return cascade(ctx, content, H, W, alpha, num_run, out, Ho, Wo); });
}

}  // namespace wct_host

extern "C" {

int wct_stylize(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha,
                int num_run, float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || !style || !out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "stylize: bad arguments");
  return stylize_impl(ctx, content, H, W, style, Hs, Ws, alpha, num_run, out, Ho, Wo);
}

int wct_stylize_prepared(wct_ctx* ctx, const float* content, int H, int W, float alpha, int num_run, float* out, int* Ho,
                         int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!content || !out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "stylize_prepared: bad arguments");
  return stylize_prepared_impl(ctx, "stylize_prepared", content, H, W, alpha, num_run, out, Ho, Wo);
}

int wct_noise_uniform(wct_ctx* ctx, uint64_t seed, uint32_t stream_id, int H, int W, float* planar) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!planar || H < 1 || W < 1) return fail(ctx, WCT_ERR_INVALID, "noise_uniform: bad arguments (%dx%d, planar %s)", H, W, planar ? "given" : "NULL");
  return noise_impl(ctx, seed, stream_id, H, W, planar);
}

int wct_synthesize(wct_ctx* ctx, const float* texture, int Ht, int Wt, int H, int W, uint64_t seed, uint32_t stream_id, float alpha, int num_run,
                   float* out, int* Ho, int* Wo) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!out || num_run < 1) return fail(ctx, WCT_ERR_INVALID, "synthesize: bad arguments (out %s, num_run %d)", out ? "given" : "NULL", num_run);
  // the cascade starts at level 5, whose reflect padding needs two samples at 1/16 scale (encode_impl): say so before anything is written
  if (H < 32 || W < 32) return fail(ctx, WCT_ERR_INVALID, "synthesize: output %dx%d is too small for the five-level cascade (32x32 at least)", H, W);
  if (texture && (Ht < 32 || Wt < 32))
    return fail(ctx, WCT_ERR_INVALID, "synthesize: texture %dx%d is too small for the five-level cascade (32x32 at least)", Ht, Wt);
  if (!texture)
    for (int level = 5; level >= 1; --level)
      if (!ctx->eigS[level].p) return fail(ctx, WCT_ERR_STATE, "synthesize: no style statistics for level %d (wct_style_prepare / wct_style_import)", level);
  if (int rc = ensure(ctx, ctx->noise, (size_t)3 * H * W * sizeof(float))) return rc;
  float* noise = reinterpret_cast<float*>(ctx->noise.p);
  if (int rc = noise_impl(ctx, seed, stream_id, H, W, noise)) return rc;
  if (texture) return stylize_impl(ctx, noise, H, W, texture, Ht, Wt, alpha, num_run, out, Ho, Wo);
  return stylize_prepared_impl(ctx, "synthesize", noise, H, W, alpha, num_run, out, Ho, Wo);
}

}  // extern "C"

namespace {
// What a wct_stylize / wct_stylize_prepared (with its wct_style_prepare) of this size needs of every workspace buffer it touches, under the
// context's current switches: the ONE list behind wct_workspace_bytes and wct_reserve (a buffer may appear more than once: the largest counts).
struct WsNeed { DevBuf* buf; size_t bytes; };
void workspace_plan(wct_ctx* ctx, int H, int W, int Hs, int Ws, std::vector<WsNeed>& need) {
  size_t act = 0, acts = 0, featc = 0, feats = 0, momc = 0, moms = 0;
  int cmax = 2;
  for (int level = 1; level <= 5; ++level) {
    const Module& e = ctx->mod[WCT_KIND_ENC][level];
    const Module& d = ctx->mod[WCT_KIND_DEC][level];
    if (!e.loaded || !d.loaded) continue;
    int h, w, hs, ws;
    level_dims(level, H, W, h, w);
    level_dims(level, Hs, Ws, hs, ws);
    const int C = e.layers.back().d.cout;
    cmax = std::max(cmax, C);
    act = std::max(act, std::max(max_act_bytes(e, H, W, true), max_act_bytes(d, h, w, false)));
    acts = std::max(acts, max_act_bytes(e, Hs, Ws, true));
    featc = std::max(featc, (size_t)h * w * C * sizeof(float));     // content_side / style_side size these for every level, fused or not
    feats = std::max(feats, (size_t)hs * ws * C * sizeof(float));
    if (l1_fused(ctx, level)) {   // relu1_1 is never materialised: the fused moments kernel's partials, whatever the image size
      momc = std::max(momc, l1_moments_workspace_bytes());
      moms = std::max(moms, l1_moments_workspace_bytes());
    } else {
      momc = std::max(momc, moments_workspace_bytes(C, (long)h * w));
      moms = std::max(moms, moments_workspace_bytes(C, (long)hs * ws));
    }
    const LayerDev& l0 = d.layers[0];
    need.push_back({&ctx->foldW, ((size_t)l0.d.cin_chunks * 36 * l0.d.cout_pad * 4 + l0.d.cout_pad) * sizeof(float)});
    need.push_back({&ctx->foldW16, conv_f16_weight_bytes(l0.d.cin, l0.d.cout_pad, l0.d.cout_pad == 16 ? 10 : 9) + 64 + conv_phase_weight_bytes(l0.d.cin) +
                                       512 * sizeof(unsigned)});
    if (fast_fold_level(ctx, level)) need.push_back({&ctx->foldS[level], fold_style_doubles(l0.d.cout, l0.d.cin) * sizeof(double)});
    need.push_back({&ctx->eigS[level], eig_result_bytes(C)});
  }
  need.push_back({&ctx->main.actA, act});
  need.push_back({&ctx->main.actB, act});
  need.push_back({&ctx->side.actA, acts});
  need.push_back({&ctx->side.actB, acts});
  need.push_back({&ctx->featC, featc});
  need.push_back({&ctx->featS, feats});
  need.push_back({&ctx->main.wsMom, momc});
  need.push_back({&ctx->side.wsMom, moms});
  need.push_back({&ctx->tmpT, (size_t)3 * H * W * sizeof(float)});
  need.push_back({&ctx->eigC, eig_result_bytes(cmax)});
  need.push_back({&ctx->wsAsm, assemble_workspace_bytes(cmax)});
  if (ctx->transform == WCT_TRANSFORM_OT) need.push_back({&ctx->trBuf, ot_workspace_bytes(cmax)});
  for (Lane* ln : {&ctx->main, &ctx->side}) {
    need.push_back({&ln->wsEig, eig_workspace_bytes(cmax)});
    need.push_back({&ln->sums, SUMS_BYTES});
  }
  need.push_back({&ctx->small, SMALL_BYTES});
}
}  // namespace

extern "C" {

size_t wct_workspace_bytes(const wct_ctx* cctx, int H, int W, int Hs, int Ws) {
  if (!cctx) return 0;
  wct_ctx* ctx = const_cast<wct_ctx*>(cctx);   // the plan names the context's buffers; nothing is modified
  WCT_GUARD(ctx);
  std::vector<WsNeed> need;
  workspace_plan(ctx, H, W, Hs, Ws, need);
  std::map<DevBuf*, size_t> per;
  for (const WsNeed& n : need) per[n.buf] = std::max(per[n.buf], n.bytes);
  size_t total = 0;
  for (const auto& kv : per)
    if (kv.second) total += (kv.second + 255) & ~(size_t)255;    // ensure()'s rounding
  return total;
}

int wct_reserve(wct_ctx* ctx, int H, int W, int Hs, int Ws) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  std::vector<WsNeed> need;
  workspace_plan(ctx, H, W, Hs, Ws, need);
  for (const WsNeed& n : need)
    if (n.bytes)
      if (int rc = ensure(ctx, *n.buf, n.bytes)) return rc;
  return WCT_OK;
}

int wct_set_numpy_variant(wct_ctx* ctx, int on) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (on && ctx->transform != WCT_TRANSFORM_WCT) return fail(ctx, WCT_ERR_INVALID, "set_numpy_variant: the + I variant is defined for the wct transform only (wct_set_transform)");
  ctx->numpy_variant = on ? 1 : 0;
  return WCT_OK;
}

int wct_set_overlap(wct_ctx* ctx, int on) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  ctx->overlap = on != 0;
  return WCT_OK;
}

int wct_set_conv_mode(wct_ctx* ctx, int mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (mode != 0 && mode != 1) return fail(ctx, WCT_ERR_INVALID, "conv mode must be 0 (fp32) or 1 (f16x3)");
  ctx->conv_mode = mode;
  return WCT_OK;
}

int wct_profile_enable(wct_ctx* ctx, int on) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!on) prof_collect(ctx);
  ctx->prof = on != 0;
  return WCT_OK;
}

int wct_profile_reset(wct_ctx* ctx) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  prof_collect(ctx);
  ctx->prof_acc.clear();
  return WCT_OK;
}

int wct_profile_read(wct_ctx* ctx, wct_prof_entry* entries, int max_entries, int* n_entries) {
  if (!ctx || !n_entries) return WCT_ERR_INVALID;
  prof_collect(ctx);
  int n = 0;
  for (auto& kv : ctx->prof_acc) {
    if (entries && n < max_entries) entries[n] = kv.second;
    ++n;
  }
  *n_entries = n;
  return WCT_OK;
}

}  // extern "C"
