// C ABI of libwct_hip (see include/wct_hip.h): context, module loading, the per-level pipeline and the
// 5-level cascade.  Host-side C++ only orchestrates launches on the context's HIP stream; all arithmetic is
// in the kernels of conv3x3.hip / moments.hip / solve.hip / misc.hip.
#include "../../include/wct_hip.h"
#include "../../include/wct_hip_color.h"
#include "../../include/wct_hip_guided.h"
#include "../../include/wct_hip_scale.h"
#include "../../include/wct_hip_smooth.h"
#include "../../include/wct_hip_swap.h"
#include "../../include/wct_hip_transform.h"
#include "wct_common.h"

#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <atomic>
#include <cstring>
#include <dlfcn.h>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

struct LayerDev {
  ConvDesc d{};
  int pool_after = 0, up_after = 0;
  float* w_oihw = nullptr;  // device copy of the original weights (first decoder layer only: needed by the fold)
  double* fold_rows = nullptr;  // ... and, for the wide models' decoders, as fp64 GEMM rows + tap sums (launch_fold_gemm)
  float* bias_raw = nullptr;
  float* wpk = nullptr;
  float* bias = nullptr;
  void* wpk16 = nullptr;  // split-f16 weights (all but the 3-channel first conv)
  void* l1w16 = nullptr;  // 3-channel first conv with <= 32 couts: f16x3 slot packing for the level-1 kernels
  void* wph16 = nullptr;  // last decoder conv (-> 3 couts): block-packed split-f16 weights for the fused tails
  void* wup16 = nullptr;  // 16 -> 16 conv behind an upsample: per-parity 2x2 weights (ConvDesc::wup16)
  float* l1bias = nullptr;
};

struct Module {
  bool loaded = false;
  std::vector<LayerDev> layers;
};

// weight tables of one resize axis on the device (resize.hip)
struct ResizeAxis {
  int in_size = 0, out_size = 0, filter = 0, ksize = 0, first = 0, last = 0;   // [first, last): input rows / columns any output touches
  int* bounds = nullptr;          // [2 * out]            -- the three tables share ONE allocation (base = bounds)
  int* bounds_shifted = nullptr;  // the same with `first` subtracted from every start (the vertical pass reads a cropped image)
  int* kk = nullptr;              // [out * ksize]
  unsigned long long used = 0;    // LRU stamp
};

struct ProfRec {
  hipEvent_t e0, e1;
  std::string name;
  double flops, bytes;
  bool side = false;   // recorded on the side lane's stream
};

}  // namespace

__thread LaunchForm wct_launch_form = {0, 0, false, {0}};   // wct_common.h

// An in-order execution lane: a stream plus the scratch only that stream touches.  `main` runs on the caller's
// stream (content side, assembly, decode); `side` is a context-owned stream on which the style side (encode,
// moments, eigen-decomposition -- independent of the content) runs ahead and overlaps the content side.
struct Lane {
  hipStream_t stream = nullptr;
  DevBuf actA, actB, wsMom, wsEig, sums;  // sums: sum[512] | sumsq[512*512] (doubles) | info (ints)
  int xcd = 0;   // where this lane's single-launch Newton-Schulz iterations run (launch_eig coop_xcd): one XCD per lane, process-wide round robin
  unsigned* coop = nullptr;   // ... their two sets of barrier state (64 bytes, zeroed at creation) ...
  int coop_epoch = 0;         // ... and which set the next one counts in
  // health of the single-launch solves on this lane, from the mirrored abort counter (coop_usable)
  unsigned coop_solves = 0;   // single-launch solves enqueued
  bool coop_off = false;      // they kept aborting here (rocprof serialising the dispatches, a partitioned device, the other lane owning the XCD): multi-launch from now on
};

struct wct_ctx {
  int device = 0;
  Lane main, side;
  hipEvent_t ev_join = nullptr;   // side -> main (wct_style_moments: the style strip's sums are ready)
  hipEvent_t ev_smom[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // wct_stylize_sharded, strips: level L's style sums are ready (side -> main)
  hipEvent_t ev_sar[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};    // ... and level L's all-reduce has been issued (main -> side)
  hipEvent_t ev_switch = nullptr;   // wct_set_stream: old caller stream -> new caller stream (the workspace is shared between them)
  hipEvent_t ev_fork = nullptr, ev_style[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int eig_skip = 0, eig_calls = 0;
  int foldgemm = 1;   // 1: the wide models' folds as fp64 matrix-core GEMMs (debug key "foldgemm"; 0: misc.hip fold_block_kernel)
  int nscoop = 1;     // 1: the Newton-Schulz iteration of a 128-channel level (--mode 16x) is ONE launch (debug key "nscoop")
  int interleave = 1; // 1: wct_stylize enqueues the style side of level L - 1 behind the content side of level L (debug key "interleave"; 0: all five up front)
  std::string err;
  Module mod[2][6];
  // workspace
  DevBuf featC, featS, tmpT, wsAsm, small, foldW, foldW16, eigC, eigS[6];
  DevBuf foldS[6];    // per level: the style-side part of the fast fold (misc.hip fold_style_kernel), valid when fold_ready[level]
  bool fold_ready[6] = {false, false, false, false, false, false};
  int cur_level = 0, cur_h = 0, cur_w = 0;  // content feature held in featC by wct_content_encode
  DevBuf u8c, u8s, u8o;   // fp32 planar staging of wct_stylize_u8 (content, style, result)
  DevBuf rsz_tmp;         // wct_resize_u8: uint8 image between the horizontal and the vertical pass
  std::vector<ResizeAxis> rsz_axes;   // weight tables per (in, out, filter), built on first use; least recently used evicted at 16
  unsigned long long rsz_clock = 0;
  DevBuf noise;       // wct_synthesize: the noise image (3 H W floats) the cascade reads as its content; kept until wct_destroy
  // colour preservation (include/wct_hip_color.h): the matched style of wct_stylize_color (3 Hs Ws floats), its un-merged result (3 H W
  // floats), and [sum_s 3 | sumsq_s 9 | sum_c 3 | sumsq_c 9 | A 9 | t 3 | pad to 64 doubles | stage-1 partials of the colour moments]
  DevBuf colStyle, colOut, colWs;
  // guided-filter smoothing (include/wct_hip_smooth.h): the window sums between the two directions of a box (21 fp64 planes) and the
  // coefficients a, b between the two stages (12 fp32 planes); wct_stylize_smooth keeps its un-filtered result in colOut
  DevBuf smSums, smAB;
  // patch swap (include/wct_hip_swap.h): the two encoded features, the two projected maps, the blended feature, the indices, the running
  // (score, index) of every query between the key chunks' launches, the key norms, and the all-zero label map of the one-label affine apply
  DevBuf swFc, swFs, swQ, swK, swOut, swIdx, swRun, swNorm, swLab;
  int swap_key_chunk = 0;   // debug key "swap_key_chunk": keys per launch of the match; 0 = WCT_SWAP_KEY_CHUNK
  // scale control (include/wct_hip_scale.h): the content at the working size of every distinct divisor of wct_stylize_scaled, and the
  // image its merges and levels ping-pong through with the caller's `out`
  DevBuf scF[5], scStage, scTab;   // scTab: the weight tables of one resampler / merge launch (scale.hip)
  DevBuf l1img;       // level 1 fused: copy of the content image between wct_content_encode and wct_content_decode
  int cur_H = 0, cur_W = 0;
  int numpy_variant = 0;  // 1: `--numpy` semantics (util_wct.py:143): + I on the CONTENT covariance
  int transform = 0;      // WCT_TRANSFORM_* (include/wct_hip_transform.h): which T the (M, b) of a level is made of (transform_mb)
  DevBuf trBuf;           // ot: B = sym(S cov_c S) [C*C] | a product in flight [C*C] | zeros [C]  (ot_workspace_bytes)
  bool wide_model = false;  // a loaded encoder ends wider than 128 channels (--mode original): see launch_eig
  int l1fuse = 1;     // 1: level 1 of the 16x cascade without materialising relu1_1 (level1.hip)
  int sp = 1;         // 1: intermediate activations of the f16x3 path in SP16 (split at the producer, DMA-staged consumers)
  int u8fuse = 1;     // 1: wct_stylize_u8 reads / writes uint8 inside the first / last kernel where one exists (reserved)
  int fastfold = 1;   // 1: (W Ss) Wc fold without T = Ss Wc / M / b on the content side's critical path where the decoder allows (cin <= 128)
  int upconv = 1;     // 1: decoder layers behind an upsample run as per-parity 2x2 convolutions of the low-resolution map (4/9 of the products)
  int mom32 = 1;      // 1: moments of maps with >= MOM32_MIN_PIXELS pixels take their products on the fp32 matrix cores in 64-pixel blocks, block sums in
                      //    fp64 (moments.hip F32 variant; debug key "mom32"); 0: fp64 products throughout (2: fp32 products at every size)
  int in3wide = 2;    // the 3 -> 64 first conv of the un-pruned encoders: 2 = exact-fp32 MFMA, four cout tiles per operand read (level1.hip in3_wide_f32_kernel);
                      // 1 = f16x3 (in3_wide_kernel: measurably further from the reference at K = 27, see there); 0 = the generic fp32 kernel (debug key "in3wide")
  int fuse = 1;       // 1: fused conv11+conv12+pool / conv12+conv11 kernels at the full-resolution ends of the 16x networks
  int overlap = 1;    // 1: style side on the side lane (overlaps the content side); 0: everything on the caller's stream
  int conv_mode = 1;  // 0: exact-fp32 MFMA everywhere; 1: split-f16 (f16x3) MFMA for all but the first conv
  unsigned* sat_dev = nullptr;   // saturation counter (conv_f16_dev.h SatTrack): threads that clamped an activation to +-65504 (saturating)
  // --mode original (C > 128): outcomes of the deflated iterations of ONE API call, checked once at the call's end instead of one
  // stream synchronisation per solve (launch_eig ok_defer)
  int* ok_log = nullptr;         // device [64]
  int* ok_host = nullptr;        // pinned [64]: outcomes [0, OK_SLOTS), the saturation counter read with them at [OK_SLOTS]
  int ok_n = 0;
  bool defer_big = false;
  // sat_dev is a 256-byte block of counters (unsigned): [0] the saturation counter; [1] its snapshot at the start of a deferred
  // wide-model call (with_deferred_solves); [2], [3] single-launch Newton-Schulz solves that ABORTED on the main / side lane
  unsigned* sat_host = nullptr;  // pinned host mirror, refreshed asynchronously at the end of every compute entry point (wct_range_poll)
  // sat_host[SAT_SIDE_WORD]: the side lane's own mirror of counter [0] (range_readback_side).  Two words, one per stream: each is written in
  // its stream's order, so neither can be overwritten by an older value of the other stream's copy; wct_range_poll reports the larger
  // RCCL communicator of a column-sharded job (wct_comm_*, wct_level_sharded); the library resolves RCCL at run time (no link-time dependency)
  void* comm = nullptr;
  bool comm_owned = false;
  int comm_ranks = 0, comm_rank = 0;
  DevBuf packed;      // wct_level_sharded / wct_stylize_sharded: [sum C | sumsq C*C | range flag | style sums of levels 5..1] fp64, all-reduced in place
  // how the context talks to its peers (wct_comm_init / _attach: RCCL on `comm`; wct_comm_attach_collectives: the caller's transport)
  wct_collectives coll{};
  bool coll_set = false, coll_rccl = false;
  bool quiet_readback = false;
  bool shard_emulate = false;   // MEASUREMENT ONLY (debug key "shard_emulate"): comm_ranks / comm_rank are an emulated job's, the real communicator has ONE rank
  // wct_stylize_sharded: the level's cropped input, the decoded strip, the next level's assembled input (exchange mode), the four edge blocks
  // (send left | send right | recv left | recv right), the rank's style strip, a level's style statistics in transit, (M | b) in transit
  DevBuf shIn, shOut, shNext, shEdge, shStyle, shStats, shMb;
  // profiling
  bool prof = false;
  bool prof_forms = false;   // debug key "prof_forms": profile names carry the launcher's chosen form (ProfScope)
  std::vector<ProfRec> recs;
  std::map<std::string, wct_prof_entry> prof_acc;
  // spatial control (wct_stylize_regions, wct_moments_labeled, wct_apply_labeled): K style slots per level (cov_s^(1/2), mu_s), the
  // regions' content results, the level label maps, per-label moments [n K | sum K*C | sumsq K*C*C], the K maps [M K*C*C | b K*C],
  // the transformed feature map, the kernels' workspaces; pinned [6][256] label histograms read back once per call
  DevBuf eigR[8][6], eigCR[8], regLab, regHist, regSums, regMb, regFeat, wsRegMom, wsRegApply;
  unsigned* reg_hist_host = nullptr;
  // region-to-region transfer (include/wct_hip_guided.h).  wct_stylize_guided: the mapped styles' level label maps and histograms (made on
  // the caller's stream in the pre-pass), and the SIDE lane's own per-label sums and moments workspace -- the main lane's regSums / wsRegMom
  // are in use at the same time; pinned [8][6][256] style histograms read back with the content's.  K-means: the two encoded maps, the
  // kernels' partials, and [sh_c C | sc_c C | sh_s C | sc_s C | centroids 2 K C | n K | sum K C | cost 1 | idx K | lab_c | lab_s]
  DevBuf gdLab, gdHist, gdSums, wsGdMom, kmFeatC, kmFeatS, kmWs, kmStat;
  unsigned* gd_hist_host = nullptr;
  // style interpolation / weights (wct_stylize_interp, wct_style_blend, wct_stylize_blend): the pooled level weight maps, (V1, V2) per
  // (level, k) + the weight check's counts, the pooling workspace, the mixed apply's workspace; pinned copy of blendStat read back once
  // per wct_stylize_blend call (the regions' moments / maps / feature buffers are reused)
  DevBuf blendW, blendStat, wsBlendPool, wsBlendApply;
  void* blend_host = nullptr;
  // debug hooks (wct_debug_set "poison", wct_debug_get "ws_allocs" / "ws_bytes")
  int poison = -1;                     // 0..255: every ensure() allocation is filled with this byte; -1: off
  unsigned long long ws_allocs = 0;    // ensure() allocations so far
  bool pair_open = false;              // between wct_content_encode and wct_content_decode: featC / l1img are state

  // EVERY DevBuf of the context, once, with its class: f(buf, owning lane, scratch).  Scratch = no later call is documented to read
  // what an earlier call left there, so the "poison" hook may overwrite it between calls; state must survive (style slots, the
  // style-side folds, and the content feature / image of an open wct_content_encode -> wct_content_decode pair).  wct_destroy
  // releases through this list: a DevBuf added to the struct has to be classified here or it leaks.
  template <typename F>
  void each_buf(F&& f) {
    for (Lane* ln : {&main, &side})
      for (DevBuf* b : {&ln->actA, &ln->actB, &ln->wsMom, &ln->wsEig, &ln->sums}) f(*b, ln, true);
    for (DevBuf* b : {&featS, &tmpT, &wsAsm, &trBuf, &small, &foldW, &foldW16, &eigC, &u8c, &u8s, &u8o, &rsz_tmp, &noise, &colStyle, &colOut, &colWs, &smSums, &smAB, &swFc, &swFs, &swQ, &swK, &swOut, &swIdx, &swRun, &swNorm, &swLab, &packed,
                      &shIn, &shOut, &shNext, &shEdge, &shStyle, &shStats, &shMb,
                      &regLab, &regHist, &regSums, &regMb, &regFeat, &wsRegMom, &wsRegApply,
                      &blendW, &blendStat, &wsBlendPool, &wsBlendApply, &gdLab, &gdHist, &kmFeatC, &kmFeatS, &kmWs, &kmStat})
      f(*b, &main, true);
    for (DevBuf* b : {&gdSums, &wsGdMom}) f(*b, &side, true);   // the guided call's style side
    for (DevBuf& b : scF) f(b, &main, true);
    f(scStage, &main, true);
    f(scTab, &main, true);
    for (DevBuf& b : eigCR) f(b, &main, true);       // the regions' content-side results: rewritten by every level that reads them
    for (DevBuf* b : {&featC, &l1img}) f(*b, &main, !pair_open);
    for (int l = 0; l < 6; ++l) {
      f(eigS[l], &side, false);                      // prepared style statistics (wct_style_prepare / _import / _blend / wct_stylize_interp)
      f(foldS[l], &side, false);                     // their style-side fold, valid while fold_ready[l]
      for (int k = 0; k < 8; ++k) f(eigR[k][l], &side, false);   // the K style slots of the regions / blend / interpolation calls
    }
  }
};

// RCCL, resolved at run time (wct_comm_load): the library keeps no link-time dependency on it
struct NcclUid { char b[128]; };      // nccl.h ncclUniqueId: 128 opaque bytes, passed BY VALUE to ncclCommInitRank
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, NcclUid, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;   // (send, recv, count, datatype, root, comm, stream)
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;               // (buf, count, datatype, peer, comm, stream)
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  std::string path;
};
static RcclApi g_rccl;
static std::mutex g_rccl_mutex;                  // wct_comm_load may be called from several contexts' threads
constexpr int NCCL_FLOAT64 = 8, NCCL_INT8 = 0, NCCL_SUM = 0;    // nccl.h: ncclDataType_t ncclFloat64 = 8, ncclInt8 = ncclChar = 0; ncclRedOp_t ncclSum = 0

namespace {

int fail(wct_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

#define HIPCHK(ctx, expr)                                                                          \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess)                                                                         \
      return fail(ctx, e__ == hipErrorOutOfMemory ? WCT_ERR_NOMEM : WCT_ERR_HIP, "%s: %s (%s:%d)", \
                  #expr, hipGetErrorString(e__), __FILE__, __LINE__);                              \
  } while (0)

// Every entry point runs with the context's device current and restores the caller's device on return: the process's
// current device is the caller's (PyTorch's) state, and streams / allocations of a context live on ctx->device.
struct DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(const wct_ctx* ctx) {
    if (!ctx) return;
    if (hipGetDevice(&prev) == hipSuccess && prev != ctx->device) switched = hipSetDevice(ctx->device) == hipSuccess;
  }
  ~DevGuard() { if (switched) (void)hipSetDevice(prev); }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};
#define WCT_GUARD(ctx) DevGuard dev_guard__(ctx)

constexpr int SAT_SIDE_WORD = 4;

void range_host_set(wct_ctx* ctx, unsigned n) {    // both lanes idle (the callers have synchronised them)
  if (ctx->sat_host) ctx->sat_host[0] = ctx->sat_host[SAT_SIDE_WORD] = n;
}

// An entry point whose clamping kernels ran on the SIDE lane and that does not join the caller's stream to it (wct_style_prepare*: the
// style side is meant to overlap whatever the caller enqueues next) mirrors the counter on that lane, behind those kernels in stream
// order -- the caller's stream neither waits for the side lane nor does the host
int range_readback_side(wct_ctx* ctx, Lane& ln) {
  if (ctx->quiet_readback || &ln == &ctx->main) return WCT_OK;
  if (ctx->sat_host) HIPCHK(ctx, hipMemcpyAsync(ctx->sat_host + SAT_SIDE_WORD, ctx->sat_dev, sizeof(unsigned), hipMemcpyDeviceToHost, ln.stream));
  return WCT_OK;
}

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

int pad_cout(int c) {
  if (c <= 16) return 16;
  if (c <= 32) return 32;
  if (c <= 64) return 64;
  return (c + 127) / 128 * 128;
}

bool valid_level(int l) { return l >= 1 && l <= 5; }

constexpr int OK_SLOTS = 63;   // deferred solve outcomes per API call (a cascade has at most 4 C > 128 levels x 2 sides x num_run); see with_deferred_solves

// ---- profiling wrapper -----------------------------------------------------------------------------
struct ProfScope {
  wct_ctx* ctx;
  hipStream_t st;
  bool on;
  ProfRec r;
  ProfScope(wct_ctx* c, hipStream_t stream, const char* name, double flops, double bytes) : ctx(c), st(stream), on(c->prof) {
    if (!on) return;
    r.name = name; r.flops = flops; r.bytes = bytes; r.side = stream == c->side.stream;
    wct_launch_form = LaunchForm{0, 0, false, {0}};
    (void)hipEventCreate(&r.e0); (void)hipEventCreate(&r.e1);
    (void)hipEventRecord(r.e0, st);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(r.e1, st);
    // debug key "prof_forms": what the size-selected launcher inside this scope chose, e.g. "dec_tail_fused<16-16-3>#u16m"
    if (ctx->prof_forms && wct_launch_form.text[0]) {
      r.name += ":";                       // ':' not '#': tests tell the conv forms from everything else by the '#'
      r.name += wct_launch_form.text;      // the plan-driven launchers' own suffix (moments family, folds)
    } else if (ctx->prof_forms && wct_launch_form.form) {
      char sfx[16];
      snprintf(sfx, sizeof sfx, "#%c%d%s", wct_launch_form.form, wct_launch_form.tile_h, wct_launch_form.multi ? "m" : "");
      r.name += sfx;
    }
    ctx->recs.push_back(r);
  }
};

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

// pack OIHW host weights into [chunk][tap][kq][cout_pad][4]; optional conv0 fold (first encoder conv)
void pack_weights(const float* w, const float* b, int cout, int cin, int cout_pad, bool in3, const float* c0w,
                  const float* c0b, std::vector<float>& wpk, std::vector<float>& bias) {
  bias.assign(cout_pad, 0.f);
  if (in3) {
    // [tap][k = cin 0..3][cout_pad];  W'[o][i][t] = sum_c W[o][c][t] * W0[c][i],  b' = b + sum_{c,t} W[o][c][t] b0[c]
    wpk.assign((size_t)36 * cout_pad, 0.f);
    for (int o = 0; o < cout; ++o) {
      double bb = b[o];
      for (int t = 0; t < 9; ++t)
        for (int i = 0; i < 3; ++i) {
          double s = 0.;
          for (int c = 0; c < 3; ++c) {
            const double wv = w[((size_t)o * 3 + c) * 9 + t];
            s += c0w ? wv * c0w[c * 3 + i] : (c == i ? wv : 0.);
          }
          wpk[((size_t)t * 4 + i) * cout_pad + o] = (float)s;
        }
      if (c0b)
        for (int c = 0; c < 3; ++c)
          for (int t = 0; t < 9; ++t) bb += (double)w[((size_t)o * 3 + c) * 9 + t] * c0b[c];
      bias[o] = (float)bb;
    }
    return;
  }
  const int chunks = (cin + 15) / 16;
  wpk.assign((size_t)chunks * 36 * cout_pad * 4, 0.f);
  for (int o = 0; o < cout; ++o) {
    bias[o] = b[o];
    for (int i = 0; i < cin; ++i) {
      const int chunk = i / 16, kq = (i % 16) / 4, r = i % 4;
      for (int t = 0; t < 9; ++t)
        wpk[((((size_t)chunk * 9 + t) * 4 + kq) * cout_pad + o) * 4 + r] = w[((size_t)o * cin + i) * 9 + t];
    }
  }
}

// split-f16 packing of a static layer: [chunk][taps][hl][kh][cout_pad] x 8 halfs, scaled by 2^e with
// max|w| * 2^e in [256, 512) so that the lo parts are normal f16 numbers; returns 2^-e
float pack_weights_f16(const float* w, int cout, int cin, int cout_pad, int taps, std::vector<_Float16>& out) {
  float mx = 0.f;
  for (size_t i = 0; i < (size_t)cout * cin * 9; ++i) mx = std::max(mx, std::fabs(w[i]));
  int ex = 0;
  if (mx > 0.f && std::isfinite(mx)) { (void)std::frexp(mx, &ex); ex = 9 - ex; }
  const float scale = std::ldexp(1.f, ex);
  const int chunks = (cin + 15) / 16;
  out.assign((size_t)chunks * taps * 4 * cout_pad * 8, (_Float16)0.f);
  for (int o = 0; o < cout; ++o)
    for (int i = 0; i < cin; ++i) {
      const int chunk = i / 16, kh = (i % 16) / 8, j = i % 8;
      for (int t = 0; t < 9; ++t) {
        const float x = w[((size_t)o * cin + i) * 9 + t] * scale;
        const _Float16 h = (_Float16)x;
        const _Float16 l = (_Float16)(x - (float)h);
        const size_t base = ((size_t)chunk * taps + t) * 4;
        out[((base + 0 * 2 + kh) * cout_pad + o) * 8 + j] = h;
        out[((base + 1 * 2 + kh) * cout_pad + o) * 8 + j] = l;
      }
    }
  return std::ldexp(1.f, -ex);
}

// the same split (same scale) of a layer with 3 real couts in the block-packed layout of conv_f16_dev.h c3_block_compute:
// [chunk][8 ks][hl][kq][16 m] x 8 halfs;  K-step ks: window row wy = ks >> 1, column wx = 2 (ks & 1) + (kq >> 1), channels 8 (kq & 1) + j;
// A[m = 4 (2 py + px) + cout] = w[cout][ch][wy - py][wx - px] where both offsets are in 0..2, else 0
void pack_out3_phase_f16(const float* w, int cout, int cin, std::vector<_Float16>& out) {
  float mx = 0.f;
  for (size_t i = 0; i < (size_t)cout * cin * 9; ++i) mx = std::max(mx, std::fabs(w[i]));
  int ex = 0;
  if (mx > 0.f && std::isfinite(mx)) { (void)std::frexp(mx, &ex); ex = 9 - ex; }
  const float scale = std::ldexp(1.f, ex);
  const int chunks = (cin + 15) / 16;
  out.assign((size_t)chunks * 8 * 2 * 4 * 16 * 8, (_Float16)0.f);
  for (int chunk = 0; chunk < chunks; ++chunk)
    for (int ks = 0; ks < 8; ++ks)
      for (int kq = 0; kq < 4; ++kq)
        for (int m = 0; m < 16; ++m)
          for (int j = 0; j < 8; ++j) {
            const int co = m & 3, py = m >> 3, px = (m >> 2) & 1, dy = (ks >> 1) - py, dxr = 2 * (ks & 1) + (kq >> 1) - px;
            const int ch = chunk * 16 + (kq & 1) * 8 + j;
            if (co >= cout || co >= 3 || ch >= cin || dy < 0 || dy > 2 || dxr < 0 || dxr > 2) continue;
            const float x = w[((size_t)co * cin + ch) * 9 + dy * 3 + dxr] * scale;
            const _Float16 h = (_Float16)x;
            const size_t base = ((size_t)chunk * 8 + ks) * 2;
            out[(((base + 0) * 4 + kq) * 16 + m) * 8 + j] = h;
            out[(((base + 1) * 4 + kq) * 16 + m) * 8 + j] = (_Float16)(x - (float)h);
          }
}

// A 3x3 convolution (reflect padding) of a nearest-x2 upsampled map U[y][x] = X[y >> 1][x >> 1]:  an output row y = 2Y + a reads
// U rows y - 1, y, y + 1 = X rows (Y - 1, Y, Y) for a = 0 and (Y, Y, Y + 1) for a = 1 -- two distinct rows, the taps that fall on
// the same row summed; columns alike.  So each output parity (a, b) is a 2x2 convolution of X with window origin
// (Y - 1 + a, X - 1 + b) and weights  Wab[i][j] = SUM_{dy in R(a,i)} SUM_{dx in R(b,j)} w[dy][dx],  R(0,0) = {0}, R(0,1) = {1,2},
// R(1,0) = {0,1}, R(1,1) = {2}: 4 instead of 9 products per output and channel pair.  (U's reflect padding maps to CLAMPING X's
// coordinates: U[-1] = U[1] = X[0], U[H] = U[H - 2] = X[H/2 - 1].)  Sums in double, then the usual scaled hi/lo split.
// Layout for 16 -> 16: [phase 2a + b][i][hl][kq][16 couts] x 8 halfs; K = 32 per tap row: kq -> column j = kq >> 1, channels
// 8 (kq & 1) + e.  Returns 2^-e of its own scale.
float pack_up_phase_f16(const float* w, int cout, int cin, std::vector<_Float16>& out) {
  static const int R0[2][2] = {{0, 1}, {0, 2}}, R1[2][2] = {{0, 2}, {1, 2}};   // [a][i] -> first / last tap of the run R(a, i)
  std::vector<double> comb((size_t)4 * 2 * 2 * 16 * 16, 0.0);   // [p][i][j][co][ch]
  double mx = 0.0;
  for (int pa = 0; pa < 2; ++pa)
    for (int pb = 0; pb < 2; ++pb)
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
          for (int co = 0; co < cout && co < 16; ++co)
            for (int ch = 0; ch < cin && ch < 16; ++ch) {
              double sum = 0.0;
              for (int dy = R0[pa][i]; dy <= R1[pa][i]; ++dy)
                for (int dx = R0[pb][j]; dx <= R1[pb][j]; ++dx) sum += (double)w[((size_t)co * cin + ch) * 9 + dy * 3 + dx];
              comb[(((((size_t)(pa * 2 + pb) * 2 + i) * 2 + j) * 16 + co) * 16) + ch] = sum;
              mx = std::max(mx, std::fabs(sum));
            }
  int ex = 0;
  if (mx > 0.0 && std::isfinite(mx)) { (void)std::frexp((float)mx, &ex); ex = 9 - ex; }
  const float scale = std::ldexp(1.f, ex);
  out.assign((size_t)4 * 2 * 2 * 4 * 16 * 8, (_Float16)0.f);
  for (int p = 0; p < 4; ++p)
    for (int i = 0; i < 2; ++i)
      for (int kq = 0; kq < 4; ++kq)
        for (int co = 0; co < 16; ++co)
          for (int e = 0; e < 8; ++e) {
            const int j = kq >> 1, ch = 8 * (kq & 1) + e;
            const float x = (float)(comb[(((((size_t)p * 2 + i) * 2 + j) * 16 + co) * 16) + ch] * (double)scale);
            const _Float16 h = (_Float16)x;
            const size_t base = ((size_t)p * 2 + i) * 2;
            out[(((base + 0) * 4 + kq) * 16 + co) * 8 + e] = h;
            out[(((base + 1) * 4 + kq) * 16 + co) * 8 + e] = (_Float16)(x - (float)h);
          }
  return std::ldexp(1.f, -ex);
}

// The same per-parity weights for the DMA kernel's upsample form (conv3x3_sp.hip conv3x3_sp_up_kernel), any cin % 16 == 0 and cout:
// [chunk][a][r = (((b * 2 + i) * 2 + j) * 2 + hl) * 2 + kh][cout_pad] x 8 halfs (channels chunk * 16 + kh * 8 + e).  Returns 2^-e.
float pack_up_sp_f16(const float* w, int cout, int cin, int cout_pad, std::vector<_Float16>& out) {
  static const int R0[2][2] = {{0, 1}, {0, 2}}, R1[2][2] = {{0, 2}, {1, 2}};
  const int chunks = (cin + 15) / 16;
  auto comb = [&](int co, int ch, int pa, int pb, int i, int j) {
    double sum = 0.0;
    for (int dy = R0[pa][i]; dy <= R1[pa][i]; ++dy)
      for (int dx = R0[pb][j]; dx <= R1[pb][j]; ++dx) sum += (double)w[((size_t)co * cin + ch) * 9 + dy * 3 + dx];
    return sum;
  };
  double mx = 0.0;
  for (int co = 0; co < cout; ++co)
    for (int ch = 0; ch < cin; ++ch)
      for (int k = 0; k < 16; ++k) mx = std::max(mx, std::fabs(comb(co, ch, k >> 3, (k >> 2) & 1, (k >> 1) & 1, k & 1)));
  int ex = 0;
  if (mx > 0.0 && std::isfinite(mx)) { (void)std::frexp((float)mx, &ex); ex = 9 - ex; }
  const double scale = std::ldexp(1.0, ex);
  out.assign((size_t)chunks * 2 * 32 * cout_pad * 8, (_Float16)0.f);
  for (int co = 0; co < cout; ++co)
    for (int ch = 0; ch < cin; ++ch) {
      const int chunk = ch / 16, kh = (ch % 16) / 8, e = ch % 8;
      for (int pa = 0; pa < 2; ++pa)
        for (int pb = 0; pb < 2; ++pb)
          for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
              const float x = (float)(comb(co, ch, pa, pb, i, j) * scale);
              const _Float16 h = (_Float16)x;
              const size_t row = (size_t)(chunk * 2 + pa) * 32 + (size_t)((((pb * 2 + i) * 2 + j) * 2) * 2);
              out[((row + 0 * 2 + kh) * cout_pad + co) * 8 + e] = h;
              out[((row + 1 * 2 + kh) * cout_pad + co) * 8 + e] = (_Float16)(x - (float)h);
            }
    }
  return (float)std::ldexp(1.0, -ex);
}

// split-f16 packing of the 3-channel first conv for the fused encoder head (conv3x3_f16.hip enc_head_kernel) and the level-1
// kernels (conv_f16_dev.h l1_conv_group): K = 4 steps of 32 halfs in "singles" of 4 (one window pixel's RGB0; term 0: w_hi . x_hi,
// 1: w_hi . x_lo, 2: w_lo . x_hi; pos = 3 dy + dx); lane group kq of step s holds the singles l1_single(s, kq, 0 / 1) of
// wct_common.h, 27 real ones, the rest zero.  Layout [cout tile][s][kq][16 couts] x 8 halfs.  in3: the fp32 packing
// [tap][4][cout_pad] (conv0 already folded).  Returns 2^-e.
float pack_head_f16(const std::vector<float>& in3, int cout_pad, int ntile, std::vector<_Float16>& out) {
  float mx = 0.f;
  for (float x : in3) mx = std::max(mx, std::fabs(x));
  int ex = 0;
  if (mx > 0.f && std::isfinite(mx)) { (void)std::frexp(mx, &ex); ex = 9 - ex; }
  const float scale = std::ldexp(1.f, ex);
  out.assign((size_t)ntile * 4 * 4 * 16 * 8, (_Float16)0.f);
  for (int ct = 0; ct < ntile; ++ct)
    for (int s = 0; s < 4; ++s)
      for (int kq = 0; kq < 4; ++kq)
        for (int oo = 0; oo < 16; ++oo)
          for (int j = 0; j < 8; ++j) {
            const L1Single t = l1_single(s, kq, j >> 2);     // wct_common.h: the K order shared with the kernels
            const int ch = j & 3, o = ct * 16 + oo;
            if (t.zero || ch > 2 || o >= cout_pad) continue;
            const float x = in3[((size_t)t.pos * 4 + ch) * cout_pad + o] * scale;
            const _Float16 h = (_Float16)x;
            out[((((size_t)ct * 4 + s) * 4 + kq) * 16 + oo) * 8 + j] = t.term == 2 ? (_Float16)(x - (float)h) : h;
          }
  return std::ldexp(1.f, -ex);
}

int upload(wct_ctx* ctx, float** dst, const std::vector<float>& v) {
  HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(dst), v.size() * sizeof(float)));
  HIPCHK(ctx, hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return WCT_OK;
}

void free_module(Module& m) {
  for (auto& l : m.layers) {
    if (l.w_oihw) (void)hipFree(l.w_oihw);
    if (l.fold_rows) (void)hipFree(l.fold_rows);
    if (l.bias_raw) (void)hipFree(l.bias_raw);
    if (l.wpk) (void)hipFree(l.wpk);
    if (l.wpk16) (void)hipFree(l.wpk16);
    if (l.l1w16) (void)hipFree(l.l1w16);
    if (l.wph16) (void)hipFree(l.wph16);
    if (l.wup16) (void)hipFree(l.wup16);
    if (l.l1bias) (void)hipFree(l.l1bias);
    if (l.bias) (void)hipFree(l.bias);
  }
  m.layers.clear();
  m.loaded = false;
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

struct SumsView { double *sum, *sumsq; int* info; };

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

// (n, sum, sumsq) of one feature map -> EigResult in `res` (covariance, Jacobi eigen-decomposition)
// ot_sched: the matrix is the ot transform's B = S cov_c S entering as pseudo-moments (transform_mb) -- its own iteration schedule, never + I
int eig_impl(wct_ctx* ctx, Lane& ln, int C, double n, const double* sum, const double* sumsq, int inverse, DevBuf& res, int* info_dev, bool ot_sched = false) {
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

// --mode original: run `body` with the C > 128 solves' outcomes deferred (no stream synchronisation inside the solves: the host
// enqueues the whole call, so the style lane really overlaps the content lane), then ONE synchronisation and a look at the
// outcomes; if an iteration did not converge (singular beyond the deflation, NaN) the call is repeated the synchronous way,
// where each solve falls back to the global-memory Jacobi on the spot.  The 16x path (C <= 128) never synchronises.
template <typename BODY>
int with_deferred_solves(wct_ctx* ctx, bool wait_side, BODY&& body) {
  if (!ctx->wide_model) return body();
  ctx->defer_big = true;
  ctx->ok_n = 0;
  // the counter as of NOW, in stream order (everything enqueued before this call -- wct_encode / wct_decode / ... included -- has
  // counted by then): what a failed optimistic pass is rolled back to.  (It used to be rolled back to a host-side mark taken at the
  // last verified wide-model call, which erased clamps raised since by the non-deferred entry points: ADVICE r3.)
  HIPCHK(ctx, hipMemcpyAsync(ctx->sat_dev + 1, ctx->sat_dev, sizeof(unsigned), hipMemcpyDeviceToDevice, ctx->main.stream));
  int rc = body();
  ctx->defer_big = false;
  const int n = ctx->ok_n;
  ctx->ok_n = 0;
  if (rc) return rc;
  if (n == 0) return WCT_OK;
  if (wait_side) HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->ok_host, ctx->ok_log, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->main.stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->ok_host + OK_SLOTS, ctx->sat_dev, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->main.stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->main.stream));
  bool all = true;
  for (int i = 0; i < n; ++i) all = all && ctx->ok_host[i] == 1;
  if (all) return WCT_OK;
  // the optimistic pass ran its decoders on unconverged matrix functions: whatever it clamped says nothing about the real result --
  // put the saturation counter back to where it stood when this call began before repeating the call
  HIPCHK(ctx, hipStreamSynchronize(ctx->side.stream));
  unsigned before = 0;
  HIPCHK(ctx, hipMemcpy(&before, ctx->sat_dev + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
  HIPCHK(ctx, hipMemcpy(ctx->sat_dev, &before, sizeof(unsigned), hipMemcpyHostToDevice));
  range_host_set(ctx, before);
  return body();     // defer_big is off: every solve checks (and repairs) itself
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

// the style-side part of the fast fold for `level`, on `st`, from the style EigResult in ctx->eigS[level] (F = cov_s^(1/2), mu_s)
bool fast_fold_level(const wct_ctx* ctx, int level) {
  const Module& m = ctx->mod[WCT_KIND_DEC][level];
  return ctx->fastfold && m.loaded && m.layers[0].w_oihw && fold_fast_capable(m.layers[0].d.cin);
}

int style_fold(wct_ctx* ctx, int level, hipStream_t st) {
  ctx->fold_ready[level] = false;
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
int style_side(wct_ctx* ctx, int level, const float* style, int Hs, int Ws, int slot = -1) {
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

// The five levels 5..1 of WCT.py:120-125, num_run times over.  `out` doubles as the running image: level L reads one buffer and
// writes the other (ping-pong with tmpT), the parity chosen so that the last level writes into `out`.
//   level_fn(level, cur, h, w, dst, &ho, &wo): level L of the h x w image `cur` into `dst`, ho x wo
//   after_level(level): in the first run behind every level L > 1 -- where a caller enqueues the style side of level L - 1
// Deferred solves and the range read-back stay with the caller: the entry points place them differently.
template <typename LEVEL, typename AFTER>
int run_cascade(wct_ctx* ctx, const float* content, int H, int W, int num_run, float* out, int* Ho, int* Wo, LEVEL&& level_fn, AFTER&& after_level) {
  if (int rc = ensure(ctx, ctx->tmpT, (size_t)3 * H * W * sizeof(float))) return rc;
  float* bufs[2] = {reinterpret_cast<float*>(ctx->tmpT.p), out};
  const float* cur = content;
  int h = H, w = W, which = (5 * num_run) & 1;
  for (int run = 0; run < num_run; ++run)
    for (int level = 5; level >= 1; --level) {
      int ho = 0, wo = 0;
      float* dst = bufs[which];
      if (int rc = level_fn(level, cur, h, w, dst, &ho, &wo)) return rc;
      if (run == 0 && level > 1)
        if (int rc = after_level(level)) return rc;
      cur = dst; h = ho; w = wo; which ^= 1;
    }
  if (cur != out) HIPCHK(ctx, hipMemcpyAsync(out, cur, (size_t)3 * h * w * sizeof(float), hipMemcpyDeviceToDevice, ctx->main.stream));
  if (Ho) *Ho = h;
  if (Wo) *Wo = w;
  return WCT_OK;
}

// an NHWC map operation apply_nhwc(in, out) on an NCHW map of npix pixels: transposed through the two halves of tmpT
template <typename APPLY>
int apply_nchw(wct_ctx* ctx, const float* feat, int C, long npix, float* out, APPLY&& apply_nhwc) {
  if (int rc = ensure(ctx, ctx->tmpT, 2 * (size_t)npix * C * sizeof(float))) return rc;
  float* t0 = reinterpret_cast<float*>(ctx->tmpT.p);
  float* t1 = t0 + (size_t)npix * C;
  HIPCHK(ctx, launch_nchw_to_nhwc(feat, t0, C, (int)npix, ctx->main.stream));
  if (int rc = apply_nhwc(t0, t1)) return rc;
  HIPCHK(ctx, launch_nhwc_to_nchw(t1, out, C, (int)npix, ctx->main.stream));
  return WCT_OK;
}

}  // namespace

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
  if (ctx->comm && ctx->comm_owned && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(ctx->comm);
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
  else return fail(ctx, WCT_ERR_INVALID, "debug_set: unknown key '%s' (fuse, sp, l1fuse, u8fuse, upconv, fastfold, interleave, foldgemm, nscoop, in3wide, mom32, eig_skip, side_priority, poison, prof_forms, swap_key_chunk)", key);
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

int wct_load_module(wct_ctx* ctx, int kind, int level, int n_layers, const wct_layer* layers, const float* c0w,
                    const float* c0b) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if ((kind != WCT_KIND_ENC && kind != WCT_KIND_DEC) || !valid_level(level) || n_layers < 1 || !layers)
    return fail(ctx, WCT_ERR_INVALID, "load_module: bad kind/level/layers (%d, %d, %d)", kind, level, n_layers);
  for (int i = 0; i < n_layers; ++i) {
    const wct_layer& L = layers[i];
    if (!L.weight || !L.bias || L.cin < 1 || L.cout < 1 || L.cin > 512 || L.cout > 512)
      return fail(ctx, WCT_ERR_INVALID, "load_module: layer %d has bad shape %d->%d or NULL weights", i, L.cin, L.cout);
    if (i > 0 && layers[i - 1].cout != L.cin) return fail(ctx, WCT_ERR_INVALID, "load_module: layer %d cin %d != previous cout %d", i, L.cin, layers[i - 1].cout);
    const bool first = i == 0, last = i == n_layers - 1;
    if (kind == WCT_KIND_ENC && first && L.cin != 3) return fail(ctx, WCT_ERR_INVALID, "encoder must start from 3 channels");
    if (kind == WCT_KIND_DEC && last && L.cout != 3) return fail(ctx, WCT_ERR_INVALID, "decoder must end in 3 channels");
    if (!(kind == WCT_KIND_ENC && first) && (L.cin & 3)) return fail(ctx, WCT_ERR_INVALID, "layer %d: cin %d must be a multiple of 4", i, L.cin);
    if (!(kind == WCT_KIND_DEC && last) && (L.cout & 3)) return fail(ctx, WCT_ERR_INVALID, "layer %d: cout %d must be a multiple of 4", i, L.cout);
    for (size_t e = 0; e < (size_t)L.cout * L.cin * 9; ++e)
      if (!std::isfinite(L.weight[e])) return fail(ctx, WCT_ERR_INVALID, "load_module: layer %d has a non-finite weight", i);
    for (int e = 0; e < L.cout; ++e)
      if (!std::isfinite(L.bias[e])) return fail(ctx, WCT_ERR_INVALID, "load_module: layer %d has a non-finite bias", i);
    if (kind == WCT_KIND_ENC && last && L.pool_after) return fail(ctx, WCT_ERR_INVALID, "encoder cannot end in a pool");
    // shapes no conv kernel runs (launch_conv3x3 / launch_conv3x3_f16 would refuse them at the first encode or decode)
    if (kind == WCT_KIND_ENC && first && L.cout > 64)
      return fail(ctx, WCT_ERR_INVALID, "load_module: the first encoder conv has %d output channels; at most 64 are supported", L.cout);
    if (kind == WCT_KIND_ENC && first && L.pool_after) return fail(ctx, WCT_ERR_INVALID, "load_module: the first encoder conv cannot pool");
    if (kind == WCT_KIND_ENC && L.up_after) return fail(ctx, WCT_ERR_INVALID, "load_module: encoder layer %d cannot upsample", i);
    if (kind == WCT_KIND_DEC && L.pool_after) return fail(ctx, WCT_ERR_INVALID, "load_module: decoder layer %d cannot pool", i);
    if (kind == WCT_KIND_DEC && last && L.up_after) return fail(ctx, WCT_ERR_INVALID, "decoder cannot end in an upsample");
  }
  Module& m = ctx->mod[kind][level];
  free_module(m);
  ctx->fold_ready[level] = false;   // a style-side fold of the old decoder is stale
  m.layers.resize(n_layers);
  for (int i = 0; i < n_layers; ++i) {
    const wct_layer& L = layers[i];
    LayerDev& ld = m.layers[i];
    const bool in3 = kind == WCT_KIND_ENC && i == 0;
    const bool out3 = kind == WCT_KIND_DEC && i == n_layers - 1;
    ld.pool_after = L.pool_after; ld.up_after = L.up_after;
    ld.d.cin = L.cin; ld.d.cout = L.cout;
    ld.d.sat = ctx->sat_dev;
    ld.d.cin_chunks = in3 ? 1 : (L.cin + 15) / 16;
    ld.d.cout_pad = pad_cout(L.cout);
    ld.d.flags = (in3 ? CONV_IN_NCHW3 : 0) | (out3 ? CONV_OUT_NCHW3 : 0) | (L.pool_after ? CONV_POOL_OUT : 0) |
                 ((kind == WCT_KIND_DEC && i > 0 && layers[i - 1].up_after) ? CONV_UP_IN : 0);
    std::vector<float> wpk, bias;
    pack_weights(L.weight, L.bias, L.cout, L.cin, ld.d.cout_pad, in3, in3 ? c0w : nullptr, in3 ? c0b : nullptr, wpk, bias);
    if (int rc = upload(ctx, &ld.wpk, wpk)) return rc;
    if (int rc = upload(ctx, &ld.bias, bias)) return rc;
    ld.d.wpk = ld.wpk; ld.d.bias = ld.bias;
    if (in3 && ld.d.cout_pad <= 32) {   // level-1 kernels (level1.hip): two cout tiles, bias padded to 32
      std::vector<_Float16> w16;
      ld.d.l1inv = pack_head_f16(wpk, ld.d.cout_pad, 2, w16);
      HIPCHK(ctx, hipMalloc(&ld.l1w16, w16.size() * sizeof(_Float16)));
      HIPCHK(ctx, hipMemcpy(ld.l1w16, w16.data(), w16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
      std::vector<float> b32(32, 0.f);
      for (int o = 0; o < ld.d.cout_pad && o < 32; ++o) b32[o] = bias[o];
      if (int rc = upload(ctx, &ld.l1bias, b32)) return rc;
      ld.d.l1w16 = ld.l1w16; ld.d.l1bias = ld.l1bias;
    }
    if (in3 && ld.d.cout_pad == 64 && L.cout == 64) {   // un-pruned encoders: four cout tiles for level1.hip in3_wide_kernel
      std::vector<_Float16> w16;
      ld.d.l1inv = pack_head_f16(wpk, ld.d.cout_pad, 4, w16);
      HIPCHK(ctx, hipMalloc(&ld.l1w16, w16.size() * sizeof(_Float16)));
      HIPCHK(ctx, hipMemcpy(ld.l1w16, w16.data(), w16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
      if (int rc = upload(ctx, &ld.l1bias, bias)) return rc;
      ld.d.l1w16 = ld.l1w16; ld.d.l1bias = ld.l1bias;
    }
    if (in3 && ld.d.cout_pad == 16) {
      std::vector<_Float16> w16;
      ld.d.inv_scale = pack_head_f16(wpk, 16, 1, w16);
      HIPCHK(ctx, hipMalloc(&ld.wpk16, w16.size() * sizeof(_Float16)));
      HIPCHK(ctx, hipMemcpy(ld.wpk16, w16.data(), w16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
      ld.d.wpk16 = ld.wpk16;
    }
    if (!in3) {
      std::vector<_Float16> w16;
      const int taps = ld.d.cout_pad == 16 ? 10 : 9;
      ld.d.inv_scale = pack_weights_f16(L.weight, L.cout, L.cin, ld.d.cout_pad, taps, w16);
      HIPCHK(ctx, hipMalloc(&ld.wpk16, w16.size() * sizeof(_Float16)));
      HIPCHK(ctx, hipMemcpy(ld.wpk16, w16.data(), w16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
      ld.d.wpk16 = ld.wpk16;
      if ((ld.d.flags & CONV_UP_IN) && ld.d.cout_pad >= 32 && (L.cin % 16) == 0 && !out3 && !L.pool_after) {   // ... for the DMA kernel
        std::vector<_Float16> wup;
        ld.d.inv_scale_up = pack_up_sp_f16(L.weight, L.cout, L.cin, ld.d.cout_pad, wup);
        HIPCHK(ctx, hipMalloc(&ld.wup16, wup.size() * sizeof(_Float16)));
        HIPCHK(ctx, hipMemcpy(ld.wup16, wup.data(), wup.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        ld.d.wup16 = ld.wup16;
      }
      if ((ld.d.flags & CONV_UP_IN) && L.cin == 16 && L.cout == 16) {   // per-parity 2x2 form for the fused tail's first conv
        std::vector<_Float16> wup;
        ld.d.inv_scale_up = pack_up_phase_f16(L.weight, L.cout, L.cin, wup);
        HIPCHK(ctx, hipMalloc(&ld.wup16, wup.size() * sizeof(_Float16)));
        HIPCHK(ctx, hipMemcpy(ld.wup16, wup.data(), wup.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        ld.d.wup16 = ld.wup16;
      }
      if (out3 && ld.d.cout_pad == 16) {   // block-packed form for the fused tails
        std::vector<_Float16> wph;
        pack_out3_phase_f16(L.weight, L.cout, L.cin, wph);
        HIPCHK(ctx, hipMalloc(&ld.wph16, wph.size() * sizeof(_Float16)));
        HIPCHK(ctx, hipMemcpy(ld.wph16, wph.data(), wph.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        ld.d.wph16 = ld.wph16;
      }
    }
    if (kind == WCT_KIND_DEC && i == 0) {
      std::vector<float> raw(L.weight, L.weight + (size_t)L.cout * L.cin * 9), rb(L.bias, L.bias + L.cout);
      if (int rc = upload(ctx, &ld.w_oihw, raw)) return rc;
      if (int rc = upload(ctx, &ld.bias_raw, rb)) return rc;
      if (fold_gemm_capable(L.cout, L.cin, ld.d.cout_pad)) {
        HIPCHK(ctx, hipMalloc(reinterpret_cast<void**>(&ld.fold_rows), fold_gemm_rows_doubles(L.cout, L.cin) * sizeof(double)));
        HIPCHK(ctx, launch_fold_rows(ld.w_oihw, L.cout, L.cin, ld.fold_rows, nullptr));
        HIPCHK(ctx, hipDeviceSynchronize());
      }
    }
  }
  m.loaded = true;
  // a loaded encoder ends wider than 128 channels (--mode original): recomputed over ALL loaded encoders on every load, so
  // that re-loading narrower modules clears it
  ctx->wide_model = false;
  for (int l = 1; l <= 5; ++l) {
    const Module& e = ctx->mod[WCT_KIND_ENC][l];
    if (e.loaded && e.layers.back().d.cout > 128) ctx->wide_model = true;
  }
  return WCT_OK;
}

int wct_feature_shape(const wct_ctx* ctx, int level, int H, int W, int* C, int* h, int* w) {
  if (!ctx || !valid_level(level) || H < 1 || W < 1) return WCT_ERR_INVALID;
  const Module& m = ctx->mod[WCT_KIND_ENC][level];
  if (!m.loaded) return WCT_ERR_STATE;
  for (int i = 1; i < level; ++i) { H /= 2; W /= 2; }
  if (C) *C = m.layers.back().d.cout;
  if (h) *h = H;
  if (w) *w = W;
  return WCT_OK;
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

// the column-sharded cascade and its transport table (wct_stylize_sharded, wct_comm_attach_collectives, ...): same translation unit
#include "wct_sharded_impl.h"

extern "C" {

// ---------------------------------------------------------------------------------------------------------------------
// RCCL inside the boundary ("multi-GPU variant takes an ncclComm_t").  One level of a column-sharded cascade is ONE call:
// encoder + raw moments over the owned feature columns -> ncclAllReduce(SUM, fp64) of [sum | sumsq | range flag] on the context's
// stream -> matrix functions against the level's (imported) style statistics -> fold -> decoder.  RCCL's entry points are looked up
// at run time in the librccl the host process names (wct_comm_load; the Python mirror passes the one torch has loaded), so the
// library links against nothing new and single-GPU users never touch RCCL.
namespace {
int rccl_ready(wct_ctx* ctx) {
  if (g_rccl.AllReduce) return WCT_OK;
  return fail(ctx, WCT_ERR_STATE, "RCCL is not loaded: call wct_comm_load(path of librccl.so) first");
}
}  // namespace

int wct_comm_load(const char* path) {
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  if (g_rccl.AllReduce) return WCT_OK;
  // an explicit path is THE library the host process uses (torch's bundled librccl.so): if it cannot be opened, fail -- mapping a second,
  // different RCCL into the process silently is worse than an error.  Without a path: the loader's search path, then /opt/rocm.
  const char* search[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"};
  void* h = nullptr;
  if (path && *path) {
    h = dlopen(path, RTLD_NOW | RTLD_LOCAL);      // a library the process has already mapped is reused, not loaded twice
    if (h) g_rccl.path = path;
  } else {
    for (const char* c : search) {
      h = dlopen(c, RTLD_NOW | RTLD_LOCAL);
      if (h) { g_rccl.path = c; break; }
    }
  }
  if (!h) return WCT_ERR_STATE;
  RcclApi api;
  api.lib = h;
  api.path = g_rccl.path;
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
  api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(h, "ncclAllReduce"));
  api.Broadcast = reinterpret_cast<decltype(api.Broadcast)>(dlsym(h, "ncclBroadcast"));
  api.Send = reinterpret_cast<decltype(api.Send)>(dlsym(h, "ncclSend"));
  api.Recv = reinterpret_cast<decltype(api.Recv)>(dlsym(h, "ncclRecv"));
  api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(h, "ncclGroupStart"));
  api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(h, "ncclGroupEnd"));
  if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllReduce || !api.Broadcast || !api.Send || !api.Recv || !api.GroupStart || !api.GroupEnd) {
    g_rccl.path.clear();
    return WCT_ERR_STATE;
  }
  g_rccl = api;
  return WCT_OK;
}

const char* wct_comm_library(void) { return g_rccl.AllReduce ? g_rccl.path.c_str() : ""; }

int wct_comm_unique_id(unsigned char* id128) {
  if (!g_rccl.AllReduce || !id128) return WCT_ERR_STATE;
  return g_rccl.GetUniqueId(id128) == 0 ? WCT_OK : WCT_ERR_HIP;
}

int wct_comm_init(wct_ctx* ctx, int nranks, int rank, const unsigned char* id128) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = rccl_ready(ctx)) return rc;
  if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, WCT_ERR_INVALID, "comm_init: bad arguments (nranks %d, rank %d)", nranks, rank);
  if (ctx->comm || ctx->coll_set) return fail(ctx, WCT_ERR_STATE, "comm_init: the context already has a communicator");
  NcclUid uid;
  memcpy(uid.b, id128, 128);
  void* comm = nullptr;
  const int r = g_rccl.CommInitRank(&comm, nranks, uid, rank);     // collective over the job's ranks; the context's device is current
  if (r != 0 || !comm) return fail(ctx, WCT_ERR_HIP, "ncclCommInitRank(%d ranks, rank %d): %s", nranks, rank, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error");
  ctx->comm = comm; ctx->comm_owned = true; ctx->comm_ranks = nranks; ctx->comm_rank = rank;
  shard::install_rccl(ctx);
  ctx->coll_set = true;
  return WCT_OK;
}

int wct_comm_attach(wct_ctx* ctx, void* nccl_comm, int nranks, int rank) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (int rc = rccl_ready(ctx)) return rc;
  if (!nccl_comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(ctx, WCT_ERR_INVALID, "comm_attach: bad arguments");
  if (ctx->comm || ctx->coll_set) return fail(ctx, WCT_ERR_STATE, "comm_attach: the context already has a communicator");
  ctx->comm = nccl_comm; ctx->comm_owned = false; ctx->comm_ranks = nranks; ctx->comm_rank = rank;
  shard::install_rccl(ctx);
  ctx->coll_set = true;
  return WCT_OK;
}

int wct_comm_destroy(wct_ctx* ctx) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (ctx->comm && ctx->comm_owned && g_rccl.CommDestroy) {
    (void)hipStreamSynchronize(ctx->main.stream);
    (void)g_rccl.CommDestroy(ctx->comm);
  }
  ctx->comm = nullptr; ctx->comm_owned = false; ctx->comm_ranks = 0; ctx->comm_rank = 0;
  ctx->coll = wct_collectives{}; ctx->coll_set = false; ctx->coll_rccl = false; ctx->shard_emulate = false;
  return WCT_OK;
}

int wct_level_sharded(wct_ctx* ctx, int level, const float* content, int H, int W, int x0, int x1, double n_total, float alpha,
                      float* out, int* Ho, int* Wo, double* range_total) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!ctx->coll_set) return fail(ctx, WCT_ERR_STATE, "level_sharded: no communicator (wct_comm_init / wct_comm_attach / wct_comm_attach_collectives)");
  if (!valid_level(level) || !content || !out || !(n_total >= 1.0)) return fail(ctx, WCT_ERR_INVALID, "level_sharded: bad arguments");
  Module& me = ctx->mod[WCT_KIND_ENC][level];
  if (!me.loaded) return fail(ctx, WCT_ERR_STATE, "encoder %d not loaded", level);
  if (!ctx->eigS[level].p) return fail(ctx, WCT_ERR_STATE, "level_sharded: no style statistics for level %d (wct_style_prepare / wct_style_import)", level);
  const int C = me.layers.back().d.cout;
  const size_t npk = (size_t)C * C + C + 1;
  if (int rc = ensure(ctx, ctx->packed, npk * sizeof(double))) return rc;
  double* pk = reinterpret_cast<double*>(ctx->packed.p);
  // the four steps below are wct_content_encode / wct_range_flag_f64 / [all-reduce] / wct_content_solve / wct_content_decode in this order,
  // on the same buffers' worth of arithmetic: results are those of the split-level path bit for bit (tests/test_sharded_gpu.py)
  int h = 0, w = 0;
  if (int rc = wct_content_encode(ctx, level, content, H, W, x0, x1, pk, pk + C, &h, &w)) return rc;
  HIPCHK(ctx, launch_counter_to_f64(ctx->sat_dev, pk + C + (size_t)C * C, ctx->main.stream));
  COLLCHK(ctx, "all-reduce (content moments)", ctx->coll.all_reduce_sum_f64(ctx->coll.user, pk, npk, ctx->main.stream));
  if (range_total) HIPCHK(ctx, hipMemcpyAsync(range_total, pk + C + (size_t)C * C, sizeof(double), hipMemcpyDeviceToDevice, ctx->main.stream));
  double *M, *b;
  if (int rc = mb_view(ctx, &M, &b)) return rc;
  if (int rc = wct_content_solve(ctx, level, n_total, pk, pk + C, alpha, M, b)) return rc;
  return wct_content_decode(ctx, level, M, b, out, Ho, Wo);
}

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

int noise_impl(wct_ctx* ctx, uint64_t seed, uint32_t stream_id, int H, int W, float* planar) {
  ProfScope ps(ctx, ctx->main.stream, "noise_uniform<philox4x32-10>", 0, 12.0 * H * W);
  HIPCHK(ctx, launch_noise_uniform(seed, stream_id, H, W, planar, ctx->main.stream));
  return WCT_OK;
}
}  // namespace

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

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + nb && b0 < a0 + na;
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

int wct_set_transform(wct_ctx* ctx, int mode) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (mode != WCT_TRANSFORM_WCT && mode != WCT_TRANSFORM_OT && mode != WCT_TRANSFORM_ADAIN) return fail(ctx, WCT_ERR_INVALID, "set_transform: mode %d outside 0..2", mode);
  if (mode != WCT_TRANSFORM_WCT && ctx->numpy_variant) return fail(ctx, WCT_ERR_INVALID, "set_transform: the numpy variant (+ I on cov_c) is defined for the wct transform only");
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

int apply_labeled_impl(wct_ctx* ctx, const float* feat, int C, long npix, const uint8_t* lab, int K, const double* M, const double* b, float* out) {
  if (int rc = ensure(ctx, ctx->wsRegApply, apply_labeled_workspace_bytes(C, K))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "apply_labeled", 2.0 * C * C * npix, 8.0 * C * npix + npix);
  HIPCHK(ctx, launch_apply_labeled(feat, C, npix, lab, K, M, b, out, ctx->wsRegApply.p, ctx->wsRegApply.cap, ctx->main.stream));
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

// dst = W (feat - mu), W = cov^(-1/2) of the map itself: wct_moments + wct_transform_solve(WCT_TRANSFORM_WCT, [I, 0], alpha = 1) + wct_apply_labeled
int swap_whiten(wct_ctx* ctx, const float* feat, int C, int h, int w, float* dst) {
  Lane& ln = ctx->main;
  SumsView sv;
  if (int rc = sums_view(ctx, ln, sv)) return rc;
  double *M, *b;
  if (int rc = mb_view(ctx, &M, &b)) return rc;
  if (int rc = moments_impl(ctx, ln, feat, C, h, w, 0, w, sv.sum, sv.sumsq)) return rc;
  if (int rc = solve_against_slot(ctx, WCT_TRANSFORM_WCT, C, (double)h * w, sv.sum, sv.sumsq, nullptr, 1.0, M, b, sv.info)) return rc;
  const long npix = (long)h * w;
  HIPCHK(ctx, hipMemsetAsync(ctx->swLab.p, 0, (size_t)npix, ln.stream));
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
