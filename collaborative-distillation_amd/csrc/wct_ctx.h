// What the host translation units behind the C ABI share (wct_api.hip and the api_*.hip files): the context, its error / device / profiling
// helpers, the driver templates, and the declarations of the internals that more than one file calls (namespace wct_host; each is defined
// in exactly one .hip file).  Private to csrc/: not installed, never included from include/.  A helper only one file uses stays in that
// file's anonymous namespace.
#pragma once
#include "../../include/wct_hip.h"
#include "../../include/wct_hip_transform.h"
#include "wct_common.h"

#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <atomic>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace wct_host {

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

}  // namespace wct_host

// wct_ctx is the C ABI's global struct; its field types are named unqualified.  The internals below are not: a host file says
// `using namespace wct_host;` itself.
using wct_host::DevBuf;
using wct_host::Lane;
using wct_host::Module;
using wct_host::ProfRec;
using wct_host::ResizeAxis;

struct wct_clip;   // the state of one frame sequence (include/wct_hip_video.h; defined in wct_clip.h)

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
  // proxy mode (include/wct_hip_bgrid.h): the fit's sums and partial sums, and for wct_stylize_proxy the reduced content, its
  // stylisation and the grid
  DevBuf bgWs, bgGrid, pxCl, pxSl;
  // the device JPEG encoder (include/wct_hip_jpeg.h): the coefficients of wct_jpeg_encode, the blocks' bit offsets and the scans' partial sums,
  // and the unstuffed stream
  DevBuf jpCoef, jpWs, jpStream;
  // the device JPEG decoder (include/wct_hip_jdec.h): the coefficients of wct_jdec_decode, the unstuffing's counts with the anchors, states,
  // block offsets and DC partial sums, the compacted stream, and the component planes of wct_jdec_pixels
  DevBuf jdCoef, jdWs, jdStream, jdPlanes;
  int bgrid_lds = 1;   // debug key "bgrid_lds": 0 = the slice reads every tile's vertices from global memory (same bits)
  // patch swap (include/wct_hip_swap.h): the two encoded features, the two projected maps, the blended feature, the indices, the running
  // (score, index) of every query between the key chunks' launches, the key norms, and the all-zero label map of the one-label affine apply
  DevBuf swFc, swFs, swQ, swK, swOut, swIdx, swRun, swNorm, swLab;
  int swap_key_chunk = 0;   // debug key "swap_key_chunk": keys per launch of the match; 0 = WCT_SWAP_KEY_CHUNK
  // attention statistics (include/wct_hip_attn.h): the two encoded features, the standardised maps and the unit rows of both sides, the
  // whitened map in front of its unit rows, (mean, var), the blended feature, and [mu_s | sigma_s | partial maxima of |V| | scale of V^2]
  // ... and the transposed whitening matrix of the whitened domain [C * C doubles]
  DevBuf atFc, atFs, atCs, atSs, atQ, atK, atProj, atMean, atVar, atOut, atStat, atMt;
  int attn_query_chunk = 0;   // debug key "attn_query_chunk": queries per launch of the statistics; 0 = WCT_ATTN_QUERY_CHUNK
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
  // video mode (include/wct_hip_video.h): set ONLY for the duration of wct_stylize_clip -- content_side then passes every level's content
  // sums through the clip's tracking step.  The clip's memory is the clip's own: no DevBuf of the context, nothing for each_buf
  wct_clip* track = nullptr;
  // motion compensation (include/wct_hip_motion.h), the standalone entries: [pyramid of cur | pyramid of prev | the coarser levels' fields]
  DevBuf motionWs;
  int clip_channels = 0;               // debug key "clip_channels": the channel count of every level of clips created from now on; 0: the loaded encoders'
  // style diversification (include/wct_hip_diverse.h): the rotation's workspace (rotate.hip rotation_workspace_bytes) and [Z C*C | the slot's F
  // before the product C*C]; neither is part of wct_reserve / wct_workspace_bytes.  rotated[level]: the slot holds F Z, no longer the symmetric
  // cov_s^(1/2) -- set by wct_style_diversify, cleared by style_fold, which everything that rewrites a slot ends with
  DevBuf dvWs, dvZ;
  bool rotated[6] = {false, false, false, false, false, false};

  // EVERY DevBuf of the context, once, with its class: f(buf, owning lane, scratch).  Scratch = no later call is documented to read
  // what an earlier call left there, so the "poison" hook may overwrite it between calls; state must survive (style slots, the
  // style-side folds, and the content feature / image of an open wct_content_encode -> wct_content_decode pair).  wct_destroy
  // releases through this list: a DevBuf added to the struct has to be classified here or it leaks.
  template <typename F>
  void each_buf(F&& f) {
    for (Lane* ln : {&main, &side})
      for (DevBuf* b : {&ln->actA, &ln->actB, &ln->wsMom, &ln->wsEig, &ln->sums}) f(*b, ln, true);
    for (DevBuf* b : {&featS, &tmpT, &wsAsm, &trBuf, &small, &foldW, &foldW16, &eigC, &u8c, &u8s, &u8o, &rsz_tmp, &noise, &colStyle, &colOut, &colWs, &smSums, &smAB, &swFc, &swFs, &swQ, &swK, &swOut, &swIdx, &swRun, &swNorm, &swLab, &packed,
                      &atFc, &atFs, &atCs, &atSs, &atQ, &atK, &atProj, &atMean, &atVar, &atOut, &atStat, &atMt,
                      &shIn, &shOut, &shNext, &shEdge, &shStyle, &shStats, &shMb,
                      &regLab, &regHist, &regSums, &regMb, &regFeat, &wsRegMom, &wsRegApply,
                      &blendW, &blendStat, &wsBlendPool, &wsBlendApply, &gdLab, &gdHist, &kmFeatC, &kmFeatS, &kmWs, &kmStat, &motionWs, &dvWs, &dvZ,
                      &bgWs, &bgGrid, &pxCl, &pxSl, &jpCoef, &jpWs, &jpStream, &jdCoef, &jdWs, &jdStream, &jdPlanes})
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

namespace wct_host {

int fail(wct_ctx* ctx, int code, const char* fmt, ...);

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

inline bool valid_level(int l) { return l >= 1 && l <= 5; }

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

struct SumsView { double *sum, *sumsq; int* info; };

// ---- internals that more than one host file calls; the comment at each definition says what it does ------------------
// wct_api.hip
void range_host_set(wct_ctx* ctx, unsigned n);
int range_readback(wct_ctx* ctx);
int ensure(wct_ctx* ctx, DevBuf& b, size_t bytes);
int pad_cout(int c);
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb);
int encode_impl(wct_ctx* ctx, Lane& ln, int level, const float* img, int H, int W, float* feat_nhwc, int* ho, int* wo);
int decode_impl(wct_ctx* ctx, int level, const float* feat, int h, int w, const ConvDesc* first, float* img);
int sums_view(wct_ctx* ctx, Lane& ln, SumsView& v);
int mb_view(wct_ctx* ctx, double** M, double** b);
bool mom32_on(const wct_ctx* ctx, long npix);
int moments_impl(wct_ctx* ctx, Lane& ln, const float* feat, int C, int h, int w, int x0, int x1, double* sum, double* sumsq);
int eig_impl(wct_ctx* ctx, Lane& ln, int C, double n, const double* sum, const double* sumsq, int inverse, DevBuf& res, int* info_dev, bool ot_sched = false);
int assemble_impl(wct_ctx* ctx, int C, const DevBuf& eig_c, const DevBuf& eig_s, double alpha, double* M, double* b);
int transform_mb(wct_ctx* ctx, int mode, int C, double n, const double* sum, const double* sumsq, const DevBuf& eig_s, double alpha, double* M,
                 double* b, int* info_dev, hipEvent_t style_ready);
bool fast_fold_level(const wct_ctx* ctx, int level);
int style_fold(wct_ctx* ctx, int level, hipStream_t st);
int fold_fast_impl(wct_ctx* ctx, int level, double alpha, ConvDesc& out);
void level_dims(int level, int H, int W, int& h, int& w);
bool l1_fused(const wct_ctx* ctx, int level);
int l1_moments_impl(wct_ctx* ctx, Lane& ln, int level, const float* img, int H, int W, int x0, int x1, double* sum, double* sumsq);
int l1_decode_impl(wct_ctx* ctx, int level, const float* img, int H, int W, const ConvDesc& first, float* out);
int style_side(wct_ctx* ctx, int level, const float* style, int Hs, int Ws, int slot = -1);
int fork_side(wct_ctx* ctx);
int content_side(wct_ctx* ctx, int level, const float* content, int H, int W, float alpha, float* out, int* Ho, int* Wo);
int stylize_impl(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha, int num_run, float* out,
                 int* Ho, int* Wo);
int stylize_prepared_impl(wct_ctx* ctx, const char* what, const float* content, int H, int W, float alpha, int num_run, float* out, int* Ho, int* Wo);
// api_model.hip
void free_module(Module& m);
// api_sharded.hip
void release_comm(wct_ctx* ctx);   // wct_destroy: destroys a communicator the context owns
// api_video.hip
__attribute__((visibility("hidden"))) int clip_track_level(wct_ctx* ctx, wct_clip* clip, int level, int C, double* sum, double* sumsq);   // the tracking step of wct_stylize_clip's frame: nothing committed
// api_swap.hip
__attribute__((visibility("hidden"))) int whiten_solve(wct_ctx* ctx, const float* feat, int C, int h, int w, SumsView& sv, double** M, double** b);   // needs eigS[0] sized by the caller
// api_multi.hip
int apply_labeled_impl(wct_ctx* ctx, const float* feat, int C, long npix, const uint8_t* lab, int K, const double* M, const double* b, float* out);

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

}  // namespace wct_host
