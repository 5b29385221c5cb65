/* libwct_hip -- C ABI of the MI355X-native WCT stylisation path.
 *
 * Drop-in boundary for ONE path of MingSun-Tse/Collaborative-Distillation: the 5-level encode ->
 * whitening/colouring transform -> decode cascade of `PytorchWCT/WCT.py --mode 16x|original`.
 * The reference has no FFI of its own; its boundary is the Python call surface of WCT.py / util_wct.py.
 * Each entry point below names the reference interface it replaces (paths relative to the reference
 * repository).  INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative WCT_ERR_* code; wct_last_error() has the text.
 *     Nothing ever calls exit() (the reference does on a bad mode, util_wct.py:57-59).
 *   - all tensor arguments are DEVICE pointers to fp32 unless the name says host / f64; images are planar
 *     3 x H x W (the reference's NCHW with N = 1); feature maps are NHWC (layout 0, native) or NCHW
 *     (layout 1, the reference's layout) as selected by `layout`.
 *   - a context is bound to one device and one HIP stream; calls are asynchronous on that stream.
 *     One context per GPU / rank; a context is not thread-safe.
 *     One exception: with feature maps wider than 128 channels (--mode original) the outcome of each matrix-function iteration
 *     is read back (a slow global-memory Jacobi is the net under a non-converged one).  The cascade-type calls (wct_stylize*,
 *     wct_style_transfer_level, wct_style_prepare*) enqueue everything, synchronise ONCE at their end, look at all outcomes and
 *     repeat the call the synchronous way if one failed; the split-level calls (wct_solve, wct_content_solve, wct_transform)
 *     synchronise once per solve.  Calls of that mode therefore block the host and cannot be captured into a HIP graph; the 16x
 *     path never synchronises.
 *   - the caller owns every buffer it passes; the context owns weights and an internal workspace that
 *     grows on first use of a size (no allocation on later calls of the same or smaller size).
 */
#ifndef WCT_HIP_H
#define WCT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_OK 0
#define WCT_ERR_INVALID (-1) /* bad argument (shape, level, layout, NULL) */
#define WCT_ERR_HIP (-2)     /* a HIP runtime call failed */
#define WCT_ERR_NOMEM (-3)   /* device allocation failed */
#define WCT_ERR_STATE (-4)   /* module for this level not loaded */
#define WCT_ERR_RANGE (-5)   /* an activation left the f16x3 range (+-65504) and was clamped: results deviate from fp32 */

#define WCT_KIND_ENC 0
#define WCT_KIND_DEC 1
#define WCT_LAYOUT_NHWC 0
#define WCT_LAYOUT_NCHW 1

typedef struct wct_ctx wct_ctx;

/* One `relu(conv3x3(reflect_pad(x)))` stage, in execution order.
 * weight: HOST fp32 OIHW [cout][cin][3][3]; bias: HOST fp32 [cout] -- the tensors of the reference's
 * state_dict (model/model_cd.py:712-718).  pool_after: MaxPool2d(2,2) follows (encoder);
 * up_after: UpsamplingNearest2d(2) follows (decoder). */
typedef struct wct_layer {
  int cin, cout;
  int pool_after, up_after;
  const float* weight;
  const float* bias;
} wct_layer;

/* per-kernel-family timing collected when profiling is enabled (bench.py's roofline leg) */
typedef struct wct_prof_entry {
  char name[48];     /* e.g. "conv3x3_f16x3<co=64,dma>", "enc_head_fused<3-16-16,pool>" */
  double ms;         /* summed HIP-event time */
  double flops;      /* algorithmic FLOPs of those launches */
  double bytes;      /* algorithmic HBM bytes (input read once + output written once + weights) */
  long launches;
} wct_prof_entry;

int wct_version(void);

/* replaces `wct = WCT(args).cuda()` (WCT.py:97, util_wct.py:31-59): create, then load 10 modules */
int wct_create(int device, wct_ctx** out);
void wct_destroy(wct_ctx* ctx);
const char* wct_last_error(const wct_ctx* ctx);
/* hipStream_t; NULL = default stream.  Binding a DIFFERENT stream orders it behind the old one: the new stream waits (by an event, no
 * host synchronisation) for everything the context has enqueued on the previous stream, because calls under two streams share the
 * context's workspace.  So consecutive calls of one context issued under different streams run in issue order and return what they
 * return on one stream; they do not overlap each other (use two contexts for that).  The previous stream must still exist when the
 * next one is bound.  Re-binding the stream already bound costs nothing.  A stream that is being captured into a HIP graph is bound
 * without that dependency (synchronise before the capture begins, as torch.cuda.graph does).  A captured graph holds the workspace's
 * addresses: replaying it after a later call has GROWN the workspace (wct_debug_get "ws_allocs" moved) reads and writes freed memory --
 * capture after wct_reserve or a warm-up call of the largest size, and re-capture whenever the workspace has grown. */
int wct_set_stream(wct_ctx* ctx, void* hip_stream);
/* waits for both of the context's streams; returns WCT_ERR_RANGE -- ONCE, clearing the flag -- when an activation was clamped
 * since the last report (below), so a later WCT_ERR_RANGE always means a later clamp */
int wct_sync(wct_ctx* ctx);

/* Range check of the f16x3 arithmetic (wct_set_conv_mode 1, the default).  The reference computes its convolutions in fp32
 * (model/model_cd.py:724-743: plain nn.Conv2d); the split-f16 kernels represent an activation as hi + lo in f16 and clamp
 * it to +-65504.  A clamp that actually changed a value is a deviation from the reference, so every clamp site raises a
 * per-context device counter (threads that saw |x| >= 65504; saturating, never wraps).  A NaN in external data (an image, an
 * fp32 feature map handed to wct_decode*) is clamped to a finite value by the same instruction and raises the counter too;
 * non-finite weights are rejected by wct_load_module.  Three ways to see it:
 *   wct_saturation_count  synchronises the context and returns the counter (count may be NULL), clearing it when reset != 0
 *   wct_sync              reports a non-zero counter as WCT_ERR_RANGE once and clears it
 *   wct_range_poll        NO synchronisation: every compute entry point ends with an asynchronous 4-byte copy of the counter
 *                         to pinned host memory on the caller's stream; this returns the last copy that has landed, i.e. the
 *                         state after some COMPLETED call (callers check it at the start of their next call).  A call is
 *                         complete when ALL the work it enqueued has run.  wct_style_prepare[_levels] runs its encoders on the
 *                         context's side stream and does not join the caller's stream to it (the style side overlaps what the
 *                         caller enqueues next): its copy is made on the side stream, behind those encoders, so a clamp of
 *                         the style side shows here once the side stream has drained (a device synchronisation, wct_sync, or
 *                         any later call that consumes the style statistics and has itself completed) -- waiting for the
 *                         caller's stream alone is not enough for this one entry point
 *   wct_range_flag_f64    writes the counter as one double to flag_dev on the caller's stream, so that a sharded run can fold it
 *                         into the all-reduce of the moments it already makes and every rank sees every rank's clamps
 * Conv mode 0 (exact fp32 MFMA) has no such limit. */
int wct_saturation_count(wct_ctx* ctx, int reset, unsigned long long* count);
int wct_range_poll(wct_ctx* ctx, unsigned long long* count);
int wct_range_flag_f64(wct_ctx* ctx, double* flag_dev);

/* Context-level experiment switches (tests, A/B measurements): key in {"fuse", "sp", "l1fuse", "u8fuse", "upconv", "fastfold",
 * "interleave", "foldgemm"} with value 0 / 1, "in3wide" (2 / 1 / 0), "mom32" (0 / 1 / 2: fp64 / fp32-block products of the moments), "nscoop" (0 multi-launch, 1 single launch, 2 single launch with an injected
 * placement fault), "side_priority" (-1 / 0 / 1).  They select between kernel formulations of the same operators (fused
 * full-resolution ends, SP16 intermediates, level 1 without relu1_1 in HBM, f16x3 or exact-fp32 first conv of the un-pruned
 * encoders); results agree to fp32 round-off or bitwise (tests/test_hip_parity.py).  "eig_skip" (N: after N solves the matrix
 * functions are SKIPPED and stale results reused) is a timing experiment that produces wrong pictures by design: it is refused
 * unless the environment variable WCT_DEBUG is set; so is "shard_emulate" (100 * ranks + rank: a context holding a ONE-rank communicator runs
 * wct_stylize_sharded with the geometry of one rank of a larger job, its peers being itself -- what one rank of the job executes, with
 * other numbers; 0: off).  Environment variables WCT_* are honoured only when WCT_DEBUG is set.
 * "prof_forms" (0 / 1, default 0) changes no result: with profiling enabled, the names of wct_profile_read() gain a suffix saying which
 * kernel form the size-selected launchers chose, "#<form><tile height>[m]" -- form r = two-role head, t = plain tiles, u = upsample
 * (2x2 per parity) form, s = small-map form, 3 = three-stage persistent kernel; m = the grid is smaller than tiles x cout groups, so a
 * workgroup walks several units -- e.g. "dec_tail_fused<16-16-3>#u16m".  Launchers with one form add nothing; with the switch off the
 * names are unchanged (tests/test_geometry_gpu.py).  The launchers of the feature-space kernels, whose tiling is a function of the
 * channel count and the pixel count, report behind a ':' instead (so that '#' keeps meaning "a conv form"):
 *   "moments", "moments_labeled", "moments_weighted"   ":<family><MP>.<NLD>.<PW>[s]<d|f>" -- family l = LDS-tile kernel (MP pixels per
 *                  tile, NLD float4 loads per thread and tile, PW tile pairs per wave, s = the waves split the tile's pixels), r =
 *                  moments_reg_kernel (C = 32 / 64 with fp32 products: 256 pixels per pass, 16 loads, PW = its tile pairs), b =
 *                  moments_blk_kernel (chunks of 64 pixels, 2 steps of loads in flight, PW = its waves); d / f = fp64 / fp32-block
 *                  products -- e.g. "moments:l128.6.6sd", "moments_labeled:l64.2.2f"
 *   "fold_affine"  ":fra" / ":frg" = fold_row_kernel's aligned / generic path, ":fb" = fold_block_kernel (cin >= 256), ":fg" = the fp64
 *                  GEMM fold, ":ff" = the fast fold
 * (tests/sweep_cases.py restates the plans, tests/test_sweep_gpu.py holds every report against it).
 *   "patch_match<f16x3>"  ":q<QT>.l<L>.<nkt>/<split>.<nkt>/<split>" -- QT = query tiles (grid.x of every match launch), L = match launches
 *                  (key chunks), then the key tiles of the band and the workgroups per query tile they are dealt to (grid.y) of the
 *                  FIRST launch and of the LAST one (the same pair twice when L = 1); a workgroup walks ceil(nkt / split) key tiles at
 *                  the most -- e.g. "patch_match<f16x3>:q16.l2.68/64.34/34".  Cut at 23 characters
 *                  (tests/swap_cases.py restates the launcher, tests/test_swap_edges_gpu.py holds every report against it).
 * "poison" (a byte 0..255, or -1 = off) is the test hook for "does a call read what an earlier call left in the workspace": it
 * synchronises both of the context's streams, fills every allocated SCRATCH buffer of the context with that byte and, until it is
 * turned off, every buffer the workspace allocates later as well (a grown buffer is a fresh allocation and usually zero pages).
 * Scratch is every workspace buffer whose contents no later call is documented to read.  STATE survives a poison: module weights
 * and their packed forms, the prepared style statistics of every level and their style-side folds (wct_style_prepare*,
 * wct_style_import, wct_style_blend, wct_stylize_interp), the K style slots of the regions / blend calls, the resize weight
 * tables, the counters -- and the content feature map / image copy held between wct_content_encode and the wct_content_decode
 * that closes the pair (poison BEFORE wct_content_encode, not inside the pair; a second wct_content_decode of one encode is no
 * longer covered).  A correct library returns the same bits with and without a poison; nothing is added to any call path but one
 * branch where the workspace allocates (tests/test_state_gpu.py). */
int wct_debug_set(wct_ctx* ctx, const char* key, double value);
/* Health counters of the context (no reference counterpart): "nscoop_solves" = single-launch C = 128 matrix-function solves enqueued,
 * "nscoop_aborts" = those that aborted into the Jacobi net (watchdog / placement; synchronises the context), "nscoop_off" = bit mask
 * of lanes (1 main, 2 side) that went back to the multi-launch schedule because at least three and at least a quarter of their
 * single-launch solves aborted.  An aborted solve is repaired (same results) but costs ~7 ms: this is how that shows.
 * Workspace accounting: "ws_allocs" = device allocations the growing workspace has made so far (unchanged across a call = that call
 * allocated nothing), "ws_bytes" = sum of the capacities of all workspace buffers now (weights, resize tables and counters not
 * included). */
int wct_debug_get(wct_ctx* ctx, const char* key, double* value);

/* replaces SmallEncoder{L}_16x_aux(path) / SmallDecoder{L}_16x(path) / Encoder{L} / Decoder{L} construction
 * (util_wct.py:36-55; model_cd.py:712-718).  conv0_w [3*3] / conv0_b [3] (HOST): the encoder's 1x1 colour
 * affine (model_cd.py:725), folded into the first conv; NULL for decoders. */
int wct_load_module(wct_ctx* ctx, int kind, int level, int n_layers, const wct_layer* layers,
                    const float* conv0_w, const float* conv0_b);

/* shape of relu{level}_1 for an H x W image (floor pooling): C, h, w */
int wct_feature_shape(const wct_ctx* ctx, int level, int H, int W, int* C, int* h, int* w);

/* replaces `encoder(img)`  (WCT.py:100-101 -> model_cd.py:724-743) */
int wct_encode(wct_ctx* ctx, int level, const float* img, int H, int W, float* feat, int layout);
/* replaces `decoder(csF)`  (WCT.py:105 -> model_cd.py:276-294); image is 3 x (h<<(L-1)) x (w<<(L-1)) */
int wct_decode(wct_ctx* ctx, int level, const float* feat, int h, int w, int layout, float* img);

/* raw fp64 moments over the window rows [0,h) x cols [x0,x1) of an NHWC feature map of width w:
 *   sum[C], sumsq[C*C] (device, f64).  Replaces torch.mean + mm(cF, cF.t()) (util_wct.py:68-70, 94-96);
 * raw sums (not centred) so that a content-sharded run can all-reduce them across GPUs.
 * Arithmetic: maps of >= 65 536 pixels (h * w of the MAP, whatever the window) take their products and the sums of 64-pixel blocks in
 * fp32 on the matrix cores, block totals in fp64 (raw sums within ~1e-8 relative of the all-fp64 form); smaller maps -- the deep,
 * worst-conditioned levels -- fp64 products throughout.  Consequences: windows of ONE map share one arithmetic but cut the 64-pixel
 * blocks differently, so window sums add up to the whole map's to ~1e-8 relative, not to fp64 round-off; and a strip (+ halo) of a
 * sharded frame is its own, smaller map and may take the fp64 form where the untiled frame takes fp32 blocks (sharded and untiled
 * (M, b) agree to ~1e-8 either way; tests/test_sharded_gpu.py).  wct_debug_set("mom32", 0) selects exact fp64 products everywhere:
 * windows then add up to 1e-13. */
int wct_moments(wct_ctx* ctx, const float* feat, int C, int h, int w, int x0, int x1, double* sum, double* sumsq);

/* (n, sum, sumsq) of content and style -> csF = M cF + b.  M [C*C] row-major, b [C], device f64.
 * Replaces svd / pow / diag / mm of util_wct.py:74-125 and the blend of :219.  info (HOST, may be NULL)
 * receives, after an internal stream sync, how {content, style} were solved: n < 100 = Newton-Schulz iterations
 * (19 for the deflated iteration of C > 128), 100 + n = the Jacobi fallback ran n sweeps. */
int wct_solve(wct_ctx* ctx, int C, double n_c, const double* sum_c, const double* sumsq_c, double n_s,
              const double* sum_s, const double* sumsq_s, double alpha, double* M, double* b, int* info);

/* out = M feat + b per pixel (un-fused form).  Replaces mm(step2,cF), mm(S,.), + s_mean (util_wct.py:120-126) */
int wct_apply(wct_ctx* ctx, const float* feat, int C, int h, int w, int layout, const double* M, const double* b,
              float* out);

/* replaces `wct.transform(cF, sF, csF, alpha)` (util_wct.py:210-223); out has the shape/layout of cF */
int wct_transform(wct_ctx* ctx, const float* cF, int C, int h, int w, const float* sF, int hs, int ws,
                  float alpha, int layout, float* out);

/* decoder with csF = M feat + b folded into its first convolution (feat is NHWC) */
int wct_decode_affine(wct_ctx* ctx, int level, const float* feat, int h, int w, const double* M, const double* b,
                      float* img);

/* replaces styleTransfer(encoder, decoder, contentImg, styleImg, csF) (WCT.py:98-106) for one level */
int wct_style_transfer_level(wct_ctx* ctx, int level, const float* content, int H, int W, const float* style,
                             int Hs, int Ws, float alpha, float* out, int* Ho, int* Wo);

/* Split form of one level for content-sharded (multi-GPU) runs -- the same work as wct_style_transfer_level, cut where
 * a sharded run exchanges data (wct_hip/sharded.py):
 *   wct_style_prepare   style side of all loaded levels (encode, moments, cov^1/2), on the context's side stream
 *   wct_content_encode  cF = encoder(content) kept inside the context + raw moments over feature columns [x0,x1)
 *                       (x1 < 0: to the end) into sum[C], sumsq[C*C] (device f64) -> caller all-reduces them
 *   wct_content_solve   global (n, sum, sumsq) -> M [C*C], b [C] (device f64)  -> caller may broadcast them
 *   wct_content_decode  decoder(M cF + b) with M, b folded into the first conv
 * Together they replace styleTransfer() (WCT.py:98-106). */
int wct_style_prepare(wct_ctx* ctx, const float* style, int Hs, int Ws);
int wct_content_encode(wct_ctx* ctx, int level, const float* content, int H, int W, int x0, int x1, double* sum,
                       double* sumsq, int* h, int* w);
int wct_content_solve(wct_ctx* ctx, int level, double n_c, const double* sum_c, const double* sumsq_c, float alpha,
                      double* M, double* b);
int wct_content_decode(wct_ctx* ctx, int level, const double* M, const double* b, float* out, int* Ho, int* Wo);

/* The multi-GPU variant of one level BEHIND the boundary ("multi-GPU variant takes an ncclComm_t"; the reference is
 * single-GPU, WCT.py:97,110 -- nothing to replace but styleTransfer() itself, WCT.py:98-106, run on a column strip).
 *   wct_comm_load        dlopen the RCCL the host process uses and resolve ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllReduce /
 *                        ncclBroadcast / ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd.  A non-NULL path is THE library to use: if it
 *                        cannot be opened the call fails (no second RCCL is mapped behind the caller's back); NULL searches "librccl.so.1",
 *                        "librccl.so", /opt/rocm/lib/librccl.so.  libwct_hip.so itself links against no communication library;
 *                        single-GPU callers never load one.  wct_comm_library returns the path that was loaded ("" before).
 *   wct_comm_unique_id   ncclGetUniqueId into 128 caller bytes (rank 0; the caller ships them to the other ranks, e.g. through the
 *                        rendezvous it already has)
 *   wct_comm_init        ncclCommInitRank on the context's device: the context then OWNS a communicator over `nranks` contexts
 *                        (one per GPU / process); collective over the job -- every rank calls it
 *   wct_comm_attach      use a communicator the caller owns (`nccl_comm` is an ncclComm_t); not destroyed by the library
 *   wct_comm_destroy     ncclCommDestroy of an owned communicator (also done by wct_destroy)
 *   wct_level_sharded    one level of the column-sharded cascade in ONE call, everything on the context's stream, no host
 *                        synchronisation: encoder of `content` (3 x H x W: this rank's strip + halo) + raw moments over the OWNED feature
 *                        columns [x0, x1) (x1 < 0: to the end) -> ncclAllReduce(SUM, fp64, C*C + C + 1 values: sums, second moments, the
 *                        f16x3 range flag of wct_range_flag_f64) -> matrix functions with n_total = feature pixels of the WHOLE image,
 *                        against the level's style statistics (wct_style_prepare* on this rank, or wct_style_import of another rank's)
 *                        -> (M, b) folded into the decoder's first conv -> decoder -> out (3 x Ho x Wo).  range_total (device, one
 *                        double, may be NULL) receives the node-wide clamp count.  Same arithmetic in the same order as
 *                        wct_content_encode / all-reduce / wct_content_solve / wct_content_decode: bit-identical to that path.
 *                        With feature maps wider than 128 channels (--mode original) each solve reads one flag back (host synchronisation),
 *                        as in the split-level entries. */
int wct_comm_load(const char* librccl_path);
const char* wct_comm_library(void);
int wct_comm_unique_id(unsigned char* id128);
int wct_comm_init(wct_ctx* ctx, int nranks, int rank, const unsigned char* id128);
int wct_comm_attach(wct_ctx* ctx, void* nccl_comm, int nranks, int rank);
int wct_comm_destroy(wct_ctx* ctx);
int wct_level_sharded(wct_ctx* ctx, int level, const float* content, int H, int W, int x0, int x1, double n_total, float alpha,
                      float* out, int* Ho, int* Wo, double* range_total);

/* The WHOLE column-sharded cascade behind the boundary: WCT.py:120-125 (levels 5 -> 1 of styleTransfer, WCT.py:98-106) run by `nranks`
 * contexts -- one per GPU / process -- on column strips of ONE content image.  The reference is single-GPU (WCT.py:97,110); what
 * makes the path shardable is that every operator of it is local except the content (and style) statistics (util_wct.py:68-70,94-96).
 * Everything is enqueued on the context's stream(s): strip geometry and per-level crops, the style side, encoders, owned-column
 * moments, the collectives, matrix functions, fold, decoders, the neighbour exchange.  No host synchronisation, no allocation after the
 * first call of a size (--mode 16x; the wide models' C > 128 solves read one flag back per solve, as the split-level entries do).
 *
 * Collectives.  The cascade talks to its peers through a wct_collectives table (below).  wct_comm_init / wct_comm_attach install the
 * RCCL one (ncclAllReduce / ncclBroadcast / ncclGroupStart + ncclSend + ncclRecv + ncclGroupEnd on the context's communicator and
 * stream); wct_comm_attach_collectives installs a caller-supplied transport (another communication library; the test suite's
 * in-process world that moves device buffers between rank threads).  All functions are asynchronous on `stream` and return 0 or an
 * error code of the transport; buffers are device memory.
 *
 * Geometry (wct_shard_geometry, a pure function): rank r owns content columns [own0, own1) (origins are multiples of 16, so every
 * pooling grid coincides with the untiled image's; the last strip takes the remainder) and must be GIVEN columns [in0, in1) = its strip
 * plus the level-5 margin of the halo mode towards the image interior:
 *   WCT_HALO_EXCHANGE   every level runs on own +- (160, 72, 24, 10, 2) columns (level 5..1: the composite encode->decode receptive
 *                       field) and, between levels, neighbours exchange the (72, 24, 10, 2) outermost OWNED columns of the image just
 *                       decoded -- two messages per level boundary, 3 x H x margin floats (<= 3.5 MB at H = 4096);
 *   WCT_HALO_RECOMPUTE  cumulative margins (272, 112, 40, 16, 6), no exchange;
 *   WCT_HALO_AUTO       exchange for strips narrower than 2560 columns (and at least 144), recompute otherwise.
 * With those margins a strip's owned columns are bit-identical to the untiled level given the same (M, b).
 *
 * Style side (style_mode; the style image is given WHOLE to every rank, as the reference gives it to every level, WCT.py:121-125):
 *   WCT_STYLE_STRIPS     the style image is cut into column strips like the content: rank r encodes its strip + the ENCODER's
 *                        receptive field (80, 32, 12, 4, 1 columns at level 5..1) at every level, raw moments over its owned feature
 *                        columns; level L's style sums travel in level L's all-reduce together with the content moments, and every
 *                        rank takes the level's matrix square root on its side stream right behind it.  Per-rank style work = 1/nranks (+ margins);
 *   WCT_STYLE_OWNER      level L's style side is computed whole by rank (5 - L) mod nranks and broadcast (C*C + C doubles per level);
 *   WCT_STYLE_REPLICATE  every rank computes all five levels (no communication; tiny styles);
 *   WCT_STYLE_AUTO       = owner.  Measured at 2, 4 and 8 ranks (profiles/r06_style_arrangement_per_level_join.txt): owner beats strips by 0.5-1.3 ms per
 *                        rank frame although its rank 0 carries 45.6 % of the style FLOPs -- each style-side matrix square root occupies an XCD the
 *                        content kernels then wait for, and strips / replicate run five of them on every rank, owner at most three.
 * WCT_SHARD_BROADCAST_MAP: rank 0 alone solves for the colouring map and broadcasts (M [C*C], b [C]) doubles per level; default: every
 * rank solves for itself (the all-reduce returns identical bits everywhere and the solver is deterministic).
 *
 * Per level: ONE all-reduce of [sum C | sumsq C*C | f16x3 range flag] doubles (+ the level's style sums in strips mode), the optional
 * broadcasts above, and in exchange mode one grouped send/recv pair per neighbour.
 *
 *   content_ext   columns [in0, in1) of the content, planar 3 x H x (in1 - in0)
 *   style         the whole style image, planar 3 x Hs x Ws
 *   out_owned     receives this rank's owned columns of the result, planar 3 x Ho x Wo (Ho = 16 floor(H / 16); Wo = own1 - own0,
 *                 less what floor pooling cut off the last strip); must hold 3 * H * (own1 - own0) floats
 *   range_total   device, one double, may be NULL: the node-wide count of f16x3 clamps as of the last all-reduce (wct_range_flag_f64)
 * Results are those of the split-level entries driven by wct_hip/sharded.py over the same transport, bit for bit. */
typedef struct wct_p2p {
  int peer;       /* rank */
  int is_send;    /* 1: send `bytes` from buf to peer; 0: receive `bytes` from peer into buf */
  void* buf;
  size_t bytes;
} wct_p2p;
typedef struct wct_collectives {
  void* user;
  int (*all_reduce_sum_f64)(void* user, double* buf, size_t count, void* hip_stream);       /* in place, every rank */
  int (*broadcast)(void* user, void* buf, size_t bytes, int root, void* hip_stream);        /* in place, every rank */
  int (*sendrecv)(void* user, const wct_p2p* ops, int n_ops, void* hip_stream);             /* ONE group: all ops posted together */
} wct_collectives;
#define WCT_HALO_AUTO 0
#define WCT_HALO_RECOMPUTE 1
#define WCT_HALO_EXCHANGE 2
#define WCT_STYLE_AUTO 0
#define WCT_STYLE_OWNER 1
#define WCT_STYLE_STRIPS 2
#define WCT_STYLE_REPLICATE 3
#define WCT_SHARD_BROADCAST_MAP 1   /* flags */
#define WCT_SHARD_FAST_FOLD 2       /* the single-GPU cascade's fold -- (W cov_s^1/2) cov_c^-1/2 straight into the decoder's first conv, no (M, b) on the
                                       critical path -- where the decoder allows it and every rank folds for itself; fp32 round-off from the (M, b) form,
                                       which stays the default because wct_hip/sharded.py's split-level orchestration is bit-identical to it */
int wct_comm_attach_collectives(wct_ctx* ctx, const wct_collectives* coll, int nranks, int rank);
/* nranks / rank of the communicator or transport the context holds (0 / 0: none) */
int wct_comm_info(const wct_ctx* ctx, int* nranks, int* rank);
/* Known data through all three functions of the context's transport between the job's ranks (all-reduce; broadcast from the last rank;
 * a ring send / recv; the cascade's grouped neighbour exchange), checked on the host: 0, or WCT_ERR_HIP naming what came back wrong.
 * Collective over the job (every rank calls it), synchronises the stream: a set-up time check (bench.py runs it before timing). */
int wct_comm_selftest(wct_ctx* ctx);
/* halo_mode may be WCT_HALO_AUTO; *halo_mode_resolved (may be NULL) receives what it resolves to for this width and rank count */
int wct_shard_geometry(int W_total, int nranks, int rank, int halo_mode, int* own0, int* own1, int* in0, int* in1, int* halo_mode_resolved);
int wct_stylize_sharded(wct_ctx* ctx, const float* content_ext, int H, int W_total, int in0, int in1, const float* style, int Hs, int Ws,
                        float alpha, int halo_mode, int style_mode, int flags, float* out_owned, int* Ho, int* Wo, double* range_total);
/* The two halves of WCT_STYLE_STRIPS for callers that run the collectives themselves (wct_hip/sharded.py over torch.distributed):
 *   wct_style_moments  encoder of `style_strip` (3 x Hs x Ws_strip: the rank's style columns + margins) + raw moments over feature columns
 *                      [x0, x1) (x1 < 0: to the end) into sum[C], sumsq[C*C] (device f64) on the context's SIDE stream; the caller's
 *                      stream is made to wait for them (so that a collective enqueued next sees them)
 *   wct_style_solve    global (n_s, sum, sumsq) of the style feature map -> cov_s^(1/2), mu_s inside the context (what
 *                      wct_style_prepare leaves for the level), on the side stream behind everything enqueued on the caller's */
int wct_style_moments(wct_ctx* ctx, int level, const float* style_strip, int Hs, int Ws_strip, int x0, int x1, double* sum, double* sumsq);
int wct_style_solve(wct_ctx* ctx, int level, double n_s, const double* sum_s, const double* sumsq_s);

/* replaces the cascade of WCT.py:120-125 (levels 5..1, num_run times).  out must hold 3*H*W floats. */
int wct_stylize(wct_ctx* ctx, const float* content, int H, int W, const float* style, int Hs, int Ws, float alpha,
                int num_run, float* out, int* Ho, int* Wo);

/* Spatial control: a uint8 label map gives every content pixel a region 0 .. K-1 with its own style, or 255 (unstyled); 1 <= K <= 8.
 * Per region and level the transform is the reference's whiten_and_color (util_wct.py:62-131) on THAT REGION's feature columns, against
 * the whole style image's statistics (WCT.py:121-125: the same style at every level), blended with alpha[k] (:219); a region with fewer
 * than 2 feature pixels at a level, and label 255, keep cF there.  Level L reads the label at the centre of its pooling window in image
 * coordinates: lab_L[i][j] = labels[i s + s/2][j s + s/2], s = 2^(L-1).
 *   wct_moments_labeled  extends wct_moments: per label k < K, n[k] pixels, sum[k*C + c], sumsq[k*C*C + a*C + b] (device f64) of an NHWC
 *                        map, lab h x w (device).  Same arithmetic classes as wct_moments (fp32 products in blocks of <= 64 pixels with
 *                        fp64 block totals for maps of >= 65 536 pixels, fp64 products below; "mom32" applies), fixed-order reduction:
 *                        bitwise reproducible.  Pixels with labels >= K are ignored.
 *   wct_apply_labeled    extends wct_apply: out_p = M[lab(p)] feat_p + b[lab(p)], M [K*C*C], b [K*C] device f64 (used in fp32, fp32
 *                        accumulation); pixels with labels >= K (255) are copied through.  layout as wct_apply.
 *   wct_stylize_regions  extends wct_stylize (WCT.py:120-125): content 3 x H x W, labels H x W (device), K styles (device pointers in a
 *                        HOST array, each 3 x Hs[k] x Ws[k]), alpha[K] (HOST).  Per level: encoder -> wct_moments_labeled -> one content
 *                        solve per region against style k -> wct_apply_labeled -> decoder (unfolded first conv); the K style sides run on
 *                        the side stream.  The call reads the label histograms back ONCE at its start (one stream synchronisation: the
 *                        solvers take each region's pixel count on the host), so it cannot be captured into a HIP graph.  K outside
 *                        [1, 8] or a label value >= K other than 255 anywhere in the map return WCT_ERR_INVALID before anything is
 *                        written to out; wct_last_error names the smallest offending value.  out must hold 3*H*W floats. */
int wct_moments_labeled(wct_ctx* ctx, const float* feat, int C, int h, int w, const uint8_t* lab, int K, double* n, double* sum,
                        double* sumsq);
int wct_apply_labeled(wct_ctx* ctx, const float* feat, int C, int h, int w, int layout, const uint8_t* lab, int K, const double* M,
                      const double* b, float* out);
int wct_stylize_regions(wct_ctx* ctx, const float* content, int H, int W, const uint8_t* labels, int K, const float* const* styles,
                        const int* Hs, const int* Ws, const float* alpha, int num_run, float* out, int* Ho, int* Wo);

/* Style interpolation and per-pixel style weights, 1 <= K <= 8 styles.  whiten_and_color (util_wct.py:62-131) is linear in the style
 * statistics: with S_k = cov_s,k^(1/2) and Wc = cov_c^(-1/2), sum_k l_k (S_k Wc (x - mu_c) + mu_s,k) = (sum_k l_k S_k) Wc (x - mu_c) + sum_k
 * l_k mu_s,k, so interpolation (the WCT paper's third user control, -styleInterpWeights) is ONE blended style slot per level.
 *   wct_stylize_interp   extends wct_stylize: csF = alpha sum_k l_k whiten_and_color(cF, e_L(style_k)) + (1 - alpha) cF at every level,
 *                        l = lambda / sum(lambda) (lambda: K HOST floats, finite, >= 0, sum > 0).  The K style sides of a level run on the
 *                        side stream into K slots, one launch blends them (fixed k order: lambda = (1, 0, ..) gives style 0's statistics
 *                        bit for bit), then the unchanged single-style content path.  styles: device pointers in a HOST array.
 *   wct_style_blend      the same blend of K stat sets in wct_style_export layout (device, K * wct_style_stats_count doubles, one set
 *                        after the other) into the context's style statistics of `level` (as wct_style_import): cached styles cost one
 *                        small launch per level before wct_stylize_prepared.
 *   wct_stylize_blend    per-pixel weights: weights K x H x W (device fp32), each in [0, 1] and sum_k <= 1 at every pixel (the rest is
 *                        unstyled content), alpha[K] (HOST).  Level L uses w_k,L = the mean of w_k over each feature pixel's 2^(L-1)
 *                        square window; per k the content statistics are reliability-weighted: mu_k = sum w x / V1, cov_k = sum w (x -
 *                        mu_k)(x - mu_k)^T / (V1 - V2 / V1) (V1 = sum w_k,L, V2 = sum w_k,L^2); style k is active at a level iff V1 > 0
 *                        and V1^2 / V2 >= 2; csF(p) = x_p + sum_{k active} w_k,L(p) alpha_k (target_k(x_p) - x_p).  Constant weights
 *                        are wct_stylize_interp, 0/1 weights constant on aligned 16 x 16 blocks are wct_stylize_regions.  The call reads
 *                        (V1, V2) and the weight check back ONCE at its start (one stream synchronisation), so it cannot be captured into
 *                        a HIP graph.  Non-finite weights, weights outside [0, 1] or a pixel whose weights sum to more than 1 + 1e-6
 *                        return WCT_ERR_INVALID before anything is written to out (wct_last_error says which).
 *   wct_moments_weighted per k: sum[k*C + c] = sum_p w_k(p) x_p[c], sumsq[k*C*C + a*C + b] = sum_p w_k(p) x_p[a] x_p[b] (device f64) of an
 *                        NHWC map, weights K x h x w (device fp32).  Arithmetic classes of wct_moments_labeled; bitwise reproducible.
 *   wct_apply_mixed      out_p = x_p + sum_k w_k(p) ((M_k x_p + b_k) - x_p), M [K*C*C], b [K*C] device f64 (used in fp32); layout as
 *                        wct_apply. */
int wct_stylize_interp(wct_ctx* ctx, const float* content, int H, int W, int K, const float* const* styles, const int* Hs, const int* Ws,
                       const float* lambda, float alpha, int num_run, float* out, int* Ho, int* Wo);
int wct_style_blend(wct_ctx* ctx, int level, int K, const double* stats, const float* lambda);
int wct_stylize_blend(wct_ctx* ctx, const float* content, int H, int W, const float* weights, int K, const float* const* styles, const int* Hs,
                      const int* Ws, const float* alpha, int num_run, float* out, int* Ho, int* Wo);
int wct_moments_weighted(wct_ctx* ctx, const float* feat, int C, int h, int w, const float* weights, int K, double* sum, double* sumsq);
int wct_apply_mixed(wct_ctx* ctx, const float* feat, int C, int h, int w, int layout, const float* weights, int K, const double* M,
                    const double* b, float* out);

/* Style statistics cache.  wct_style_prepare leaves, per level, the style mean and cov^(1/2) inside the
 * context; they depend only on the style image, so
 *   wct_stylize_prepared  runs the content cascade against them (no style-side work): content x style batches pay
 *                         the style side once per style, not once per pair (data_loader.py:32-36 builds the product)
 *   wct_style_export / wct_style_import  move them (device f64: C*C matrix, then C means; wct_style_stats_count
 *                         doubles) so that the GPUs of a node compute each level ONCE and broadcast it
 *                         (wct_hip/sharded.py) instead of every rank repeating all five.
 * wct_style_prepare_levels: like wct_style_prepare for the levels in `level_mask` (bit L set = level L).
 * Lifetime of the prepared statistics: there is ONE prepared slot per level.  It is rewritten by everything that computes or installs
 * single-style statistics -- wct_style_prepare(_levels), wct_style_import, wct_style_blend, wct_style_solve, wct_stylize,
 * wct_stylize_u8, wct_style_transfer_level (its level only), wct_synthesize with a texture, wct_stylize_interp (the blend of its
 * styles), the sharded calls -- and then holds THAT style.  It survives everything else, bit for bit: wct_stylize_prepared,
 * wct_synthesize without a texture, wct_stylize_regions and wct_stylize_blend (their K styles live in slots of their own), the
 * split content calls, the un-fused entry points, the mode switches, wct_reserve, and a wct_load_module of a DECODER (the style-side
 * fold of the old decoder is dropped and rebuilt from the kept statistics; after loading another ENCODER prepare again). */
int wct_style_prepare_levels(wct_ctx* ctx, const float* style, int Hs, int Ws, unsigned level_mask);
int wct_style_stats_count(const wct_ctx* ctx, int level, size_t* n_doubles);
int wct_style_export(wct_ctx* ctx, int level, double* stats);
int wct_style_import(wct_ctx* ctx, int level, const double* stats);
int wct_stylize_prepared(wct_ctx* ctx, const float* content, int H, int W, float alpha, int num_run, float* out, int* Ho,
                         int* Wo);

/* Texture synthesis, the WCT paper's fourth application: `--synthesis` of the reference (WCT.py:26, PytorchWCT/data_loader.py:61-76) --
 * the cascade of WCT.py:120-125 with uniform noise as the content and the texture as the style.  The reference's own branch cannot
 * run (data_loader.py:74 calls torch.rand_like on a PIL image); its intent is what these entries do, with the noise made on the
 * device: an image-sized fp32 buffer never crosses the host interface.
 *   wct_noise_uniform  fills planar (3 x H x W fp32, device) with uniform noise in [0, 1 - 2^-24].  The values are DEFINED BY POSITION,
 *                      never by launch geometry, library version or any framework's generator, so that any host can reproduce them:
 *                        generator  Philox4x32-10 (Salmon et al., SC'11 / Random123): multipliers 0xD2511F53, 0xCD9E8D57, key
 *                                   increments 0x9E3779B9, 0xBB67AE85, 10 rounds
 *                        key        (seed & 0xffffffff, seed >> 32)
 *                        counter    (i & 0xffffffff, i >> 32, stream_id, 0) for block i = e >> 2 of the flat element index
 *                                   e = c H W + y W + x;  element e takes output word e & 3 of its block
 *                        value      float(word >> 8) * 2^-24 (exact in fp32; the range of torch.rand)
 *                      stream_id separates independent images of one seed (the command line uses the texture's index).  planar may
 *                      have any 4-byte alignment (16-byte stores are used where it is 16-byte aligned).  H, W >= 1.  Runs on the
 *                      context's stream; allocates nothing; does not synchronise.
 *   wct_synthesize     = wct_noise_uniform(seed, stream_id, H, W) into a buffer of the context, then wct_stylize(noise, texture, ...):
 *                      bit-identical to those two calls.  texture: planar 3 x Ht x Wt, or NULL = wct_stylize_prepared against the style
 *                      statistics already in the context (wct_style_prepare / wct_style_import / wct_style_blend: one texture, many
 *                      seeds or sizes; blended textures).  The output size H x W is independent of the texture's (both at least 32 x 32:
 *                      level 5 works at 1/16 scale); out must hold 3*H*W floats, Ho x Wo = 16 floor(H / 16) x 16 floor(W / 16).  Like
 *                      wct_stylize on the 16x path the call never synchronises, allocates nothing after the first call of a size and can
 *                      be captured into one HIP graph -- seed and stream_id are then kernel arguments BAKED into the graph: a replay
 *                      repeats the same noise; capture one graph per seed, or update the node's arguments.  The f16x3 range flag
 *                      behaves as in wct_stylize.  Bad arguments return WCT_ERR_INVALID before anything is written.
 * The noise buffer (3*H*W floats) belongs to the context: allocated on the first wct_synthesize of a size, kept until wct_destroy.  It
 * comes ON TOP of wct_workspace_bytes(H, W, Ht, Wt), and wct_reserve does not allocate it.
 * Texture interpolation needs no entry of its own: wct_noise_uniform into a caller buffer + wct_stylize_interp. */
int wct_noise_uniform(wct_ctx* ctx, uint64_t seed, uint32_t stream_id, int H, int W, float* planar);
int wct_synthesize(wct_ctx* ctx, const float* texture, int Ht, int Wt, int H, int W, uint64_t seed, uint32_t stream_id, float alpha,
                   int num_run, float* out, int* Ho, int* Wo);

/* Image edge: the reference harness's ToTensor (PytorchWCT/data_loader.py:57-58: uint8 HWC -> fp32 CHW
 * / 255) and save_image (WCT.py:128; torchvision 0.2.1: mul(255).clamp(0,255).byte()) on the device.  Pointers are
 * device pointers, uint8 images are H x W x 3 interleaved and 4-byte aligned.  round_mode 0 = truncation (the
 * reference's pinned torchvision), 1 = +0.5 before truncation (torchvision >= 0.4). */
int wct_u8_to_planar(wct_ctx* ctx, const uint8_t* hwc, int H, int W, float* planar);
int wct_planar_to_u8(wct_ctx* ctx, const float* planar, int H, int W, uint8_t* hwc, int round_mode);
/* ToTensor -> wct_stylize -> save_image conversion in one call; out_hwc must hold H*W*3 bytes */
int wct_stylize_u8(wct_ctx* ctx, const uint8_t* content_hwc, int H, int W, const uint8_t* style_hwc, int Hs, int Ws,
                   float alpha, int num_run, uint8_t* out_hwc, int* Ho, int* Wo, int round_mode);

/* transforms.Resize(size) of the reference harness (PytorchWCT/data_loader.py:52-56: torchvision 0.2.1 functional.resize ->
 * PIL Image.resize((ow, oh), Image.BILINEAR)) on the device, bit-exact with Pillow's resampler (requirements.txt: Pillow==8.2.0;
 * libImaging/Resample.c: separable, horizontal pass first, antialiased triangle filter, 22-bit fixed-point weights).
 *   wct_resize_shape         torchvision's size rule: the smaller edge becomes `size` (0 or already equal: unchanged)
 *   wct_resize_u8            uint8 HWC -> uint8 HWC of oH x oW (any target size; equal sizes copy)
 *   wct_resize_u8_to_planar  the same followed by ToTensor (data_loader.py:57: planar fp32 / 255) without a uint8 round trip
 *   wct_resize_u8_filter     the same resampler with the filter chosen by id: WCT_FILTER_BILINEAR (the two entries above, bit for
 *                            bit) or WCT_FILTER_BICUBIC = Pillow's bicubic_filter (a = -0.5, support 2.0), what Image.resize((w, h))
 *                            WITHOUT a filter argument uses at the reference's Pillow pin: the texture resize of --synthesis
 *                            (data_loader.py:72).  Exactly one of dst_hwc (uint8 HWC) / planar (fp32 / 255, ToTensor) is non-NULL.
 *                            Bit-exact with Pillow's Image.resize(..., Image.BICUBIC) (tests/test_synthesis_cpu.py, _gpu.py).
 * Pointers are device pointers (any alignment: the kernels read single bytes); H and oH <= 65535 (the row index is a grid
 * dimension).  Weight tables per (input, output, filter) are built on the host on first use (O(W + H)) and cached in the context
 * (16 axes, least recently used evicted). */
#define WCT_FILTER_BILINEAR 0
#define WCT_FILTER_BICUBIC 1
int wct_resize_shape(int H, int W, int size, int* oH, int* oW);
int wct_resize_u8(wct_ctx* ctx, const uint8_t* src_hwc, int H, int W, uint8_t* dst_hwc, int oH, int oW);
int wct_resize_u8_to_planar(wct_ctx* ctx, const uint8_t* src_hwc, int H, int W, float* planar, int oH, int oW);
int wct_resize_u8_filter(wct_ctx* ctx, const uint8_t* src_hwc, int H, int W, uint8_t* dst_hwc, float* planar, int oH, int oW, int filter);

/* Colour preservation -- the entries behind `--preserve_color match | luma`: colour moments, solve, apply, match, the luminance merge and
 * the cascade with either control -- is declared in wct_hip_color.h, a header of its own that includes this one; libwct_hip.so exports both. */

/* wct_reserve allocates, up front, every workspace buffer that wct_stylize, wct_stylize_prepared and wct_style_prepare(_levels) of
 * this content / style size touch, under the context's current mode switches: after it, those calls at this or any smaller size
 * allocate nothing (wct_debug_get "ws_allocs" does not move), and a reserve of a smaller size is a no-op.  wct_workspace_bytes is
 * meant EXACTLY: the bytes the workspace of a context that held nothing holds after wct_reserve of this size (wct_debug_get
 * "ws_bytes"), which is also an upper bound of what the calls above alone would have made it hold.  Both come from one list in the
 * library.  NOT covered -- these allocate on their first call of a size, on top: the fp32 staging of wct_stylize_u8, wct_synthesize's
 * noise buffer (3*H*W floats, see there), the slots and maps of wct_stylize_regions / _interp / _blend, the layout and resize
 * temporaries of the un-fused entry points. */
size_t wct_workspace_bytes(const wct_ctx* ctx, int H, int W, int Hs, int Ws);
int wct_reserve(wct_ctx* ctx, int H, int W, int Hs, int Ws);

/* arithmetic of the 3x3 convolutions (all but the HBM-bound 3-channel first conv):
 *   1 (default)  split-f16 "f16x3" MFMA: x = hi + lo in f16, w.x ~ hi.hi + hi.lo + lo.hi, fp32 accumulate --
 *                fp32-class accuracy (6e-7 vs 8e-7 for exact fp32 on K = 1152 dot products) at 3/16 of the issue time;
 *                operands are ~22-bit (two f16 terms), the lo.lo product is dropped, accumulation is fp32, activations
 *                beyond +-65504 are clamped and flagged (wct_saturation_count)
 *   0            exact fp32 MFMA (v_mfma_f32_16x16x4_f32)
 * (env WCT_CONV_MODE=0|fp32 selects 0 at wct_create when WCT_DEBUG is set.) */
int wct_set_conv_mode(wct_ctx* ctx, int mode);

/* `--numpy` of the reference (WCT.py:34, util_wct.py:204-208): whiten_and_color_np adds the identity to the CONTENT
 * covariance before its SVD (util_wct.py:143) -- a different operator from the default path (max-abs 0.49 on a toy case),
 * otherwise the same steps.  0 (default): off.  A variant of the wct transform only: see wct_hip_transform.h (the choice of transform). */
int wct_set_numpy_variant(wct_ctx* ctx, int on);

/* 1 (default): the style side of a level (encode, moments, eigen-decomposition -- independent of the content) runs on
 * a context-owned side stream and overlaps the content side; 0: everything runs in order on the caller's stream
 * (used when timing individual kernels). */
int wct_set_overlap(wct_ctx* ctx, int on);

/* profiling: when enabled every kernel launch is bracketed by HIP events on the context's stream */
int wct_profile_enable(wct_ctx* ctx, int on);
int wct_profile_reset(wct_ctx* ctx);
int wct_profile_read(wct_ctx* ctx, wct_prof_entry* entries, int max_entries, int* n_entries);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_H */
