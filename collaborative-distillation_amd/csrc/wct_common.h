// Shared declarations of libwct_hip (gfx950 only).  Internal -- the public C ABI is include/wct_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <stdlib.h>
#include <stdio.h>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// Experiment / debug switches read from the environment are honoured ONLY when WCT_DEBUG is set (to anything but "0"): a
// stray WCT_* variable in a production environment must never change results.  Contexts have wct_debug_set() instead.
static inline const char* wct_debug_env(const char* name) {
  const char* g = getenv("WCT_DEBUG");
  if (!g || !g[0] || (g[0] == '0' && !g[1])) return nullptr;
  return getenv(name);
}

// What a size-selected launcher chose for its last launch on this host thread (launch_enc_head, launch_dec_tail, launch_l1_decode,
// launch_conv3x3_f16, launch_conv3x3_sp).  The launchers are free functions without a context, so they leave the choice here and
// wct_ctx.h's ProfScope appends it to the profile record's name as "#<form><tile_h>[m]" when wct_debug_set("prof_forms", 1) is on
// (tests/test_geometry_gpu.py).  form: 'r' two-role head, 't' plain nine-tap tiles, 'u' upsample (2x2 per parity) form, 's' small-map
// form, '3' three-stage persistent kernel; 0 = the launcher has a single form and says nothing.  multi: the grid is smaller than
// tiles x cout groups, so some workgroup walks more than one unit.
// The plan-driven launchers of the feature-space kernels (launch_moments, launch_moments_labeled, launch_moments_weighted, the fold
// launchers, launch_patch_match) leave a ready-made suffix in `text` instead (note_launch_text; grammar: include/wct_hip.h, "prof_forms"); ProfScope
// appends ":<text>" (tests/test_sweep_gpu.py holds it against tests/sweep_cases.py).  Defined in wct_api.hip; not part of the ABI.
struct LaunchForm { char form; int tile_h; bool multi; char text[24]; };
extern __thread LaunchForm wct_launch_form __attribute__((visibility("hidden")));
static inline void note_launch_form(char form, int tile_h, long units, long grid) {
  wct_launch_form.form = form; wct_launch_form.tile_h = tile_h; wct_launch_form.multi = units > grid;
}
// moments family: "<family><MP>.<NLD>.<PW>[s]<d|f>" (s: pixel split; d / f: fp64 / fp32-block products)
static inline void note_moments_form(char family, int mp, int nld, int pw, bool pixsplit, bool f32) {
  snprintf(wct_launch_form.text, sizeof wct_launch_form.text, "%c%d.%d.%d%s%c", family, mp, nld, pw, pixsplit ? "s" : "", f32 ? 'f' : 'd');
}
static inline void note_launch_text(const char* text) { snprintf(wct_launch_form.text, sizeof wct_launch_form.text, "%s", text); }

// The context's saturation counter (wct_api.hip sat_dev): +1 per thread (or wave) that clamped an activation, SATURATING -- the
// thread that wraps the 32-bit counter sees old == 0xffffffff itself and pins it at 2^31 (so does every add above it).
__device__ __forceinline__ void sat_raise(unsigned* counter) {
  const unsigned old = atomicAdd(counter, 1u);
  if (old >= 0x80000000u) atomicMax(counter, 0x80000000u);
}

// K layout of the 3-channel first conv on 16x16x32 f16 MFMAs (conv_f16_dev.h l1_conv_group, enc_head_kernel; host packing
// api_model.hip pack_head_f16): 27 "singles" (split term 0: w_hi x_hi, 1: w_hi x_lo, 2: w_lo x_hi; window position pos = 3 dy + dx;
// 4 halfs RGB0 each) in 4 K-steps x 4 lane groups x 2.  One ds_read_b64 serves 32 lanes = two lane groups: their two singles are
// always in the SAME window row and the SAME plane (hi or lo), so the two 128-byte runs overlap on identical addresses instead of
// landing on the same banks 288 bytes apart (the contiguous order 9 term + pos did: 25 LDS cycles per 16 reads instead of 16).
// Pair q = 4 s + 2 u + (kq >> 1) of lane groups (2 h, 2 h + 1); five pairs per window row, the 16th is empty.
struct L1Single { int term, pos; bool zero; };
__host__ __device__ constexpr L1Single l1_single(int s, int kq, int u) {
  const int q = 4 * s + 2 * u + (kq >> 1), j = kq & 1;
  if (q == 15) return L1Single{0, 0, true};
  const int r = q / 5, m = q - 5 * r;
  return m == 0 ? L1Single{0, 3 * r + j, false}
       : m == 1 ? (j == 0 ? L1Single{0, 3 * r + 2, false} : L1Single{2, 3 * r, false})
       : m == 2 ? L1Single{2, 3 * r + 1 + j, false}
       : m == 3 ? L1Single{1, 3 * r + j, false}
                : L1Single{1, 3 * r + 2, j != 0};      // the partner of the row's last lo single reads the same place with zero weights
}

// ---- conv3x3 (reflect-pad + 3x3 conv + bias + ReLU, optional fused nearest-x2 input / 2x2 max-pool output)
enum ConvFlags : int {
  CONV_IN_NCHW3 = 1,   // input is a planar 3xHxW image (first encoder conv, conv0 folded in)
  CONV_UP_IN = 2,      // input tensor is stored at (H/2, W/2): nearest x2 fused into the tile load
  CONV_POOL_OUT = 4,   // write max over 2x2 (floor mode) instead of the full-resolution output
  CONV_OUT_NCHW3 = 8,  // output is a planar 3xHxW image (last decoder conv)
  CONV_NO_RELU = 16,   // affine only (used by wct_apply: centre-tap 1x1)
  CONV_IN_SP16 = 32,   // input is in the split-f16 SP16 format (conv_f16_dev.h) instead of fp32 NHWC
  CONV_OUT_SP16 = 64,  // output is written in SP16
};

struct ConvDesc {
  int cin, cout;       // logical channels
  int cin_chunks;      // ceil(cin/16)  (1 for CONV_IN_NCHW3)
  int cout_pad;        // multiple of 16
  int flags;
  const float* wpk;    // device, packed [chunk][tap][kq][cout_pad][4]  (IN_NCHW3: [tap][4][cout_pad])
  const float* bias;   // device, [cout_pad]
  // split-f16 ("f16x3") form of the same weights, conv3x3_f16.hip: [chunk][taps][hi/lo][kh][cout_pad] x 8 halfs,
  // pre-multiplied by a power of two; the epilogue multiplies by inv_scale (or *inv_scale_ptr when non-null)
  const void* wpk16 = nullptr;
  float inv_scale = 1.f;
  const float* inv_scale_ptr = nullptr;
  // 3-channel first conv with <= 32 couts (level-1 encoder): f16x3 slot packing for level1.hip, [2 cout tiles] (device)
  const void* l1w16 = nullptr;
  const float* l1bias = nullptr;   // [32], zero padded
  float l1inv = 1.f;
  // last decoder conv (16-channel chunks -> 3 couts): the same split-f16 weights (same scale) in the block-packed layout of
  // conv_f16_dev.h c3_block_compute, [chunk][8 ks][hl][kq][16 m] x 16 B, for the fused tails
  const void* wph16 = nullptr;
  // CONV_UP_IN layers with 16 -> 16 channels (the fused tail's first conv): the 3x3 convolution of a nearest-x2 upsampled map is,
  // per output parity (a, b), a 2x2 convolution of the LOW-RESOLUTION map with summed taps (conv3x3_f16.hip dec_tail_kernel) --
  // split-f16 weights [phase 2a + b][tap row][hl][kq][16 couts] x 16 B with their own power-of-two scale
  const void* wup16 = nullptr;
  float inv_scale_up = 1.f;
  // the context's sticky saturation counter (device): raised by the f16x3 kernels when an activation exceeded +-65504 and
  // was clamped (conv_f16_dev.h SatTrack); may be null
  unsigned* sat = nullptr;
};

// Launch one conv layer.  (H, W) = spatial size the convolution runs at (after the fused upsample,
// before the fused pool).  `in` is NHWC [inH*inW][cin] (or planar 3xHxW), `out` NHWC or planar.
hipError_t launch_conv3x3(const ConvDesc& d, const float* in, float* out, int H, int W, hipStream_t s);

hipError_t launch_conv3x3_f16(const ConvDesc& d, const float* in, float* out, int H, int W, hipStream_t s);
size_t conv_f16_weight_bytes(int cin, int cout_pad, int taps);
// SP16-input layers with >= 32 couts: persistent DMA-staged kernel (conv3x3_sp.hip)
bool conv_sp_supported(const ConvDesc& d);
hipError_t launch_conv3x3_sp(const ConvDesc& d, const void* in, void* out, int H, int W, hipStream_t s);
bool conv_sp_up_form(const ConvDesc& d, int H, int W);   // that launch takes the upsample form (4/9 of the products): own profile family
// fused full-resolution ends of the 16x networks (conv11+conv12+pool / conv12+conv11): see conv3x3_f16.hip
bool conv_fusable_head(const ConvDesc& d0, const ConvDesc& d1);
bool conv_fusable_tail(const ConvDesc& d0, const ConvDesc& d1);
hipError_t launch_enc_head(const ConvDesc& d0, const ConvDesc& d1, const float* img, float* out, int H, int W, hipStream_t s);   // d1.flags & CONV_OUT_SP16
hipError_t launch_dec_tail(const ConvDesc& d0, const ConvDesc& d1, const float* in, float* out, int H, int W, hipStream_t s);
// level 1 without materialising relu1_1 (level1.hip, moments.hip)
bool l1_capable(const ConvDesc& enc0);   // l1_encode: 3 -> <= 32 channels
bool l1_fusable(const ConvDesc& enc0);   // l1_moments / l1_decode: 3 -> <= 24 channels
hipError_t launch_l1_encode(const ConvDesc& enc0, const float* img, float* out, int H, int W, hipStream_t s);
hipError_t launch_l1_decode(const ConvDesc& enc0, const ConvDesc& dec0_folded, const float* img, float* out, int H, int W, hipStream_t s);
// the 3 -> 64 first conv of the un-pruned encoders in f16x3 (level1.hip in3_wide_kernel): fp32 NHWC or SP16 out
bool in3_wide_capable(const ConvDesc& enc0);
hipError_t launch_in3_wide(const ConvDesc& enc0, const float* img, void* out, int H, int W, bool out_sp, bool exact_fp32, hipStream_t s);
size_t l1_moments_workspace_bytes();
hipError_t launch_l1_moments(const ConvDesc& enc0, const float* img, int H, int W, int x0, int x1, double* sum, double* sumsq,
                             void* workspace, size_t workspace_bytes, hipStream_t s, bool f32_products = false);
// fp32 packed weights (device) -> scaled split-f16 packed weights + inverse scale (device scalar)
//   have_max: *maxbits_dev already holds max |w| (written by launch_fold_affine); otherwise it is computed here
//   nmax > 1: maxbits_dev is an ARRAY of nmax partial maxima (launch_fold_fast's rowmax) that the kernel reduces itself
hipError_t launch_split_pack(const float* wpk32, int cin, int cout_pad, int taps, unsigned* maxbits_dev, void* out,
                             float* inv_scale_out, hipStream_t s, bool have_max = false, int nmax = 1);
// the same weights (cout_pad 16, 3 real couts) in the block-packed layout; *maxbits_dev must hold max |w| (same scale as above)
size_t conv_phase_weight_bytes(int cin);
hipError_t launch_split_pack_phase(const float* wpk32, int cin, const unsigned* maxbits_dev, void* out, hipStream_t s, int nmax = 1);

// ---- image edge: uint8 HWC <-> planar fp32 (ToTensor / save_image of the reference's harness)
hipError_t launch_u8_to_planar(const uint8_t* hwc, long npix, float* planar, hipStream_t s);
hipError_t launch_planar_to_u8(const float* planar, long npix, uint8_t* hwc, int round_mode, hipStream_t s);
// ---- seeded uniform noise (noise.hip): planar 3 x H x W fp32 in [0, 1), Philox4x32-10 keyed by seed, values defined by position alone
hipError_t launch_noise_uniform(unsigned long long seed, unsigned stream_id, int H, int W, float* planar, hipStream_t s);
// ---- colour preservation (color.hip; include/wct_hip_color.h): fp64 raw colour moments of a planar image (stage-1 partials in `workspace`,
//      a fixed-order second stage; the summation tree depends on npix alone), the 3 x 3 solve A = cov_c^(1/2) cov_s^(-1/2), t = mu_c - A mu_s
//      (one thread, cyclic Jacobi), out_p = float(A x_p + t), and the luminance merge out_c = content_c + (Y(stylised) - Y(content))
long color_moments_tiles(long npix);
long color_moments_max_pixels();   // above it the second stage would add more than 4096 partials in sequence: refused by the API
size_t color_moments_workspace_bytes(long npix);
hipError_t launch_color_moments(const float* planar, long npix, double* sum, double* sumsq, void* workspace, size_t workspace_bytes, hipStream_t s);
hipError_t launch_color_solve(double n_c, const double* sum_c, const double* sumsq_c, double n_s, const double* sum_s, const double* sumsq_s,
                              double eps, double* A, double* t, hipStream_t s);
hipError_t launch_color_apply(const float* in, long npix, const double* A, const double* t, float* out, hipStream_t s);
hipError_t launch_luma_merge(const float* stylised, int Ho, int Wo, const float* content, int Hc, int Wc, float* out_planar, uint8_t* out_hwc,
                             int round_mode, hipStream_t s);
// ---- guided-filter smoothing (smooth.hip; include/wct_hip_smooth.h): four launches on `s`; `sums` (21 fp64 planes of Ho Wo) and `ab` (12 fp32
// planes) are the caller's scratch.  smooth_vseg / smooth_hseg: the rows / columns between two restarts of the running sums.
int smooth_vseg(int r);
int smooth_hseg();
size_t smooth_sums_bytes(long npix);
size_t smooth_ab_bytes(long npix);
hipError_t launch_guided_filter(const float* src, int Ho, int Wo, const float* guide, int Hg, int Wg, int r, double eps, float* out_planar,
                                uint8_t* out_hwc, int round_mode, double* sums, size_t sums_bytes, float* ab, size_t ab_bytes, hipStream_t s);
// ---- proxy mode's bilateral grid (bgrid.hip; include/wct_hip_bgrid.h).  launch_bgrid_fit: 5 + 3 smooth launches (one more when a support is taller
// than one row chunk: bgrid_fit_chunks) on `s`; `ws` (bgrid_fit_workspace_bytes) is the caller's scratch.  launch_bgrid_slice: one launch;
// use_lds false reads every tile's vertices from global memory (debug key "bgrid_lds": same bits).
__attribute__((visibility("hidden"))) int bgrid_fit_chunks(int h, int gh);
__attribute__((visibility("hidden"))) size_t bgrid_fit_workspace_bytes(int h, int gz, int gh, int gw);
__attribute__((visibility("hidden"))) hipError_t launch_bgrid_fit(const float* cl, const float* sl, int h, int w, int gz, int gh, int gw, double eps,
                                                                  int smooth, float* grid, double* ws, size_t ws_bytes, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_bgrid_slice(const float* grid, int gz, int gh, int gw, const float* content, int H, int W,
                                                                    float* out_planar, uint8_t* out_hwc, int round_mode, bool use_lds, hipStream_t s);
// ---- the device JPEG encoder (jpeg.hip; include/wct_hip_jpeg.h).  launch_jpeg_blocks: one launch.  launch_jpeg_pack: seven (eight with a
// header, which is then written in front of the segment and counted in *len); `ws` (jpeg_workspace_bytes) and `stream` (jpeg_stream_bytes) are
// the caller's scratch.  The grids are functions of (H, W) alone.
__attribute__((visibility("hidden"))) long jpeg_num_blocks(int H, int W);
__attribute__((visibility("hidden"))) size_t jpeg_workspace_bytes(long nb);
__attribute__((visibility("hidden"))) size_t jpeg_stream_bytes(long nb);
__attribute__((visibility("hidden"))) hipError_t launch_jpeg_blocks(const uint8_t* hwc, int H, int W, int quality, int16_t* coef, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_jpeg_pack(const int16_t* coef, int H, int W, const uint8_t* header, uint8_t* out,
                                                                  uint64_t capacity, uint64_t* len, void* ws, void* stream, hipStream_t s);
// ---- the device JPEG decoder (jdec.hip; include/wct_hip_jdec.h).  `f` has passed wct_jdec::info_ok.  launch_jdec_coefficients: the unstuffing,
// WCT_JDEC_LAUNCHES launches of the synchronisation, the count's scan, the write pass and the DC sums; `ws` (jdec_workspace_bytes) and `stream`
// (jdec_stream_bytes) are the caller's scratch.  launch_jdec_pixels: two launches; `planes` (jdec_planes_bytes) the caller's scratch.
struct wct_jdec_info;
__attribute__((visibility("hidden"))) size_t jdec_stream_bytes(size_t n);
__attribute__((visibility("hidden"))) size_t jdec_workspace_bytes(size_t n, const wct_jdec_info& f);
__attribute__((visibility("hidden"))) size_t jdec_planes_bytes(const wct_jdec_info& f);
__attribute__((visibility("hidden"))) hipError_t launch_jdec_coefficients(const uint8_t* scan, const wct_jdec_info& f, int rounds, int16_t* coef,
                                                                          uint32_t* status, void* ws, void* stream, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_jdec_pixels(const int16_t* coef, const wct_jdec_info& f, uint8_t* hwc, void* planes, hipStream_t s);
// ---- patch swap (swap.hip; include/wct_hip_swap.h).  launch_patch_match: the key norms, then one launch per chunk of `key_chunk` keys, then the
// read-out; `run` (swap_run_bytes(Nq): the running (score, index) of every query) and `rnorm` (swap_norm_bytes(Nk)) are the caller's scratch; `sat`:
// the context's saturation counter.  The number of launches is a function of (hs, ws, key_chunk) alone.
size_t swap_run_bytes(long nq);
size_t swap_norm_bytes(long nk);
hipError_t launch_patch_match(const float* q, int h, int w, const float* k, int hs, int ws, int C, int key_chunk, int32_t* idx, float* best,
                              void* run, size_t run_bytes, float* rnorm, size_t norm_bytes, unsigned* sat, hipStream_t s);
hipError_t launch_patch_assemble(const int32_t* idx, int h, int w, const float* v, int hs, int ws, int C, const float* base, float alpha, float* out,
                                 hipStream_t s);
// ---- attention-weighted style statistics (attn.hip; include/wct_hip_attn.h).  launch_attn_diag: (M, b) of the standardised map -- M diagonal,
// C x C -- and (mu, sigma) (may be null) from raw moments; launch_attn_unit: unit rows; launch_attn_stats: the maximum of |v| and the scale of
// v^2 into `scratch` (the float part of attn_stat_bytes), then one launch per `query_chunk` queries; launch_attn_apply: the elementwise result.
__attribute__((visibility("hidden"))) size_t attn_stat_bytes(int C);   // mu [C] | sigma [C] doubles, then 1024 partial maxima | scale | 1 / scale
__attribute__((visibility("hidden"))) hipError_t launch_attn_diag(int C, double n, double eps, const double* sum, const double* sumsq, double* M, double* b,
                                                                  double* mu_out, double* sigma_out, hipStream_t s);
// out = fp32(W (x - sum / npix)), fp64 throughout; Mt [C * C] receives the transpose of M = W
__attribute__((visibility("hidden"))) hipError_t launch_attn_whiten(const float* x, long npix, int C, const double* sum, const double* M, double* Mt,
                                                                    float* out, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_attn_unit(const float* in, long n, int C, float* out, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_attn_stats(const float* qhat, int Nq, const float* khat, const float* v, int Nk, int C, float tau,
                                                                   int query_chunk, float* mean, float* var, float* scratch, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_attn_apply(const float* mean, const float* var, const float* c_std, const float* cF, long n, int C,
                                                                   const double* mu_s, const double* sigma_s, float alpha, float* out, hipStream_t s);
// *dst = (double)*counter on the stream (wct_range_flag_f64: the saturation counter as a value a sharded run can all-reduce)
hipError_t launch_counter_to_f64(const unsigned* counter, double* dst, hipStream_t s);
// ---- image edge: transforms.Resize = Pillow's bilinear resampler, bit-exact (resize.hip)
enum ResizeFilter : int { RESIZE_BILINEAR = 0, RESIZE_BICUBIC = 1 };   // = WCT_FILTER_* of include/wct_hip.h
void resize_axis_tables(int in_size, int out_size, int filter, int& ksize, std::vector<int>& bounds, std::vector<int>& kk);   // host
hipError_t launch_resize_u8(const uint8_t* in, int H, int W, int oH, int oW, const int* bounds_h, const int* kk_h, int ksize_h,
                            const int* bounds_v_shifted, const int* kk_v, int ksize_v, int row0, int rows, uint8_t* tmp, uint8_t* out,
                            float* planar, hipStream_t s);
// ---- scale control (scale.hip; include/wct_hip_scale.h): out = R(a -> oH x oW, filter) on planar 3 x H x W fp32, or with b (3 x H x W) and c
// (3 x oH x oW) both given the merge R(a - gain b) + gain c; two launches (the weight tables into `tab`, the caller's scratch of
// scale_table_bytes; then the tiles).  scale_tile_w / _h: the kernel's output tile at mild ratios.
int scale_tile_w();
int scale_tile_h();
size_t scale_table_bytes(int H, int W, int oH, int oW, int filter);
hipError_t launch_scale(const float* a, const float* b, const float* c, float gain, int H, int W, float* out, int oH, int oW, int filter, void* tab,
                        size_t tab_bytes, hipStream_t s);
// ---- video mode (video.hip; include/wct_hip_video.h).  run / pend: a level's [rs C | rss C*C] inside a clip; flags: (frames, cut)
//   launch_clip_track      the tracking step T of one level in place on (sum, sumsq), r' also into pend; one launch, C in 1 .. 512
//   launch_clip_store      prev_content <- the top-left Ho x Wo of content, prev_out <- out (content == NULL: no images), then
//                          run[0 .. nd) <- pend[0 .. nd) and frames += 1; one launch.  Wo a multiple of 4, the two prev_ images 16-byte aligned
//   launch_temporal_blend  the blend B in one launch; blend_tile_w / _h: the kernel's output tile
// (hidden: the library's dynamic symbol table gains the header's entries only)
__attribute__((visibility("hidden"))) int blend_tile_w();
__attribute__((visibility("hidden"))) int blend_tile_h();
__attribute__((visibility("hidden"))) hipError_t launch_clip_track(int C, double n, int decide, double rate, double cut_thr, const double* run, double* pend, double* sum, double* sumsq,
                             int* flags, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_clip_store(const float* content, int Hc, int Wc, const float* out, int Ho, int Wo, float* prev_content, float* prev_out,
                             const double* pend, double* run, size_t nd, int* flags, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_temporal_blend(const float* cur, int Hc, int Wc, const float* prev, const float* sty, const float* pout, int Ho, int Wo, float blend,
                                 float sigma, int r, const int* cut_flag, float* out, uint8_t* out_hwc, int round_mode, hipStream_t s);
// ---- motion compensation (motion.hip; include/wct_hip_motion.h).  A pyramid is packed bytes: level k at pyr + lv[k].pyr_off, rows of
// lv[k].pitch bytes (W_k rounded up to a dword, the padding zero).  The fields of all levels share one block of int16: level k at lv[k].mv_off.
struct MotionLevel { int H, W, pitch, nby, nbx; size_t pyr_off, mv_off; };
struct MotionLayout { int levels; MotionLevel lv[4]; size_t pyr_bytes, mv_count; };   // pyr_bytes: a multiple of 256; mv_count: int16 values
//   motion_layout           false: levels outside 1 .. 4 or Ho / Wo < 2^(levels - 1)
//   launch_motion_pyramid   every level of the luma pyramid of the top-left Ho x Wo of a planar image in ONE launch
//   launch_motion_unpad     the pitched pyramid as the dense concatenation wct_motion_luma returns; one launch
//   launch_motion_search    one level of the block search: mv_out of that level from the two pyramids and (below the top level) the
//                           parent level's field; a non-zero *cut_flag (NULL: 0) writes zeros instead
//   launch_motion_blend     launch_temporal_blend against the previous images displaced by the level-0 field mv
__attribute__((visibility("hidden"))) bool motion_layout(int Ho, int Wo, int levels, MotionLayout& l);
__attribute__((visibility("hidden"))) hipError_t launch_motion_pyramid(const float* img, int Hc, int Wc, const MotionLayout& l, uint8_t* pyr, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_motion_unpad(const uint8_t* pyr, const MotionLayout& l, uint8_t* out, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_motion_search(const uint8_t* pyr_cur, const uint8_t* pyr_prev, const MotionLayout& l, int level, int range,
                                                                      int penalty, const int16_t* mv_parent, int16_t* mv_out, const int* cut_flag, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_motion_blend(const float* cur, int Hc, int Wc, const float* prev, const float* sty, const float* pout, int Ho,
                                                                     int Wo, float blend, float sigma, int r, const int* cut_flag, float* out, uint8_t* out_hwc,
                                                                     int round_mode, const int16_t* mv, int nbx, hipStream_t s);

// ---- pitched block copy of floats (rows x width; the sharded cascade's level crops, halo packing and assembly: a planar 3 x H x W image is
//      3H rows of pitch W)
hipError_t launch_copy_block(const float* src, long src_pitch, float* dst, long dst_pitch, long rows, int width, hipStream_t s);
struct CopySegs { const float* src[3]; float* dst[3]; long src_pitch[3], dst_pitch[3]; int width[3]; };   // width 0: segment unused
hipError_t launch_copy_blocks(const CopySegs& g, long rows, hipStream_t s);

// ---- layout
hipError_t launch_nhwc_to_nchw(const float* in, float* out, int C, int npix, hipStream_t s);
hipError_t launch_nchw_to_nhwc(const float* in, float* out, int C, int npix, hipStream_t s);

// ---- moments: raw sums  sum[c] = SUM_p x[p][c],  sumsq[a][b] = SUM_p x[p][a] x[p][b]   (fp64)
size_t moments_workspace_bytes(int C, long npix);
// window = rows [0,h) x cols [x0,x1) of an NHWC map of width wfull
// f32_products: products and 64-pixel block sums on the fp32 matrix cores, block totals in fp64 (moments.hip F32 variant); false: fp64 throughout
hipError_t launch_moments(const float* feat_nhwc, int C, int h, int wfull, int x0, int x1, double* sum,
                          double* sumsq, void* workspace, size_t workspace_bytes, hipStream_t s, bool f32_products = false);

// ---- solve, in two steps (solve.hip): moments of one map -> EigResult; two EigResults -> M (C x C), b (C)
//      csF = M cF + b   (util_wct.py:62-131, 219).  EigResult = doubles G[C*C] | lam[C] | mu[C] | floor | pad
size_t eig_result_bytes(int C);
size_t eig_result_F_offset(size_t C);   // doubles: where F = cov^(+-1/2) starts inside an EigResult (mu is at C*C + C)
size_t eig_workspace_bytes(int C);
size_t assemble_workspace_bytes(int C);
//   diag_add is added to the covariance's diagonal (1.0 on the content side = the reference's `--numpy` variant)
//   wide_model: the module set has feature maps wider than 128 channels (--mode original); its 128-channel level then takes the
//   deflated iteration too (ill-conditioned there: the 26-iteration budget ran out and the 2 ms LDS Jacobi took over)
//   ok_defer (device int, C > 128 path only -- eig_is_big): instead of reading the iteration's outcome back and synchronising the
//   stream inside the call (to decide about the slow global-memory Jacobi net), the outcome is written there and the CALLER checks
//   it at its own synchronisation point, re-running without deferral if it is 0
bool eig_is_big(int C, bool wide_model);
hipError_t launch_eig(int C, double n, const double* sum, const double* sumsq, int inverse, double* res, int* info_dev,
                      void* workspace, size_t workspace_bytes, hipStream_t s, double diag_add = 0.0, bool wide_model = false,
                      int* ok_defer = nullptr, int coop_xcd = -1, unsigned* coop_state = nullptr, int* coop_epoch = nullptr, unsigned* coop_aborts = nullptr, bool* coop_used_out = nullptr,
                      int sched_maxit = 0, double sched_guess = -1.0);
//   coop_xcd (0..7, or -1: off) + coop_state (32 device bytes of the calling lane, zero at first use) + coop_epoch (the lane's
//   HOST counter of such solves, advanced here): the 128-channel levels of --mode 16x as ONE launch on that XCD (solve.hip
//   ns_coop128_kernel); lanes that may solve at the same time are given different XCDs
//   sched_maxit > 0 (C <= 128 without deflation only; <= 32): the caller's own iteration budget and assumed lower spectral bound
//   sched_guess of the scaled iteration instead of the defaults chosen for covariances (the ot transform's B = S cov_c S: transform.hip)
hipError_t launch_assemble(int C, const double* eig_c, const double* eig_s, double alpha, double rel_thresh,
                           double* M, double* b, void* workspace, size_t workspace_bytes, hipStream_t s);

// ---- the ot / adain transforms' C x C part (transform.hip; include/wct_hip_transform.h).  S, mu_s: the style slot (cov_s^(1/2), mean)
//   launch_ot_sandwich  B = sym(S cov_c S) from the raw content moments, zeros[0..C) = 0 (B then enters launch_eig as the pseudo-moments
//                       n = 2, sum = zeros, sumsq = B); tmp: C*C doubles
//   launch_ot_assemble  T = S Z S (Z = B^(-1/2)), M = alpha T + (1 - alpha) I, b = alpha (mu_s - T sum_c / n); tmp: C*C doubles
//   launch_adain_assemble  T = diag(sqrt((SUM_k S_ik^2 + eps) / (cov_c_ii + eps))), the same M and b; *info_dev = 0
size_t ot_workspace_bytes(int C);   // B | tmp | zeros
hipError_t launch_ot_sandwich(int C, double n, const double* sum_c, const double* sumsq_c, const double* S, double* B, double* zeros, double* tmp, hipStream_t s);
hipError_t launch_ot_assemble(int C, double alpha, const double* S, const double* mu_s, const double* Z, double n, const double* sum_c, double* tmp,
                              double* M, double* b, hipStream_t s);
hipError_t launch_adain_assemble(int C, double alpha, double eps, const double* S, const double* mu_s, double n, const double* sum_c, const double* sumsq_c,
                                 double* M, double* b, int* info_dev, hipStream_t s);

// ---- the seeded rotation of style diversification (rotate.hip; include/wct_hip_diverse.h), fp64, C even, 2..512
//   launch_rotation_make   Z [C*C] = the Cayley transform of the seeded skew matrix A (skew [C*C], may be null, receives A); strength 0 writes
//                          I and needs no workspace; C > 128 synchronises the stream inside launch_eig (the outcome of the deflated iteration)
//   launch_rotation_apply  out = F Z (out overlaps neither)
__attribute__((visibility("hidden"))) size_t rotation_workspace_bytes(int C);   // A | B | U | zeros | EigResult | launch_eig's workspace | info
__attribute__((visibility("hidden"))) hipError_t launch_rotation_make(int C, unsigned long long seed, unsigned stream_id, unsigned tag, double strength, double* Z,
                                                                      double* skew, void* workspace, size_t workspace_bytes, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t launch_rotation_apply(int C, const double* F, const double* Z, double* out, hipStream_t s);

// ---- fold csF = M x + b into a decoder's first conv:  W' = W o M, b' = bias + W o b
//      w_oihw: device [cout][cin][3][3] fp32 (original weights), out: packed weights + bias for ConvDesc
//      maxbits_dev (optional): receives max |W'| as float bits for launch_split_pack(..., have_max = true)
// the same fold for the wide models' decoders (cin = 256 / 512) as an fp64 matrix-core GEMM (solve.hip fold_gemm_kernel): `rows` =
// the layer's weights as doubles [(o, tap)][c] followed by their tap sums [o][c] (fold_gemm_rows_doubles; launch_fold_rows, once)
bool fold_gemm_capable(int cout, int cin, int cout_pad);
size_t fold_gemm_rows_doubles(int cout, int cin);
hipError_t launch_fold_rows(const float* w_oihw, int cout, int cin, double* rows, hipStream_t s);
hipError_t launch_fold_gemm(const double* rows, const float* bias, int cout, int cin, int cout_pad, const double* M, const double* b,
                            float* wpk_out, float* bias_out, unsigned* maxbits_dev, hipStream_t s);
hipError_t launch_fold_affine(const float* w_oihw, const float* bias, int cout, int cin, int cout_pad,
                              const double* M, const double* b, float* wpk_out, float* bias_out,
                              unsigned* maxbits_dev, hipStream_t s);
// The same fold without C x C products on the content side's critical path (misc.hip): style-side part once per style
// (buf: fold_style_doubles(cout, cin) doubles), then Wc = cov_c^(-1/2), mu_c -> folded weights + bias + per-output-row max |W'|
// (rowmax_dev: cout_pad words, consumed by launch_split_pack(..., nmax = cout_pad)); cin <= 128
bool fold_fast_capable(int cin);
size_t fold_style_doubles(int cout, int cin);
hipError_t launch_fold_style(const float* w_oihw, int cout, int cin, const double* Ss, const double* mu_s, double* buf, hipStream_t s);
hipError_t launch_fold_fast(const float* w_oihw, const float* bias, int cout, int cin, int cout_pad, const double* style_buf, const double* Wc,
                            const double* mu_c, double alpha, float* wpk_out, float* bias_out, unsigned* rowmax_dev, hipStream_t s);
// pack [cout][cin][3][3] (+ bias) into the conv kernel's layout (device side, used for the apply conv)
hipError_t launch_pack_center_tap(const double* M, const double* b, int C, int cout_pad, float* wpk_out,
                                  float* bias_out, hipStream_t s);

// ---- spatial control (regions.hip): per-label moments and affine maps over a uint8 label map (label >= K: unstyled)
//   launch_labels_levels  lab_L[i][j] = labels[i s + s/2][j s + s/2] (s = 2^(L-1)) into out[L] (h[L] x w[L], L = 1..5) and the
//                         histograms hist[6][256] (device, zeroed here): [0] = the whole H x W map, [L] = lab_L
//   launch_moments_labeled  n[K], sum[K][C], sumsq[K][C][C] (fp64) of an NHWC map of npix pixels; f32_products as launch_moments
//   launch_apply_labeled    out_p = M_lab(p) x_p + b_lab(p) (fp64 maps used in fp32), labels >= K copied through
//   launch_mb_identity      M_k = I, b_k = 0 for the labels set in `mask`
hipError_t launch_labels_levels(const uint8_t* labels, int H, int W, const int* h, const int* w, uint8_t* const* out, unsigned* hist,
                                hipStream_t s);
size_t moments_labeled_workspace_bytes(int C, long npix, int K);
hipError_t launch_moments_labeled(const float* feat, int C, long npix, const uint8_t* lab, int K, double* n, double* sum, double* sumsq,
                                  void* workspace, size_t workspace_bytes, hipStream_t s, bool f32_products);
size_t apply_labeled_workspace_bytes(int C, int K);
hipError_t launch_apply_labeled(const float* feat, int C, long npix, const uint8_t* lab, int K, const double* M, const double* b,
                                float* out, void* workspace, size_t workspace_bytes, hipStream_t s);
hipError_t launch_mb_identity(double* M, double* b, int C, int K, unsigned mask, hipStream_t s);

// ---- k-means on NHWC fp32 feature maps (cluster.hip; include/wct_hip_guided.h); C a multiple of 4 in 4 .. 512, K <= 8, npix < 2^31
//   launch_kmeans_assign       one Lloyd step: labels (may be null), n[K], sum[K][C] (of the standardised z), cost[1], next (may be null)
//   launch_kmeans_seed         the farthest-first start: cent[K][C], idx[K]
//   launch_kmeans_standardise  shift = mean, scale = 1 / sqrt(population variance) (0 for a dead channel) from raw moments of n pixels
//   launch_kmeans_expand       out[y][x] = lab[min(y >> (level-1), h-1)][min(x >> (level-1), w-1)]
size_t kmeans_assign_workspace_bytes(int C, long npix, int K);
hipError_t launch_kmeans_assign(const float* feat, int C, long npix, const double* shift, const double* scale, const double* cent, int K,
                                uint8_t* labels, double* n, double* sum, double* cost, double* next, void* workspace, size_t workspace_bytes,
                                hipStream_t s);
size_t kmeans_seed_workspace_bytes(long npix);
hipError_t launch_kmeans_seed(const float* feat, int C, long npix, const double* shift, const double* scale, int K, double* cent, int* idx,
                              void* workspace, size_t workspace_bytes, hipStream_t s);
hipError_t launch_kmeans_standardise(const double* sum, const double* sumsq, int C, double n, double* shift, double* scale, hipStream_t s);
hipError_t launch_kmeans_expand(const uint8_t* lab, int h, int w, int level, uint8_t* out, int H, int W, hipStream_t s);

// ---- style interpolation and per-pixel style weights (blend.hip); K <= 8
//   launch_stats_blend       Fo = sum_k lam[k] F[k], muo = sum_k lam[k] mu[k] (C x C and C doubles; device pointers in host arrays), fixed
//                            k order: lam = (1, 0, ...) reproduces slot 0 bit for bit
//   launch_weights_levels    from w[K][H][W] (fp32): out[L] = [K][h[L] * wd[L]] area means over each level-L pixel's 2^(L-1) square window
//                            (L = 1..5), vv[L][8][2] = (V1, V2) = (sum w, sum w^2) of each pooled map (fp64, fixed order), cnt[0..2] =
//                            non-finite weights, finite weights outside [0, 1], pixels with sum_k w > 1 + 1e-6 (cnt: 4 device words)
//   launch_moments_weighted  sum[K][C] = sum_p w_k x, sumsq[K][C][C] = sum_p w_k x x^T (fp64) of an NHWC map, w [K][npix]; f32_products
//                            as launch_moments; bitwise reproducible
//   launch_apply_mixed       out_p = x_p + sum_k w_k(p) ((M_k x_p + b_k) - x_p) (fp64 maps used in fp32)
//   launch_scale_sums        sum_k, sumsq_k *= f[k] (f: host array)
hipError_t launch_stats_blend(int C, int K, const double* const* F, const double* const* mu, const double* lam, double* Fo, double* muo,
                              hipStream_t s);
size_t weights_levels_workspace_bytes(int H, int W);
hipError_t launch_weights_levels(const float* w, int H, int W, int K, const int* h, const int* wd, float* const* out, double* vv,
                                 unsigned* cnt, void* workspace, size_t workspace_bytes, hipStream_t s);
size_t moments_weighted_workspace_bytes(int C, long npix, int K);
hipError_t launch_moments_weighted(const float* feat, int C, long npix, const float* w, int K, double* sum, double* sumsq,
                                   void* workspace, size_t workspace_bytes, hipStream_t s, bool f32_products);
size_t apply_mixed_workspace_bytes(int C, int K);
hipError_t launch_apply_mixed(const float* feat, int C, long npix, const float* w, int K, const double* M, const double* b, float* out,
                              void* workspace, size_t workspace_bytes, hipStream_t s);
hipError_t launch_scale_sums(double* sum, double* sumsq, int C, int K, const double* f, hipStream_t s);
