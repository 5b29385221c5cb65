// The clip object of video mode (include/wct_hip_video.h) and its optional motion block (include/wct_hip_motion.h): what api_video.hip and
// api_motion.hip both see.  Private to csrc/, like wct_ctx.h.
#pragma once
#include "../../include/wct_hip_motion.h"
#include "wct_ctx.h"

// What wct_motion_attach adds to a clip: ONE device allocation, zeroed --
//   [pyramid of the frame in flight | pyramid of the previous frame | the fields of levels 0 .. levels - 1]
// each part as motion_layout (motion.hip) lays it out.  The previous pyramid is state: it is rewritten from the current one inside the
// frame's call, so one captured graph serves successive frames.
struct wct_clip_motion {
  wct_motion_params p{};
  MotionLayout lay{};
  void* base = nullptr;
  uint8_t *pyr_cur = nullptr, *pyr_prev = nullptr;
  int16_t* mv = nullptr;                // level k at mv + lay.lv[k].mv_off
};

// The state of one frame sequence: ONE device allocation, laid out as the header's Definitions say.
struct wct_clip {
  wct_ctx* owner = nullptr;
  int H = 0, W = 0, Ho = 0, Wo = 0;
  wct_clip_params p{};
  int C[6] = {0, 0, 0, 0, 0, 0};        // by level
  double n[6] = {0, 0, 0, 0, 0, 0};     // pixels of the level's feature map
  size_t off[6] = {0, 0, 0, 0, 0, 0};   // doubles in front of the level inside a block of sums
  size_t nd = 0;                        // doubles of one block of sums
  void* base = nullptr;
  double *run = nullptr, *pend = nullptr;
  int* flags = nullptr;                 // frames, cut
  float *prev_content = nullptr, *prev_out = nullptr, *stylised = nullptr;
  wct_clip_motion* motion = nullptr;    // wct_motion_attach; NULL: video mode as it was
};

namespace wct_host {
// api_video.hip
__attribute__((visibility("hidden"))) int clip_check(wct_ctx* ctx, const char* who, const wct_clip* clip);
// the blend entry of either header under the name `who`: every check, then the launch (mv == NULL: the kernel without a field)
__attribute__((visibility("hidden"))) int blend_entry(wct_ctx* ctx, const char* who, const float* cur, int Hc, int Wc, const float* prev, const float* sty,
                                                      const float* pout, int Ho, int Wo, float blend, float sigma, int radius, const int* cut_flag,
                                                      float* out_planar, uint8_t* out_hwc, int round_mode, const int16_t* mv);
// api_motion.hip
// step 2 of the frame: the field of (content's crop, the clip's previous pyramid) into the clip's level-0 field; all zero on a cut
__attribute__((visibility("hidden"))) int motion_frame_estimate(wct_ctx* ctx, wct_clip* clip, const float* content, int H, int W);
// step 4's addition: previous pyramid <- current pyramid, in stream order
__attribute__((visibility("hidden"))) int motion_frame_store(wct_ctx* ctx, wct_clip* clip);
// frees the motion block (the caller has waited for the streams)
__attribute__((visibility("hidden"))) void motion_release(wct_clip* clip);
}  // namespace wct_host
