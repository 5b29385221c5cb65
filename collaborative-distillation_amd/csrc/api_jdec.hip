// The device JPEG decoder's entry points of the C ABI (include/wct_hip_jdec.h): the parser on the host (jdec_parse.h), the coefficients,
// the pixels, and wct_jdec_decode, which is the composition of PUBLIC calls it documents.  Host orchestration only; the kernels are in jdec.hip.
#include "jdec_parse.h"
#include "wct_ctx.h"

using namespace wct_host;
using namespace wct_jdec;

namespace {
// the refusals the device entries share; `who` names the entry
int info_check(wct_ctx* ctx, const char* who, const wct_jdec_info* info) {
  if (!info) return fail(ctx, WCT_ERR_INVALID, "%s: NULL info", who);
  if (!info_ok(*info)) return fail(ctx, WCT_ERR_INVALID, "%s: the info is not one that wct_jdec_parse fills", who);
  if (info->scan_length > WCT_JDEC_MAX_SCAN_BYTES) return fail(ctx, WCT_ERR_INVALID, "%s: a segment of more than %u bytes", who, WCT_JDEC_MAX_SCAN_BYTES);
  return WCT_OK;
}
int rounds_check(wct_ctx* ctx, const char* who, int rounds) {
  if (rounds < 0 || rounds > WCT_JDEC_MAX_ROUNDS) return fail(ctx, WCT_ERR_INVALID, "%s: rounds 0 .. %d expected, got %d", who, WCT_JDEC_MAX_ROUNDS, rounds);
  return WCT_OK;
}
int align_check(wct_ctx* ctx, const char* who, const void* coef, const void* status) {
  if (reinterpret_cast<uintptr_t>(coef) % 16) return fail(ctx, WCT_ERR_INVALID, "%s: the coefficients must be 16-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(status) % 4) return fail(ctx, WCT_ERR_INVALID, "%s: the status slot must be 4-byte aligned", who);
  return WCT_OK;
}
int coef_buffers(wct_ctx* ctx, const wct_jdec_info& f) {
  if (int rc = ensure(ctx, ctx->jdWs, jdec_workspace_bytes((size_t)f.scan_length, f))) return rc;
  return ensure(ctx, ctx->jdStream, jdec_stream_bytes((size_t)f.scan_length));
}
}  // namespace

extern "C" {

int wct_jdec_parse(const uint8_t* file, size_t n, wct_jdec_info* info) { return parse(file, n, info); }

int wct_jdec_num_blocks(const wct_jdec_info* info, uint64_t* blocks) {
  if (!info || !blocks || !info_ok(*info)) return WCT_ERR_INVALID;
  *blocks = (uint64_t)geometry(*info).blocks;
  return WCT_OK;
}

int wct_jdec_coefficients(wct_ctx* ctx, const uint8_t* scan_dev, const wct_jdec_info* info, int rounds, int16_t* coef_dev, uint32_t* status_dev) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!scan_dev || !coef_dev || !status_dev) return fail(ctx, WCT_ERR_INVALID, "wct_jdec_coefficients: NULL segment, coefficients or status");
  if (int rc = info_check(ctx, "wct_jdec_coefficients", info)) return rc;
  if (int rc = rounds_check(ctx, "wct_jdec_coefficients", rounds)) return rc;
  if (int rc = align_check(ctx, "wct_jdec_coefficients", coef_dev, status_dev)) return rc;
  if (int rc = coef_buffers(ctx, *info)) return rc;
  ProfScope ps(ctx, ctx->main.stream, "jdec_coefficients", 0.0, 6.0 * info->scan_length + 2.0 * 128.0 * geometry(*info).blocks);
  HIPCHK(ctx, launch_jdec_coefficients(scan_dev, *info, rounds ? rounds : WCT_JDEC_ROUNDS, coef_dev, status_dev, ctx->jdWs.p, ctx->jdStream.p, ctx->main.stream));
  return WCT_OK;
}

int wct_jdec_pixels(wct_ctx* ctx, const int16_t* coef_dev, const wct_jdec_info* info, uint8_t* hwc_dev) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!coef_dev || !hwc_dev) return fail(ctx, WCT_ERR_INVALID, "wct_jdec_pixels: NULL coefficients or image");
  if (int rc = info_check(ctx, "wct_jdec_pixels", info)) return rc;
  if (int rc = align_check(ctx, "wct_jdec_pixels", coef_dev, nullptr)) return rc;
  if (int rc = ensure(ctx, ctx->jdPlanes, jdec_planes_bytes(*info))) return rc;
  ProfScope ps(ctx, ctx->main.stream, "jdec_pixels", 0.0, 128.0 * geometry(*info).blocks + 2.0 * jdec_planes_bytes(*info) + 3.0 * info->H * info->W);
  HIPCHK(ctx, launch_jdec_pixels(coef_dev, *info, hwc_dev, ctx->jdPlanes.p, ctx->main.stream));
  return WCT_OK;
}

int wct_jdec_decode(wct_ctx* ctx, const uint8_t* scan_dev, const wct_jdec_info* info, int rounds, uint8_t* hwc_dev, uint32_t* status_dev) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!scan_dev || !hwc_dev || !status_dev) return fail(ctx, WCT_ERR_INVALID, "wct_jdec_decode: NULL segment, image or status");
  if (int rc = info_check(ctx, "wct_jdec_decode", info)) return rc;
  if (int rc = rounds_check(ctx, "wct_jdec_decode", rounds)) return rc;
  if (int rc = align_check(ctx, "wct_jdec_decode", nullptr, status_dev)) return rc;
  // every buffer of this call first: a growing one synchronises, and nothing enqueued below may find its source moved
  if (int rc = ensure(ctx, ctx->jdCoef, (size_t)geometry(*info).blocks * 64 * sizeof(int16_t))) return rc;
  if (int rc = coef_buffers(ctx, *info)) return rc;
  if (int rc = ensure(ctx, ctx->jdPlanes, jdec_planes_bytes(*info))) return rc;
  int16_t* coef = reinterpret_cast<int16_t*>(ctx->jdCoef.p);
  if (int rc = wct_jdec_coefficients(ctx, scan_dev, info, rounds, coef, status_dev)) return rc;
  return wct_jdec_pixels(ctx, coef, info, hwc_dev);
}

}  // extern "C"
