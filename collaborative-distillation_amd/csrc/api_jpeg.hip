// The device JPEG encoder's entry points of the C ABI (include/wct_hip_jpeg.h): the header and the bound on the host, the blocks, the
// pack, and wct_jpeg_encode, which is the composition of PUBLIC calls it documents.  Host orchestration only; the kernels are in jpeg.hip.
#include "../../include/wct_hip_jpeg.h"
#include "jpeg_tables.h"
#include "wct_ctx.h"

using namespace wct_host;
using namespace wct_jpeg;

namespace {
bool dim_ok(int H, int W) { return H >= 1 && H <= WCT_JPEG_MAX_DIM && W >= 1 && W <= WCT_JPEG_MAX_DIM; }

// the refusals the device entries share; `who` names the entry
int shape_check(wct_ctx* ctx, const char* who, int H, int W) {
  if (!dim_ok(H, W)) return fail(ctx, WCT_ERR_INVALID, "%s: %d x %d is outside 1 .. %d per axis", who, H, W, WCT_JPEG_MAX_DIM);
  return WCT_OK;
}
int quality_check(wct_ctx* ctx, const char* who, int quality) {
  if (quality < 1 || quality > 100) return fail(ctx, WCT_ERR_INVALID, "%s: quality 1 .. 100 expected, got %d", who, quality);
  return WCT_OK;
}
int coef_check(wct_ctx* ctx, const char* who, const void* coef) {
  if (reinterpret_cast<uintptr_t>(coef) % 16) return fail(ctx, WCT_ERR_INVALID, "%s: the coefficients must be 16-byte aligned", who);
  return WCT_OK;
}

struct Writer {
  uint8_t* p;
  void u8(int v) { *p++ = (uint8_t)v; }
  void u16(int v) { u8(v >> 8); u8(v & 255); }
  void marker(int m, int payload) { u8(0xFF); u8(m); u16(payload + 2); }
};

int pack_impl(wct_ctx* ctx, const char* who, const int16_t* coef, int H, int W, const uint8_t* header, uint8_t* out, uint64_t capacity, uint64_t* len) {
  const long nb = jpeg_num_blocks(H, W);
  if (int rc = ensure(ctx, ctx->jpWs, jpeg_workspace_bytes(nb))) return rc;
  if (int rc = ensure(ctx, ctx->jpStream, jpeg_stream_bytes(nb))) return rc;
  ProfScope ps(ctx, ctx->main.stream, who, 0.0, 128.0 * 2.0 * nb);
  HIPCHK(ctx, launch_jpeg_pack(coef, H, W, header, out, capacity, len, ctx->jpWs.p, ctx->jpStream.p, ctx->main.stream));
  return WCT_OK;
}
}  // namespace

extern "C" {

int wct_jpeg_header(int H, int W, int quality, uint8_t* header, uint16_t* qt_y, uint16_t* qt_c) {
  if (!header || !dim_ok(H, W) || quality < 1 || quality > 100) return WCT_ERR_INVALID;
  const QuantTables q = make_quant(quality);
  Writer w{header};
  w.u8(0xFF); w.u8(0xD8);
  w.marker(0xE0, 14);
  for (char c : {'J', 'F', 'I', 'F', '\0'}) w.u8(c);
  w.u16(0x0101); w.u8(0); w.u16(1); w.u16(1); w.u8(0); w.u8(0);
  for (int t = 0; t < 2; ++t) {
    w.marker(0xDB, 65);
    w.u8(t);
    for (int z = 0; z < 64; ++z) w.u8(q.t[t][ZIGZAG[z]]);
  }
  w.marker(0xC0, 15);
  w.u8(8); w.u16(H); w.u16(W); w.u8(3);
  w.u8(1); w.u8(0x22); w.u8(0);
  w.u8(2); w.u8(0x11); w.u8(1);
  w.u8(3); w.u8(0x11); w.u8(1);
  for (int t = 0; t < 2; ++t) {
    w.marker(0xC4, 1 + 16 + 12);
    w.u8(t);
    for (int i = 0; i < 16; ++i) w.u8(DC_BITS[t][i]);
    for (int i = 0; i < 12; ++i) w.u8(DC_VALS[i]);
    w.marker(0xC4, 1 + 16 + 162);
    w.u8(0x10 | t);
    for (int i = 0; i < 16; ++i) w.u8(AC_BITS[t][i]);
    for (int i = 0; i < 162; ++i) w.u8(AC_VALS[t][i]);
  }
  w.marker(0xDA, 10);
  w.u8(3);
  w.u8(1); w.u8(0x00); w.u8(2); w.u8(0x11); w.u8(3); w.u8(0x11);
  w.u8(0); w.u8(63); w.u8(0);
  if (w.p - header != WCT_JPEG_HEADER_BYTES) return WCT_ERR_STATE;
  for (int i = 0; i < 64; ++i) {
    if (qt_y) qt_y[i] = q.t[0][i];
    if (qt_c) qt_c[i] = q.t[1][i];
  }
  return WCT_OK;
}

int wct_jpeg_bound(int H, int W, uint64_t* bytes) {
  if (!bytes || !dim_ok(H, W)) return WCT_ERR_INVALID;
  *bytes = WCT_JPEG_HEADER_BYTES + 2ull * (uint64_t)jpeg_num_blocks(H, W) * (WCT_JPEG_BLOCK_MAX_BITS / 8) + 2;
  return WCT_OK;
}

int wct_jpeg_blocks(wct_ctx* ctx, const uint8_t* hwc, int H, int W, int quality, int16_t* coef) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!hwc || !coef) return fail(ctx, WCT_ERR_INVALID, "wct_jpeg_blocks: NULL image or coefficients");
  if (int rc = shape_check(ctx, "wct_jpeg_blocks", H, W)) return rc;
  if (int rc = quality_check(ctx, "wct_jpeg_blocks", quality)) return rc;
  if (int rc = coef_check(ctx, "wct_jpeg_blocks", coef)) return rc;
  const long nb = jpeg_num_blocks(H, W);
  ProfScope ps(ctx, ctx->main.stream, "jpeg_blocks", 0.0, 3.0 * H * W + 128.0 * nb);
  HIPCHK(ctx, launch_jpeg_blocks(hwc, H, W, quality, coef, ctx->main.stream));
  return WCT_OK;
}

int wct_jpeg_pack(wct_ctx* ctx, const int16_t* coef, int H, int W, uint8_t* out, uint64_t capacity, uint64_t* len) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!coef || !out || !len) return fail(ctx, WCT_ERR_INVALID, "wct_jpeg_pack: NULL coefficients, output or length");
  if (int rc = shape_check(ctx, "wct_jpeg_pack", H, W)) return rc;
  if (int rc = coef_check(ctx, "wct_jpeg_pack", coef)) return rc;
  if (reinterpret_cast<uintptr_t>(len) % 8) return fail(ctx, WCT_ERR_INVALID, "wct_jpeg_pack: the length slot must be 8-byte aligned");
  return pack_impl(ctx, "jpeg_pack", coef, H, W, nullptr, out, capacity, len);
}

int wct_jpeg_encode(wct_ctx* ctx, const uint8_t* hwc, int H, int W, int quality, uint8_t* out, uint64_t capacity, uint64_t* len) {
  if (!ctx) return WCT_ERR_INVALID;
  WCT_GUARD(ctx);
  if (!hwc || !out || !len) return fail(ctx, WCT_ERR_INVALID, "wct_jpeg_encode: NULL image, output or length");
  if (int rc = shape_check(ctx, "wct_jpeg_encode", H, W)) return rc;
  if (int rc = quality_check(ctx, "wct_jpeg_encode", quality)) return rc;
  if (reinterpret_cast<uintptr_t>(len) % 8) return fail(ctx, WCT_ERR_INVALID, "wct_jpeg_encode: the length slot must be 8-byte aligned");
  // every buffer of this call first: a growing one synchronises, and nothing enqueued below may find its source moved
  const long nb = jpeg_num_blocks(H, W);
  if (int rc = ensure(ctx, ctx->jpCoef, (size_t)nb * 64 * sizeof(int16_t))) return rc;
  if (int rc = ensure(ctx, ctx->jpWs, jpeg_workspace_bytes(nb))) return rc;
  if (int rc = ensure(ctx, ctx->jpStream, jpeg_stream_bytes(nb))) return rc;
  uint8_t header[WCT_JPEG_HEADER_BYTES];
  if (wct_jpeg_header(H, W, quality, header, nullptr, nullptr)) return fail(ctx, WCT_ERR_STATE, "wct_jpeg_encode: the header refused %d x %d at quality %d", H, W, quality);
  int16_t* coef = reinterpret_cast<int16_t*>(ctx->jpCoef.p);
  if (int rc = wct_jpeg_blocks(ctx, hwc, H, W, quality, coef)) return rc;
  return pack_impl(ctx, "jpeg_pack", coef, H, W, header, out, capacity, len);
}

}  // extern "C"
