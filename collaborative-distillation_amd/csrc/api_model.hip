// Module loading behind the C ABI (include/wct_hip.h wct_load_module, wct_feature_shape): the host-side weight packers of every conv kernel
// family and the uploads of one layer's device copies.
#include "wct_ctx.h"

using namespace wct_host;

namespace {

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

int upload_f16(wct_ctx* ctx, void** dst, const std::vector<_Float16>& v) {
  HIPCHK(ctx, hipMalloc(dst, v.size() * sizeof(_Float16)));
  HIPCHK(ctx, hipMemcpy(*dst, v.data(), v.size() * sizeof(_Float16), hipMemcpyHostToDevice));
  return WCT_OK;
}

}  // namespace

namespace wct_host {

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

}  // namespace wct_host

extern "C" {

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
      if (int rc = upload_f16(ctx, &ld.l1w16, w16)) return rc;
      std::vector<float> b32(32, 0.f);
      for (int o = 0; o < ld.d.cout_pad && o < 32; ++o) b32[o] = bias[o];
      if (int rc = upload(ctx, &ld.l1bias, b32)) return rc;
      ld.d.l1w16 = ld.l1w16; ld.d.l1bias = ld.l1bias;
    }
    if (in3 && ld.d.cout_pad == 64 && L.cout == 64) {   // un-pruned encoders: four cout tiles for level1.hip in3_wide_kernel
      std::vector<_Float16> w16;
      ld.d.l1inv = pack_head_f16(wpk, ld.d.cout_pad, 4, w16);
      if (int rc = upload_f16(ctx, &ld.l1w16, w16)) return rc;
      if (int rc = upload(ctx, &ld.l1bias, bias)) return rc;
      ld.d.l1w16 = ld.l1w16; ld.d.l1bias = ld.l1bias;
    }
    if (in3 && ld.d.cout_pad == 16) {
      std::vector<_Float16> w16;
      ld.d.inv_scale = pack_head_f16(wpk, 16, 1, w16);
      if (int rc = upload_f16(ctx, &ld.wpk16, w16)) return rc;
      ld.d.wpk16 = ld.wpk16;
    }
    if (!in3) {
      std::vector<_Float16> w16;
      const int taps = ld.d.cout_pad == 16 ? 10 : 9;
      ld.d.inv_scale = pack_weights_f16(L.weight, L.cout, L.cin, ld.d.cout_pad, taps, w16);
      if (int rc = upload_f16(ctx, &ld.wpk16, w16)) return rc;
      ld.d.wpk16 = ld.wpk16;
      if ((ld.d.flags & CONV_UP_IN) && ld.d.cout_pad >= 32 && (L.cin % 16) == 0 && !out3 && !L.pool_after) {   // ... for the DMA kernel
        std::vector<_Float16> wup;
        ld.d.inv_scale_up = pack_up_sp_f16(L.weight, L.cout, L.cin, ld.d.cout_pad, wup);
        if (int rc = upload_f16(ctx, &ld.wup16, wup)) return rc;
        ld.d.wup16 = ld.wup16;
      }
      if ((ld.d.flags & CONV_UP_IN) && L.cin == 16 && L.cout == 16) {   // per-parity 2x2 form for the fused tail's first conv
        std::vector<_Float16> wup;
        ld.d.inv_scale_up = pack_up_phase_f16(L.weight, L.cout, L.cin, wup);
        if (int rc = upload_f16(ctx, &ld.wup16, wup)) return rc;
        ld.d.wup16 = ld.wup16;
      }
      if (out3 && ld.d.cout_pad == 16) {   // block-packed form for the fused tails
        std::vector<_Float16> wph;
        pack_out3_phase_f16(L.weight, L.cout, L.cin, wph);
        if (int rc = upload_f16(ctx, &ld.wph16, wph)) return rc;
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

}  // extern "C"
