// The host parser of the device JPEG decoder (include/wct_hip_jdec.h): plain C++, no HIP, so that tests/jdec_parse_main.cpp can hold it
// under the host sanitizers.  It reads only file[0 .. n) and writes *info only when it accepts the file.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/wct_hip_jdec.h"

namespace wct_jdec __attribute__((visibility("hidden"))) {

// zig-zag position -> natural (row-major) index
constexpr uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Geometry {
  int nY, bpm, mcu_w, mcu_h, MW, MH;   // Y blocks and all blocks per MCU, the MCU's pixels, MCUs per row and column
  long mcus, blocks;
};

// what the device entries check before they trust an info: everything a kernel indexes by
inline bool info_ok(const wct_jdec_info& f) {
  if (f.H < 1 || f.H > WCT_JDEC_MAX_DIM || f.W < 1 || f.W > WCT_JDEC_MAX_DIM) return false;
  if (f.ncomp != 1 && f.ncomp != 3) return false;
  if (f.restart_interval < 0 || f.restart_interval > 65535) return false;
  for (int c = 0; c < f.ncomp; ++c) {
    if (f.tq[c] < 0 || f.tq[c] > 3 || f.td[c] < 0 || f.td[c] > 1 || f.ta[c] < 0 || f.ta[c] > 1) return false;
    for (int i = 0; i < 64; ++i)
      if (f.qt[f.tq[c]][i] == 0) return false;
  }
  if (f.ncomp == 1) {
    if (f.hs[0] != 1 || f.vs[0] != 1) return false;
  } else {
    if (f.hs[0] < 1 || f.hs[0] > 2 || f.vs[0] < 1 || f.vs[0] > 2 || (f.hs[0] == 1 && f.vs[0] == 2)) return false;
    for (int c = 1; c < 3; ++c)
      if (f.hs[c] != 1 || f.vs[c] != 1) return false;
  }
  for (int t = 0; t < 2; ++t) {   // a table may be absent (all counts zero) when no component names it; no table may be over-full
    int ndc = 0, nac = 0;
    unsigned cdc = 0, cac = 0;
    for (int l = 0; l < 16; ++l) {
      ndc += f.dc_counts[t][l];
      nac += f.ac_counts[t][l];
      cdc = (cdc + f.dc_counts[t][l]) << 1;
      cac = (cac + f.ac_counts[t][l]) << 1;
      if (cdc > (2u << (l + 1)) || cac > (2u << (l + 1))) return false;   // more codes of a length than the code space has
    }
    if (ndc > 16 || nac > 256) return false;
    for (int i = 0; i < ndc; ++i)
      if (f.dc_vals[t][i] > 11) return false;
  }
  for (int c = 0; c < f.ncomp; ++c) {
    int ndc = 0, nac = 0;
    for (int l = 0; l < 16; ++l) ndc += f.dc_counts[f.td[c]][l], nac += f.ac_counts[f.ta[c]][l];
    if (!ndc || !nac) return false;
  }
  return true;
}

inline Geometry geometry(const wct_jdec_info& f) {
  Geometry g{};
  g.nY = f.ncomp == 1 ? 1 : f.hs[0] * f.vs[0];
  g.bpm = f.ncomp == 1 ? 1 : g.nY + 2;
  g.mcu_w = 8 * (f.ncomp == 1 ? 1 : f.hs[0]);
  g.mcu_h = 8 * (f.ncomp == 1 ? 1 : f.vs[0]);
  g.MW = (f.W + g.mcu_w - 1) / g.mcu_w;
  g.MH = (f.H + g.mcu_h - 1) / g.mcu_h;
  g.mcus = (long)g.MW * g.MH;
  g.blocks = g.mcus * g.bpm;
  return g;
}

inline int parse(const uint8_t* p, size_t n, wct_jdec_info* out) {
  if (!p || !out) return WCT_ERR_INVALID;
  const int NO = WCT_JDEC_UNSUPPORTED;
  wct_jdec_info f;
  memset(&f, 0, sizeof f);
  bool have_q[4] = {false, false, false, false}, have_dc[2] = {false, false}, have_ac[2] = {false, false}, have_sof = false, have_jfif = false;
  int comp_id[3] = {0, 0, 0};
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return NO;
  size_t at = 2;
  for (;;) {
    if (at + 4 > n || p[at] != 0xFF) return NO;
    const int m = p[at + 1];
    if (m == 0xFF) { ++at; continue; }   // a fill byte
    const size_t len = (size_t)p[at + 2] << 8 | p[at + 3];
    if (len < 2 || at + 2 + len > n) return NO;
    const uint8_t* s = p + at + 4;
    const size_t pl = len - 2;
    at += 2 + len;
    if (m == 0xDB) {
      for (size_t i = 0; i < pl;) {
        const int pq = s[i] >> 4, tq = s[i] & 15;
        if (pq != 0 || tq > 3 || i + 65 > pl) return NO;
        for (int z = 0; z < 64; ++z) f.qt[tq][ZIGZAG[z]] = s[i + 1 + z];
        have_q[tq] = true;
        i += 65;
      }
    } else if (m == 0xC4) {
      for (size_t i = 0; i < pl;) {
        if (i + 17 > pl) return NO;
        const int tc = s[i] >> 4, th = s[i] & 15;
        if (tc > 1 || th > 1) return NO;
        size_t total = 0;
        unsigned code = 0;
        for (int l = 0; l < 16; ++l) {
          total += s[i + 1 + l];
          code = (code + s[i + 1 + l]) << 1;
          if (code > (2u << (l + 1))) return NO;
        }
        if (total > (tc ? 256u : 16u) || i + 17 + total > pl) return NO;
        uint8_t* counts = tc ? f.ac_counts[th] : f.dc_counts[th];
        uint8_t* vals = tc ? f.ac_vals[th] : f.dc_vals[th];
        memset(vals, 0, tc ? 256 : 16);
        memcpy(counts, s + i + 1, 16);
        for (size_t k = 0; k < total; ++k) {
          if (!tc && s[i + 17 + k] > 11) return NO;
          vals[k] = s[i + 17 + k];
        }
        (tc ? have_ac : have_dc)[th] = total > 0;
        i += 17 + total;
      }
    } else if (m == 0xC0) {
      if (have_sof || pl < 6 || s[0] != 8) return NO;
      f.H = s[1] << 8 | s[2];
      f.W = s[3] << 8 | s[4];
      f.ncomp = s[5];
      if ((f.ncomp != 1 && f.ncomp != 3) || pl != (size_t)(6 + 3 * f.ncomp) || f.H < 1 || f.W < 1 || f.H > WCT_JDEC_MAX_DIM || f.W > WCT_JDEC_MAX_DIM) return NO;
      for (int c = 0; c < f.ncomp; ++c) {
        comp_id[c] = s[6 + 3 * c];
        f.hs[c] = s[7 + 3 * c] >> 4;
        f.vs[c] = s[7 + 3 * c] & 15;
        f.tq[c] = s[8 + 3 * c];
        if (f.tq[c] > 3 || f.hs[c] < 1 || f.vs[c] < 1) return NO;
      }
      if (f.ncomp == 1) f.hs[0] = f.vs[0] = 1;
      have_sof = true;
    } else if (m == 0xDD) {
      if (pl != 2) return NO;
      f.restart_interval = s[0] << 8 | s[1];
    } else if (m == 0xDA) {
      if (!have_sof || pl != (size_t)(4 + 2 * f.ncomp) || s[0] != f.ncomp) return NO;
      for (int c = 0; c < f.ncomp; ++c) {
        if (s[1 + 2 * c] != comp_id[c]) return NO;
        f.td[c] = s[2 + 2 * c] >> 4;
        f.ta[c] = s[2 + 2 * c] & 15;
        if (f.td[c] > 1 || f.ta[c] > 1 || !have_dc[f.td[c]] || !have_ac[f.ta[c]] || !have_q[f.tq[c]]) return NO;
      }
      if (s[1 + 2 * f.ncomp] != 0 || s[2 + 2 * f.ncomp] != 63 || s[3 + 2 * f.ncomp] != 0) return NO;
      break;
    } else if (m == 0xEE) {
      return NO;                                        // Adobe APP14: its transform flag changes the colour model
    } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
      // APPn, COM: skipped; a JFIF APP0 settles the colour model (YCbCr)
      if (m == 0xE0 && pl >= 5 && !memcmp(s, "JFIF", 5)) have_jfif = true;
    } else {
      return NO;                                        // SOF1 .. SOF15, DAC, DNL, EOI before a scan, anything unknown
    }
  }
  // the segment: to the first marker that is neither FF 00 nor RSTn; that marker has to be EOI
  size_t i = at;
  for (;; ++i) {
    if (i + 1 >= n) return NO;
    if (p[i] != 0xFF) continue;
    const int m = p[i + 1];
    if (m == 0x00 || (m >= 0xD0 && m <= 0xD7)) { ++i; continue; }
    if (m != 0xD9) return NO;
    break;
  }
  // libjpeg takes three components named 'R', 'G', 'B' as RGB, without a colour conversion, unless a JFIF segment says otherwise
  if (f.ncomp == 3 && !have_jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return NO;
  f.scan_offset = at;
  f.scan_length = i - at;
  if (!info_ok(f)) return NO;
  *out = f;
  return WCT_OK;
}

}  // namespace wct_jdec
