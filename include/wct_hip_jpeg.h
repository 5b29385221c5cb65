/* libwct_hip -- a baseline JPEG encoder on the device, byte-identical to the file Pillow (libjpeg-turbo) writes for the same pixels:
 * the part of the C ABI behind `--device_jpeg`.
 *
 * The image to save is on the device as uint8 H x W x 3 (wct_planar_to_u8 and the fused conversions).  These entries turn it into the
 * file image there, so that what crosses to the host is the compressed file and no CPU thread spends its time in an encoder.
 * Everything in wct_hip.h holds here too: return codes, wct_last_error, device pointers, one context = one stream, asynchronous calls.
 * The device entries run on the context's stream, never synchronise, read nothing back, and return WCT_ERR_INVALID -- wct_last_error
 * names the entry -- before anything is written when an argument is bad.  Their launch geometry is a function of (H, W, capacity)
 * alone, so a call can be captured into a HIP graph and replayed on other pixels.
 *
 * SUPPORTED: exactly what Pillow's Image.fromarray(rgb).save(path) / save(path, quality=q) produces -- baseline sequential DCT, 8 bit,
 * three components, 4:2:0 (Y 2x2, Cb and Cr 1x1), the standard Huffman tables of Annex K.3, one scan, the JFIF APP0 segment.  NOT
 * supported: restart markers, optimize, progressive, 4:4:4 / 4:2:2, grey or CMYK images, metadata (EXIF, ICC, comments), a dpi.
 * Decoding stays on the host.
 *
 * Definition.  All arithmetic is 32-bit integer; >> is arithmetic.
 *
 * Geometry.  MH = ceil(H / 16), MW = ceil(W / 16) MCUs of 16 x 16 pixels.  Pixel columns >= W take column W - 1.  If H is odd, pixel
 * row H takes row H - 1.
 *
 * Colour, per pixel.   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *                      Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *                      Cr = ( 32768 R - 27439 G -  5329 B + 8388608 + 32767) >> 16
 *
 * Chroma.  c[y][x] = (C[2y][2x] + C[2y][2x+1] + C[2y+1][2x] + C[2y+1][2x+1] + bias) >> 2 for y < ceil(H / 2); bias = 1 for even x, 2
 * for odd x.  Chroma rows >= ceil(H / 2) take THE DOWNSAMPLED ROW ceil(H / 2) - 1 (not the downsampling of replicated pixel rows: the
 * two differ for even H).  Y rows >= H take row H - 1.
 *
 * Blocks.  Every chroma block of an MCU is real.  Y has ceil(W / 8) x ceil(H / 8) real blocks; a Y block of an MCU outside that range
 * is a DUMMY: 63 zero AC coefficients and a DC equal to the QUANTISED DC of the preceding Y block of the same MCU (order 00, 01, 10,
 * 11; the preceding block may itself be a dummy).  Dummies take part in DC prediction like any block.
 *
 * DCT.  Samples - 128, then libjpeg's jfdctint (CONST_BITS 13, PASS1_BITS 2; constants 2446, 3196, 4433, 6270, 7373, 9633, 12299,
 * 15137, 16069, 16819, 20995, 25172): rows first, outputs 0 and 4 shifted left by 2 and the others descaled by 11; then columns,
 * descaled by 2 and by 15.  DESCALE(x, n) = (x + (1 << (n - 1))) >> n.  The result is 8 x the DCT.
 *
 * Quantisation.  Base tables: Annex K.1 (Y) and K.2 (Cb, Cr).  scale = 5000 / q (integer) for q < 50, else 200 - 2 q;
 * t = clamp((base scale + 50) / 100, 1, 255); coefficient = sign(v) ((|v| + 4 t) / (8 t)).
 *
 * Entropy coding.  Annex F baseline with the Annex K.3 tables: the DC category is the bit length of |diff|, negative values are
 * written as v - 1 in n bits, ZRL for runs above 15, EOB when the last coefficient is zero, one predictor per component over the whole
 * scan.  Blocks in scan order: per MCU Y00 Y01 Y10 Y11 Cb Cr, MCUs row-major.
 *
 * Domain of the coder.  The segment is baseline JPEG when |DC difference| <= 2047 and |AC| <= 1023 in every block: the categories the
 * tables have codes for, and all that wct_jpeg_blocks produces.  wct_jpeg_pack takes any int16 from its caller.  Outside the domain the
 * category n is capped at 11 (DC) or 10 (AC), the symbol is formed with the capped n, and the low n bits of v (of v - 1 for a negative
 * v) are written behind its code; v is the 32-bit DC difference or the AC coefficient.  Such a segment is not a valid file -- a decoder
 * reads other values from it -- but it is deterministic, a function of the coefficients alone, and the call is memory safe: a block has
 * at most WCT_JPEG_BLOCK_MAX_BITS bits whatever its coefficients, so the segment stays within wct_jpeg_bound.
 *
 * Tail.  The bits are padded with 1-bits to a byte; 00 follows every FF byte, the padded last byte included; FF D9 ends the file.
 *
 * Header (WCT_JPEG_HEADER_BYTES = 623).  SOI; APP0 "JFIF\0", version 1.01, units 0, density 1 x 1, no thumbnail; DQT 0, DQT 1, each in
 * zig-zag order; SOF0: 8 bit, H, W, components 1:22:0 2:11:1 3:11:1; DHT 00, 10, 01, 11 as four segments; SOS 1:00 2:11 3:11, Ss 0,
 * Se 63, AhAl 0.
 *
 * Determinism.  The bytes are a function of (pixels, H, W, quality) alone: never of CU count, launch split, capacity (when it
 * suffices), alignment or call history.  Every sum that crosses threads is an integer sum and every shared word is combined by
 * integer OR, so no order can show.
 *
 * Launches.  wct_jpeg_blocks: one, a workgroup per WCT_JPEG_SEG_MCUS MCUs of an MCU row, staged through LDS.  wct_jpeg_pack: the
 * blocks' bit counts with their prefix inside tiles of WCT_JPEG_SCAN_TILE blocks; the tiles' prefix, WCT_JPEG_SCAN_CHUNK tiles per step
 * of one workgroup; the bits of WCT_JPEG_PACK_SPAN blocks per workgroup assembled in LDS and stored, only the first and the last word
 * of a span combined by atomic OR into the zeroed stream; the FF bytes counted per WCT_JPEG_STUFF_CHUNK bytes, their prefix, and the
 * scatter that inserts the 00 bytes, appends FF D9 and writes the length.
 *
 * Context memory.  The coefficients when wct_jpeg_encode owns them, the blocks' bit offsets, the scan partials and the unstuffed
 * stream belong to the context: allocated on first use of a size, ON TOP of wct_workspace_bytes, not covered by wct_reserve, like the
 * buffers of proxy mode; scratch in the sense of the "poison" hook.
 */
#ifndef WCT_HIP_JPEG_H
#define WCT_HIP_JPEG_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_JPEG_HEADER_BYTES 623
#define WCT_JPEG_MAX_DIM 65500
#define WCT_JPEG_BLOCK_MAX_BITS 1728   /* 64 coefficients x (a 16-bit code + 11 value bits) */
#define WCT_JPEG_SEG_MCUS 8            /* MCUs of one MCU row per workgroup of the blocks kernel */
#define WCT_JPEG_SCAN_TILE 256         /* blocks per partial sum of the bit counts */
#define WCT_JPEG_SCAN_CHUNK 256        /* partial sums per step of the one-workgroup scans */
#define WCT_JPEG_PACK_SPAN 64          /* blocks whose bits one workgroup assembles in LDS */
#define WCT_JPEG_STUFF_CHUNK 1024      /* bytes of the padded stream per FF count */
#define WCT_JPEG_OVERFLOW 0xFFFFFFFFFFFFFFFFull   /* the length slot of a call whose capacity did not suffice */

/* Host only.  header: WCT_JPEG_HEADER_BYTES bytes, SOI to the end of SOS.  qt_y, qt_c (either may be NULL): the two scaled tables, 64
 * entries each in NATURAL (row-major) order.  WCT_ERR_INVALID (no context: no message): a NULL header, H or W outside 1 ..
 * WCT_JPEG_MAX_DIM, quality outside 1 .. 100. */
int wct_jpeg_header(int H, int W, int quality, uint8_t* header, uint16_t* qt_y, uint16_t* qt_c);
/* Host only.  *bytes = a capacity no H x W image can overflow, header and FF D9 included: every coefficient of the 6 ceil(H / 16)
 * ceil(W / 16) blocks at the longest code (WCT_JPEG_BLOCK_MAX_BITS per block), every byte of that stuffed.  WCT_ERR_INVALID: NULL, or
 * H or W outside 1 .. WCT_JPEG_MAX_DIM. */
int wct_jpeg_bound(int H, int W, uint64_t* bytes);
/* coef (int16, 16-byte aligned, 6 MH MW blocks of 64 in zig-zag order, blocks in scan order) = the quantised coefficients of the image
 * (uint8 H x W x 3, any alignment).  WCT_ERR_INVALID: NULL, H, W or quality out of range, a misaligned coef. */
int wct_jpeg_blocks(wct_ctx* ctx, const uint8_t* hwc, int H, int W, int quality, int16_t* coef);
/* out[0 .. *len) = the entropy-coded segment of the coefficients: stuffed, padded, followed by FF D9; *len (a DEVICE uint64) its
 * length.  When capacity does not suffice nothing at or beyond out + capacity is written and *len = WCT_JPEG_OVERFLOW: the length
 * slot is the status, the host sees it with the length.  coef may hold any int16: baseline JPEG for |DC difference| <= 2047 and
 * |AC| <= 1023, the capped categories of "Domain of the coder" above otherwise -- never more than WCT_JPEG_BLOCK_MAX_BITS a block, so
 * wct_jpeg_bound(H, W) - WCT_JPEG_HEADER_BYTES suffices as a capacity for every input.  WCT_ERR_INVALID: NULL, H or W out of range, a
 * misaligned coef or len. */
int wct_jpeg_pack(wct_ctx* ctx, const int16_t* coef, int H, int W, uint8_t* out, uint64_t capacity, uint64_t* len);
/* The complete file image: wct_jpeg_header, then wct_jpeg_pack of wct_jpeg_blocks (the coefficients in the context's scratch);
 * bit-identical to that composition.  *len counts the header.  Overflow and refusals as above. */
int wct_jpeg_encode(wct_ctx* ctx, const uint8_t* hwc, int H, int W, int quality, uint8_t* out, uint64_t capacity, uint64_t* len);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_JPEG_H */
