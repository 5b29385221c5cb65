/* libwct_hip -- a baseline JPEG decoder on the device, pixel-identical to Pillow's Image.open(path).convert("RGB") (libjpeg-turbo):
 * the part of the C ABI behind `--device_decode`.
 *
 * What crosses to the device is the file's entropy-coded segment; the pixels (uint8 H x W x 3) are made there.  Everything in
 * wct_hip.h holds here too: return codes, wct_last_error, device pointers, one context = one stream, asynchronous calls.  The device
 * entries run on the context's stream, never synchronise, read nothing back, take `info` from the host at call time as launch
 * arguments (no call depends on an earlier upload), and return WCT_ERR_INVALID -- wct_last_error names the entry -- before anything is
 * written when an argument is bad.  Their launch geometry is a function of (info, rounds) alone; they are legal inside a stream
 * capture, but a captured call decodes only files with the same tables and scan length.
 *
 * SUPPORTED (wct_jdec_parse): SOF0, 8 bit, one interleaved scan over all components (Ss 0, Se 63, Ah / Al 0) that is followed by EOI;
 * one component (grey), or three (YCbCr) with Y sampled 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and Cb, Cr 1x1; any Huffman tables
 * (`optimize`) with DC categories <= 11; 8-bit quantisation tables; DRI with any interval.  APPn and COM segments are skipped; EXIF
 * orientation is not applied (as in Image.open).  Everything else -- progressive, extended, arithmetic, 12 bit, 16-bit quantisation
 * tables, several scans, four components, any Adobe APP14 segment, three components with the ids 'R', 'G', 'B' and no JFIF
 * segment (libjpeg reads those as RGB), other sampling factors, a table that a component names but no
 * segment defines, a file that ends anywhere before its EOI -- is WCT_JDEC_UNSUPPORTED, and *info is then not written.
 *
 * Definition of the pixels.  All arithmetic is 32-bit integer, wrapping; >> is arithmetic.
 *
 * Geometry.  Three components: MCUs of 8 hs x 8 vs pixels (hs, vs: Y's factors), MW = ceil(W / (8 hs)), MH = ceil(H / (8 vs)); an
 * MCU holds hs vs Y blocks (row-major), then Cb, then Cr.  One component: one block per MCU, ceil(W / 8) x ceil(H / 8) of them,
 * whatever the file's sampling factors say (wct_jdec_parse reports them as 1 x 1).  MCUs row-major.  A chroma plane's TRUE size is
 * ceil(H / vs) x ceil(W / hs).
 *
 * Dequantisation.  coefficient x table entry.
 * IDCT.  libjpeg's jidctint (islow): CONST_BITS 13, PASS1_BITS 2, the twelve constants of wct_hip_jpeg.h (2446, 3196, 4433, 6270,
 * 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172); columns first, descaled by 11, then rows, descaled by 18;
 * DESCALE(x, n) = (x + (1 << (n - 1))) >> n; then + 128 and clamp to 0 .. 255.
 * 4:2:0 chroma (h2v2 fancy).  For output row y: cy = y >> 1, the neighbour row ny = cy - 1 for even y, cy + 1 for odd y; s[x] =
 * 3 c[cy][x] + c[ny][x].  For output column x: cx = x >> 1; even x: (3 s[cx] + s[cx - 1] + 8) >> 4; odd x: (3 s[cx] + s[cx + 1] + 7)
 * >> 4.  Neighbour rows and columns are clamped to the plane's TRUE size (not to the padded block plane), which is libjpeg's
 * (4 s[0] + 8) >> 4 and (4 s[last] + 7) >> 4 at the first and last column.
 * 4:2:2 chroma (h2v1 fancy).  even x: (3 c[cx] + c[cx - 1] + 1) >> 2; odd x: (3 c[cx] + c[cx + 1] + 2) >> 2; columns clamped alike.
 * Colour.  cb = Cb - 128, cr = Cr - 128: R = Y + ((91881 cr + 32768) >> 16); G = Y + ((-22554 cb - 46802 cr + 32768) >> 16);
 * B = Y + ((116130 cb + 32768) >> 16); each clamped to 0 .. 255.  Grey: R = G = B = Y.
 *
 * Entropy decoding (wct_jdec_coefficients).
 * 1. Unstuff.  Per WCT_JDEC_CHUNK bytes of the segment: a byte behind an FF is dropped (the 00 of FF 00, the n of RSTn), an FF in
 *    front of D0 .. D7 is dropped and counted as a marker; the prefix of the counts; the kept bytes compacted.  The bit position of
 *    the compacted stream at every marker is an ANCHOR (byte aligned); the end of the stream is the last anchor.  A file has
 *    ceil(MCUs / interval) - 1 markers; any other number is CORRUPT.
 * 2. The decoder.  A state is (p, b, z): bit position, block of the MCU, zig-zag position.  Bits at or beyond the next anchor read
 *    as 1.  At a step with the next anchor a > p:
 *      - p is itself an anchor: (b, z) becomes (0, 0) (a FLAW unless it was), and the next anchor is taken;
 *      - (b, z) = (0, 0), a - p < 8 and all bits of [p, a) are 1: p = a (the pad bits);
 *      - the next 16 bits match no code: p += 1 (FLAW);
 *      - the symbol (code and value bits) would end beyond a: (p, b, z) = (a, 0, 0), the block in progress is abandoned (FLAW);
 *      - z = 0: the DC difference.  Else run = symbol >> 4, size = symbol & 15.  size 0 and run 15: z += 16, the block ends when z >=
 *        64 (FLAW when z > 64).  size 0 otherwise: the block ends.  Else z += run; z > 63 ends the block (FLAW); otherwise the
 *        coefficient at z, and z += 1, the block ends at 64.  A value of n bits with a leading 0 is negative: bits - (1 << n) + 1.
 *    A block that ends is completed: b = (b + 1) mod blocks per MCU, z = 0.
 * 3. Synchronise.  The stream is cut into subsequences of S = WCT_JDEC_SUBSEQ_BITS bits; thread i owns [i S, (i + 1) S) and decodes
 *    from a state while p < (i + 1) S; the state it stops in is its exit state e_i.  WCT_JDEC_LAUNCHES launches; a workgroup holds
 *    WCT_JDEC_SYNC_THREADS consecutive subsequences.  Launch 0: every thread decodes from (i S, 0, 0) -- thread 0 of the stream
 *    thereby from the true start.  Then in every launch up to `rounds` Jacobi rounds over LDS with a barrier between them:
 *    e_i <- f_i(e_(i-1)), where the first thread of a workgroup takes its predecessor's state from global memory as the PREVIOUS
 *    launch left it (none in launch 0: it keeps its guess); a round that changes no exit state of the workgroup ends its launch.
 *    The exit states ping-pong between two arrays, so no launch reads what it writes.  The status is thereby a function of the file
 *    and `rounds` alone.
 * 4. Count, scan, write.  Each thread's completed blocks (from its last decode) are summed to block offsets; the write pass decodes
 *    every subsequence once more from e_(i-1) into the zeroed coefficients, every store bounded by the block count, and compares the
 *    state it started from, its exit state and its count with the stored ones: any difference is UNSYNC.  With no UNSYNC the
 *    coefficients are exact by induction from thread 0, whatever the synchronisation did.  A FLAW met in the write pass, a restart
 *    anchor not at a multiple of the interval's blocks, a stream not ending in state (end, 0, 0), or a block count other than the
 *    geometry's is CORRUPT.  The status is UNSYNC if anything was UNSYNC, else CORRUPT if anything was, else OK.
 * 5. DC.  Per component the prefix sums of the differences along the scan, restarting at every `interval` MCUs: integer sums, so no
 *    launch split can show.  Stored as int16.
 *
 * The synchronisation survey (tools/jdec_sync_survey.py, profiles/jdec_sync_survey.json; run on a CPU, the property is the file's):
 * the 3840 x 2160 content fixture and the 2048 x 2048 style fixture, as committed and re-encoded at quality 30 / 75 / 95 (1500 to
 * 23474 subsequences).  Every one of the eight ends OK from `rounds` = 3 on (the style fixture as committed from 2); run to the
 * fixpoint, no workgroup needs more than 12 rounds in launch 0 or 6 in launch 1, and launches 2 and 3 change nothing.
 * WCT_JDEC_ROUNDS = 32 and WCT_JDEC_LAUNCHES = 4 are over twice that.  Flat or noise images move one subsequence a round and can
 * end UNSYNC: their callers fall back to a host decoder.
 *
 * Context memory.  The compacted stream, the anchors, the states, counts and offsets, the DC partial sums, the component planes of
 * wct_jdec_pixels and the coefficients when wct_jdec_decode owns them belong to the context: allocated on first use of a size, ON TOP
 * of wct_workspace_bytes, not covered by wct_reserve; scratch in the sense of the "poison" hook.
 */
#ifndef WCT_HIP_JDEC_H
#define WCT_HIP_JDEC_H

#include "wct_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WCT_JDEC_UNSUPPORTED 1           /* wct_jdec_parse: not a file this decoder takes (no error: use another decoder) */
#define WCT_JDEC_STATUS_OK 0u
#define WCT_JDEC_STATUS_UNSYNC 1u        /* the synchronisation did not converge within `rounds`: the coefficients are not to be used */
#define WCT_JDEC_STATUS_CORRUPT 2u       /* the scan is not what its header promises */
#define WCT_JDEC_SUBSEQ_BITS 1024        /* S */
#define WCT_JDEC_SYNC_THREADS 256        /* subsequences per workgroup of the synchronisation */
#define WCT_JDEC_LAUNCHES 4              /* launches of the synchronisation */
#define WCT_JDEC_ROUNDS 32               /* Jacobi rounds per launch when `rounds` is 0 */
#define WCT_JDEC_MAX_ROUNDS 4096
#define WCT_JDEC_CHUNK 1024              /* segment bytes per count of the unstuffing */
#define WCT_JDEC_SCAN_CHUNK 256          /* values per step of the one-workgroup scans */
#define WCT_JDEC_DC_TILE 256             /* MCUs per partial sum of the DC differences */
#define WCT_JDEC_MAX_DIM 65500
#define WCT_JDEC_MAX_SCAN_BYTES 0x0FFFFFFFu   /* bit positions are 32 bit */

typedef struct wct_jdec_info {
  int32_t H, W, ncomp;                   /* ncomp: 1 or 3 */
  int32_t restart_interval;              /* MCUs; 0 = none */
  int32_t hs[3], vs[3];                  /* sampling factors per component (1 x 1 for a one-component file) */
  int32_t tq[3], td[3], ta[3];           /* per component: quantisation table 0 .. 3, DC and AC Huffman table 0 .. 1 */
  int32_t reserved;
  uint64_t scan_offset, scan_length;     /* the entropy-coded segment file[scan_offset .. scan_offset + scan_length): it ends at the first
                                            marker that is neither FF 00 nor RSTn */
  uint8_t qt[4][64];                     /* NATURAL (row-major) order; tables no component names are zero */
  uint8_t dc_counts[2][16], dc_vals[2][16];     /* codes per length 1 .. 16, symbols in code order */
  uint8_t ac_counts[2][16], ac_vals[2][256];
} wct_jdec_info;

/* Host only; takes no context and reads only file[0 .. n).  WCT_OK: *info describes the file.  WCT_JDEC_UNSUPPORTED: see SUPPORTED
 * above; *info is not written.  WCT_ERR_INVALID: NULL. */
int wct_jdec_parse(const uint8_t* file, size_t n, wct_jdec_info* info);
/* Host only.  *blocks = the blocks of the scan, MW MH (hs vs + 2) or ceil(W / 8) ceil(H / 8).  WCT_ERR_INVALID: NULL, or an info that
 * wct_jdec_parse cannot have filled. */
int wct_jdec_num_blocks(const wct_jdec_info* info, uint64_t* blocks);
/* coef (int16, 16-byte aligned, 64 per block in zig-zag order, blocks in scan order: the layout of wct_jpeg_blocks; DC absolute) =
 * the coefficients of the segment scan_dev[0 .. info->scan_length) (device, any alignment).  *status_dev (a DEVICE uint32, 4-byte
 * aligned) = WCT_JDEC_STATUS_*; unless it is OK the coefficients are unspecified (but every store stayed inside coef).  rounds: 0 =
 * WCT_JDEC_ROUNDS, else 1 .. WCT_JDEC_MAX_ROUNDS.  WCT_ERR_INVALID: NULL, misalignment, rounds out of range, an info that
 * wct_jdec_parse cannot have filled, a segment of more than WCT_JDEC_MAX_SCAN_BYTES. */
int wct_jdec_coefficients(wct_ctx* ctx, const uint8_t* scan_dev, const wct_jdec_info* info, int rounds, int16_t* coef_dev, uint32_t* status_dev);
/* hwc (uint8 H x W x 3, any alignment) = the pixels of the coefficients (layout as above). */
int wct_jdec_pixels(wct_ctx* ctx, const int16_t* coef_dev, const wct_jdec_info* info, uint8_t* hwc_dev);
/* wct_jdec_pixels of wct_jdec_coefficients, the coefficients in the context's scratch; bit-identical to that composition. */
int wct_jdec_decode(wct_ctx* ctx, const uint8_t* scan_dev, const wct_jdec_info* info, int rounds, uint8_t* hwc_dev, uint32_t* status_dev);

#ifdef __cplusplus
}
#endif
#endif /* WCT_HIP_JDEC_H */
