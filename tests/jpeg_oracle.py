"""numpy restatement of the device JPEG encoder's definition (include/wct_hip_jpeg.h): baseline, 8 bit, 4:2:0, standard Huffman
tables -- what Pillow's Image.fromarray(rgb).save(path, quality=q) writes.  The transform is vectorised over blocks; the entropy
coder walks them.  encode(rgb, quality) -> (coefficients int16 [blocks, 64] in zig-zag order, blocks in scan order; the file's bytes).
tests/test_jpeg_cpu.py holds the bytes against Pillow, tests/test_jpeg_gpu.py the library against both.  walk() is the coder on its own,
with wct_jpeg_pack's rule for coefficients outside baseline JPEG behind cap=True (tests/test_jpeg_pack_cpu.py, tests/test_jpeg_pack_gpu.py)."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# Annex K.1 / K.2, natural order
BASE_Y = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                   18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_C = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# Annex K.3: (code counts per length 1 .. 16, symbols in code order)
DC_Y = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_C = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_Y = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa])
AC_C = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa])


def _codes(table):
    """symbol -> (code, length): Annex C."""
    bits, vals = table
    out, code, vi = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[vi]] = (code, length)
            vi += 1
            code += 1
        code <<= 1
    return out


DC_CODES = (_codes(DC_Y), _codes(DC_C))
AC_CODES = (_codes(AC_Y), _codes(AC_C))


def quant_tables(quality):
    """(Y, chroma) scaled tables, natural order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_Y, BASE_C))


def header(H, W, quality):
    """SOI .. end of SOS: 623 bytes."""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)
    qy, qc = quant_tables(quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += seg(0xDB, [0] + [int(x) for x in qy[ZIGZAG]]) + seg(0xDB, [1] + [int(x) for x in qc[ZIGZAG]])
    out += seg(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, t in ((0x00, DC_Y), (0x10, AC_Y), (0x01, DC_C), (0x11, AC_C)):
        out += seg(0xC4, [tc] + t[0] + t[1])
    return out + seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


def _fdct_pass(d, first):
    """jfdctint along the LAST axis of an int64 array [..., 8]."""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    v = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = v[0] + v[7], v[0] - v[7], v[1] + v[6], v[1] - v[6]
    t2, t5, t3, t4 = v[2] + v[5], v[2] - v[5], v[3] + v[4], v[3] - v[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4], n = (t10 + t11) << 2, (t10 - t11) << 2, 11
    else:
        o[0], o[4], n = descale(t10 + t11, 2), descale(t10 - t11, 2), 15
    z1 = (t12 + t13) * 4433
    o[2], o[6] = descale(z1 + t13 * 6270, n), descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def coefficients(rgb, quality):
    """int16 [6 MH MW, 64]: quantised, zig-zag order, blocks in scan order (per MCU Y00 Y01 Y10 Y11 Cb Cr, MCUs row-major)."""
    H, W, _ = rgb.shape
    MH, MW = (H + 15) // 16, (W + 15) // 16
    pad = np.pad(rgb, ((0, H % 2), (0, MW * 16 - W), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = pad[..., 0], pad[..., 1], pad[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16

    def down(c):
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        return (s + np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)[None, :]) >> 2

    Y = np.pad(Y[:H], ((0, MH * 16 - H), (0, 0)), mode="edge")
    planes = [Y] + [np.pad(c, ((0, MH * 8 - c.shape[0]), (0, 0)), mode="edge") for c in (down(Cb), down(Cr))]   # the DOWNSAMPLED row repeats
    # [MH, MW, 6, 8, 8] in scan order
    yb = Y.reshape(MH, 2, 8, MW, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(MH, MW, 4, 8, 8)
    cb = [p.reshape(MH, 8, MW, 8).transpose(0, 2, 1, 3)[:, :, None] for p in planes[1:]]
    blocks = np.concatenate([yb] + cb, axis=2) - 128
    d = _fdct_pass(blocks, True)                                   # rows
    d = _fdct_pass(d.swapaxes(-1, -2), False).swapaxes(-1, -2)     # columns
    qy, qc = quant_tables(quality)
    t = np.stack([qy] * 4 + [qc] * 2).reshape(1, 1, 6, 8, 8)
    q = np.sign(d) * ((np.abs(d) + 4 * t) // (8 * t))
    q = q.reshape(MH, MW, 6, 64)
    # dummies: Y blocks outside the ceil(W / 8) x ceil(H / 8) real ones
    gy = np.arange(MH)[:, None, None] * 2 + np.array([0, 0, 1, 1])[None, None, :]
    gx = np.arange(MW)[None, :, None] * 2 + np.array([0, 1, 0, 1])[None, None, :]
    dummy = (gy >= (H + 7) // 8) | (gx >= (W + 7) // 8)
    for b in range(1, 4):
        q[:, :, b] = np.where(dummy[:, :, b, None], 0, q[:, :, b])
        q[:, :, b, 0] = np.where(dummy[:, :, b], q[:, :, b - 1, 0], q[:, :, b, 0])
    return q[..., ZIGZAG].reshape(MH * MW * 6, 64).astype(np.int16)


DC_MAX_CATEGORY, AC_MAX_CATEGORY = 11, 10      # all that baseline JPEG has codes for: |DC difference| <= 2047, |AC| <= 1023


def walk(coef, cap=False):
    """What the coder emits for [blocks, 64] coefficients, in order: (block, table, "dc" or "ac", symbol, value bits, their number).
    The pack is baseline JPEG on |DC difference| <= 2047 and |AC| <= 1023.  cap=False: anything else raises ValueError.  cap=True: what
    wct_jpeg_pack defines there (include/wct_hip_jpeg.h) -- the category is capped at 11 (DC) or 10 (AC) and the low n bits of v, or of
    v - 1 for a negative v, are written."""
    def sized(v, most, b, what):
        n = abs(v).bit_length()
        if n > most:
            if not cap:
                raise ValueError("block %d: %s %d needs category %d; baseline JPEG has codes up to %d (cap=True applies wct_jpeg_pack's "
                                 "rule for such input)" % (b, what, v, n, most))
            n = most
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    pred = [0, 0, 0]
    for b, zz in enumerate(np.asarray(coef).astype(np.int64).tolist()):
        k = b % 6
        comp, t = (0, 0) if k < 4 else (k - 3, 1)
        diff = zz[0] - pred[comp]
        pred[comp] = zz[0]
        n, bits = sized(diff, DC_MAX_CATEGORY, b, "DC difference")
        yield b, t, "dc", n, bits, n
        run = 0
        for v in zz[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                yield b, t, "ac", 0xF0, 0, 0
                run -= 16
            n, bits = sized(v, AC_MAX_CATEGORY, b, "AC coefficient")
            yield b, t, "ac", run << 4 | n, bits, n
            run = 0
        if run:
            yield b, t, "ac", 0x00, 0, 0


def bitstring(coef, cap=False, starts=None):
    """The Huffman-coded bits of [blocks, 64] coefficients as a string of 0 / 1, before padding.  cap: see walk().  starts: a list that
    receives the bit offset of every block."""
    parts, at, last = [], 0, -1
    for b, t, kind, symbol, bits, n in walk(coef, cap):
        if b != last and starts is not None:
            starts.append(at)
        last = b
        code, length = (DC_CODES if kind == "dc" else AC_CODES)[t][symbol]
        parts.append(format(code, "0%db" % length))
        if n:
            parts.append(format(bits, "0%db" % n))
        at += length + n
    return "".join(parts)


def padded_stream(coef, cap=False):
    """The bytes of the bits, padded with ones to a byte: what the stuffing reads."""
    bits = bitstring(coef, cap)
    bits += "1" * (-len(bits) % 8)
    return int(bits, 2).to_bytes(len(bits) // 8, "big") if bits else b""


def entropy(coef, cap=False):
    """The entropy-coded segment of [blocks, 64] coefficients: stuffed, padded with ones, followed by FF D9.  cap: see walk()."""
    return padded_stream(coef, cap).replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


def encode(rgb, quality=75):
    """(coefficients, the complete file) of a uint8 H x W x 3 array."""
    coef = coefficients(rgb, quality)
    return coef, header(rgb.shape[0], rgb.shape[1], quality) + entropy(coef)


# the 15 cases the definition was checked on: (H, W, quality, class)
CASES = [(1, 1, 75, "noise"), (8, 250, 75, "noise"), (23, 47, 30, "noise"), (18, 34, 75, "noise"), (16, 16, 75, "noise"), (41, 70, 90, "noise"),
         (9, 7, 50, "noise"), (24, 40, 95, "noise"), (33, 50, 1, "noise"), (64, 64, 100, "noise"),
         (130, 15, 85, "smooth"), (32, 48, 75, "smooth"), (37, 29, 75, "smooth"), (50, 33, 20, "smooth"), (17, 17, 75, "sat")]
# and three that carry the largest categories through the transform and Pillow (tests/test_jpeg_pack_cpu.py says what they reach)
CASES += [(40, 72, 100, "extremes"), (27, 90, 1, "extremes"), (35, 52, 100, "sat")]


def make_image(H, W, kind, seed=0):
    """uniform noise, smooth ramps with a sine, random 0 / 255, or "extremes": left of the 16-aligned column nearest W / 2 an 8 x 8 chequer
    of black and white (at quality 100 the Y DC alternates between -1024 and +1016), right of it a 16 x 16 chequer of (0, 0, 255) and
    (255, 255, 0) (Cb is 255 and 0 there, so the Cb DC makes the same step from MCU to MCU)."""
    rng = np.random.default_rng([seed, H, W])
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "sat":
        return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    if kind == "extremes":
        yy, xx = np.mgrid[0:H, 0:W]
        split = (W // 2 + 8) // 16 * 16
        grey = ((yy // 8 + xx // 8) % 2 * 255)[..., None].repeat(3, 2)
        odd = ((yy // 16 + xx // 16) % 2)[..., None]
        colour = np.where(odd, np.array([255, 255, 0]), np.array([0, 0, 255]))
        return np.where((xx < split)[..., None], grey, colour).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(yy * 5 + xx * 3) % 256, (xx * 7) % 256, (yy * 11 + 40 * np.sin(xx / 3.0)) % 256], -1).astype(np.uint8)


def pillow_bytes(rgb, quality=None):
    import io
    from PIL import Image
    buf = io.BytesIO()
    if quality is None:
        Image.fromarray(rgb).save(buf, format="JPEG")
    else:
        Image.fromarray(rgb).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()
