"""Python / numpy restatement of the device JPEG decoder's definition (include/wct_hip_jdec.h): the parser, the unstuffing with its
anchors, the decoder of one subsequence (sequential decoding is the same function run to the stream's end), the DC sums, the pixel
rules, and the synchronisation schedule launch by launch and round by round.  tests/test_jdec_cpu.py holds the pixels against Pillow
and the parser against wct_jdec_parse; tests/test_jdec_gpu.py holds the library against this file."""
import bisect

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# WCT_JDEC_* of the header, mirrored by wct_hip.lib (tests/test_jdec_cpu.py checks all three agree)
SUBSEQ_BITS, SYNC_THREADS, LAUNCHES, ROUNDS = 1024, 256, 4, 32
OK, UNSYNC, CORRUPT = 0, 1, 2


class Unsupported(Exception):
    pass


def _code_space_ok(counts):
    code = 0
    for l, c in enumerate(counts):
        code = (code + c) << 1
        if code > (2 << (l + 1)):
            return False
    return True


def parse(data):
    """The fields of wct_jdec_info as a dict, or Unsupported(reason)."""
    p, n = data, len(data)
    no = Unsupported
    f = dict(H=0, W=0, ncomp=0, restart_interval=0, hs=[0, 0, 0], vs=[0, 0, 0], tq=[0, 0, 0], td=[0, 0, 0], ta=[0, 0, 0],
             qt=np.zeros((4, 64), np.uint8), dc_counts=np.zeros((2, 16), np.uint8), dc_vals=np.zeros((2, 16), np.uint8),
             ac_counts=np.zeros((2, 16), np.uint8), ac_vals=np.zeros((2, 256), np.uint8))
    have_q, have_dc, have_ac, have_sof, have_jfif, comp_id = set(), set(), set(), False, False, [0, 0, 0]
    if n < 4 or p[0] != 0xFF or p[1] != 0xD8:
        raise no("no SOI")
    at = 2
    while True:
        if at + 4 > n or p[at] != 0xFF:
            raise no("truncated or no marker")
        m = p[at + 1]
        if m == 0xFF:
            at += 1
            continue
        ln = p[at + 2] << 8 | p[at + 3]
        if ln < 2 or at + 2 + ln > n:
            raise no("truncated segment")
        s, pl = p[at + 4:at + 2 + ln], ln - 2
        at += 2 + ln
        if m == 0xDB:
            i = 0
            while i < pl:
                pq, tq = s[i] >> 4, s[i] & 15
                if pq != 0 or tq > 3 or i + 65 > pl:
                    raise no("quantisation table")
                f["qt"][tq][ZIGZAG] = np.frombuffer(s[i + 1:i + 65], np.uint8)
                have_q.add(tq)
                i += 65
        elif m == 0xC4:
            i = 0
            while i < pl:
                if i + 17 > pl:
                    raise no("Huffman table")
                tc, th = s[i] >> 4, s[i] & 15
                counts = list(s[i + 1:i + 17])
                total = sum(counts)
                if tc > 1 or th > 1 or not _code_space_ok(counts) or total > (256 if tc else 16) or i + 17 + total > pl:
                    raise no("Huffman table")
                vals = list(s[i + 17:i + 17 + total])
                if not tc and any(v > 11 for v in vals):
                    raise no("DC category")
                cc, vv = (f["ac_counts"], f["ac_vals"]) if tc else (f["dc_counts"], f["dc_vals"])
                cc[th] = counts
                vv[th] = 0
                vv[th][:total] = vals
                (have_ac if tc else have_dc).discard(th)
                if total:
                    (have_ac if tc else have_dc).add(th)
                i += 17 + total
        elif m == 0xC0:
            if have_sof or pl < 6 or s[0] != 8:
                raise no("frame")
            f["H"], f["W"], f["ncomp"] = s[1] << 8 | s[2], s[3] << 8 | s[4], s[5]
            nc = f["ncomp"]
            if nc not in (1, 3) or pl != 6 + 3 * nc or not (1 <= f["H"] <= 65500 and 1 <= f["W"] <= 65500):
                raise no("frame")
            for c in range(nc):
                comp_id[c], f["hs"][c], f["vs"][c], f["tq"][c] = s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]
                if f["tq"][c] > 3 or f["hs"][c] < 1 or f["vs"][c] < 1:
                    raise no("component")
            if nc == 1:
                f["hs"][0] = f["vs"][0] = 1
            have_sof = True
        elif m == 0xDD:
            if pl != 2:
                raise no("DRI")
            f["restart_interval"] = s[0] << 8 | s[1]
        elif m == 0xDA:
            nc = f["ncomp"]
            if not have_sof or pl != 4 + 2 * nc or s[0] != nc:
                raise no("scan")
            for c in range(nc):
                if s[1 + 2 * c] != comp_id[c]:
                    raise no("scan order")
                f["td"][c], f["ta"][c] = s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if f["td"][c] > 1 or f["ta"][c] > 1 or f["td"][c] not in have_dc or f["ta"][c] not in have_ac or f["tq"][c] not in have_q:
                    raise no("missing table")
            if tuple(s[1 + 2 * nc:4 + 2 * nc]) != (0, 63, 0):
                raise no("spectral selection")
            break
        elif m == 0xEE:
            raise no("Adobe")
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            have_jfif = have_jfif or (m == 0xE0 and bytes(s[:5]) == b"JFIF\0")
        else:
            raise no("marker %02X" % m)
    i = at
    while True:
        if i + 1 >= n:
            raise no("truncated scan")
        if p[i] != 0xFF:
            i += 1
            continue
        m = p[i + 1]
        if m == 0 or 0xD0 <= m <= 0xD7:
            i += 2
            continue
        if m != 0xD9:
            raise no("more than one scan")
        break
    if f["ncomp"] == 3 and not have_jfif and comp_id == [82, 71, 66]:
        raise no("components named R, G, B without JFIF: libjpeg reads RGB")
    f["scan_offset"], f["scan_length"] = at, i - at
    nc = f["ncomp"]
    if nc == 3 and ((f["hs"][0], f["vs"][0]) not in ((1, 1), (2, 1), (2, 2)) or f["hs"][1:] != [1, 1] or f["vs"][1:] != [1, 1]):
        raise no("sampling")
    if any((f["qt"][f["tq"][c]] == 0).any() for c in range(nc)):
        raise no("zero quantiser")
    return f


def geometry(f):
    grey = f["ncomp"] == 1
    nY = 1 if grey else f["hs"][0] * f["vs"][0]
    g = dict(nY=nY, bpm=1 if grey else nY + 2, mcu_w=8 if grey else 8 * f["hs"][0], mcu_h=8 if grey else 8 * f["vs"][0])
    g["MW"], g["MH"] = -(-f["W"] // g["mcu_w"]), -(-f["H"] // g["mcu_h"])
    g["mcus"] = g["MW"] * g["MH"]
    g["blocks"] = g["mcus"] * g["bpm"]
    ri = f["restart_interval"]
    g["expected_markers"] = -(-g["mcus"] // ri) - 1 if ri else 0
    return g


def unstuff(scan, expected):
    """(compacted stream, anchors as bit positions with the stream's end last, whether the marker count is the expected one)."""
    out, anchors, markers, prev, n = bytearray(), [], 0, 0, len(scan)
    for i, x in enumerate(scan):
        nxt = scan[i + 1] if i + 1 < n else 0
        mk = x == 0xFF and 0xD0 <= nxt <= 0xD7
        if mk:
            if markers < expected:
                anchors.append(len(out) * 8)
            markers += 1
        if not (mk or prev == 0xFF):
            out.append(x)
        prev = x
    anchors = anchors[:min(markers, expected)] + [len(out) * 8]
    return bytes(out), anchors, markers == expected


class Decoder:
    """The decoder of the definition over one file's compacted stream."""

    def __init__(self, f, scan=None):
        self.f, self.g = f, geometry(f)
        self.stream, self.anchors, self.markers_ok = unstuff(scan, self.g["expected_markers"])
        self.total = self.anchors[-1]
        self.padded = self.stream + b"\xff" * 16
        self.lut = [self._lut(f["dc_counts"][t], f["dc_vals"][t]) for t in range(2)] + [self._lut(f["ac_counts"][t], f["ac_vals"][t]) for t in range(2)]
        g, nc = self.g, f["ncomp"]
        comp = [0 if b < g["nY"] else min(b - g["nY"] + 1, 2) for b in range(g["bpm"])]
        self.dct = [f["td"][0 if nc == 1 else c] for c in comp]
        self.act = [2 + f["ta"][0 if nc == 1 else c] for c in comp]
        self.cache = {}

    @staticmethod
    def _lut(counts, vals):
        """16-bit prefix -> length << 8 | symbol, 0 where no code matches."""
        lut = np.zeros(65536, np.int32)
        code, k = 0, 0
        for l in range(1, 17):
            for _ in range(int(counts[l - 1])):
                lut[code << (16 - l):(code + 1) << (16 - l)] = l << 8 | int(vals[k])
                code += 1
                k += 1
            code <<= 1
        return lut.tolist()

    def decode(self, state, stop, coef=None, blk0=0):
        """From `state` while p < stop: (exit state, completed blocks, flaw).  coef: an int array [blocks, 64] that takes the values."""
        p, b, z = state
        A, padded, bpm = self.anchors, self.padded, self.g["bpm"]
        nb, ri = self.g["blocks"], self.f["restart_interval"]
        cnt, flaw = 0, False
        k = bisect.bisect_left(A, p)
        while p < stop:
            a = A[k]
            if p >= a:
                if b or z:
                    flaw = True
                b = z = 0
                k = bisect.bisect_right(A, p)
                if coef is not None and blk0 + cnt != k * ri * bpm:
                    flaw = True
                continue
            avail = a - p
            q, sh = p >> 3, p & 7
            w = (int.from_bytes(padded[q:q + 8], "big") << sh) & 0xFFFFFFFFFFFFFFFF
            if not (b or z) and avail < 8 and (w >> (64 - avail)) == (1 << avail) - 1:
                p = a
                continue
            v = w >> 48
            if avail < 16:
                v |= 0xFFFF >> avail
            e = self.lut[self.dct[b] if z == 0 else self.act[b]][v]
            if not e:
                flaw = True
                p += 1
                continue
            ln, sym = e >> 8, e & 255
            size = sym & 15
            if ln + size > avail:
                flaw = True
                p, b, z = a, 0, 0
                continue
            val = 0
            if size:
                bits = (w >> (64 - ln - size)) & ((1 << size) - 1)
                val = bits if bits >> (size - 1) else bits - (1 << size) + 1
            p += ln + size
            done, at = False, -1
            if z == 0:
                at, z = 0, 1
            elif size == 0:
                if sym >> 4 == 15:
                    z += 16
                    if z >= 64:
                        flaw = flaw or z > 64
                        done = True
                else:
                    done = True
            else:
                z += sym >> 4
                if z > 63:
                    flaw = done = True
                else:
                    at = z
                    z += 1
                    done = z == 64
            if coef is not None and at >= 0 and blk0 + cnt < nb:
                coef[blk0 + cnt, at] = val
            if done:
                cnt += 1
                b = b + 1 if b + 1 < bpm else 0
                z = 0
        return (p, b, z), cnt, flaw

    def sub(self, i, state):
        """Thread i's decode of its subsequence from `state`, remembered: (exit state, count)."""
        key = (i, state)
        r = self.cache.get(key)
        if r is None:
            e, c, _ = self.decode(state, min((i + 1) * SUBSEQ_BITS, self.total))
            r = self.cache[key] = (e, c)
        return r

    @property
    def nsub(self):
        return -(-self.total // SUBSEQ_BITS)

    def coefficients(self):
        """Sequential decoding: (int16 [blocks, 64], zig-zag order, DC absolute; OK or CORRUPT)."""
        g, f = self.g, self.f
        coef = np.zeros((g["blocks"], 64), np.int64)
        (p, b, z), cnt, flaw = self.decode((0, 0, 0), self.total, coef)
        bad = flaw or b or z or cnt != g["blocks"] or not self.markers_ok
        d = coef[:, 0].reshape(g["mcus"], g["bpm"])
        ri = f["restart_interval"] or g["mcus"]
        seg = np.arange(g["mcus"]) // ri
        out = np.zeros_like(d)
        for s in np.unique(seg):
            rows = d[seg == s]
            y = np.cumsum(rows[:, :g["nY"]].reshape(-1)).reshape(-1, g["nY"])
            out[seg == s] = np.concatenate([y] + [np.cumsum(rows[:, g["nY"] + c])[:, None] for c in range(g["bpm"] - g["nY"])], 1)
        coef[:, 0] = out.reshape(-1)
        return coef.astype(np.int16), CORRUPT if bad else OK

    # ---- the synchronisation ------------------------------------------------------------------------------------------------------
    def schedule(self, rounds=ROUNDS, launches=LAUNCHES, threads=SYNC_THREADS):
        """The schedule of the header, restated: (whether the write pass would find every stored state in place, the most rounds any
        workgroup ran in each launch)."""
        n, S = self.nsub, SUBSEQ_BITS
        start = [(i * S, 0, 0) for i in range(n)]
        ins = list(start)
        e = [self.sub(i, start[i])[0] for i in range(n)]
        used = []
        for launch in range(launches):
            prev, most = list(e), 0
            for g0 in range(0, n, threads):
                g1 = min(g0 + threads, n)
                head = (0, 0, 0) if g0 == 0 else (prev[g0 - 1] if launch else None)
                for r in range(rounds):
                    sh, changed = e[g0:g1], False
                    for i in range(g0, g1):
                        pred = sh[i - g0 - 1] if i > g0 else head
                        if pred is not None and pred != ins[i]:
                            ins[i] = pred
                            ne = self.sub(i, pred)[0]
                            changed = changed or ne != e[i]
                            e[i] = ne
                    most = max(most, r + 1)
                    if not changed:
                        break
            used.append(most)
        synced = all(ins[i] == ((0, 0, 0) if i == 0 else e[i - 1]) for i in range(n))
        return synced, used

    def status(self, rounds=ROUNDS):
        if not self.schedule(rounds)[0]:
            return UNSYNC
        return self.coefficients()[1]

    def jacobi(self, limit=100000, sets=False):
        """Whole-stream Jacobi rounds to the fixpoint: the number of wrong exit states after each round (the first entry: after the
        initial guesses); sets=True: the wrong subsequences themselves, as a set per round."""
        n, S = self.nsub, SUBSEQ_BITS
        true, st = [], (0, 0, 0)
        for i in range(n):
            st = self.sub(i, st)[0]
            true.append(st)
        e = [self.sub(i, (i * S, 0, 0))[0] for i in range(n)]
        wrong = [{i for i in range(n) if e[i] != true[i]}]
        while wrong[-1] and len(wrong) <= limit:
            e = [self.sub(i, (0, 0, 0) if i == 0 else e[i - 1])[0] for i in range(n)]
            wrong.append({i for i in range(n) if e[i] != true[i]})
        return wrong if sets else [len(w) for w in wrong]


def decoder(data):
    f = parse(data)
    return Decoder(f, data[f["scan_offset"]:f["scan_offset"] + f["scan_length"]])


# ---- the pixels ---------------------------------------------------------------------------------------------------------------------

def _idct_pass(d, n):
    """jidctint along the LAST axis of an int32 array [..., 8], descaled by n; wrapping."""
    v = [d[..., i] for i in range(8)]
    r = np.int32(1 << (n - 1))
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (v[0] + v[4]) << 13, (v[0] - v[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    o = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([(x + r) >> n for x in o], -1)


def planes(coef, f):
    """The component planes (uint8, padded to whole MCUs) of [blocks, 64] coefficients."""
    g = geometry(f)
    nat = np.zeros((g["blocks"], 64), np.int32)
    nat[:, ZIGZAG] = coef.astype(np.int32)
    blocks = nat.reshape(g["MH"], g["MW"], g["bpm"], 8, 8)
    out = []
    for c in range(f["ncomp"]):
        q = f["qt"][f["tq"][c]].astype(np.int32).reshape(8, 8)
        if c == 0:
            hs, vs = g["mcu_w"] // 8, g["mcu_h"] // 8
            b = blocks[:, :, :g["nY"]].reshape(g["MH"], g["MW"], vs, hs, 8, 8)
        else:
            hs = vs = 1
            b = blocks[:, :, g["nY"] + c - 1].reshape(g["MH"], g["MW"], 1, 1, 8, 8)
        with np.errstate(over="ignore"):
            d = b * q
            d = _idct_pass(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)     # columns
            d = _idct_pass(d, 18)                                       # rows
        d = np.clip(d + 128, 0, 255)
        out.append(d.transpose(0, 2, 4, 1, 3, 5).reshape(g["MH"] * vs * 8, g["MW"] * hs * 8))
    return out


def pixels(coef, f):
    """uint8 H x W x 3 of the coefficients: the definition of wct_jdec_pixels."""
    H, W = f["H"], f["W"]
    pl = planes(coef, f)
    Y = pl[0][:H, :W].astype(np.int32)
    if f["ncomp"] == 1:
        return np.stack([Y, Y, Y], -1).astype(np.uint8)
    hs, vs = f["hs"][0], f["vs"][0]
    ch, cw = -(-H // vs), -(-W // hs)
    yy, xx = np.arange(H), np.arange(W)
    up = []
    for c in pl[1:]:
        c = c[:ch, :cw].astype(np.int32)
        if hs == 1:
            up.append(c)
            continue
        cx = xx >> 1
        nx = np.clip(np.where(xx & 1, cx + 1, cx - 1), 0, cw - 1)
        if vs == 1:
            up.append((3 * c[:, cx] + c[:, nx] + np.where(xx & 1, 2, 1)[None, :]) >> 2)
        else:
            cy = yy >> 1
            ny = np.clip(np.where(yy & 1, cy + 1, cy - 1), 0, ch - 1)
            s = 3 * c[cy] + c[ny]
            up.append((3 * s[:, cx] + s[:, nx] + np.where(xx & 1, 7, 8)[None, :]) >> 4)
    cb, cr = up[0] - 128, up[1] - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], -1), 0, 255).astype(np.uint8)


def decode(data):
    """(pixels, status) of a file's bytes by sequential decoding."""
    d = decoder(data)
    coef, status = d.coefficients()
    return pixels(coef, d.f), status


def pillow_pixels(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
