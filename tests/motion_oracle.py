"""numpy reference of motion compensation (include/wct_hip_motion.h): the uint8 luma pyramid, the block search -- integer arithmetic, so the
device's field is this one bit for bit -- the gather of the compensated blend, and the rule that says which blocks of a pure translation
must come out exact."""
import numpy as np

from tests import video_oracle as V

BLOCK, MAX_LEVELS, MAX_RANGE = 8, 4, 7
F = np.float32


def luma(img, Ho=None, Wo=None):
    """uint8 luma of the top-left Ho x Wo: (0.299 r + 0.587 g) + 0.114 b, every operation rounded to fp32 on its own (numpy does), then
    * 255, + 0.5, clamp to [0, 255] with NaN -> 0, truncation."""
    img = np.asarray(img, np.float32)
    Ho, Wo = img.shape[1] if Ho is None else Ho, img.shape[2] if Wo is None else Wo
    r, g, b = (img[c, :Ho, :Wo] for c in range(3))
    with np.errstate(all="ignore"):
        t = (F(0.299) * r + F(0.587) * g) + F(0.114) * b
        x = t * F(255.0) + F(0.5)
        x = np.where(np.isnan(x), F(0.0), np.minimum(np.maximum(x, F(0.0)), F(255.0)))
    assert x.dtype == np.float32
    return x.astype(np.uint8)


def down(a):
    """(a + b + c + d + 2) >> 2 over 2 x 2 cells; an odd last row / column is dropped."""
    a = a[:a.shape[0] // 2 * 2, :a.shape[1] // 2 * 2].astype(np.uint16)
    return ((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(img, levels, Ho=None, Wo=None):
    p = [luma(img, Ho, Wo)]
    assert 1 <= levels <= MAX_LEVELS and min(p[0].shape) >= 1 << (levels - 1)
    for _ in range(levels - 1):
        p.append(down(p[-1]))
    return p


def grid(H, W):
    return (H + BLOCK - 1) // BLOCK, (W + BLOCK - 1) // BLOCK


def search_level(cur, prev, candidates, penalty):
    """One level: per block the admissible candidate with the smallest (cost, index), as the 32-bit key cost << 8 | index."""
    H, W = cur.shape
    nby, nbx = grid(H, W)
    c, p = cur.astype(np.int32), prev.astype(np.int32)
    mv = np.zeros((nby, nbx, 2), np.int16)
    for by in range(nby):
        for bx in range(nbx):
            y0, x0 = BLOCK * by, BLOCK * bx
            bh, bw = min(BLOCK, H - y0), min(BLOCK, W - x0)
            blk = c[y0:y0 + bh, x0:x0 + bw]
            best = None
            for idx, (vy, vx) in enumerate(candidates(by, bx)):
                if y0 + vy < 0 or y0 + bh + vy > H or x0 + vx < 0 or x0 + bw + vx > W:
                    continue                                            # not admissible: the displaced block leaves the image
                cost = int(np.abs(blk - p[y0 + vy:y0 + vy + bh, x0 + vx:x0 + vx + bw]).sum()) + penalty * (abs(vy) + abs(vx))
                assert cost < 1 << 16 and idx < 1 << 8
                key = cost << 8 | idx
                if best is None or key < best[0]:
                    best = (key, vy, vx)
            mv[by, bx] = best[1:]                                       # candidate 0, the zero vector, is always admissible
    return mv


def estimate_pyramids(pc, pp, rng, penalty):
    """The fields of every level, level 0 first, from two pyramids."""
    assert len(pc) == len(pp) and 0 <= rng <= MAX_RANGE and 0 <= penalty <= 255
    square = lambda r: [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
    fields = [None] * len(pc)
    for k in range(len(pc) - 1, -1, -1):
        if k == len(pc) - 1:
            cands = lambda by, bx: [(0, 0)] + square(rng)
        else:
            parent = fields[k + 1]

            def cands(by, bx, parent=parent):
                vy, vx = (int(v) for v in parent[min(by >> 1, parent.shape[0] - 1), min(bx >> 1, parent.shape[1] - 1)])
                return [(0, 0)] + [(2 * vy + dy, 2 * vx + dx) for dy, dx in square(1)]
        fields[k] = search_level(pc[k], pp[k], cands, penalty)
    return fields


def estimate(cur, prev, levels, rng, penalty):
    """wct_motion_estimate: int16 [nby, nbx, 2] between the top-left of cur (3 x Hc x Wc) and prev (3 x Ho x Wo)."""
    Ho, Wo = prev.shape[1:]
    return estimate_pyramids(pyramid(cur, levels, Ho, Wo), pyramid(prev, levels), rng, penalty)[0]


def gather(q, mv):
    """q'(ch, y, x) = q(ch, clamp(y + vy), clamp(x + vx)) with the vector of block (y >> 3, x >> 3)."""
    _, Ho, Wo = q.shape
    y, x = np.arange(Ho)[:, None], np.arange(Wo)[None, :]
    v = np.asarray(mv, np.int64)[y >> 3, x >> 3]
    return q[:, np.clip(y + v[..., 0], 0, Ho - 1), np.clip(x + v[..., 1], 0, Wo - 1)]


def weights(cur, prev, blend_w, sigma, radius, mv=None):
    """The blend's per-pixel weight w = blend exp(-d / 2 sigma^2) (video_oracle.blend), against prev displaced by mv when given."""
    q = np.asarray(prev, np.float64) if mv is None else gather(np.asarray(prev, np.float64), mv)
    _, Ho, Wo = q.shape
    e = ((np.asarray(cur, np.float64)[:, :Ho, :Wo] - q) ** 2).sum(0)
    sg = float(np.float32(sigma))
    return float(np.float32(blend_w)) * np.exp(-V.window_mean(e, radius) / (2.0 * sg * sg))


def translated_pair(H, W, shift, seed=7):
    """(cur, prev), H x W windows of one larger video_oracle.image with cur(y, x) = prev(y + sy, x + sx)."""
    sy, sx = shift
    m = max(abs(sy), abs(sx))
    big = V.image((H + 2 * m, W + 2 * m), seed)
    prev = big[:, m:m + H, m:m + W]
    cur = big[:, m + sy:m + sy + H, m + sx:m + sx + W]
    return np.ascontiguousarray(cur), np.ascontiguousarray(prev)


def claimed_blocks(H, W, shift, levels):
    """The rule of a pure translation: a level-0 block is claimed -- its vector must be exactly the shift -- when its top-level ancestor,
    in level-0 pixels and widened by a margin of 2^(levels - 1) on every side, lies inside the frame both where it is and displaced by
    the shift.  Border blocks are not claimed: there the search window leaves the image, a 2 x 2 cell of a coarser level straddles
    the frame's edge, and the estimator may settle for a neighbour.  -> bool [nby, nbx]"""
    sy, sx = shift
    L = levels - 1
    dims = [(H >> k, W >> k) for k in range(levels)]
    nby, nbx = grid(H, W)
    out = np.zeros((nby, nbx), bool)
    for by in range(nby):
        for bx in range(nbx):
            ay, ax = by, bx
            for k in range(1, levels):
                gy, gx = grid(*dims[k])
                ay, ax = min(ay >> 1, gy - 1), min(ax >> 1, gx - 1)
            Ht, Wt = dims[L]
            y0, y1 = BLOCK * ay << L, min(BLOCK * (ay + 1), Ht) << L
            x0, x1 = BLOCK * ax << L, min(BLOCK * (ax + 1), Wt) << L
            m = 1 << L
            out[by, bx] = all(y0 + dy - m >= 0 and y1 + dy + m <= H and x0 + dx - m >= 0 and x1 + dx + m <= W for dy, dx in ((0, 0), (sy, sx)))
    return out


def assert_translation(mv, H, W, shift, levels):
    """Every claimed block of the field holds exactly the shift; returns how many were claimed."""
    claimed = claimed_blocks(H, W, shift, levels)
    got = np.asarray(mv)[claimed]
    assert claimed.any() and np.array_equal(got, np.broadcast_to(np.asarray(shift, np.int16), got.shape)), (shift, got[np.any(got != shift, axis=1)][:8])
    return int(claimed.sum())
