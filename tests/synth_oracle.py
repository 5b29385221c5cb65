"""CPU restatements for texture synthesis -- TEST INFRASTRUCTURE ONLY (the product never imports this).

  philox4x32_10 / noise   the noise image of wct_noise_uniform exactly as include/wct_hip.h defines it: Philox4x32-10 (Salmon et al.,
                          SC'11 / Random123) keyed by the seed, counter = (block index, stream id), value = (word >> 8) * 2^-24
  synthesis_shape         the texture size rule of PytorchWCT/data_loader.py:64-72, written as the reference writes it
  resize_bicubic_u8       Pillow's Image.resize((ow, oh), Image.BICUBIC) -- what Image.resize((w, h)) without a filter is at the
                          reference's Pillow pin (data_loader.py:72) -- built on oracle.resize_oracle: its tables with bicubic_filter
                          (a = -0.5, support 2.0) in place of the triangle, the same rounding, accumulator and pass order
"""
import math

import numpy as np

from oracle import resize_oracle as R

M0, M1 = 0xD2511F53, 0xCD9E8D57          # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl increments of the key
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) of one shape, key: two uint32 scalars -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in ctr]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(MASK),
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(MASK)]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [v.astype(np.uint32) for v in c]


def noise(seed: int, H: int, W: int, stream_id: int = 0) -> np.ndarray:
    """The planar 3 x H x W fp32 image of wct_noise_uniform(seed, stream_id, H, W)."""
    total = 3 * H * W
    i = np.arange((total + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((i & np.uint64(MASK), i >> np.uint64(32), np.full(i.shape, stream_id, np.uint64), np.zeros(i.shape, np.uint64)),
                          (seed & MASK, (seed >> 32) & MASK))
    flat = np.stack(words, axis=1).reshape(-1)[:total]              # element e = word e & 3 of block e >> 2
    return ((flat >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(3, H, W)


def synthesis_shape(H: int, W: int, size: int):
    """data_loader.py:64-72, literally (w, h = textureImg.size).  Returns (newh, neww)."""
    if not size:
        return H, W
    w, h = W, H
    if w > h:
        neww = size
        newh = int(h * neww / w)
    else:
        newh = size
        neww = int(w * newh / h)
    return newh, neww


def _bicubic(x: float) -> float:
    """Pillow's bicubic_filter (libImaging/Resample.c), a = -0.5."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def axis_tables(in_size: int, out_size: int):
    """oracle.resize_oracle.axis_tables with the bicubic filter and its support of 2.0; everything else as there."""
    scale = float(np.float32(in_size) - np.float32(0.0)) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int64)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            p = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + p * (1 << R.PRECISION_BITS)) if p < 0 else int(0.5 + p * (1 << R.PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return ksize, bounds, kk


def _pass(img: np.ndarray, out_size: int, axis: int) -> np.ndarray:
    _, bounds, kk = axis_tables(img.shape[axis], out_size)
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for i in range(out_size):
        lo, n = int(bounds[i, 0]), int(bounds[i, 1])
        acc = (1 << (R.PRECISION_BITS - 1)) + np.tensordot(kk[i, :n].astype(np.int64), src[lo:lo + n], axes=(0, 0))
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)      # the C accumulator is a 32-bit int (never wraps: sum |w| * 255 < 2^31)
        out[i] = R._clip8(acc)
    return np.moveaxis(out, 0, axis)


def resize_bicubic_u8(img: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """Image.resize((ow, oh), Image.BICUBIC) of a uint8 H x W x 3 image: horizontal pass first, uint8 in between."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w = img.shape[:2]
    out = img
    if ow != w:
        out = _pass(out, ow, 1)
    if oh != h:
        out = _pass(out, oh, 0)
    return np.ascontiguousarray(out)
