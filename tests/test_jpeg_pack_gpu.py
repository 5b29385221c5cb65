"""The device JPEG encoder's entropy coder (wct_jpeg_pack) on the GPU, on coefficients that no image reaches through the DCT and the
quantiser (tests/jpeg_coef_cases.py; tests/test_jpeg_pack_cpu.py proves what they contain): every Huffman symbol of both tables, the
longest block the tables allow at every launcher edge, any int16 under the capping rule of include/wct_hip_jpeg.h, and FF bytes at the
edges of the stuffing kernels.  Every comparison is equality of bytes with the numpy oracle's entropy()."""
import bisect
import functools
import types

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_coef_cases as cc
from tests import jpeg_oracle as jo
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = cc.sizes()
WORST_SIZES = SIZES + [("full_span",) + cc.FF_DENSE]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "-m gpu tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    from wct_hip import WCT
    return WCT(types.SimpleNamespace(mode="16x", alpha=1.0))


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the cached coefficients are read-only


@functools.lru_cache(maxsize=None)
def expected(kind, H, W, seed=0, density=0.0):
    """(coefficients, the oracle's segment, is the cap needed) of a case, computed once."""
    coef = {"dense": lambda: cc.dense(H, W, seed, density), "worst": lambda: cc.worst(H, W), "wild": lambda: cc.wild(H, W, seed)}[kind]()
    coef.setflags(write=False)
    return coef, jo.entropy(coef, cap=kind == "wild"), kind == "wild"


def entropy_bound(eng, H, W):
    return eng.jpeg_bound(H, W) - _lib.JPEG_HEADER_BYTES


def pack(torch, eng, coef, H, W, capacity=None):
    """wct.jpeg_pack into `capacity` bytes (default: the bound less the header) with GUARD bytes of A5 behind them, which must stay:
    (the capacity's bytes on the host, the length slot)."""
    cap = entropy_bound(eng, H, W) if capacity is None else capacity
    buf = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    length = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    c = coef if isinstance(coef, torch.Tensor) else dev(torch, coef)
    eng.jpeg_pack(c, H, W, capacity=cap, out=buf, length=length)
    host = buf.cpu().numpy()
    assert (host[cap:] == 0xA5).all(), "the pack wrote behind a capacity of %d bytes" % cap
    return host[:cap], int(length.item())


def where(got, want, coef, cap):
    """The first differing byte and the block whose bits it holds."""
    n = min(len(got), len(want))
    at = next((i for i in range(n) if got[i] != want[i]), n)
    starts = []
    jo.bitstring(coef, cap, starts=starts)
    raw = at - want[:at].count(b"\xff\x00")                    # its index in the unstuffed stream (exact unless `at` is a stuffed 00)
    block = bisect.bisect_right(starts, raw * 8 + 7) - 1       # the last block that has a bit in that byte
    first = bisect.bisect_right(starts, raw * 8) - 1
    return "lengths %d / %d, first difference at byte %d (got %s, want %s): blocks %d .. %d of %d (component %s), block bit offsets %s" % (
        len(got), len(want), at, got[at:at + 4].hex(), want[at:at + 4].hex(), first, block, len(coef), "Y Y Y Y Cb Cr".split()[first % 6],
        starts[first:block + 2])


def check(torch, eng, kind, H, W, seed=0, density=0.0):
    coef, want, cap = expected(kind, H, W, seed, density)
    host, n = pack(torch, eng, coef, H, W)
    assert n >= 0, "%d bytes overflowed the bound's %d" % (len(want), len(host))
    got = host[:n].tobytes()
    assert got == want, where(got, want, coef, cap)
    return got


# ---- dense: every symbol of both tables ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density", cc.DENSITIES)
@pytest.mark.parametrize("size", SIZES + [("cover",) + cc.COVER[:2]], ids=lambda s: s[0])
def test_dense_equals_the_oracle(torch, eng, size, density):
    name, H, W = size
    check(torch, eng, "dense", H, W, cc.COVER[2] if name == "cover" else 1, density)


# ---- worst: the longest block at every edge, the exact capacity, the zeroing kernel's reach ---------------------------------------------

@pytest.mark.parametrize("size", WORST_SIZES, ids=lambda s: s[0])
def test_worst_equals_the_oracle_at_the_exact_capacity_and_over_poison(torch, eng, size):
    name, H, W = size
    coef, want, _ = expected("worst", H, W)
    m = len(want)
    assert m <= entropy_bound(eng, H, W)
    check(torch, eng, "worst", H, W)                       # capacity = wct_jpeg_bound - 623: nothing overflows
    c = dev(torch, coef)
    host, n = pack(torch, eng, c, H, W, capacity=m)
    assert n == m and host.tobytes() == want, "a capacity of exactly the length"
    host, n = pack(torch, eng, c, H, W, capacity=m - 1)
    assert n == -1, "one byte short: the length slot must be UINT64_MAX"
    assert host.tobytes() == want[:m - 1], "what fits below the capacity is the segment's start"
    try:
        for byte in (0xFF, 0x00):                          # the longest stream of the size: every word the pack ORs into was cleared
            eng.debug_set("poison", byte)
            host, n = pack(torch, eng, c, H, W)
            got = host[:max(n, 0)].tobytes()
            assert got == want, "scratch poisoned with 0x%02X: %s" % (byte, where(got, want, coef, False))
    finally:
        eng.debug_set("poison", -1)


# ---- wild: any int16 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: s[0])
def test_wild_equals_the_capped_oracle_and_harms_nothing(torch, eng, size):
    name, H, W = size
    got = check(torch, eng, "wild", H, W, 1)               # the guard behind `out` is checked in pack()
    assert len(got) <= entropy_bound(eng, H, W)
    # the context is none the worse: an image of the same size, then one of another
    for h, w, q, kind in ((H, W, 75, "noise"), jo.CASES[5]):
        a = jo.make_image(h, w, kind)
        assert eng.jpeg_encode(dev(torch, a), q) == jo.pillow_bytes(a, q)


# ---- FF bytes at the edges of the stuffing kernels -------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", cc.FF_EDGES, ids=lambda e: e[0])
def test_ff_at_the_stuffing_edges(torch, eng, edge):
    name, H, W, seed, density, places = edge
    got = check(torch, eng, "dense", H, W, seed, density)
    stream = jo.padded_stream(expected("dense", H, W, seed, density)[0])
    for i in places:
        o = i + stream[:i].count(b"\xff")
        assert got[o:o + 2] == b"\xff\x00", "%s: byte %d of the stream is FF and must be FF 00 at %d of the output, which has %s" % (name, i, o, got[o:o + 2].hex())


def test_ff_at_high_density(torch, eng):
    H, W = cc.FF_DENSE
    got = check(torch, eng, "worst", H, W)
    stream = jo.padded_stream(expected("worst", H, W)[0])
    assert len(stream) >= 2 * _lib.JPEG_STUFF_CHUNK and stream.count(b"\xff") > 0.05 * len(stream)
    assert len(got) == len(stream) + stream.count(b"\xff") + 2


# ---- the new image cases: encode is header + pack of blocks ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", jo.CASES[15:], ids=lambda c: "%dx%d-q%d-%s" % c)
def test_encode_is_the_composition_of_its_parts_on_the_new_cases(torch, eng, case):
    H, W, q, kind = case
    a = jo.make_image(H, W, kind)
    x = dev(torch, a)
    whole = eng.jpeg_encode(x, q)
    hdr, _, _ = eng.jpeg_header(H, W, q)
    buf, length = eng.jpeg_pack(eng.jpeg_blocks(x, q), H, W)
    n = int(length.item())
    parts = hdr + buf[:n].cpu().numpy().tobytes()
    assert whole == parts
    assert buf[:n].cpu().numpy().tobytes() == jo.entropy(jo.coefficients(a, q))
    assert whole == jo.pillow_bytes(a, q)


# ---- determinism -----------------------------------------------------------------------------------------------------------------------

def test_the_bytes_do_not_depend_on_the_call_or_on_where_the_coefficients_lie(torch, eng):
    H, W = 13, 679                                         # tile_above: 258 blocks
    coef, want, _ = expected("dense", H, W, 1, 0.3)
    first = check(torch, eng, "dense", H, W, 1, 0.3)
    assert check(torch, eng, "dense", H, W, 1, 0.3) == first
    for offset in (8, 24, 1000):                           # int16 elements: 16, 48 and 2000 bytes, all 16-byte aligned
        big = torch.full((offset + coef.size + 77,), 0x7FFF, dtype=torch.int16, device="cuda")
        view = big[offset:offset + coef.size].view(len(coef), 64)
        view.copy_(dev(torch, coef))
        assert view.data_ptr() % 16 == 0 and view.data_ptr() == big.data_ptr() + 2 * offset
        host, n = pack(torch, eng, view, H, W)
        got = host[:max(n, 0)].tobytes()
        assert got == want, "coefficients at element offset %d: %s" % (offset, where(got, want, coef, False))
