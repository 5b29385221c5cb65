"""Coefficients handed straight to the device JPEG encoder's entropy coder (wct_jpeg_pack): what no image reaches through the DCT and the
quantiser -- every Huffman symbol of both tables, the longest block, any int16 at all, and FF bytes at the stuffing kernels' edges.  Pure
numpy, seeded like jpeg_oracle.make_image; shapes are int16 [6 MH MW, 64].  tests/test_jpeg_pack_cpu.py proves each claim made here from
the oracle alone; tests/test_jpeg_pack_gpu.py holds the library against the oracle on them."""
import numpy as np

from tests import jpeg_cases as jc
from tests import jpeg_oracle as jo

DENSITIES = (0.06, 0.3, 1.0)
# (H, W, seed) at which dense() over DENSITIES uses all 162 AC symbols and all 12 DC categories of both tables: 3 x 27 MCUs = 486
# blocks.  Found by walking W up one MCU at a time at H = 41 for seeds 1, 2 and 3: the smallest count at which the claim held (seed 1
# needs 612 blocks, seed 3 522; below 486 each seed misses between 1 and 7 symbols, most of them of the chroma table).
COVER = (41, 425, 2)
# the DC values planted at the start of every component: differences 0, -1, +2, -4, .. +512, -1024, one of every category 0 .. 11
DC_PLANT = np.cumsum([0] + [(-1) ** k * 2 ** (k - 1) for k in range(1, 12)])


def component_blocks(nb):
    """The block indices of Y, Cb and Cr, each in scan order: the chains the DC prediction runs along."""
    k = np.arange(nb) % 6
    return [np.flatnonzero(k < 4), np.flatnonzero(k == 4), np.flatnonzero(k == 5)]


def symbols_used(coef, cap=False):
    """What the oracle's walk emits for the coefficients: (DC categories per table, AC symbols per table, the longest block in bits,
    the longest chain of ZRLs)."""
    dc, ac = [set(), set()], [set(), set()]
    bits, chain, longest, longest_chain, last = 0, 0, 0, 0, -1
    for b, t, kind, symbol, _, n in jo.walk(coef, cap):
        if b != last:
            last, bits = b, 0
        (dc if kind == "dc" else ac)[t].add(symbol)
        bits += (jo.DC_CODES if kind == "dc" else jo.AC_CODES)[t][symbol][1] + n
        chain = chain + 1 if (kind, symbol) == ("ac", 0xF0) else 0
        longest, longest_chain = max(longest, bits), max(longest_chain, chain)
    return dc, ac, longest, longest_chain


def dense(H, W, seed, density):
    """Each AC position non-zero with probability `density`, its category uniform in 1 .. 10, the magnitude uniform inside the category,
    the sign random; DC uniform in -1023 .. 1023, with DC_PLANT at the start of each component (as much of it as the size has blocks)."""
    rng = np.random.default_rng([seed, H, W])
    nb = jc.num_blocks(H, W)
    cat = rng.integers(1, 11, (nb, 64))
    low = 1 << (cat - 1)
    mag = low + rng.integers(0, 1 << 9, (nb, 64)) % low        # bit length == cat
    sign = rng.choice([-1, 1], (nb, 64))
    c = np.where(rng.random((nb, 64)) < density, sign * mag, 0)
    c[:, 0] = rng.integers(-1023, 1024, nb)
    for chain in component_blocks(nb):
        n = min(len(chain), len(DC_PLANT))
        c[chain[:n], 0] = DC_PLANT[:n]
    return c.astype(np.int16)


def worst(H, W):
    """The longest stream of a size that is baseline JPEG: every AC coefficient -1023 (symbol 0x0A: 16 + 10 bits in the luminance table),
    DC alternating +1023, -1023 along each component, so that every difference but a component's first is of category 11."""
    nb = jc.num_blocks(H, W)
    c = np.full((nb, 64), -1023, np.int64)
    for chain in component_blocks(nb):
        c[chain, 0] = np.where(np.arange(len(chain)) % 2 == 0, 1023, -1023)
    return c.astype(np.int16)


def wild(H, W, seed):
    """Uniform over all of int16, with -32768 and 32767 planted in DC and AC positions and DC steps from -32768 to 32767 (a difference of
    65535) in the luminance and in a chroma chain.  Outside baseline JPEG: only wct_jpeg_pack's capping rule defines the result."""
    rng = np.random.default_rng([seed, H, W])
    nb = jc.num_blocks(H, W)
    assert nb >= 12, "two MCUs at the least"
    c = rng.integers(-32768, 32768, (nb, 64))
    c[0, 0], c[1, 0], c[2, 0] = -32768, 32767, -32768      # Y
    c[4, 0], c[10, 0] = -32768, 32767                      # Cb of the first two MCUs
    c[0, 1], c[0, 63], c[5, 1], c[5, 63] = -32768, 32767, 32767, -32768
    return c.astype(np.int16)


# (name, H, W, seed, density, byte indices): dense(H, W, seed, density), whose padded, unstuffed stream has FF at every index listed.
# Found by a search over seeds on the CPU.  chunk = WCT_JPEG_STUFF_CHUNK bytes, one workgroup of the FF count and of the scatter; a
# thread of those takes 4 bytes.
#   chunk_last      index = 1023 (mod chunk): the last byte of a chunk, its 00 is the first byte behind the chunk's output
#   chunk_first     index = 0 (mod chunk), not chunk 0: every FF in front of it was counted by other workgroups
#   chunk_straddle  both, side by side
#   thread_straddle FF FF at indices 4 j + 3 and 4 j + 4: the last byte of one thread and the first of the next
FF_EDGES = [
    ("chunk_last", 27, 70, 1, 1.0, (3071,)),
    ("chunk_first", 27, 70, 8, 1.0, (3072,)),
    ("chunk_straddle", 27, 70, 3876, 1.0, (2047, 2048)),
    ("thread_straddle", 27, 70, 3, 1.0, (2671, 2672)),
]
# worst(H, W): at least 2 STUFF_CHUNK bytes of stream, more than 5 % of them FF
FF_DENSE = (9, 170)


def sizes():
    """(name, H, W) of the launcher edges these inputs run at: both sides of PACK_SPAN, of SCAN_TILE and of STUFF_CHUNK (for noise images:
    denser input is above it everywhere), and of SEG_MCUS.  Not the 1670 x 1675 one."""
    return [(e[0], e[1], e[2]) for e in jc.EDGES if e[0] != "two_scan_steps"]
