"""The claims of tests/jpeg_coef_cases.py, proved from the numpy oracle alone: the capping rule of wct_jpeg_pack as the header states it,
full coverage of both Huffman tables, the longest block and the bounds, any int16 under the cap, the FF bytes at the stuffing edges,
and DC category 11 through the transform and Pillow.  A fixture that drifts fails here, not on the GPU."""
import os

import numpy as np
import pytest

from tests import jpeg_cases as jc
from tests import jpeg_coef_cases as cc
from tests import jpeg_oracle as jo
from wct_hip import lib as _lib

MAX_BITS = _lib.JPEG_BLOCK_MAX_BITS
CHUNK = _lib.JPEG_STUFF_CHUNK
SIZES = cc.sizes()


def code(table, symbol):
    c, n = table[symbol]
    return format(c, "0%db" % n)


def block(dc=0, **ac):
    """One block; block(5, p1=7, p63=-2): DC 5, zig-zag positions 1 and 63 set."""
    z = np.zeros((1, 64), np.int16)
    z[0, 0] = dc
    for k, v in ac.items():
        z[0, int(k[1:])] = v
    return z


def entropy_bound(H, W):
    from wct_hip import WCT
    return WCT.jpeg_bound(H, W) - _lib.JPEG_HEADER_BYTES


# ---- the domain and the capping rule ---------------------------------------------------------------------------------------------------

def test_the_oracle_refuses_what_baseline_jpeg_has_no_code_for():
    for ok in (block(2047), block(-2047), block(0, p1=1023), block(0, p63=-1023)):
        assert jo.bitstring(ok) == jo.bitstring(ok, cap=True)
    for bad in (block(2048), block(-2048), block(0, p1=1024), block(0, p63=-1024), block(-32768), block(0, p7=32767)):
        with pytest.raises(ValueError, match="baseline JPEG"):
            jo.bitstring(bad)
        with pytest.raises(ValueError, match="baseline JPEG"):
            jo.entropy(bad)
        jo.entropy(bad, cap=True)
    # a difference, not a value: 1023 after -1025 is a step of 2048
    two = np.concatenate([block(-1025), block(1023)])
    with pytest.raises(ValueError, match="DC difference"):
        jo.bitstring(two)


def test_the_capping_rule_written_out_by_hand():
    """Category capped at 11 (DC) or 10 (AC); the low n bits of v, or of v - 1 for a negative v."""
    dcy, acy = jo.DC_CODES[0], jo.AC_CODES[0]
    eob = code(acy, 0)
    cases = [
        (block(0, p1=1024), code(dcy, 0) + code(acy, 0x0A) + "0000000000" + eob),                 # 1024 = 1 00000 00000
        (block(0, p1=-1024), code(dcy, 0) + code(acy, 0x0A) + "1111111111" + eob),                # -1025 = .. 011 11111 11111
        (block(0, p1=32767), code(dcy, 0) + code(acy, 0x0A) + "1111111111" + eob),
        (block(0, p1=-32768), code(dcy, 0) + code(acy, 0x0A) + "1111111111" + eob),               # -32769 = .. 0111 1111 1111 1111
        (block(0, p2=1025), code(dcy, 0) + code(acy, 0x1A) + "0000000001" + eob),
        (block(0, p63=-1026), code(dcy, 0) + code(acy, 0xF0) * 3 + code(acy, 0xEA) + "1111111101"),   # -1027 = .. 011 11111 11101
        (block(2048), code(dcy, 11) + "00000000000" + eob),
        (block(-2048), code(dcy, 11) + "11111111111" + eob),
        (block(32767), code(dcy, 11) + "11111111111" + eob),
        (block(-32768), code(dcy, 11) + "11111111111" + eob),
        (block(2049), code(dcy, 11) + "00000000001" + eob),
    ]
    for z, want in cases:
        assert jo.bitstring(z, cap=True) == want, z[0, :3]
    # a step from -32768 to 32767: 65535 = 1111 1111 1111 1111, and back: -65535 - 1 = .. 1 0000 0000 0000 0000
    three = np.concatenate([block(-32768), block(32767), block(-32768)])
    assert jo.bitstring(three, cap=True) == (code(dcy, 11) + "11111111111" + eob) * 2 + code(dcy, 11) + "00000000000" + eob
    # the chroma table has its own codes
    chroma = np.concatenate([np.zeros((4, 64), np.int16), block(-4096, p1=5000)])
    assert jo.bitstring(chroma, cap=True)[-(jo.DC_CODES[1][11][1] + 11 + jo.AC_CODES[1][0x0A][1] + 10 + 2):] == \
        code(jo.DC_CODES[1], 11) + "11111111111" + code(jo.AC_CODES[1], 0x0A) + format(5000 & 1023, "010b") + code(jo.AC_CODES[1], 0)


def test_block_starts_are_the_bit_offsets_of_the_blocks():
    coef = cc.dense(27, 70, 1, 0.3)
    starts = []
    bits = jo.bitstring(coef, starts=starts)
    assert len(starts) == len(coef) and starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:]))
    # the bits of block 6 alone (the first block of the second MCU: its predictor is block 3)
    alone = jo.bitstring(np.concatenate([np.zeros((3, 64), np.int16), coef[3:4], np.zeros((2, 64), np.int16), coef[6:7]]))
    assert alone.endswith(bits[starts[6]:starts[7]])


def test_the_header_states_the_rule_the_oracle_implements():
    from tests.conftest import REPO
    text = " ".join(open(os.path.join(REPO, "include", "wct_hip_jpeg.h")).read().replace("*", " ").split())
    for phrase in ("|DC difference| <= 2047", "|AC| <= 1023", "capped at 11 (DC) or 10 (AC)", "low n bits of v", "v - 1", "not a valid file",
                   "deterministic", "memory safe", "WCT_JPEG_BLOCK_MAX_BITS", "wct_jpeg_bound"):
        assert phrase in text, phrase
    assert (jo.DC_MAX_CATEGORY, jo.AC_MAX_CATEGORY) == (11, 10)
    assert max(jo.DC_CODES[0]) == max(jo.DC_CODES[1]) == 11 and max(s & 15 for s in jo.AC_CODES[0]) == max(s & 15 for s in jo.AC_CODES[1]) == 10


# ---- dense: every symbol ---------------------------------------------------------------------------------------------------------------

def zero_runs(coef):
    """The runs of zeros in front of every non-zero AC coefficient, all blocks together."""
    runs = []
    for b in coef:
        nz = np.flatnonzero(b[1:])
        runs.extend(np.diff(np.concatenate([[-1], nz])) - 1)
    return np.array(runs)


def test_dense_uses_every_symbol_of_both_tables():
    H, W, seed = cc.COVER
    dc, ac = [set(), set()], [set(), set()]
    chains, longest = set(), 0
    coefs = [cc.dense(H, W, seed, d) for d in cc.DENSITIES]
    for coef in coefs:
        assert coef.shape == (jc.num_blocks(H, W), 64) and coef.dtype == np.int16
        d, a, bits, chain = cc.symbols_used(coef)
        for t in (0, 1):
            dc[t] |= d[t]
            ac[t] |= a[t]
        longest = max(longest, bits)
        chains |= set((zero_runs(coef) // 16).tolist())
        assert chain == (zero_runs(coef) // 16).max()
    for t in (0, 1):
        assert ac[t] == set(jo.AC_CODES[t]) and len(ac[t]) == 162, "table %d misses %s" % (t, sorted(hex(s) for s in set(jo.AC_CODES[t]) - ac[t]))
        assert dc[t] == set(range(12)), "table %d misses DC categories %s" % (t, sorted(set(range(12)) - dc[t]))
    assert {1, 2, 3} <= chains, "chains of 1, 2 and 3 ZRLs"
    assert longest <= MAX_BITS
    all_ac = np.concatenate([c[:, 1:] for c in coefs])
    last = np.concatenate([c[:, 63] for c in coefs])
    assert (last != 0).any() and (last == 0).any(), "blocks that end with and without EOB"
    for k in (0, 1):      # Y blocks and chroma blocks
        part = all_ac[(np.arange(len(all_ac)) % 6 >= 4) == bool(k)]
        assert (part == 1).any() and (part == -1).any(), "both signs at size 1"
        assert ((part >= 512) & (part <= 1023)).any() and ((part <= -512) & (part >= -1023)).any(), "both signs at size 10"
    assert np.abs(all_ac).max() <= 1023
    # what the 26-bit emits are: a 16-bit code with 10 value bits, in both tables
    assert any(jo.AC_CODES[t][s][1] == 16 and s & 15 == 10 for t in (0, 1) for s in ac[t])


def test_the_covering_size_is_recorded_with_its_block_count():
    H, W, seed = cc.COVER
    assert jc.num_blocks(H, W) == 486 and H % 16 and W % 16
    assert jc.num_blocks(H, W) > _lib.JPEG_SCAN_TILE, "more than one tile of the bit-count scan"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: s[0])
def test_dense_is_in_the_domain_at_every_size(size):
    name, H, W = size
    for density in cc.DENSITIES:
        coef = cc.dense(H, W, 1, density)
        assert coef.shape == (jc.num_blocks(H, W), 64)
        assert jo.entropy(coef) == jo.entropy(coef, cap=True)
        assert len(jo.entropy(coef)) <= entropy_bound(H, W)
        nz = np.count_nonzero(coef[:, 1:]) / coef[:, 1:].size
        assert abs(nz - density) < 0.05
    chains = cc.component_blocks(len(coef))
    for chain in chains:      # what fits of the planted DC differences is there
        n = min(len(chain), 12)
        diffs = np.diff(np.concatenate([[0], coef[chain[:n], 0].astype(np.int64)]))
        assert [abs(int(d)).bit_length() for d in diffs] == list(range(n))


# ---- worst: the bit bound --------------------------------------------------------------------------------------------------------------

def longest_block(t):
    """The most bits a block of table t can have inside the domain, by exhausting the choice at every position: f[run] = the most bits
    the positions from here on can add when `run` zeros are pending.  A position is zero or takes the category that costs most."""
    dc = max(n + jo.DC_CODES[t][n][1] for n in range(12))
    ac = jo.AC_CODES[t]
    f = [ac[0x00][1] if run else 0 for run in range(64)]      # behind position 63: EOB when zeros are pending
    for pos in range(63, 0, -1):
        g = [0] * 64
        for run in range(pos):                                   # at most pos - 1 zeros can be pending in front of position pos
            coded = (run // 16) * ac[0xF0][1] + max(ac[(run % 16) << 4 | n][1] + n for n in range(1, 11)) + f[0]
            g[run] = max(coded, f[run + 1])
        f = g
    return dc + f[0]


def test_worst_is_the_longest_block_there_is():
    assert longest_block(0) == 1658 and longest_block(1) < 1658
    assert 1658 <= MAX_BITS
    assert jo.AC_CODES[0][0x0A][1] == 16 and jo.DC_CODES[0][11][1] + 11 + 63 * 26 == 1658
    coef = cc.worst(*cc.FF_DENSE)
    dc, ac, bits, chain = cc.symbols_used(coef)
    assert bits == 1658 and ac == [{0x0A}, {0x0A}] and dc[0] == {10, 11} and dc[1] == {10, 11} and chain == 0
    starts = []
    total = len(jo.bitstring(coef, starts=starts))
    lengths = np.diff(starts + [total])
    assert (lengths[np.arange(len(coef)) % 6 < 4][1:] == 1658).all(), "every Y block but the first"


@pytest.mark.parametrize("size", SIZES + [("full_span",) + cc.FF_DENSE], ids=lambda s: s[0])
def test_worst_stays_within_the_bound(size):
    name, H, W = size
    coef = cc.worst(H, W)
    assert coef.shape == (jc.num_blocks(H, W), 64) and np.abs(coef).max() == 1023
    assert len(jo.entropy(coef)) <= entropy_bound(H, W)
    assert len(jo.padded_stream(coef)) <= len(coef) * MAX_BITS // 8


def test_how_close_worst_comes_to_the_bound():
    """Recorded, not a limit: at 9 x 170 (66 blocks; the first span of 64 is full of worst-case blocks) the segment has 14064 bytes where
    wct_jpeg_bound less the header allows 28514: the bound counts 1728 bits a block, all of them stuffed; the longest stream has 1658 a Y block, 1408 a
    chroma block, and 8.2 % of its bytes are FF."""
    H, W = cc.FF_DENSE
    assert jc.num_blocks(H, W) == 66 > _lib.JPEG_PACK_SPAN
    coef = cc.worst(H, W)
    assert len(jo.entropy(coef)) == 14064 and entropy_bound(H, W) == 28514
    stream = jo.padded_stream(coef)
    assert len(stream) == 12991 >= 2 * CHUNK and stream.count(b"\xff") == 1071 > 0.05 * len(stream)
    # the first span alone: 64 blocks of this in the LDS array of the pack kernel, which holds 64 x 1728 / 32 + 2 words
    starts = []
    jo.bitstring(coef, starts=starts)
    assert 0.9 * 64 * MAX_BITS < starts[64] <= 64 * MAX_BITS


# ---- wild: any int16 -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: s[0])
def test_wild_is_defined_only_by_the_cap_and_stays_within_the_bounds(size):
    name, H, W = size
    coef = cc.wild(H, W, 1)
    assert coef.shape == (jc.num_blocks(H, W), 64) and coef.dtype == np.int16
    assert coef.min() == -32768 and coef.max() == 32767
    assert {int(coef[0, 0]), int(coef[1, 0])} == {-32768, 32767} and {int(coef[4, 0]), int(coef[10, 0])} == {-32768, 32767}
    assert {-32768, 32767} <= set(coef[:, 1:].ravel().tolist())
    with pytest.raises(ValueError, match="baseline JPEG"):
        jo.entropy(coef)
    dc, ac, bits, chain = cc.symbols_used(coef, cap=True)
    assert bits <= MAX_BITS
    assert len(jo.entropy(coef, cap=True)) <= entropy_bound(H, W)


# ---- FF bytes at the stuffing kernels' edges -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", cc.FF_EDGES, ids=lambda e: e[0])
def test_ff_edges_are_where_they_claim(edge):
    name, H, W, seed, density, places = edge
    stream = jo.padded_stream(cc.dense(H, W, seed, density))
    assert len(stream) >= 2 * CHUNK
    assert places and all(stream[i] == 0xFF for i in places), [(i, stream[i]) for i in places]
    want = {"chunk_last": [CHUNK - 1], "chunk_first": [0], "chunk_straddle": [CHUNK - 1, 0], "thread_straddle": None}[name]
    if want is not None:
        assert [i % CHUNK for i in places] == want and places[-1] >= CHUNK
    if name == "chunk_last":
        assert places[0] + 1 < len(stream), "a chunk follows"
    if len(places) == 2:
        assert places[1] == places[0] + 1 and places[0] % 4 == 3, "two FF bytes side by side across a thread's 4-byte edge"
    if name == "thread_straddle":
        assert places[0] % CHUNK != CHUNK - 1


def test_ff_edges_cover_every_named_place():
    assert sorted(e[0] for e in cc.FF_EDGES) == ["chunk_first", "chunk_last", "chunk_straddle", "thread_straddle"]


# ---- the largest categories through the transform and Pillow ----------------------------------------------------------------------------

def test_extremes_reaches_dc_category_11_in_both_tables():
    new = jo.CASES[15:]
    assert [c[3] for c in new] == ["extremes", "extremes", "sat"] and [c[2] for c in new] == [100, 1, 100]
    assert all(H % 16 and W % 16 for H, W, _, _ in new), "ragged sizes"
    H, W, q, kind = new[0]
    a = jo.make_image(H, W, kind)
    coef, data = jo.encode(a, q)
    assert data == jo.pillow_bytes(a, q)
    dc, ac, bits, chain = cc.symbols_used(coef)
    assert 11 in dc[0] and 11 in dc[1]
    y = coef[np.arange(len(coef)) % 6 < 4, 0]
    assert y.min() == -1024 and y.max() == 1016
    cb = coef[4::6, 0]
    assert cb.min() == -1024 and cb.max() == 1016
    # before these, the image cases reached category 8 at the most
    assert max(max(max(d) for d in cc.symbols_used(jo.coefficients(jo.make_image(H, W, k), q))[0]) for H, W, q, k in jo.CASES[:15]) == 8
    # the saturated case at quality 100: DC categories 9 (Y) and 10 (chroma), AC size 9 in both tables, and a block of 882 bits where the
    # longest of the earlier image cases has 792
    H, W, q, kind = new[2]
    dc, ac, bits, chain = cc.symbols_used(jo.coefficients(jo.make_image(H, W, kind), q))
    assert max(dc[0]) >= 9 and max(dc[1]) >= 10 and all(max(s & 15 for s in a) >= 9 for a in ac) and bits > 792
