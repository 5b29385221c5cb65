"""The inputs of the device JPEG decoder's tests: files written by Pillow at run time (no fixtures), eleven sizes crossed with the nine
variants the definition was checked on, and the files at the edges of the schedule and the launchers, read off the constants of
include/wct_hip_jdec.h.  tests/test_jdec_cpu.py checks that each edge case is where it claims; tests/test_jdec_gpu.py runs them."""
import functools
import io
import os

import numpy as np

from tests import jpeg_oracle as jo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SIZES = [(1, 1, "noise"), (9, 7, "noise"), (23, 47, "noise"), (18, 34, "noise"), (16, 16, "noise"), (41, 70, "noise"), (33, 50, "noise"),
         (37, 29, "smooth"), (40, 72, "extremes"), (35, 52, "sat"), (48, 80, "smooth")]
VARIANTS = {
    "420": dict(subsampling=2), "444": dict(subsampling=0), "422": dict(subsampling=1), "grey": dict(grey=True),
    "420opt": dict(subsampling=2, optimize=True), "444opt": dict(subsampling=0, optimize=True),
    "420rb3": dict(subsampling=2, restart_marker_blocks=3), "444rr1": dict(subsampling=0, restart_marker_rows=1),
    "422opt-rb1": dict(subsampling=1, optimize=True, restart_marker_blocks=1),
}
QUALITIES = [1, 10, 30, 50, 75, 85, 90, 95, 100]
# every size with every variant; the qualities 1 .. 100 dealt round robin
CASES = [(H, W, kind, v, QUALITIES[(i + j) % len(QUALITIES)]) for i, (H, W, kind) in enumerate(SIZES) for j, v in enumerate(VARIANTS)]


def case_id(c):
    return "%dx%d-%s-%s-q%d" % c


def save(img, quality, **kw):
    """Pillow's file of a uint8 H x W x 3 array; grey=True: of its luminance."""
    from PIL import Image
    kw = dict(kw)
    im = Image.fromarray(img)
    if kw.pop("grey", False):
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, format="JPEG", quality=quality, **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def case_bytes(case):
    H, W, kind, variant, q = case
    return save(jo.make_image(H, W, kind), q, **VARIANTS[variant])


@functools.lru_cache(maxsize=None)
def fixture():
    from PIL import Image
    return np.asarray(Image.open(os.path.join(GOLDEN, "g11_uhd_content_3840x2160.jpg")).convert("RGB"))


@functools.lru_cache(maxsize=None)
def photo_crop(quality=75, **kw):
    """The 640 x 480 crop of the 4K content fixture the synchronisation was studied on."""
    return save(np.ascontiguousarray(fixture()[840:1320, 1600:2240]), quality, **(kw or dict(subsampling=2)))


@functools.lru_cache(maxsize=None)
def flat(optimize=True):
    return save(np.full((320, 320, 3), (200, 60, 30), np.uint8), 75, subsampling=2, optimize=optimize)


@functools.lru_cache(maxsize=None)
def large():
    """A 4:4:4 photograph of over WCT_JDEC_DC_TILE x WCT_JDEC_SCAN_CHUNK MCUs: two steps of every one-workgroup scan."""
    return save(np.ascontiguousarray(fixture()[40:2104, 900:2964]), 90, subsampling=0)


# Seeds found by search (tests/test_jdec_cpu.py proves what they claim): a 32 x 32 noise image whose compacted stream is a whole number
# of subsequences, and a 24 x 40 noise image with a restart marker per MCU one of whose padded anchors falls on a subsequence boundary.
# They hold for the bytes one build of Pillow / libjpeg-turbo writes; where test_edge_cases_are_where_they_claim fails under another
# build, search again with find_seeds() below (about a minute) and put in what it returns.
EXACT_SEED, EXACT_QUALITY = 716, 90
ANCHOR_SEED, ANCHOR_QUALITY = 5, 85


def find_seeds(seeds=range(1, 3000), qualities=(90, 85, 95, 80)):
    """((EXACT_SEED, EXACT_QUALITY), (ANCHOR_SEED, ANCHOR_QUALITY)) by the search that found the committed ones: the first seed and
    quality whose file has the property test_edge_cases_are_where_they_claim asks for, and synchronises within half the default."""
    from tests import jdec_oracle as jd
    found = [None, None]
    for seed in seeds:
        for q in qualities:
            if found[0] is None:
                d = jd.decoder(save(jo.make_image(32, 32, "noise", seed), q, subsampling=2))
                if d.total % jd.SUBSEQ_BITS == 0 and d.nsub >= 2 and d.schedule(jd.ROUNDS // 2)[0]:
                    found[0] = (seed, q)
            if found[1] is None:
                d = jd.decoder(save(jo.make_image(24, 40, "noise", seed), q, subsampling=2, restart_marker_blocks=1))
                if any(a % jd.SUBSEQ_BITS == 0 and d.stream[a // 8 - 1] & 1 and d.stream[a // 8 - 1] & 0x7F != 0x7F for a in d.anchors[:-1]) \
                        and d.schedule(jd.ROUNDS // 2)[0]:
                    found[1] = (seed, q)
        if None not in found:
            break
    return tuple(found)


@functools.lru_cache(maxsize=None)
def exact():
    return save(jo.make_image(32, 32, "noise", EXACT_SEED), EXACT_QUALITY, subsampling=2)


@functools.lru_cache(maxsize=None)
def anchor_edge():
    return save(jo.make_image(24, 40, "noise", ANCHOR_SEED), ANCHOR_QUALITY, subsampling=2, restart_marker_blocks=1)


@functools.lru_cache(maxsize=None)
def saturated():
    """Saturated blocks at quality 100, 64 x 64: every block half black and half white with a random polarity, and one pixel in twenty
    flipped.  The first AC coefficient is beyond +-512, whose symbol is a 16-bit code and 10 value bits: the longest Pillow writes
    (uniform saturated noise stays at 25 bits)."""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:64, 0:64]
    polarity = rng.integers(0, 2, (8, 8)).repeat(8, 0).repeat(8, 1)
    a = ((xx % 8 < 4) ^ polarity ^ (rng.random((64, 64)) < 0.05)) * 255
    return save(a.astype(np.uint8)[..., None].repeat(3, 2), 100, subsampling=0)


# The files of the synchronisation study (the table of tests/test_jdec_cpu.py), beside photo_crop() and flat() above
def smooth_opt():
    return save(jo.make_image(320, 320, "smooth"), 75, subsampling=2, optimize=True)


def noise_q100():
    return save(jo.make_image(128, 128, "noise"), 100, subsampling=2)


def flat_standard():
    """Flat colour with the standard tables: 32 bits an MCU, so a guess at a multiple of 1024 bits is right exactly when the first MCU's
    longer DC codes leave the MCU boundaries on multiples of 32 -- (255, 0, 0) does not (grey and the colour of flat() do)."""
    return save(np.full((320, 320, 3), (255, 0, 0), np.uint8), 75, subsampling=2)


EDGES = {"short": lambda: case_bytes(CASES[0]), "exact": exact, "anchor_edge": anchor_edge, "saturated": saturated, "photo": photo_crop,
         "flat_opt": flat}
