"""Texture synthesis, the part that needs no GPU: the noise definition (Philox4x32-10 against Random123's known answers), the bicubic
resize checker against Pillow, the texture size rule and the command line's helpers, and the library's new symbols."""
import os
import re
import types

import numpy as np
import pytest

from tests import synth_oracle as S
from tests.conftest import REPO
from wct_hip import cli


# ---------------------------------------------------------------------------------------------------------------- noise
def test_philox_known_answer_vectors():
    """The three vectors of Random123's kat_vectors for philox4x32-10: counter / key -> output."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = tuple(int(v) for v in S.philox4x32_10(ctr, key))
        assert got == want, (ctr, key, ["%08x" % v for v in got])
    # vectorised over counters = one at a time (two counters under the third vector's key)
    key = kat[2][1]
    pair = [kat[0][0], kat[2][0]]
    out = S.philox4x32_10([np.array([c[j] for c in pair], np.uint64) for j in range(4)], key)
    for n, c in enumerate(pair):
        assert [int(out[j][n]) for j in range(4)] == [int(v) for v in S.philox4x32_10(c, key)]
    assert tuple(int(out[j][1]) for j in range(4)) == kat[2][2]


@pytest.mark.parametrize("H,W", [(4, 4), (5, 7), (1, 2), (1, 1), (33, 65)])
def test_noise_mapping(H, W):
    """Element e = c H W + y W + x is word e & 3 of block e >> 2, value = (word >> 8) * 2^-24; 3 H W mod 4 covers 0, 1, 2, 3."""
    seed, sid = 0x1234567890ABCDEF, 5
    n = S.noise(seed, H, W, sid)
    assert n.shape == (3, H, W) and n.dtype == np.float32
    flat = n.reshape(-1)
    for e in range(flat.size):
        i = e >> 2
        words = S.philox4x32_10((i & 0xffffffff, i >> 32, sid, 0), (seed & 0xffffffff, seed >> 32))
        assert flat[e] == np.float32(int(words[e & 3]) >> 8) * np.float32(2.0 ** -24), e
    assert float(flat.max()) < 1.0 and float(flat.min()) >= 0.0


def test_noise_shapes_cover_every_tail():
    assert sorted((3 * h * w) % 4 for h, w in ((4, 4), (5, 7), (1, 2), (1, 1))) == [0, 1, 2, 3]


def test_noise_range_seeds_and_streams():
    a = S.noise(0, 216, 384)
    assert a.max() < 1.0 and a.min() >= 0.0
    assert abs(float(a.mean(dtype=np.float64)) - 0.5) < 5e-3 and abs(float(a.var(dtype=np.float64)) - 1 / 12) < 2e-3
    assert np.array_equal(a, S.noise(0, 216, 384))
    for other in (S.noise(1, 216, 384), S.noise(1 << 32, 216, 384), S.noise(0, 216, 384, stream_id=1)):
        assert not np.array_equal(a, other) and float(np.mean(a == other)) < 1e-3
    # the high half of the seed is the second key word: seeds that agree in their low 32 bits still differ
    assert not np.array_equal(S.noise(7, 8, 8), S.noise(7 + (1 << 32), 8, 8))
    # the largest value the mapping can produce is exactly 1 - 2^-24, which fp32 holds
    assert np.float32(0xFFFFFF) * np.float32(2.0 ** -24) == np.float32(1.0) - np.float32(2.0 ** -24) < 1.0


# ---------------------------------------------------------------------------------------------------------------- bicubic resize
def test_bicubic_oracle_matches_pillow_live():
    """The shapes of test_resize.py::test_oracle_matches_pillow_live plus a x5 enlargement, against Pillow's Image.BICUBIC -- and
    Pillow's resize() without a filter where that is bicubic too (the reference's call, data_loader.py:72)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    shapes = [tuple(int(v) for v in rng.integers(1, 160, 4)) for _ in range(60)]
    shapes += [(240, 426, 4, 7), (3, 500, 3, 499), (500, 3, 7, 3), (64, 64, 64, 64), (270, 480, 135, 240), (40, 56, 200, 280)]
    for (h, w, oh, ow) in shapes:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        pil = Image.fromarray(img)
        ref = np.asarray(pil.resize((ow, oh), Image.BICUBIC))
        assert np.array_equal(S.resize_bicubic_u8(img, oh, ow), ref), (h, w, oh, ow)
        assert np.array_equal(np.asarray(pil.resize((ow, oh))), ref), ("default filter", h, w, oh, ow)


def test_bicubic_tables_are_normalised_and_have_negative_lobes():
    for (n, m) in ((2048, 512), (100, 500), (7, 3), (1, 5)):
        ksize, bounds, kk = S.axis_tables(n, m)
        assert ksize == int(np.ceil(2.0 * max(n / m, 1.0))) * 2 + 1
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n).all()
        assert np.abs(kk.sum(1) - (1 << 22)).max() <= ksize          # rounding of <= ksize weights
        assert np.abs(kk.astype(np.int64)).sum(1).max() * 255 < 2 ** 31
    assert (S.axis_tables(2048, 512)[2] < 0).any()


# ---------------------------------------------------------------------------------------------------------------- size rule, CLI helpers
def _literal_rule(h, w, s):
    """data_loader.py:64-72 as written there."""
    if w > h:
        neww = s
        newh = int(h * neww / w)
    else:
        newh = s
        neww = int(w * newh / h)
    return newh, neww


def test_synthesis_shape_is_the_reference_rule():
    rng = np.random.default_rng(3)
    cases = [(h, w, s) for h in range(1, 25) for w in range(1, 25) for s in (1, 5, 16, 24, 31)]
    cases += [tuple(int(v) for v in rng.integers(1, 12000, 3)) for _ in range(500)]
    cases += [(2048, 2048, 512), (2160, 3840, 512), (3840, 2160, 512), (1365, 2048, 256), (2048, 1365, 256), (512, 300, 512)]
    n_err = 0
    for (h, w, s) in cases:
        want = _literal_rule(h, w, s)
        assert S.synthesis_shape(h, w, s) == want
        if min(want) < 1:
            n_err += 1
            with pytest.raises(ValueError, match="style_size"):
                cli.synthesis_shape(h, w, s)
        else:
            assert cli.synthesis_shape(h, w, s) == want, (h, w, s)
    assert n_err > 0                                            # e.g. a 1 x 24 texture at size 5: int(1 * 5 / 24) = 0
    assert cli.synthesis_shape(300, 512, 512) == (300, 512)    # applies even when the long side already equals the size ...
    assert cli.synthesis_shape(301, 512, 512) == (301, 512)
    assert cli.synthesis_shape(100, 100, 64) == (64, 64)       # ... a square takes the second branch
    assert cli.synthesis_shape(77, 33, 0) == (77, 33) == S.synthesis_shape(77, 33, 0)   # --style_size 0: no resize


def test_texture_jobs_and_names(tmp_path):
    t = tmp_path / "tex"
    t.mkdir()
    for n in ("bricks.jpg", "moss.v2.png", "notes.txt", "wood.jpeg", "sub.JPG"):
        (t / n).write_bytes(b"")
    jobs = cli.texture_jobs(str(t))
    assert jobs == [x for x in os.listdir(t) if cli.is_image_file(x)] and sorted(jobs) == ["bricks.jpg", "moss.v2.png", "wood.jpeg"]
    a = cli.build_parser().parse_args(["--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6", "--synthesis",
                                       "--picked_style_mark", "bricks"])
    assert cli.texture_jobs(str(t)) == jobs                                                    # no --picked_* filter (data_loader.py:28)
    assert cli.synthesis_out_name(a, "moss.v2.png") == os.path.join("o", "L_mode=16x_alpha=0.6_moss.jpg")   # data_loader.py:76 + WCT.py:127
    assert cli.synthesis_out_name(a, "bricks.jpg") == cli.out_name(a, "bricks.jpg")


def test_parser_defaults_and_argument_checks():
    P = cli.build_parser()
    a = P.parse_args([])
    assert (a.seed, a.synthesis_size, a.synthesis, a.texturePath) == (0, None, False, "style/texture")
    cli.check_synthesis_args(a)
    ok = [["--synthesis"], ["--synthesis", "--seed", "7"], ["--synthesis", "--synthesis_size", "3840x2160", "--seed", str(2 ** 64 - 1)],
          ["--synthesis", "--style_size", "512", "--num_run", "2", "--alpha", "0.6"]]
    for argv in ok:
        cli.check_synthesis_args(P.parse_args(argv))
    bad = [(["--seed", "7"], "--seed needs --synthesis"), (["--synthesis_size", "64x64"], "--synthesis_size needs --synthesis"),
           (["--synthesis", "--maskPath", "m", "--region_styles", "a.png"], "--maskPath"),
           (["--synthesis", "--interp_styles", "a.png", "--interp_weights", "1"], "--interp_styles"),
           (["--synthesis", "--weightPath", "w"], "--weightPath"),
           (["--synthesis", "--seed", "-1"], "--seed"), (["--synthesis", "--seed", str(2 ** 64)], "--seed"),
           (["--synthesis", "--synthesis_size", "64"], "WxH"), (["--synthesis", "--synthesis_size", "64x"], "WxH"),
           (["--synthesis", "--synthesis_size", "0x64"], "positive"), (["--synthesis", "--synthesis_size", "axb"], "WxH")]
    for argv, msg in bad:
        with pytest.raises(ValueError, match=msg):
            cli.check_synthesis_args(P.parse_args(argv))
    assert cli.synthesis_size("320x200") == (200, 320) and cli.synthesis_size("3840X2160") == (2160, 3840)
    # the noise behind a --synthesis_size file: the next multiples of 16 (the cascade floors, the file is cropped)
    assert cli.synthesis_noise_shape(200, 320) == (208, 320) and cli.synthesis_noise_shape(2160, 3840) == (2160, 3840)
    assert cli.synthesis_noise_shape(1, 17) == (16, 32)
    # main() checks the arguments before it touches the GPU or the file system
    with pytest.raises(ValueError, match="--seed needs --synthesis"):
        cli.main(["--mode", "16x", "--seed", "3", "--outf", os.path.join(os.sep, "nonexistent", "never_made")])


# ---------------------------------------------------------------------------------------------------------------- library surface
def test_library_exports_the_synthesis_entries():
    import __graft_entry__ as g
    g.build()
    from wct_hip import lib
    L = lib.load()
    hdr = open(os.path.join(REPO, "include", "wct_hip.h")).read()
    for sym in ("wct_noise_uniform", "wct_synthesize", "wct_resize_u8_filter"):
        assert sym in lib.SYMBOLS and hasattr(L, sym), sym
        assert re.search(r"^int %s\(wct_ctx\* ctx," % sym, hdr, re.M), sym
    assert re.search(r"#define WCT_FILTER_BILINEAR 0\b", hdr) and re.search(r"#define WCT_FILTER_BICUBIC 1\b", hdr)
    assert lib.RESIZE_FILTERS == {"bilinear": 0, "bicubic": 1}
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):       # the header states the generator
        assert word in hdr
    # NULL contexts are rejected, never dereferenced (no GPU needed)
    assert L.wct_noise_uniform(None, 0, 0, 4, 4, None) == lib.WCT_ERR_INVALID
    assert L.wct_synthesize(None, None, 0, 0, 64, 64, 0, 0, 1.0, 1, None, None, None) == lib.WCT_ERR_INVALID
    assert L.wct_resize_u8_filter(None, None, 4, 4, None, None, 2, 2, 1) == lib.WCT_ERR_INVALID


def test_python_surface_has_the_synthesis_methods():
    import inspect
    from wct_hip import WCT
    sig = inspect.signature(WCT.noise)
    assert list(sig.parameters)[1:] == ["H", "W", "seed", "stream_id", "out"]
    assert (sig.parameters["seed"].default, sig.parameters["stream_id"].default, sig.parameters["out"].default) == (0, 0, None)
    sig = inspect.signature(WCT.synthesize)
    assert list(sig.parameters)[1:] == ["texture", "H", "W", "seed", "stream_id", "alpha", "num_run", "out"]
    assert [sig.parameters[k].default for k in ("H", "W", "seed", "stream_id", "alpha", "num_run", "out")] == [None, None, 0, 0, None, 1, None]
    assert inspect.signature(WCT.resize_u8).parameters["filter"].default == "bilinear"
