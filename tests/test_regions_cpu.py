"""Spatial control (wct_stylize_regions), CPU part: the region oracle against the single-style oracle, the level label maps, the CLI's
--maskPath / --region_styles handling and the C ABI's new entries."""
import os
import re

import numpy as np
import pytest

from tests import region_oracle
from tests.conftest import PKG, REPO
from wct_hip import cli, model_zoo


def _smooth(rng, shape):
    x = rng.random(shape, dtype=np.float32)
    for _ in range(2):
        x = (x + np.roll(x, 1, 1) + np.roll(x, 1, 2) + np.roll(x, -1, 1) + np.roll(x, -1, 2)) / 5
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("alpha", [1.0, 0.6])
def test_uniform_single_region_is_the_single_style_oracle(oracle, weights16x, alpha):
    """K = 1, every label 0: the region definition IS the reference's cascade, bit for bit."""
    mods = oracle.Modules("16x", weights16x)
    rng = np.random.default_rng(3)
    c, s = _smooth(rng, (3, 64, 80)), _smooth(rng, (3, 48, 56))
    labels = np.zeros((64, 80), np.uint8)
    got = region_oracle.stylize_regions(mods, c, [s], labels, alpha)
    ref = oracle.stylize(mods, c, s, alpha)
    assert got.dtype == ref.dtype and np.array_equal(got, ref)


@pytest.mark.parametrize("H,W", [(37, 53), (64, 64), (129, 77), (16, 31)])
def test_level_labels_match_an_explicit_loop(H, W):
    rng = np.random.default_rng(H * W)
    labels = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    for level in (5, 4, 3, 2, 1):
        s = 1 << (level - 1)
        h, w = ((H >> 4) << (5 - level), (W >> 4) << (5 - level))   # the sizes the cascade visits (cropped to 16 at level 5)
        got = region_oracle.level_labels(labels, level, h, w)
        ref = np.empty((h, w), np.uint8)
        for i in range(h):
            for j in range(w):
                ref[i, j] = labels[i * s + s // 2, j * s + s // 2]
        assert np.array_equal(got, ref)


def test_unstyled_and_tiny_regions_keep_the_content_features(oracle, weights16x):
    """label 255 and a region with < 2 feature pixels leave cF as it is: with every pixel in such a region the level is d(e(img))."""
    mods = oracle.Modules("16x", weights16x)
    rng = np.random.default_rng(5)
    c, s = _smooth(rng, (3, 48, 48)), _smooth(rng, (3, 40, 40))
    labels = np.full((48, 48), 255, np.uint8)
    labels[8, 8] = 0                                  # one pixel of region 0 at level 5 (s = 16: centre 8)
    got = region_oracle.region_transfer(mods, 5, c, labels, [s], [1.0])
    ref = mods.decode(5, mods.encode(5, c))
    assert np.array_equal(got, ref)


def test_cli_region_flags_parse_and_pair(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    a = cli.build_parser().parse_args(["--maskPath", "m", "--region_styles", "a.jpg,b.jpg", "--mode", "16x"])
    assert a.maskPath == "m" and a.region_styles == "a.jpg,b.jpg"
    cli.check_region_args(a)
    d = cli.build_parser().parse_args([])
    assert d.maskPath is None and d.region_styles is None
    cli.check_region_args(d)
    with pytest.raises(ValueError):
        cli.check_region_args(cli.build_parser().parse_args(["--maskPath", "m"]))
    with pytest.raises(ValueError):
        cli.check_region_args(cli.build_parser().parse_args(["--region_styles", "a.jpg"]))
    with pytest.raises(ValueError):
        cli.check_region_args(cli.build_parser().parse_args(["--maskPath", "m", "--region_styles", ",".join("s%d.jpg" % i for i in range(9))]))

    c, m = tmp_path / "c", tmp_path / "m"
    c.mkdir(); m.mkdir()
    for n in ("a.jpg", "b.v2.png", "notes.txt"):
        (c / n).write_bytes(b"")
    Image.fromarray(np.zeros((40, 60), np.uint8), mode="L").save(m / "a.png")
    Image.fromarray(np.ones((40, 60), np.uint8), mode="L").convert("P").save(m / "b.png")
    jobs = cli.region_jobs(str(c), str(m))
    assert sorted(jobs) == sorted([("a.jpg", str(m / "a.png")), ("b.v2.png", str(m / "b.png"))])
    assert cli.region_jobs(str(c), str(m), "v2") == [("b.v2.png", str(m / "b.png"))]
    (c / "z.jpg").write_bytes(b"")
    with pytest.raises(FileNotFoundError, match="z.png"):
        cli.region_jobs(str(c), str(m))

    assert cli.load_mask(str(m / "a.png"), (40, 60)).dtype == np.uint8
    assert cli.load_mask(str(m / "b.png"), (40, 60)).max() == 1          # mode P: the palette index is the label
    with pytest.raises(ValueError, match="a.png"):
        cli.load_mask(str(m / "a.png"), (20, 30))                         # never resampled
    Image.fromarray(np.zeros((40, 60, 3), np.uint8)).save(m / "rgb.png")
    with pytest.raises(ValueError, match="rgb.png"):
        cli.load_mask(str(m / "rgb.png"), (40, 60))

    # the mask must match the content's size AFTER --content_size (smaller edge -> size, as load_rgb_u8 / wct_resize_shape)
    assert cli.resized_shape(40, 60, 0) == (40, 60)
    assert cli.resized_shape(40, 60, 20) == (20, 30)
    assert cli.resized_shape(60, 40, 20) == (30, 20)
    assert cli.resized_shape(40, 60, 40) == (40, 60)
    a = cli.build_parser().parse_args(["--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.5"])
    assert cli.region_out_name(a, "b.v2.png") == os.path.join("o", "L_mode=16x_alpha=0.5_b+regions.jpg")


def test_region_entries_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from wct_hip import lib
    hdr = open(os.path.join(REPO, "include", "wct_hip.h")).read()
    for name in ("wct_moments_labeled", "wct_apply_labeled", "wct_stylize_regions"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in lib.SYMBOLS
        assert hasattr(lib.load(), name)
    from wct_hip import WCT
    for m in ("moments_labeled", "apply_labeled", "stylize_regions"):
        assert callable(getattr(WCT, m))
