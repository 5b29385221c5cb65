"""Style interpolation and per-pixel style weights, CPU part: the blend oracle's three reductions (single style, interpolation, regions)
and the linearity identity in fp64, the pooled level maps and (V1, V2), the (n_eff, scaled sums) form of the weighted covariance, the
CLI's --interp_styles / --interp_weights / --weightPath handling and the C ABI's new entries."""
import os
import re

import numpy as np
import pytest

from tests import blend_oracle, region_oracle
from tests.conftest import REPO, rel_err
from wct_hip import cli


def _smooth(rng, shape):
    x = rng.random(shape, dtype=np.float32)
    for _ in range(2):
        x = (x + np.roll(x, 1, -1) + np.roll(x, 1, -2) + np.roll(x, -1, -1) + np.roll(x, -1, -2)) / 5
    return np.ascontiguousarray(x)


@pytest.fixture(scope="module")
def mods64(oracle, weights16x):
    return oracle.Modules("16x", weights16x, precision="fp64")


@pytest.mark.parametrize("alpha", [1.0, 0.6])
def test_one_hot_constant_weights_are_the_single_style_oracle(oracle, mods64, alpha):
    rng = np.random.default_rng(1)
    c, s0, s1 = _smooth(rng, (3, 64, 80)), _smooth(rng, (3, 48, 56)), _smooth(rng, (3, 40, 48))
    wts = np.zeros((2, 64, 80), np.float32)
    wts[0] = 1.0
    got = blend_oracle.stylize_blend(mods64, c, [s0, s1], wts, alpha)
    ref = oracle.stylize(mods64, c, s0, alpha)
    assert rel_err(got, ref) <= 1e-10


@pytest.mark.parametrize("lam,alpha", [((0.3, 0.7), 1.0), ((2.0, 1.0, 1.0), 0.6)])
def test_constant_weight_maps_are_interpolation(mods64, lam, alpha):
    # (level 5 needs more feature pixels than its 128 channels: a singular content covariance amplifies rounding far above 1e-10)
    rng = np.random.default_rng(len(lam))
    c = _smooth(rng, (3, 256, 224))
    styles = [_smooth(rng, (3, 48 + 8 * k, 56)) for k in range(len(lam))]
    lh = blend_oracle.normalised(lam)
    wts = np.broadcast_to(lh[:, None, None], (len(lam), 256, 224)).astype(np.float64)
    got = blend_oracle.stylize_blend(mods64, c, styles, wts, alpha)
    ref = blend_oracle.stylize_interp(mods64, c, styles, lam, alpha)
    assert rel_err(got, ref) <= 1e-10


def test_block_constant_binary_maps_are_regions(mods64):
    rng = np.random.default_rng(7)
    H, W = 288, 448
    c = _smooth(rng, (3, H, W))
    styles = [_smooth(rng, (3, 48, 56)), _smooth(rng, (3, 40, 40))]
    blocks = np.zeros((H // 16, W // 16), np.int64)            # 0, 1: a style, 2: unstyled; >= 144 level-5 pixels each
    blocks[:, 9:18] = 1
    blocks[:, 18:] = 2
    blocks[rng.random(blocks.shape) < 0.1] = 1
    lab16 = np.kron(blocks, np.ones((16, 16), np.int64))
    labels = np.where(lab16 == 2, 255, lab16).astype(np.uint8)
    wts = np.stack([(lab16 == k).astype(np.float32) for k in range(2)])
    alpha = [1.0, 0.7]
    got = blend_oracle.stylize_blend(mods64, c, styles, wts, alpha)
    ref = region_oracle.stylize_regions(mods64, c, styles, labels, alpha)
    assert rel_err(got, ref) <= 1e-10


def test_interpolation_is_one_blended_style_slot():
    rng = np.random.default_rng(9)
    C = 16
    c = rng.standard_normal((C, C)) @ rng.standard_normal((C, 300))
    sFs = [rng.standard_normal((C, C)) @ rng.standard_normal((C, 200 + 50 * k)) + k for k in range(3)]
    lam = [0.2, 1.3, 0.5]
    lh = blend_oracle.normalised(lam)
    from oracle import wct_oracle
    per_style = sum(lh[k] * wct_oracle.whiten_and_color(c, s) for k, s in enumerate(sFs))
    one_slot = blend_oracle.interp_blended_slot(c, sFs, lam)
    assert rel_err(one_slot, per_style) <= 1e-10


@pytest.mark.parametrize("H,W", [(37, 53), (64, 64), (129, 77)])
def test_pooled_maps_and_V_match_an_explicit_loop(H, W):
    rng = np.random.default_rng(H * W)
    K = 3
    wts = rng.random((K, H, W)).astype(np.float32) / K
    for level in (5, 4, 3, 2, 1):
        s = 1 << (level - 1)
        h, w = (H >> 4) << (5 - level), (W >> 4) << (5 - level)
        got = blend_oracle.pool_weights(wts, level, h, w)
        ref = np.empty((K, h, w))
        for k in range(K):
            for i in range(h):
                for j in range(w):
                    acc = 0.0
                    for r in range(s):
                        for q in range(s):
                            acc += float(wts[k, i * s + r, j * s + q])
                    ref[k, i, j] = acc / (s * s)
        assert np.allclose(got, ref, rtol=1e-12, atol=0)
        for k in range(K):
            V1, V2, _, _ = blend_oracle.weighted_moments(np.ones((1, h * w)), got[k].reshape(-1))
            assert V1 == pytest.approx(sum(float(v) for v in ref[k].flat), rel=1e-12)
            assert V2 == pytest.approx(sum(float(v) ** 2 for v in ref[k].flat), rel=1e-12)


@pytest.mark.parametrize("kind", ["random", "binary", "constant"])
def test_weighted_covariance_through_n_eff_and_scaled_sums(kind):
    """The library hands its solver n = V1^2 / V2 and the raw weighted sums scaled by V1 / V2; the solver's (sumsq - n mu mu^T) / (n - 1)
    is then the reliability-weighted covariance, and its mean sum / n the weighted mean."""
    rng = np.random.default_rng(len(kind))
    C, n = 12, 500
    x = rng.standard_normal((C, C)) @ rng.standard_normal((C, n)) + 2.0
    wk = {"random": rng.random(n), "binary": (rng.random(n) > 0.4).astype(np.float64), "constant": np.full(n, 0.35)}[kind]
    V1, V2, mu, cov = blend_oracle.weighted_moments(x, wk)
    # direct: numpy's reliability-weighted covariance
    ref = np.cov(x, aweights=wk, ddof=1)
    assert rel_err(cov, ref) <= 1e-12
    assert rel_err(mu, np.average(x, axis=1, weights=wk)) <= 1e-14
    s1, s2 = (x * wk).sum(axis=1), (x * wk) @ x.T
    ne, f = V1 * V1 / V2, V1 / V2
    mu_s = s1 * f / ne
    cov_s = (s2 * f - ne * np.outer(mu_s, mu_s)) / (ne - 1)
    assert rel_err(mu_s, mu) <= 1e-13
    assert rel_err(cov_s, cov) <= 1e-10
    if kind != "random":                       # 0/1 and constant weights: the plain n - 1 covariance of the selected columns
        xs = x[:, wk > 0]
        assert rel_err(cov, np.cov(xs, ddof=1)) <= 1e-12


def test_cli_interp_flags_parse_and_pair(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    P = cli.build_parser()
    a = P.parse_args(["--interp_styles", "a.jpg,b.jpg", "--interp_weights", "0.3,0.7", "--mode", "16x"])
    cli.check_interp_args(a)
    assert cli.interp_style_list(a) == ["a.jpg", "b.jpg"] and cli.interp_weight_list(a) == [0.3, 0.7]
    d = P.parse_args([])
    assert d.interp_styles is None and d.interp_weights is None and d.weightPath is None
    cli.check_interp_args(d)
    cli.check_interp_args(P.parse_args(["--interp_styles", "a.jpg,b.jpg", "--weightPath", "w"]))
    bad = {
        "needs --interp_styles": [["--interp_weights", "1"], ["--weightPath", "w"]],
        "goes with": [["--interp_styles", "a.jpg"]],
        "1 to 8": [["--interp_styles", ",".join("s%d.jpg" % i for i in range(9)), "--interp_weights", ",".join(["1"] * 9)]],
        "one weight per style": [["--interp_styles", "a.jpg,b.jpg", "--interp_weights", "1"]],
        "finite and >= 0": [["--interp_styles", "a.jpg,b.jpg", "--interp_weights", "1,-1"],
                            ["--interp_styles", "a.jpg,b.jpg", "--interp_weights", "0,0"],
                            ["--interp_styles", "a.jpg,b.jpg", "--interp_weights", "1,nan"]],
        "numbers expected": [["--interp_styles", "a.jpg", "--interp_weights", "x"]],
        "does not mix with --maskPath": [["--interp_styles", "a.jpg", "--interp_weights", "1", "--maskPath", "m", "--region_styles", "a.jpg"]],
        "does not mix with --weightPath": [["--interp_styles", "a.jpg", "--interp_weights", "1", "--weightPath", "w"]],
    }
    for msg, cases in bad.items():
        for argv in cases:
            with pytest.raises(ValueError, match=re.escape(msg)):
                cli.check_interp_args(P.parse_args(argv))

    c, w = tmp_path / "c", tmp_path / "w"
    c.mkdir(); w.mkdir()
    for n in ("a.jpg", "b.v2.png", "notes.txt"):
        (c / n).write_bytes(b"")
    for stem in ("a", "b"):
        for k in range(2):
            Image.fromarray(np.full((40, 60), 100 * k, np.uint8), mode="L").save(w / ("%s_%d.png" % (stem, k)))
    jobs = cli.weight_jobs(str(c), str(w), 2)
    assert sorted(jobs) == sorted([("a.jpg", [str(w / "a_0.png"), str(w / "a_1.png")]),
                                   ("b.v2.png", [str(w / "b_0.png"), str(w / "b_1.png")])])
    assert cli.weight_jobs(str(c), str(w), 2, "v2") == [("b.v2.png", [str(w / "b_0.png"), str(w / "b_1.png")])]
    with pytest.raises(FileNotFoundError, match="a_2.png"):
        cli.weight_jobs(str(c), str(w), 3)
    m = cli.load_weights([str(w / "a_0.png"), str(w / "a_1.png")], (40, 60))
    assert m.dtype == np.float32 and m.shape == (2, 40, 60)
    assert m[0].max() == 0 and m[1].min() == np.float32(100) / np.float32(255)
    with pytest.raises(ValueError, match="a_0.png"):
        cli.load_weights([str(w / "a_0.png")], (20, 30))                  # never resampled
    Image.fromarray(np.zeros((40, 60, 3), np.uint8)).save(w / "rgb_0.png")
    with pytest.raises(ValueError, match="rgb_0.png"):
        cli.load_weights([str(w / "rgb_0.png")], (40, 60))
    a = P.parse_args(["--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.5"])
    assert cli.interp_out_name(a, "b.v2.png") == os.path.join("o", "L_mode=16x_alpha=0.5_b+interp.jpg")
    assert cli.interp_out_name(a, "b.v2.png", blend=True) == os.path.join("o", "L_mode=16x_alpha=0.5_b+blend.jpg")


def test_blend_entries_declared_and_exported():
    import __graft_entry__ as g
    g.build()
    from wct_hip import lib
    hdr = open(os.path.join(REPO, "include", "wct_hip.h")).read()
    for name in ("wct_stylize_interp", "wct_style_blend", "wct_stylize_blend", "wct_moments_weighted", "wct_apply_mixed"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in lib.SYMBOLS
        assert hasattr(lib.load(), name)
    from wct_hip import WCT
    for m in ("stylize_interp", "style_blend", "stylize_blend", "moments_weighted", "apply_mixed"):
        assert callable(getattr(WCT, m))
