"""The width helper (tests/width_models.py) against model_zoo and the oracle, the width cases against wct_load_module's rules, and
the sensitivity of the GPU width tests' gates (tests/test_widths_gpu.py).  CPU only."""
import numpy as np
import pytest

from tests import width_models as wm
from tests.conftest import rel_err
from wct_hip import model_zoo


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5])
def test_layer_graph_matches_model_zoo(level):
    assert wm.encoder_layers(wm.W16X, level) == model_zoo.encoder_layers("16x", level)
    assert wm.decoder_layers(wm.W16X, level) == model_zoo.decoder_layers("16x", level)
    assert wm.feature_channels(wm.W16X, level) == model_zoo.feature_channels("16x", level)


def test_synth_matches_model_zoo_stream():
    """With model_zoo's widths the helper's weights are model_zoo.synth_weights' (same draws in the same order)."""
    widths = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512, "l1": 64}
    a, b = wm.synth(widths, 3), model_zoo.synth_weights("original", 3)
    assert sorted(a) == sorted(b)
    assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5])
def test_references_match_oracle_modules(oracle, weights16x, level):
    """fp32 arm == oracle.Modules("16x") bit for bit; fp64 arm within fp32 round-off of it."""
    m32 = oracle.Modules("16x", weights16x)
    rng = np.random.default_rng(level)
    img = wm.smooth_image(rng, 37, 45)
    ref = m32.encode(level, img)
    assert np.array_equal(wm.encode(wm.W16X, weights16x, level, img, f64=False), ref)
    assert rel_err(wm.encode(wm.W16X, weights16x, level, img), ref) < 1e-5
    f = np.ascontiguousarray(ref, np.float32)
    refd = m32.decode(level, f)
    assert np.array_equal(wm.decode(wm.W16X, weights16x, level, f, f64=False), refd)
    assert rel_err(wm.decode(wm.W16X, weights16x, level, f), refd) < 1e-5


def test_width_cases_obey_load_rules():
    for name, widths in wm.MODELS.items():
        for level in range(1, 6):
            assert wm.loadable("enc", wm.encoder_layers(widths, level)), (name, level)
            assert wm.loadable("dec", wm.decoder_layers(widths, level)), (name, level)
    assert sorted(wm.FAMILIES) == sorted(wm.MODELS)
    for C in wm.L1_WIDTHS:
        w = wm.level1_widths(C)
        assert wm.loadable("enc", wm.encoder_layers(w, 1)) and wm.loadable("dec", wm.decoder_layers(w, 1))
    assert all(4 <= C <= 512 and C % 4 == 0 for C in wm.MOMENT_WIDTHS)
    # the shipped graphs stay loadable under the load-time refusals
    for mode in ("16x", "original"):
        for level in range(1, 6):
            assert wm.loadable("enc", model_zoo.encoder_layers(mode, level)) and wm.loadable("dec", model_zoo.decoder_layers(mode, level))
    for name, kind, level, spec in wm.REFUSED:
        layers = [wm.Layer("c%d" % i, a, b, bool(p), bool(u)) for i, (a, b, p, u) in enumerate(spec)]
        assert not wm.loadable(kind, layers), name
        # ... and every one of them passes the width rules that held before the refusals
        assert all(l.cin <= 512 and l.cout <= 512 and (l.cout % 4 == 0 or kind == "dec") for l in layers)


def test_level1_gates_catch_dropped_channels(oracle):
    """The fault the level-1 width tests guard against: a 32-channel level 1 that loses channels 24..31 (the fused kernels' 24-channel
    coverage).  Its error must sit at least 10x above the gates of test_level1_width_vs_fp64, for the decode and the moments."""
    C = 32
    widths = wm.level1_widths(C)
    w = wm.synth(widths, seed=100 + C, levels=(1,))
    rng = np.random.default_rng(C)
    H, W = 29, 45
    img = wm.smooth_image(rng, H, W)
    F = wm.encode(widths, w, 1, img)
    M = np.eye(C) + 0.1 * rng.standard_normal((C, C)) / np.sqrt(C)
    b = rng.standard_normal(C) * 0.1 * np.abs(F).max()
    cut = F.copy()
    cut[24:] = 0
    d_full = wm.decode_affine(widths, w, 1, F, M, b)
    assert rel_err(wm.decode_affine(widths, w, 1, cut, M, b), d_full) > 10 * wm.ENC_DEC_GATE
    # the decoder alone dropping relu1_1 channels 24..31 (l1_decode_kernel's fault), with the map applied in full
    Mcut = M.copy()
    Mcut[24:] = 0
    bcut = b.copy()
    bcut[24:] = 0
    assert rel_err(wm.decode_affine(widths, w, 1, F, Mcut, bcut), d_full) > 10 * wm.ENC_DEC_GATE
    for x0, x1 in ((0, W), (W // 3, W // 3 + 17)):
        s, ss = wm.raw_moments(F, x0, x1)
        sc, ssc = wm.raw_moments(cut, x0, x1)
        assert rel_err(sc, s) > 10 * wm.MOM_GATE and rel_err(ssc, ss) > 10 * wm.MOM_GATE


def test_refusal_message_cases_cover_the_launch_guards():
    """The two first-conv shapes launch_conv3x3 cannot run (in3 with cout > 64, in3 with a pool) are among the refused cases."""
    firsts = [(spec[0][1], spec[0][2]) for _, kind, _, spec in wm.REFUSED if kind == "enc"]
    assert any(cout > 64 for cout, _ in firsts) and any(pool for _, pool in firsts)
