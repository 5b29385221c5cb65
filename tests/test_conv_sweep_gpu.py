"""Every loadable conv layer shape through wct_encode / wct_decode on the MI355X against fp64 (tests/conv_cases.py).

Parametrised by (band, variant) like tests/test_sweep_gpu.py: 16 bands of 8 widths, each width as the cin (Line I) and as the cout
(Line II) of a layer under test in the middle of a module, at two map sizes; plus the first layers 3 -> b and the switch arms
(sp / upconv / fuse / conv mode 0), one module per (cin class, cout class, variant) cell.  One context per test, its scratch poisoned
with 0xFF: the padding lanes of SP16 records and of cout_pad tails hold NaNs unless the producer wrote them or zero weights mask them.

Per case: He-uniform weights, a smooth image or a positive feature, the fp64 walk (conv3x3_reflect_f64, floor pooling, nearest
upsampling) as the yardstick, the gate of the width tests (max(ENC_DEC_GATE, 4 x the fp32 walk's own distance from fp64)), and the
profile names equal to conv_cases.predict, launch for launch: no case passes on another kernel.  Every test prints its largest error
against the gate ("conv sweep <variant> band <b>: ...")."""
import collections

import numpy as np
import pytest

from oracle import wct_oracle
from tests import conv_cases as K
from tests import sweep_cases as S
from tests import width_models as wm
from tests.conftest import rel_err
from tests.geometry_cases import locate
from tests.gpu_ctx import Ctx
from tests.test_sweep_gpu import Worst, _layer_weights

pytestmark = pytest.mark.gpu

ENC_DEC_GATE = wm.ENC_DEC_GATE


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture
def ctx(torch):
    c = Ctx(torch)
    c.set("poison", 0xFF)
    yield c
    c.close()


def _walk(m, w, x, f64):
    """the module on a CHW image / feature: fp64 (the yardstick) or fp32 (the reference's arithmetic)"""
    key = m.key
    conv = wct_oracle.conv3x3_reflect_f64 if f64 else wct_oracle.conv3x3_reflect
    if m.kind == "enc" and f64:
        w0 = np.asarray(w[key + ".conv0.weight"], np.float64).reshape(3, 3)
        y = np.einsum("kc,chw->khw", w0, np.asarray(x, np.float64)) + np.asarray(w[key + ".conv0.bias"], np.float64)[:, None, None]
    elif m.kind == "enc":
        y = wct_oracle.conv1x1(x, w[key + ".conv0.weight"], w[key + ".conv0.bias"])
    else:
        y = np.ascontiguousarray(x, np.float64 if f64 else np.float32)
    for l in m.layers:
        y = conv(y, w["%s.%s.weight" % (key, l.name)], w["%s.%s.bias" % (key, l.name)], True)
        if l.pool_after:
            y = wct_oracle.maxpool2(y)
        if l.up_after:
            y = wct_oracle.upsample2(y)
    return y


def _run(ctx, m, worst, arms=False):
    """Load m, run it at its sizes (under the default switches, or under each switch of conv_cases.arms(m)), hold every run against the
    fp64 walk and the predicted launches.  Returns the number of device runs."""
    rng = np.random.default_rng(m.seed)
    w = _layer_weights(rng, m.key, m.layers)
    ctx.chk(ctx.load_layers(m.kind, m.level, m.layers, w, m.key))
    runs = 0
    for h, wd in m.sizes:
        x = wm.smooth_image(rng, h, wd) if m.kind == "enc" else np.maximum(rng.standard_normal((m.layers[0].cin, h, wd)) + 0.3, 0).astype(np.float32)
        ref = _walk(m, w, x, True)
        e32 = rel_err(_walk(m, w, x, False), ref)
        gate = max(ENC_DEC_GATE, 4 * e32)
        for sw in (K.arms(m) if arms else ((),)):
            want = K.predict(m.kind, m.layers, h, wd, dict(sw))
            for key, v in sw:
                ctx.conv_mode(v) if key == "conv_mode" else ctx.set(key, v)
            try:
                ctx.profile_start()
                got = ctx.encode(m.level, x) if m.kind == "enc" else ctx.decode(m.level, x)
                ran = ctx.profile_counts()
            finally:
                for key, v in sw:
                    ctx.conv_mode(1) if key == "conv_mode" else ctx.set(key, 1)
            runs += 1
            what = "%s (cin %d, cout %d) at %dx%d, switches %s" % (m.id, m.cin, m.cout, h, wd, dict(sw) or "default")
            assert ran == dict(collections.Counter(want.names)), "%s: launched %s, predicted %s (hand-overs %s)" % (what, ran, want.names, want.hand)
            assert got.shape == ref.shape, (what, got.shape, ref.shape)
            err = rel_err(got, ref)
            worst.add(err, gate, what)
            assert err < gate, "%s: %.3e against the gate %.3e (fp32 walk %.3e); kernels %s, hand-overs %s; %s" % (
                what, err, gate, e32, want.names, want.hand, locate(got, ref, 32, 8))
    return runs


# ---------------------------------------------------------------------------------------------------- Lines I and II
@pytest.mark.parametrize("variant", K.VARIANTS)
@pytest.mark.parametrize("b", range(S.N_BANDS))
def test_lines(ctx, b, variant):
    worst, runs = Worst(), 0
    for m in K.modules(b, variant):
        runs += _run(ctx, m, worst)
    assert runs == sum(len(m.sizes) for m in K.modules(b, variant))          # every planned case ran
    assert ctx.saturation() == 0
    print("conv sweep %s band %d: %d cases, %s" % (variant, b, runs, worst))


# ---------------------------------------------------------------------------------------------------- Line III: the first layers 3 -> b
@pytest.mark.parametrize("followed", [False, True], ids=["alone", "pool"])
def test_first_layers(ctx, followed):
    worst, runs = Worst(), 0
    for m in K.first_modules(followed):
        runs += _run(ctx, m, worst)
        runs += _run(ctx, m, worst, arms=True)
    assert ctx.saturation() == 0
    print("conv sweep first layers %s: %d cases, %s" % ("followed by a pooled layer" if followed else "alone", runs, worst))


# ---------------------------------------------------------------------------------------------------- the switch arms
@pytest.mark.parametrize("variant", K.VARIANTS)
def test_switch_arms(ctx, variant):
    worst, runs = Worst(), 0
    for m in K.switch_modules(variant):
        assert K.arms(m), m.id          # conv mode 0 changes every path
        runs += _run(ctx, m, worst, arms=True)
    assert ctx.saturation() == 0
    print("conv sweep %s switch arms: %d cases, %s" % (variant, runs, worst))
