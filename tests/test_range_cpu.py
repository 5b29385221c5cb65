"""tests/range_cases.py against the source text and against fp64: the catalogue of clamp sites cannot fall behind the kernels, every probe
has the properties the GPU test relies on, and `clamped_walk` is the existing walk where nothing is over range.  Runs without a GPU."""
import os
import re

import numpy as np
import pytest

from tests import range_cases as rc
from tests import state_cases as sc
from tests import width_models as wm
from tests.conftest import PKG
from wct_hip import lib

CSRC = os.path.join(PKG, "csrc")


def _global_kernels():
    """{kernel name: (file, body text)} of every __global__ function under csrc/"""
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", text):
            i = text.index("{", m.end())
            depth, j = 1, i + 1
            while depth:
                depth += {"{": 1, "}": -1}.get(text[j], 0)
                j += 1
            assert m.group(1) not in out, m.group(1)
            out[m.group(1)] = (fn, text[i:j])
    return out


def test_sites_cover_every_kernel_that_can_raise_the_flag():
    kernels = _global_kernels()
    assert len(kernels) >= 80
    raising = {k for k, (_, body) in kernels.items() if ".commit(" in body or "sat_raise(" in body}
    listed = {s.kernel for s in rc.SITES}
    assert listed == raising, "kernels with a clamp and no entry in range_cases.SITES: %s; entries without such a kernel: %s" % (
        sorted(raising - listed), sorted(listed - raising))
    for s in rc.SITES:
        assert kernels[s.kernel][0] == s.file and s.kind in ("input", "lds", "sp16") and s.what, s
    assert len({(s.kernel, s.name) for s in rc.SITES}) == len(rc.SITES)


def test_probe_names_resolve():
    used = set()
    for s in rc.SITES:
        assert s.probes, "no probe drives %s / %s" % (s.kernel, s.name)
        for name in s.probes:
            if name == "swap":
                continue
            model, t = name.split("@")[0].split(":")
            m = rc.MODELS[model]
            assert t == "in" or 0 <= int(t) < len(m.spec) - 1, name          # a target is followed by a layer that consumes the clamped value
            # an input site is driven through the call's input -- or, with the SP16 hand-over off, through the fp32 map in front of the kernel
            assert (s.kind == "input") == (t == "in" or ("sp", 0) in m.switches), (s, name)
            assert rc.TARGET_FAMILY[model + ":" + t] in m.families + ("l1_decode_fused<3-24-3>",), name
            used.add(model)
    for model, t in rc.BIG.items():        # more units than workgroups, and a workgroup of XCD 0 with a successor unit (sp_spot asserts it)
        for cus in (64, 256, 304):
            m = rc.model_for(model, cus)
            assert rc.sp_spot(m, t, cus, "parked") != rc.sp_spot(m, t, cus, "final"), (model, cus)
            assert rc.gc.sp_form(*rc.target_dims(m, t)[:2], m.spec[t][0], wm.pad_cout(m.spec[t][1]), model == "bigup", cus).endswith("m")
    for name, (model, targets, family, form) in rc.TALL.items():
        assert model in rc.MODELS and family in rc.MODELS[model].families, name
    assert used == set(rc.MODELS)
    ids = [p.id for p in rc.probes()]
    assert len(ids) == len(set(ids))
    for name, m in rc.MODELS.items():
        H, W = m.size
        assert H % 8 and W % 32, name
        assert m.kind == "dec" or m.slot == 1 + sum(1 for l in m.spec if l[2]), name       # wct_feature_shape halves (level - 1) times


@pytest.mark.parametrize("model", sorted(rc.MODELS))
def test_probe_properties_fp64(model):
    """over: the target (and nothing else) passes 1.1 x 65504, everything else that is clamped stays below half the range, and the clamp moves
    the output by at least 100 x the gate; under: the same weights, the target peaks in [0.85, 0.92] x 65504 -- below 65488, where note_hi fires."""
    m = rc.model_for(model)
    probes = [p for p in rc.probes() if p.model == model]
    assert probes
    for p in probes:
        b = rc.build(p)
        twin = rc.build(p._replace(variant="under" if p.variant == "over" else "over"))
        assert all(np.array_equal(b.weights[k], twin.weights[k]) for k in b.weights), p.id
        if p.value == "nan":
            assert np.isnan(b.x).sum() == 1
            trace = []
            out = rc.clamped_walk(m.kind, b.layers, b.weights, b.key, b.x, True, True, trace)
            assert np.isfinite(out).all() and max(v for k, v in trace if k != "in") <= rc.OTHERS_MAX * rc.RANGE, p.id
            continue
        trace = []
        plain = rc.clamped_walk(m.kind, b.layers, b.weights, b.key, b.x, True, False, trace)
        seen = dict(trace)
        peak = seen.pop(p.target) / rc.RANGE
        assert max(seen.values()) <= rc.OTHERS_MAX * rc.RANGE, (p.id, seen)
        clamped = rc.clamped_walk(m.kind, b.layers, b.weights, b.key, b.x, True, True)
        if p.variant == "over":
            assert peak >= rc.OVER_MIN, (p.id, peak)
            moved = np.abs(clamped - plain).max() / np.abs(clamped).max()
            assert moved >= 100 * wm.ENC_DEC_GATE, (p.id, moved)
        else:
            assert rc.UNDER_LO <= peak <= rc.UNDER_HI and peak * rc.RANGE < rc.NOTE_HI_FROM, (p.id, peak)
            assert np.array_equal(clamped, plain), p.id


@pytest.mark.parametrize("f64", [True, False])
def test_clamped_walk_is_the_plain_walk_in_range(f64):
    widths = wm.MODELS["B"]
    w = wm.synth(widths, seed=3, levels=(3,))
    rng = np.random.default_rng(3)
    img = wm.smooth_image(rng, 37, 53)
    ref = wm.encode(widths, w, 3, img, f64)
    got = rc.clamped_walk("enc", wm.encoder_layers(widths, 3), w, "e3", img, f64)
    assert got.dtype == ref.dtype and np.array_equal(got, ref)
    feat = np.maximum(ref, 0).astype(np.float32)
    refd = wm.decode(widths, w, 3, feat, f64)
    gotd = rc.clamped_walk("dec", wm.decoder_layers(widths, 3), w, "d3", feat, f64)
    assert gotd.dtype == refd.dtype and np.array_equal(gotd, refd)


def test_clamped_walk_clamps_where_the_device_does():
    layers = rc.layers_of([(3, 8, 0, 0), (8, 8, 0, 0)])
    w = rc.base_weights("e1", "enc", layers, 1)
    x = np.full((3, 6, 6), 0.5, np.float32)
    x[0, 2, 2], x[1, 3, 3], x[2, 4, 4] = 1e6, -1e6, np.nan
    xc = x.copy()
    xc[0, 2, 2], xc[1, 3, 3], xc[2, 4, 4] = rc.RANGE, -rc.RANGE, -rc.RANGE
    assert np.array_equal(rc.clamped_walk("enc", layers, w, "e1", x), rc.clamped_walk("enc", layers, w, "e1", xc, clamp=False))
    w["e1.L0.weight"] = w["e1.L0.weight"] * 1e5           # relu(conv) of layer 0 passes the range: clipped before layer 1, not after it
    mid = np.clip(rc.clamped_walk("enc", layers[:1], w, "e1", x), 0, rc.RANGE)
    assert mid.max() == rc.RANGE
    want = rc.wct_oracle.conv3x3_reflect_f64(mid, w["e1.L1.weight"], w["e1.L1.bias"], True)
    assert np.array_equal(rc.clamped_walk("enc", layers, w, "e1", x), want) and want.max() > rc.RANGE


def test_every_entry_point_family_is_classified():
    families = {c.family for c in sc.CASES.values()}
    extra = lib.SYMBOLS_COLOR + lib.SYMBOLS_SMOOTH + lib.SYMBOLS_TRANSFORM + lib.SYMBOLS_SWAP
    assert set(rc.METHOD_OF) == set(extra), sorted(set(rc.METHOD_OF) ^ set(extra))
    src = open(os.path.join(PKG, "wct_hip", "wct.py")).read()
    methods = set()
    for sym, meth in rc.METHOD_OF.items():
        name = sym[len("wct_"):]
        has = re.search(r"^    def %s\(" % re.escape(name), src, re.M) is not None
        assert (meth == name) if has else (meth is None), "%s: a Python method %s" % (sym, "exists" if has else "does not exist")
        if meth:
            assert "_lib.%s(" % sym in src
            methods.add(meth)
    assert not families & methods
    assert set(rc.RANGE_EXPECT) == families | methods, sorted(set(rc.RANGE_EXPECT) ^ (families | methods))
    assert set(rc.RANGE_EXPECT.values()) == {"flags", "clean"}
