"""The f16x3 range flag on the MI355X (tests/range_cases.py): every clamp site is asked to raise it, and to stay quiet just below the range.

a. one probe per (site, position, value, over | under): the flag (wct_saturation_count, wct_sync's WCT_ERR_RANGE once, conv mode 0 silent), the
   kernel family read back from the profile, and the values against `clamped_walk` in fp64 -- whole map and outside the spike's receptive field;
   among the models the two-role head at the size where the launcher takes it, and the persistent kernels over more (tile, cout group) units
   than workgroups (a parked epilogue, the final flush), both sized for the device's CU count with the form read back (prof_forms);
b. the tall instantiations at their threshold sizes (flag only), and wct_patch_match's Q and K;
c. entry points: every family that runs f16x3 convolutions on its inputs shows a clamp through wct_range_poll after a device synchronisation
   and nothing else, the next call of another family raises, one sync() clears; every other family leaves the counter at 0; the split calls
   (style_prepare, content_encode, content_solve, content_decode) each on its own."""
import ctypes
from ctypes import byref, c_int

import numpy as np
import pytest

from tests import geometry_cases as gc
from tests import range_cases as rc
from tests import state_cases as sc
from tests import width_models as wm
from tests.gpu_ctx import Ctx
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

GATE = wm.ENC_DEC_GATE


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    c = Ctx(torch)
    yield c
    c.close()


def _rel(a, b, where=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if where is not None:
        a, b = a[:, where], b[:, where]
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ---------------------------------------------------------------------------------------------------- running a probe model (no wct_sync inside)
def _load(ctx, m, b):
    if m.op == "l1":
        ctx.chk(ctx.load_layers("enc", 1, b.layers[:1], b.weights, b.key))
        ctx.chk(ctx.load_layers("dec", 1, b.layers[1:], b.weights, b.key))
    else:
        ctx.chk(ctx.load_layers(m.kind, m.slot, b.layers, b.weights, b.key))


def _encode(ctx, level, x):
    H, W = x.shape[1:]
    C, h, w = ctx._shape(level, H, W)
    assert (h, w) == (H >> (level - 1), W >> (level - 1))
    xd = ctx.dev(x)
    out = ctx.t.empty((h, w, C), device="cuda", dtype=ctx.t.float32)
    ctx.chk(ctx.L.wct_encode(ctx.ctx, level, xd.data_ptr(), H, W, out.data_ptr(), _lib.LAYOUT_NHWC))
    ctx.t.cuda.synchronize()
    return out.cpu().numpy().transpose(2, 0, 1)


def _decode(ctx, m, x):
    C, h, w = x.shape
    ups = 2 ** sum(1 for s in m.spec if s[3])
    f = ctx.dev(x.transpose(1, 2, 0), np.float32)
    out = ctx.t.empty((3, h * ups, w * ups), device="cuda", dtype=ctx.t.float32)
    ctx.chk(ctx.L.wct_decode(ctx.ctx, m.slot, f.data_ptr(), h, w, _lib.LAYOUT_NHWC, out.data_ptr()))
    ctx.t.cuda.synchronize()
    return out.cpu().numpy()


def _l1_split(ctx, x):
    """wct_content_encode (l1_moments_kernel) then wct_content_decode with M = I, b = 0 (l1_decode_kernel); the counter after each"""
    H, W = x.shape[1:]
    xd = ctx.dev(x)
    s = ctx.t.empty(24, device="cuda", dtype=ctx.t.float64)
    ss = ctx.t.empty(24, 24, device="cuda", dtype=ctx.t.float64)
    h, w = c_int(), c_int()
    ctx.chk(ctx.L.wct_content_encode(ctx.ctx, 1, xd.data_ptr(), H, W, 0, -1, s.data_ptr(), ss.data_ptr(), byref(h), byref(w)))
    ctx.t.cuda.synchronize()
    n_mom = ctx.saturation(reset=True)
    M, b = ctx.dev(np.eye(24), np.float64), ctx.dev(np.zeros(24), np.float64)
    out = ctx.t.empty((3, H, W), device="cuda", dtype=ctx.t.float32)
    ho, wo = c_int(), c_int()
    ctx.chk(ctx.L.wct_content_decode(ctx.ctx, 1, M.data_ptr(), b.data_ptr(), out.data_ptr(), byref(ho), byref(wo)))
    ctx.t.cuda.synchronize()
    return n_mom, out.cpu().numpy()


def _report(tag, pairs):
    print("range %s: %s" % (tag, "  ".join("%s gpu %.2e fp32 %.2e" % (k, g, o) for k, (g, o) in pairs.items())))


def _check_values(tag, got, b, m, clamp, layers=None):
    """got against clamped_walk in fp64, the fp32 walk of the same probe as the yardstick (no further than the oracle, + 50 %): over the whole
    map, and outside the spike's receptive field (where the fp64 walks of the input with and without its spike differ)"""
    layers = b.layers if layers is None else layers
    ref = rc.clamped_walk(m.kind, layers, b.weights, b.key, b.x, True, clamp)
    r32 = rc.clamped_walk(m.kind, layers, b.weights, b.key, b.x, False, clamp)
    quiet = rc.clamped_walk(m.kind, layers, b.weights, b.key, b.plain, True, clamp)
    assert got.shape == ref.shape and np.isfinite(got).all(), tag
    outside = ~(ref != quiet).any(axis=0)
    assert outside.any() and not outside.all(), tag
    pairs = {"map": (_rel(got, ref), _rel(r32, ref)), "outside": (_rel(got, ref, outside), _rel(r32, ref, outside))}
    _report(tag, pairs)
    for k, (e_gpu, e32) in pairs.items():
        assert e_gpu <= max(GATE, 1.5 * e32), "%s %s: gpu %.3e, fp32 walk %.3e" % (tag, k, e_gpu, e32)


def _expect_flag(ctx, over, tag):
    n = ctx.saturation()
    assert (n > 0) if over else (n == 0), "%s: counter %d" % (tag, n)
    if over:
        assert ctx.sync_rc() == _lib.WCT_ERR_RANGE, tag       # reported once ...
    assert ctx.sync_rc() == _lib.WCT_OK, tag                  # ... and cleared
    assert ctx.saturation() == 0 and ctx.poll() == 0, tag


def _cus(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _form_wanted(p, m, cus):
    """the profile name, with the launcher's form, that a size-selected probe must show (None: the family alone)"""
    if p.model == "roles":
        return rc.TARGET_FAMILY["roles:in"] + gc.head_form(*m.size, cus)
    if p.model in rc.BIG:
        t = rc.BIG[p.model]
        h, w, f = rc.target_dims(m, t)
        form = gc.sp_form(h, w, m.spec[t][0], wm.pad_cout(m.spec[t][1]), f < 0, cus)
        assert form.endswith("m"), form             # more units than workgroups: epilogues ride on the next job
        return rc.TARGET_FAMILY["%s:%d" % (p.model, t)] + form
    return None


def _run(ctx, m, x):
    """(counters after l1_encode and l1_moments, or None; the output; the level-1 feature or None)"""
    if m.op == "l1":
        feat = _encode(ctx, 1, x)
        n_enc = ctx.saturation(reset=True)
        n_mom, got = _l1_split(ctx, x)
        return (n_enc, n_mom), got, feat
    return None, (_encode(ctx, m.slot, x) if m.op == "encode" else _decode(ctx, m, x)), None


@pytest.mark.parametrize("p", rc.probes(), ids=lambda p: p.id)
def test_site_flag_and_values(ctx, torch, p):
    cus = _cus(torch)
    m = rc.model_for(p.model, cus)
    b = rc.build(p, cus)
    over = p.variant == "over"
    _load(ctx, m, b)
    for k, v in m.switches:
        ctx.set(k, v)
    ctx.set("prof_forms", 1)
    try:
        ctx.conv_mode(1)
        ctx.saturation(reset=True)
        ctx.profile_start()
        early, got, feat = _run(ctx, m, b.x)
        names = ctx.profile_names()
        if early is not None:
            # the image is split by all three level-1 kernels; the 24-channel map is clamped only where it is stored split (l1_decode's LDS)
            want = (over, over) if p.target == "in" else (False, False)
            assert (early[0] > 0, early[1] > 0) == want, (p.id, early)
        plain = {n.split("#")[0] for n in names}
        target = rc.TARGET_FAMILY["%s:%s" % (p.model, p.target)]
        missing = [f for f in m.families + (target,) if f not in plain]
        assert not missing, "%s: kernel families %s did not run; ran %s" % (p.id, missing, sorted(names))
        form = _form_wanted(p, m, cus)
        assert form is None or form in names, (p.id, form, sorted(names))
        _expect_flag(ctx, over, p.id)
        _check_values(p.id, got, b, m, clamp=over)
        if feat is not None:      # l1_encode writes fp32: only the image is clamped on the way in
            ref = rc.clamped_walk("enc", b.layers[:1], b.weights, b.key, b.x, True, over)
            assert _rel(feat, ref) <= GATE, p.id
        if over:
            ctx.conv_mode(0)
            try:
                early0, _, _ = _run(ctx, m, b.x)
                assert ctx.saturation() == 0 and early0 in (None, (0, 0)), "%s: conv mode 0 counted" % p.id
            finally:
                ctx.conv_mode(1)
    finally:
        ctx.set("prof_forms", 0)
        for k, _ in m.switches:
            ctx.set(k, 2 if k == "in3wide" else 1)
        ctx.saturation(reset=True)


# ---------------------------------------------------------------------------------------------------- b. tall forms, patch match
def _tall_size(name, cus):
    """the smallest ragged size at which the restated launcher (tests/geometry_cases.py) takes the form `name` on a device with `cus` CUs"""
    pred, W, H, step = {
        "dec_tail#t16": (lambda H, W: gc.tail_form(H, W, cus, False), 1022, 14, 16),
        "dec_tail#t24": (lambda H, W: gc.tail_form(H, W, cus, False), 1022, 14, 16),
        "dec_tail_up#u16": (lambda H, W: gc.tail_form(2 * H, 2 * W, cus, True), 510, 9, 8),      # H, W: the feature in front of the upsample
        "l1_decode#t16": (lambda H, W: gc.l1dec_form(H, W, cus), 1001, 11, 16),
        "conv3x3_f16#t16": (lambda H, W: gc.f16_form(H, W, 128, cus), 500, 13, 16),
    }[name]
    while not pred(H, W).startswith(rc.TALL[name][3]):
        H += step
        assert H * W <= gc.MAX_PIXELS, name
    return H, W, pred(H, W)


@pytest.mark.parametrize("variant", ["over", "under"])
@pytest.mark.parametrize("name,target", [(n, t) for n, v in sorted(rc.TALL.items()) for t in v[1]], ids=lambda v: str(v))
def test_tall_forms_flag(ctx, torch, name, target, variant):
    """dec_tail* at 16 / 24 rows, l1_decode at 16, conv3x3_f16 on 32 x 16 tiles: other instantiations of templates probed small above.  One over
    and one under probe each at the size where the launcher takes the form, the spike in the last (ragged) tile; the flag only."""
    model, _, family, _ = rc.TALL[name]
    cus = _cus(torch)
    H, W, form = _tall_size(name, cus)
    m = rc.MODELS[model]._replace(size=(H, W))
    p = rc.Probe("%s-%s-%s" % (name, target, variant), model, target, "last", 0, "pos", variant)
    b = rc.build_on(p, m, cus)
    _load(ctx, m, b)
    ctx.set("prof_forms", 1)
    try:
        ctx.saturation(reset=True)
        ctx.profile_start()
        if m.op == "l1":
            _, got = _l1_split(ctx, b.x)
        else:
            got = _decode(ctx, m, b.x)
        names = ctx.profile_names()
    finally:
        ctx.set("prof_forms", 0)
    assert family + form in names, (family + form, sorted(names))
    assert np.isfinite(got).all()
    _expect_flag(ctx, variant == "over", p.id)


@pytest.fixture(scope="module")
def eng(torch):
    e = sc.make_engine("16x")
    yield e
    e.strict_range = False


def _poll(e):
    n = ctypes.c_ulonglong()
    e._lib.wct_range_poll(e._ctx, byref(n))
    return n.value


@pytest.mark.parametrize("which", ["q", "k"])
@pytest.mark.parametrize("value", [1.1 * rc.RANGE, -1.1 * rc.RANGE, float("nan"), 0.885 * rc.RANGE, -0.885 * rc.RANGE])
@pytest.mark.parametrize("pos", ["first", "last"])
def test_patch_match_inputs(eng, torch, which, value, pos):
    """swap_match_kernel splits Q and K (external fp32 maps, either sign) on the way into LDS: 21 x 37 and 19 x 45, 32 channels"""
    eng.strict_range = False
    eng.saturation_count(reset=True)
    g = torch.Generator().manual_seed(3)
    q, k = torch.rand((1, 21, 37, 32), generator=g).cuda(), torch.rand((1, 19, 45, 32), generator=g).cuda()
    t = q if which == "q" else k
    y, x, c = (0, 0, 0) if pos == "first" else (t.shape[1] - 1, t.shape[2] - 1, 31)
    t[0, y, x, c] = value
    idx = eng.patch_match(q, k)
    torch.cuda.synchronize()
    over = not abs(value) < rc.RANGE
    assert (_poll(eng) > 0) == over and (eng.saturation_count(reset=True) > 0) == over
    assert int(idx.min()) >= 0 and int(idx.max()) < 17 * 43


# ---------------------------------------------------------------------------------------------------- c. entry points
#: flags families of tests/state_cases.py: which call of state_cases.image() (or feature()) inside the case is the content, which the style
POISON = {
    "stylize": {"content": ("image", 0), "style": ("image", 1)}, "prepared": {"content": ("image", 0), "style": ("image", 1)},
    "export_import": {"content": ("image", 0)},                      # the style goes to a peer engine, whose flag is its own
    "level": {"content": ("image", 0), "style": ("image", 1)}, "encode_decode": {"content": ("image", 0)},
    "decode_affine": {"feature": ("feature", 0)}, "split_level": {"content": ("image", 0), "style": ("image", 1)},
    "style_split": {"style": ("image", 0)}, "regions": {"content": ("image", 0), "style": ("image", 1)},
    "interp": {"content": ("image", 0), "style": ("image", 1)}, "style_blend": {"content": ("image", 0), "style": ("image", 1)},
    "blend": {"content": ("image", 0), "style": ("image", 1)}, "synthesize": {"texture": ("image", 0)},
    "reserve": {"content": ("image", 0), "style": ("image", 1)},
}


def _flag_cases():
    out = []
    for fam, kind in sorted(rc.RANGE_EXPECT.items()):
        if kind != "flags":
            continue
        if fam in POISON:
            out += [(fam, side) for side in POISON[fam]]
        elif fam == "stylize_u8":
            out.append((fam, "weights"))         # uint8 images cannot leave the range: a scaled layer does (as test_f16x3_saturation_is_flagged)
        elif fam == "patch_match":
            continue                             # test_patch_match_inputs
        else:
            out += [(fam, "content"), (fam, "style")]
    return out


def _poisoned(monkeypatch, torch, fn, index):
    """state_cases.image / feature with the `index`-th call of the case returning a 1e6 pixel (image) or a NaN (feature)"""
    real, calls = getattr(sc, fn), []

    def wrapped(*a):
        t = real(*a)
        if len(calls) == index:
            if fn == "image":
                t[0, 1, t.shape[2] // 2, t.shape[3] // 3] = 1e6
            else:
                t[0, t.shape[1] // 2, t.shape[2] // 3, 5] = float("nan")
        calls.append(1)
        return t
    monkeypatch.setattr(sc, fn, wrapped)


def _run_method(e, torch, fam, side):
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(sc.SEED, H, W), sc.image(sc.SEED + 1, Hs, Ws)
    bad = c if side == "content" else s
    bad[0, 1, bad.shape[2] // 2, bad.shape[3] // 3] = 1e6
    if fam == "stylize_color":
        e.stylize_color(c, s, "luma")
    elif fam == "stylize_smooth":
        e.stylize_smooth(c, s, 3)
    elif fam == "swap_level":
        e.swap_level(3, c, s)
    else:
        e.stylize_swap(c, s, 4)


@pytest.mark.parametrize("fam,side", _flag_cases(), ids=lambda v: v)
def test_flags_family_reports_through_poll(eng, torch, monkeypatch, fam, side):
    e = eng
    if side == "weights":
        w = dict(sc.weights("16x"))
        w["e3.conv12.weight"], w["e3.conv12.bias"] = w["e3.conv12.weight"] * np.float32(3e4), w["e3.conv12.bias"] * np.float32(3e4)
        e = sc.make_engine("16x", w=w)
    e.strict_range = False
    assert e.saturation_count(reset=True) >= 0 and _poll(e) == 0          # 1. reset
    if fam in POISON:                                                       # 2. the over-range condition comes from the case's own inputs
        _poisoned(monkeypatch, torch, *POISON[fam][side])
        sc.run(e, fam + "/small")
        monkeypatch.undo()
    elif side == "weights":
        sc.run(e, fam + "/small")
    else:
        _run_method(e, torch, fam, side)
    torch.cuda.synchronize()                                                # 3. and nothing else
    assert _poll(e) > 0, "%s (%s): wct_range_poll shows nothing after the device has drained" % (fam, side)        # 4.
    e.strict_range = True
    with pytest.raises(OverflowError):                                      # 5. the next call of another family
        e.noise(32, 32, seed=1)
    with pytest.raises(OverflowError):
        e.sync()                                                            # 6. reported once ...
    e.sync()
    assert _poll(e) == 0 and e.saturation_count() == 0                      # ... and clear
    e.noise(32, 32, seed=1)
    e.strict_range = False


CLEAN = sorted(f for f, k in rc.RANGE_EXPECT.items() if k == "clean")


def _run_clean_method(e, torch, fam):
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(sc.SEED, H, W), sc.image(sc.SEED + 1, Hs, Ws)
    if fam == "color_moments":
        e.color_moments(c)
    elif fam in ("color_solve", "color_apply"):
        A, t = e.color_solve(*e.color_moments(c), *e.color_moments(s))
        e.color_apply(s, A, t)
    elif fam == "color_match":
        e.color_match(s, c)
    elif fam == "luma_merge":
        e.luma_merge(c * 0.5, c)
    elif fam == "guided_filter":
        e.guided_filter(c * 0.5, c, 3)
    elif fam == "set_transform":
        e.set_transform("wct")
    elif fam == "transform_solve":
        C = 64
        e.style_prepare(s)
        e.transform_solve("ot", *sc.raw_moments(sc.SEED, C, 5000, 1e-3), e.style_export(3))
    else:
        assert fam == "patch_assemble", fam
        f = sc.feature(sc.SEED, 12, 15, 32)
        idx = e.patch_match(f, f)
        e.patch_assemble(idx, 12, 15, f)


@pytest.mark.parametrize("fam", CLEAN)
def test_clean_family_leaves_the_counter(eng, torch, fam):
    e = eng
    e.strict_range = True
    assert e.saturation_count(reset=True) >= 0
    if fam + "/small" in sc.CASES:
        sc.run(e, fam + "/small")
    else:
        _run_clean_method(e, torch, fam)
    torch.cuda.synchronize()
    assert _poll(e) == 0
    e.sync()
    assert e.saturation_count() == 0


@pytest.mark.parametrize("overlap", [1, 0])
def test_split_calls_each_report_on_their_own(eng, torch, overlap):
    """style_prepare -> content_encode -> content_solve -> content_decode as split calls (wct_hip/sharded.py, pipeline.py), each step checked by
    wct_range_poll after a device synchronisation and nothing else.  The style side of style_prepare runs on the side stream (overlap 1):
    its mirror must be ordered behind those kernels, not behind the caller's stream."""
    e = eng
    e.strict_range = False
    e.set_overlap(overlap)
    try:
        H, W, Hs, Ws = sc.SIZES["small"]
        c, s = sc.image(sc.SEED, H, W), sc.image(sc.SEED + 1, Hs, Ws)
        c_bad, s_bad = c.clone(), s.clone()
        c_bad[0, 1, H // 2, W // 3] = 1e6
        s_bad[0, 1, Hs // 2, Ws // 3] = 1e6
        e.saturation_count(reset=True)

        wrong = []                        # every step is looked at, so that one silent entry point does not hide the next

        def step(what, over, fn):
            out = fn()
            torch.cuda.synchronize()
            n = _poll(e)
            if (n > 0) != over:
                wrong.append("%s: wct_range_poll = %d after the device has drained" % (what, n))
            assert (e.saturation_count(reset=True) > 0) == over, what
            assert _poll(e) == 0
            return out

        for levels in ((5, 4, 3, 2, 1), (4,), (1,)):
            step("style_prepare%s of a 1e6 style" % (levels,), True, lambda: e.style_prepare(s_bad, levels=levels))
        step("style_prepare", False, lambda: e.style_prepare(s))
        for L in (4, 1):                  # the layer-wise encoder, and the fused level-1 moments
            step("content_encode(%d) of a 1e6 content" % L, True, lambda: e.content_encode(L, c_bad))
            h, w, sm, ss = step("content_encode(%d)" % L, False, lambda: e.content_encode(L, c))
            M, b = step("content_solve(%d)" % L, False, lambda: e.content_solve(L, float(h * w), sm, ss, alpha=0.9))
            step("content_decode(%d)" % L, False, lambda: e.content_decode(L, M, b, H, W))
            if L > 1:                     # (level 1 decodes in one conv that writes fp32: nothing behind it is stored split)
                e.content_encode(L, c)
                step("content_decode(%d) of a 1e6 map" % L, True, lambda: e.content_decode(L, M * 1e6, b, H, W))
        assert not wrong, "overlap %d: %s" % (overlap, "; ".join(wrong))
    finally:
        e.set_overlap(1)
        e.saturation_count(reset=True)
