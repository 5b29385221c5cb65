"""Does a call return the same bits whatever the context did before it?

Every case of tests/state_cases.py has a *control*: its outputs on a fresh engine (a new wct_ctx).  The arms below run the same
cases on engines with a past -- a poisoned workspace, other sizes and entry points, refused calls, mode switches, other streams,
other contexts, a reserve -- and compare every output with the control by torch.equal.  Nothing here has a tolerance.

Arm a found every case reproducible fresh against fresh; no case is compared through an fp64 gate instead."""
import ctypes
import gc

import numpy as np
import pytest

from tests import state_cases as sc
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

POISON = (0xFF, 0x3C)      # NaN in every float format, 255 as a label or pixel, -1 as a counter / ~1.06 as f16, ~0.0115 as fp32: finite, plausible


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


class Controls:
    """name -> outputs of the case on a fresh engine of its own, computed once per module run."""

    def __init__(self, torch):
        self.t, self.c = torch, {}

    def __call__(self, kind, name):
        if (kind, name) not in self.c:
            eng = sc.make_engine(kind)
            out = sc.run(eng, name)
            self.t.cuda.synchronize()
            clean(eng, "control of %s on %s" % (name, kind))
            self.c[kind, name] = out
        return self.c[kind, name]

    def custom(self, key, fn, kind="16x", w=None):
        """Control of a call sequence that is not a catalogue case: fn(fresh engine) -> outputs."""
        if key not in self.c:
            eng = sc.make_engine(kind, w)
            out = fn(eng)
            self.t.cuda.synchronize()
            clean(eng, "control %s" % (key,))
            self.c[key] = out
        return self.c[key]


@pytest.fixture(scope="module")
def controls(torch):
    return Controls(torch)


def clean(eng, what):
    """No f16x3 clamp was counted and none is reported: a range flag raised by stale workspace contents is a failure."""
    n = ctypes.c_ulonglong()
    assert eng.saturation_count() == 0, "%s: saturation counter %d" % (what, eng.saturation_count())
    eng._chk(eng._lib.wct_range_poll(eng._ctx, ctypes.byref(n)))
    assert n.value == 0, "%s: wct_range_poll reports %d" % (what, n.value)


def same(torch, got, want, what):
    torch.cuda.synchronize()
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    bad = []
    for k in sorted(want):
        g, w = got[k], want[k]
        if g.shape != w.shape or g.dtype != w.dtype or not torch.equal(g, w):
            if g.shape == w.shape and g.is_floating_point():
                d = (g.double() - w.double()).abs()
                nan = int(torch.isnan(g).sum())
                bad.append("%s: %d of %d values differ, max |diff| %.3e, %d NaN" % (k, int((g != w).sum()), g.numel(), float(d[~torch.isnan(d)].max()) if nan < g.numel() else float("nan"), nan))
            elif g.shape == w.shape:
                bad.append("%s: %d of %d values differ" % (k, int((g != w).sum()), g.numel()))
            else:
                bad.append("%s: shape %s, control %s" % (k, tuple(g.shape), tuple(w.shape)))
    assert not bad, "%s differs from its control on a fresh engine: %s" % (what, "; ".join(bad))


def check(torch, controls, eng, name, what):
    same(torch, sc.run(eng, name), controls(eng.state_kind, name), "%s [%s, %s engine]" % (name, what, eng.state_kind))
    clean(eng, "%s [%s]" % (name, what))


ALL = [(k, n) for k in ("16x", "wide") for n in sc.names(k)]


# ------------------------------------------------------------------------------------------------ a. control
@pytest.mark.parametrize("kind,name", ALL, ids=["%s-%s" % kn for kn in ALL])
def test_a_fresh_engines_agree(torch, controls, kind, name):
    """The claim every other arm leans on: a case on two fresh engines, bit for bit."""
    check(torch, controls, sc.make_engine(kind), name, "second fresh engine")


# ------------------------------------------------------------------------------------------------ b. poison
def _other(kind, name):
    """A case of a DIFFERENT family: its large variant on the 16x engine, another small one on the wide engine."""
    pool = sc.names(kind, "large") if kind == "16x" else sc.names(kind)
    fams = [n for n in pool if sc.CASES[n].family != sc.CASES[name].family]
    return fams[(sc.names(kind).index(name) * 7 + 3) % len(fams)]


SMALL = [(k, n) for k in ("16x", "wide") for n in sc.names(k, "small")]


@pytest.mark.parametrize("byte", POISON, ids=["ff", "3c"])
@pytest.mark.parametrize("kind,name", SMALL, ids=["%s-%s" % kn for kn in SMALL])
def test_b_poisoned_workspace(torch, controls, kind, name, byte):
    """Every scratch buffer filled with the byte (allocations made later too): the case, the large variant of another family, poison
    again, the case again.  A kernel that reads what its producer did not write shows here."""
    eng = sc.make_engine(kind)
    eng.debug_set("poison", byte)
    check(torch, controls, eng, name, "poison 0x%02X on a fresh engine" % byte)
    other = _other(kind, name)
    check(torch, controls, eng, other, "poison 0x%02X, after %s" % (byte, name))
    eng.debug_set("poison", byte)
    check(torch, controls, eng, name, "poison 0x%02X again after %s" % (byte, other))
    eng.debug_set("poison", -1)


# ------------------------------------------------------------------------------------------------ c. history
def _load_decoder(eng, level, w):
    """wct_load_module of ONE decoder (wct_hip.WCT loads all ten at construction)."""
    from wct_hip import model_zoo
    layers = model_zoo.decoder_layers(eng.mode, level)
    arr = (_lib.WctLayer * len(layers))()
    hold = []
    fp = ctypes.POINTER(ctypes.c_float)
    for i, l in enumerate(layers):
        wt = np.ascontiguousarray(w["d%d.%s.weight" % (level, l.name)], np.float32)
        bs = np.ascontiguousarray(w["d%d.%s.bias" % (level, l.name)], np.float32)
        hold += [wt, bs]
        arr[i] = _lib.WctLayer(l.cin, l.cout, int(l.pool_after), int(l.up_after), wt.ctypes.data_as(fp), bs.ctypes.data_as(fp))
    eng._chk(eng._lib.wct_load_module(eng._ctx, _lib.KIND_DEC, level, len(layers), arr, None, None))


N_REFUSED = 9


def _refused(torch, eng, which):
    """Calls the library refuses, some of them after kernels were enqueued: they must leave no trace."""
    H, W = 70, 90
    c, s = sc.image(1, H, W), sc.image(2, 64, 80)
    K = 3
    lab = sc.label_map(H, W, K)
    with pytest.raises((ValueError, _lib.WctError)):
        if which == 0:      # content below 32 pixels
            eng.stylize_regions(sc.image(3, 24, 90), [s], sc.label_map(24, 90, 1))
        elif which == 1:    # K = 0
            eng.stylize_interp(c, [], [])
        elif which == 2:    # K = 9
            eng.stylize_regions(c, [s] * 9, sc.label_map(H, W, 9))
        elif which == 3:    # weights that sum to 0
            eng.stylize_interp(c, [s, s], [0.0, 0.0])
        elif which == 4:    # a NaN in a weight map: refused after the pooling kernel ran
            wm = sc.weight_maps(4, 2, H, W)
            wm[1, 5, 7] = float("nan")
            eng.stylize_blend(c, [s, s], wm)
        elif which == 5:    # a label above K: refused after the label kernel ran
            bad = lab.clone()
            bad[3, 4] = K + 1
            eng.stylize_regions(c, [s] * K, bad)
        elif which == 6:    # a channel count no kernel takes
            eng.moments(sc.feature(5, 9, 11, 6))
        elif which == 7:    # a feature map of another model's width
            eng.decode(3, sc.feature(5, 9, 11, sc.channels(eng, 3) + 4), layout="nhwc")
        else:               # wct_content_decode without its wct_content_encode (the catalogue's split case ends at level 1)
            C = sc.channels(eng, 2)
            M, b = sc.affine(6, 1, C)
            eng.content_decode(2, M[0], b[0], H, W)
    return which


def _action(torch, eng, rng):
    """Something between two cases that changes host-side or device-side state and is undone before the next comparison."""
    which = int(rng.integers(0, 8))
    small = lambda: eng.stylize(sc.image(7, 72, 88), sc.image(8, 66, 70))
    if which == 0:
        eng.set_conv_mode("fp32"); small(); eng.set_conv_mode("f16x3")
    elif which == 1:
        eng._chk(eng._lib.wct_set_numpy_variant(eng._ctx, 1)); small(); eng._chk(eng._lib.wct_set_numpy_variant(eng._ctx, 0))
    elif which == 2:
        eng.set_overlap(False); small(); eng.set_overlap(True)
    elif which == 3:
        key = ("fuse", "sp", "l1fuse", "u8fuse", "upconv", "fastfold", "interleave", "foldgemm")[int(rng.integers(0, 8))]
        eng.debug_set(key, 0); small(); eng.stylize_u8(sc.image_u8(9, 64, 80), sc.image_u8(10, 48, 64)); eng.debug_set(key, 1)
        return "debug %s" % key
    elif which == 4:
        eng.profile(True); eng.profile_reset(); small()
        assert eng.profile_read()
        eng.profile_reset(); eng.profile(False)
    elif which == 5:
        assert eng.saturation_count(reset=True) == 0
    elif which == 6:
        eng.sync()
        assert eng._lib.wct_version() >= 1 and eng.style_stats_count(5) == sc.channels(eng, 5) ** 2 + sc.channels(eng, 5)
        assert eng.feature_shape(3, 100, 130)[1:] == (25, 32) and eng.resize_shape(100, 130, 50) == (50, 65)
    else:
        return "refused call %d" % _refused(torch, eng, int(rng.integers(0, N_REFUSED)))
    return "action %d" % which


@pytest.mark.parametrize("kind,draws", [("16x", 28), ("wide", 6)])
def test_c_drawn_history(torch, controls, kind, draws):
    """ONE engine, a seeded sequence of cases with actions and refused calls between them; every case against its control."""
    rng = np.random.default_rng(31 if kind == "16x" else 32)
    eng = sc.make_engine(kind)
    small, large = sc.names(kind, "small"), sc.names(kind, "large")
    past = []
    for i in range(draws):
        pool = large if (large and rng.random() < 0.25) else small
        name = pool[int(rng.integers(0, len(pool)))]
        check(torch, controls, eng, name, "step %d after %s" % (i, past[-6:]))
        past.append(name)
        for _ in range(int(rng.integers(0, 3))):
            past.append(_action(torch, eng, rng))
    check(torch, controls, eng, small[0], "last step after %s" % past[-6:])


@pytest.mark.parametrize("kind", ["16x", "wide"])
def test_c_refused_calls_leave_no_trace(torch, controls, kind):
    """Every kind of refused call once, each followed by cases that share its buffers."""
    eng = sc.make_engine(kind)
    after = ["regions/small", "interp/small", "stylize/small", "split_level/small"]
    for which in range(N_REFUSED):
        assert _refused(torch, eng, which) == which
        check(torch, controls, eng, after[which % len(after)], "after refused call %d" % which)
    if kind == "16x":
        check(torch, controls, eng, "blend/small", "after all refused calls")


def test_c_large_small_large_and_k_sequences(torch, controls):
    """By construction: large -> small -> large of one entry; K = 8 -> 2 -> 8 for the regions and the weights cascade."""
    eng = sc.make_engine("16x")
    for fam in ("stylize", "level", "encode_decode", "stylize_u8", "synthesize"):
        for size in ("large", "small", "large"):
            check(torch, controls, eng, "%s/%s" % (fam, size), "large-small-large")
    H, W = sc.SIZES["small"][:2]
    c = sc.image(40, H, W)
    regions = lambda K: (lambda e: {"out": e.stylize_regions(c, sc.styles(41, K, "small"), sc.label_map(H, W, K), alpha=0.9)})
    blend = lambda K: (lambda e: {"out": e.stylize_blend(c, sc.styles(41, K, "small"), sc.weight_maps(42, K, H, W), alpha=0.9)})
    for tag, make in (("regions", regions), ("blend", blend)):
        for K in (8, 2, 8):
            want = controls.custom((tag, K), make(K))
            same(torch, make(K)(eng), want, "%s K = %d in the sequence 8, 2, 8" % (tag, K))
            clean(eng, "%s K = %d" % (tag, K))


def test_c_prepared_style_slot_lifetime(torch, controls):
    """include/wct_hip.h, 'Lifetime of the prepared statistics': wct_stylize_interp rewrites the slot and a later wct_style_prepare
    replaces it again; wct_stylize_regions, wct_stylize_blend and wct_synthesize WITHOUT a texture leave it alone; wct_synthesize WITH a
    texture leaves the texture's statistics there."""
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s, tex = sc.image(50, H, W), sc.image(51, Hs, Ws), sc.image(52, Hs - 9, Ws + 11)
    eng = sc.make_engine("16x")
    prepared = lambda style: (lambda e: (e.style_prepare(style), {"out": e.stylize_prepared(c, alpha=0.9)})[1])
    want_s = controls.custom("prepared s", prepared(s))
    want_tex = controls.custom("prepared tex", prepared(tex))
    check(torch, controls, eng, "interp/small", "before style_prepare")
    same(torch, prepared(s)(eng), want_s, "style_prepare + stylize_prepared after stylize_interp")
    eng.style_prepare(s)
    check(torch, controls, eng, "regions/small", "between style_prepare and stylize_prepared")
    same(torch, {"out": eng.stylize_prepared(c, alpha=0.9)}, want_s, "stylize_prepared after stylize_regions")
    check(torch, controls, eng, "blend/small", "between style_prepare and stylize_prepared")
    same(torch, {"out": eng.stylize_prepared(c, alpha=0.9)}, want_s, "stylize_prepared after stylize_blend")
    eng.synthesize(None, H, W, seed=5)
    same(torch, {"out": eng.stylize_prepared(c, alpha=0.9)}, want_s, "stylize_prepared after synthesize without a texture")
    eng.synthesize(tex, H, W, seed=5)
    same(torch, {"out": eng.stylize_prepared(c, alpha=0.9)}, want_tex, "stylize_prepared after synthesize with a texture (the slot holds the texture)")
    clean(eng, "slot lifetime")


def test_c_fold_state_follows_the_switches(torch, controls):
    """The style-side fold (foldS, fold_ready) belongs to one decoder and one fastfold setting: style_prepare under fastfold = 1, the
    content side under fastfold = 0 and exact fp32, and back; then another decoder 3 loaded after style_prepare, against a fresh engine
    built with those weights."""
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(60, H, W), sc.image(61, Hs, Ws)

    def slow_content(e, fastfold_at_prepare):
        e.debug_set("fastfold", fastfold_at_prepare)
        e.style_prepare(s)
        e.debug_set("fastfold", 0)
        e.set_conv_mode("fp32")
        out = {"out": e.stylize_prepared(c)}
        e.set_conv_mode("f16x3")
        e.debug_set("fastfold", 1)
        return out

    eng = sc.make_engine("16x")
    want = controls.custom("fold never built", lambda e: slow_content(e, 0))
    same(torch, slow_content(eng, 1), want, "content side under fastfold = 0 / fp32 after style_prepare under fastfold = 1")
    want = controls.custom("prepared default", lambda e: (e.style_prepare(s), {"out": e.stylize_prepared(c)})[1])
    same(torch, {"out": eng.stylize_prepared(c)}, want, "back under fastfold = 1 / f16x3, same prepared style")
    w2 = dict(sc.weights("16x"))
    rng = np.random.default_rng(62)
    for k in [k for k in w2 if k.startswith("d3.")]:
        w2[k] = (w2[k] * (1.0 + 0.1 * rng.standard_normal(w2[k].shape))).astype(np.float32)
    want = controls.custom("decoder 3 replaced", lambda e: (e.style_prepare(s), {"out": e.stylize_prepared(c)})[1], w=w2)
    eng.style_prepare(s)
    _load_decoder(eng, 3, w2)
    same(torch, {"out": eng.stylize_prepared(c)}, want, "stylize_prepared after wct_load_module replaced decoder 3 behind style_prepare")
    clean(eng, "fold state")


def test_c_aborted_single_launch_solves_leave_no_trace(torch, controls):
    """nscoop = 2 (the injected placement fault of test_single_launch_newton_schulz...) for a few solves, then nscoop = 1."""
    eng = sc.make_engine("16x")
    eng.debug_set("nscoop", 2)
    sc.run(eng, "solve/large")
    sc.run(eng, "stylize/small")
    eng.debug_set("nscoop", 1)
    off = "nscoop_off = %d, aborts = %d" % (eng.debug_get("nscoop_off"), eng.debug_get("nscoop_aborts"))
    assert eng.debug_get("nscoop_aborts") >= 4, off
    for name in ("solve/large", "stylize/small", "prepared/small", "level/large"):
        check(torch, controls, eng, name, "after aborted single-launch solves (%s)" % off)


# ------------------------------------------------------------------------------------------------ d. resize table cache
def test_d_resize_table_cache_eviction(torch, controls):
    """More than 16 distinct (in, out, filter) axes, then the first ones again -- each bit-exact against oracle/resize_oracle.py as
    tests/test_resize.py compares -- with a cascade in flight on the same engine when the evicted tables are freed."""
    from oracle import resize_oracle as R
    eng = sc.make_engine("16x")
    rng = np.random.default_rng(70)
    img = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    x = torch.from_numpy(img).cuda()
    targets = [(40 + 3 * i, 50 + 5 * i) for i in range(12)]         # 24 bilinear axes
    cubic = {}
    for t in targets:
        assert np.array_equal(eng.resize_u8(x, t).cpu().numpy(), R.resize_bilinear_u8(img, *t)), t
        cubic[t] = eng.resize_u8(x, t, filter="bicubic").clone()    # 24 bicubic axes more
    flight = sc.run(eng, "stylize/large")                            # not synchronised: the evictions below free tables under it
    first = [eng.resize_u8(x, t) for t in targets[:6]]
    first_cubic = [eng.resize_u8(x, t, filter="bicubic") for t in targets[:6]]
    same(torch, flight, controls("16x", "stylize/large"), "cascade in flight over resize table evictions")
    for t, got, gc_ in zip(targets, first, first_cubic):
        assert np.array_equal(got.cpu().numpy(), R.resize_bilinear_u8(img, *t)), ("after eviction", t)
        assert torch.equal(gc_, cubic[t]), ("bicubic after eviction", t)
    check(torch, controls, eng, "resize/small", "after the table cache turned over")


# ------------------------------------------------------------------------------------------------ e. streams
def test_e_calls_under_two_streams(torch, controls):
    """include/wct_hip.h wct_set_stream: binding another stream orders it behind the old one.  The larger call under stream 1, then --
    no synchronisation -- another case under stream 2; both sizes warmed up first so that nothing is allocated or freed in the pair."""
    eng = sc.make_engine("16x")
    pairs = [("stylize/large", "level/small"), ("regions/large", "stylize/small"), ("encode_decode/large", "prepared/small")]
    for big, little in pairs:
        sc.run(eng, big), sc.run(eng, little)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for big, little in pairs:
        allocs = eng.debug_get("ws_allocs")
        with torch.cuda.stream(s1):
            a = sc.run(eng, big)
        with torch.cuda.stream(s2):
            b = sc.run(eng, little)
        assert eng.debug_get("ws_allocs") == allocs, "the pair (%s, %s) allocated" % (big, little)
        same(torch, a, controls("16x", big), "%s under stream 1" % big)
        same(torch, b, controls("16x", little), "%s under stream 2, right behind %s under stream 1" % (little, big))
    check(torch, controls, eng, "stylize/small", "back on the default stream")


# ------------------------------------------------------------------------------------------------ f. two contexts
def test_f_two_contexts_interleaved(torch, controls):
    """Two engines alive in one process, calls interleaved A, B, A, B; then A destroyed, C created, again (the process-wide round
    robin of the lanes' XCDs)."""
    a, b = sc.make_engine("16x"), sc.make_engine("16x")
    seq = [("stylize/small", "level/large"), ("regions/small", "stylize/large"), ("solve/large", "prepared/small")]
    for round_ in range(2):
        for na, nb in seq:
            ra = sc.run(a, na)
            rb = sc.run(b, nb)
            same(torch, ra, controls("16x", na), "%s on engine %s, interleaved" % (na, "AC"[round_]))
            same(torch, rb, controls("16x", nb), "%s on engine B, interleaved" % nb)
        clean(a, "engine %s" % "AC"[round_]), clean(b, "engine B")
        del a
        gc.collect()
        a = sc.make_engine("16x")


# ------------------------------------------------------------------------------------------------ g. reserve
@pytest.mark.parametrize("H,W,Hs,Ws", [sc.SIZES["small"], sc.SIZES["large"], (200, 264, 616, 840)])
def test_g_reserve_is_what_the_header_says(torch, controls, H, W, Hs, Ws):
    """include/wct_hip.h: after wct_reserve, wct_stylize / wct_style_prepare / wct_stylize_prepared of that size allocate nothing;
    wct_workspace_bytes is EXACTLY what the workspace of a fresh context holds after the reserve; a smaller reserve is a no-op;
    wct_stylize_u8's staging comes on top."""
    c, s = sc.image(80, H, W), sc.image(81, Hs, Ws)
    plain = lambda e: {"stylize": e.stylize(c, s, alpha=0.8), "prepared": (e.style_prepare(s), e.stylize_prepared(c, num_run=2))[1]}
    want = controls.custom(("reserve", H, W, Hs, Ws), plain)
    eng = sc.make_engine("16x")
    assert eng.debug_get("ws_allocs") == 0 and eng.debug_get("ws_bytes") == 0
    eng.reserve(H, W, Hs, Ws)
    allocs, held = eng.debug_get("ws_allocs"), eng.debug_get("ws_bytes")
    print("reserve %dx%d / %dx%d: %d allocations, %d bytes held, wct_workspace_bytes %d" % (H, W, Hs, Ws, allocs, held, sc.workspace_bytes(eng, H, W, Hs, Ws)))
    assert allocs > 0 and held == sc.workspace_bytes(eng, H, W, Hs, Ws)
    same(torch, plain(eng), want, "stylize / stylize_prepared after reserve")
    assert (eng.debug_get("ws_allocs"), eng.debug_get("ws_bytes")) == (allocs, held), "wct_stylize / wct_stylize_prepared allocated after wct_reserve of their size"
    eng.reserve(H // 2, W // 2, Hs // 2, Ws // 2)
    assert (eng.debug_get("ws_allocs"), eng.debug_get("ws_bytes")) == (allocs, held), "a smaller wct_reserve allocated"
    same(torch, plain(eng), want, "after the smaller reserve")
    eng.stylize_u8(sc.image_u8(82, H, W), sc.image_u8(83, Hs, Ws))
    assert eng.debug_get("ws_allocs") == allocs + 3, "wct_stylize_u8: three staging buffers on top of the reserve, nothing else"
    clean(eng, "reserve")
