"""Video mode on the device (include/wct_hip_video.h): the tracking step against numpy bit for bit, the temporal blend against fp64 inside
its first-order bound, and wct_stylize_clip against wct_stylize_prepared and against the compositions of public calls written out here,
with its graph, allocation, isolation and refusal behaviour."""
import ctypes
import subprocess
import sys
from ctypes import byref, c_void_p

import numpy as np
import pytest

from tests import state_cases as sc
from tests import video_oracle as O
from tests.conftest import PKG, REPO
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu
STYLE = (84, 108)
SIZES = [(96, 128), (100, 135)]          # the second is cropped to 96 x 128 by the cascade, with strides that differ
INF = float("inf")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "-m gpu tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def wct(torch):
    eng = sc.make_engine("16x")
    eng.style_prepare(sc.image(90, *STYLE))
    return eng


def shape_id(v):
    return "x".join(str(t) for t in v) if isinstance(v, tuple) else str(v)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------- 1. tracking, bitwise
def sums_of(rng, C, n, scale=1.0, shift=0.0, base=None):
    X = (rng.random((C, n)) if base is None else base) * scale + shift
    return X.sum(1), X @ X.T, X


class RawClip:
    """A clip through the C ABI with `C` channels at every level (the "clip_channels" test key)."""

    def __init__(self, torch, wct, C, rate, cut):
        self.t, self.w, self.C = torch, wct, C
        wct.debug_set("clip_channels", C)
        self.h = c_void_p()
        p = _lib.WctClipParams(rate, cut, 0.6, 0.05, 2)
        wct._chk(wct._lib.wct_clip_create(wct._ctx, 96, 128, byref(p), byref(self.h)))
        wct.debug_set("clip_channels", 0)

    def track(self, level, decide, s, ss):
        t, w = self.t, self.w
        sd, ssd = t.from_numpy(np.ascontiguousarray(s)).cuda(), t.from_numpy(np.ascontiguousarray(ss)).cuda()
        w._stream()
        w._chk(w._lib.wct_moments_track(w._ctx, self.h, level, decide, sd.data_ptr(), ssd.data_ptr()))
        rs, rss = t.empty(self.C, device="cuda", dtype=t.float64), t.empty((self.C, self.C), device="cuda", dtype=t.float64)
        fl = t.empty(2, device="cuda", dtype=t.int32)
        w._chk(w._lib.wct_clip_export(w._ctx, self.h, level, rs.data_ptr(), rss.data_ptr(), fl.data_ptr()))
        t.cuda.synchronize()
        got = (sd.cpu().numpy(), ssd.cpu().numpy())
        assert same_bits(got[0], rs.cpu().numpy()) and same_bits(got[1], rss.cpu().numpy())     # what was committed is what was returned
        return got, [int(v) for v in fl.cpu()]

    def close(self):
        self.w._lib.wct_clip_destroy(self.w._ctx, self.h)


@pytest.mark.parametrize("rate", [1.0, 0.25])
@pytest.mark.parametrize("C", [1, 17, 24, 64, 128, 512])
def test_track_against_numpy_bitwise(torch, wct, C, rate):
    """First frame, not-cut, cut, decide = 0 behind a stored flag of either value, NaN sums.  n of level 5 at 96 x 128 is 48, of level 4
    192.  The decisions' input condition: |D - cut| >= 1e-6 cut in the oracle, so the reduction order cannot flip one."""
    cut_thr, n5, n4 = 0.5, 48.0, 192.0
    rng = np.random.default_rng(100 + C)
    clip = RawClip(torch, wct, C, rate, cut_thr)
    try:
        def decided(c, r, frames):
            cut, D = O.decision(n5, c[0], r[0], r[1], frames, cut_thr)
            assert frames == 0 or abs(D - cut_thr) >= 1e-6 * cut_thr, D
            return cut
        zero = (np.zeros(C), np.zeros((C, C)))
        # first frame: a cut whatever D is
        s0, ss0, X0 = sums_of(rng, C, 48)
        assert decided((s0, ss0), zero, 0)
        r5, fl = clip.track(5, 1, s0, ss0)
        assert same_bits(r5[0], s0) and same_bits(r5[1], ss0) and fl == [1, 1]
        # a small change: no cut, the exponential average
        c1 = sums_of(rng, C, 48, base=X0 + 0.01 * rng.random((C, 48)))[:2]
        assert not decided(c1, r5, 1)
        want = (O.track(r5[0], c1[0], rate, False), O.track(r5[1], c1[1], rate, False))
        r5, fl = clip.track(5, 1, *c1)
        assert same_bits(r5[0], want[0]) and same_bits(r5[1], want[1]) and fl == [2, 0]
        # decide = 0 at level 4 behind the stored flag 0: averaged against that level's (still zero) running sums
        c4 = sums_of(rng, C, 192)[:2]
        want = (O.track(zero[0], c4[0], rate, False), O.track(zero[1], c4[1], rate, False))
        r4, fl = clip.track(4, 0, *c4)
        assert same_bits(r4[0], want[0]) and same_bits(r4[1], want[1]) and fl == [3, 0]
        # the same sums again: c == r gives r when they are equal (rate 1 made them so)
        if rate == 1.0:
            again, _ = clip.track(4, 0, *r4)
            assert same_bits(again[0], r4[0]) and same_bits(again[1], r4[1])
        # another scene: a cut, r' = c
        c2 = sums_of(rng, C, 48, scale=3.0, shift=2.0)[:2]
        assert decided(c2, r5, 4)
        r5, fl = clip.track(5, 1, *c2)
        assert same_bits(r5[0], c2[0]) and same_bits(r5[1], c2[1]) and fl[1] == 1
        # decide = 0 behind the stored flag 1: r' = c
        c4b = sums_of(rng, C, 192)[:2]
        r4, fl = clip.track(4, 0, *c4b)
        assert same_bits(r4[0], c4b[0]) and same_bits(r4[1], c4b[1]) and fl[1] == 1
        # NaN sums count as a cut
        c3 = (c2[0].copy(), c2[1].copy())
        c3[0][0] = np.nan
        assert O.decision(n5, c3[0], r5[0], r5[1], 7, cut_thr)[0]
        r5, fl = clip.track(5, 1, *c3)
        assert same_bits(r5[0], c3[0]) and same_bits(r5[1], c3[1]) and fl[1] == 1
        assert n4 == 4 * n5
    finally:
        clip.close()
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 2. blend against fp64
BLEND_SHAPES = [((1, 1), (1, 1)), ((37, 53), (41, 60)), ((O.TILE_H - 1, O.TILE_W - 1), (O.TILE_H + 3, O.TILE_W + 7)),
                ((O.TILE_H, O.TILE_W), (O.TILE_H + 4, O.TILE_W + 8)), ((O.TILE_H + 1, O.TILE_W + 1), (O.TILE_H + 1, O.TILE_W + 1)),
                ((96, 128), (100, 135)), ((96, 128), (96, 128))]


def carve(torch, a, shift, fill=-7.0):
    """`a` as a view `shift` floats into a larger buffer filled with `fill` (4-byte alignment for odd shifts) -> (view, buffer)"""
    n = a.size
    buf = torch.full((n + 8,), fill, device="cuda", dtype=torch.float32)
    view = buf[shift:shift + n].view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    return view, buf


@pytest.mark.parametrize("out_shape,content_shape", BLEND_SHAPES, ids=shape_id)
def test_blend_against_fp64(torch, wct, out_shape, content_shape):
    """Radius 0, 2 and 8 (larger than the smallest images), the cut flag 0, 1 and NULL, 16-byte and 4-byte aligned views, the uint8 image
    of both round modes, and guard values around the outputs.  Sizes: one pixel, an odd one, one below / at / one above the 64 x 16
    tile in each axis, and the frame sizes of the other tests."""
    Ho, Wo = out_shape
    blend, sigma = 0.6, 0.05
    cur = O.image(content_shape, 11)
    prev = (cur[:, :Ho, :Wo] + 0.03 * (O.image(out_shape, 12) - 0.5)).astype(np.float32)
    s, p = O.image(out_shape, 13), O.image(out_shape, 14)
    flags = {0: torch.zeros(1, device="cuda", dtype=torch.int32), 1: torch.ones(1, device="cuda", dtype=torch.int32), None: None}
    worst = 0.0
    for shift in (0, 1):
        (c_d, _), (q_d, _), (s_d, _), (p_d, _) = (carve(torch, a, shift) for a in (cur, prev, s, p))
        for radius in (0, 2, 8):
            bound = O.blend_bound(radius, blend, p, s)
            for key, flag in flags.items():
                want = O.blend(cur, prev, s, p, blend, sigma, radius, cut=bool(key))
                out_v, out_buf = carve(torch, np.zeros((3, Ho, Wo), np.float32), shift)
                for round_mode in (0, 1):
                    out_buf.fill_(-7.0)
                    got, hwc = wct.temporal_blend(c_d, q_d, s_d, p_d, blend, sigma, radius, cut_flag=flag, out=out_v, u8=True, round_mode=round_mode)
                    torch.cuda.synchronize()
                    assert got.data_ptr() == out_v.data_ptr()
                    assert bool((out_buf[:shift] == -7.0).all()) and bool((out_buf[shift + 3 * Ho * Wo:] == -7.0).all())   # nothing past either end
                    dist = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
                    worst = max(worst, dist / bound)
                    assert dist <= bound, (shift, radius, key, dist, bound)
                    if key:
                        assert torch.equal(got[0], s_d)                                                  # a cut: s itself
                    assert torch.equal(hwc, wct.to_u8(got, round_mode)), (shift, radius, key, round_mode)
                plain = wct.temporal_blend(c_d, q_d, s_d, p_d, blend, sigma, radius, cut_flag=flag)      # without the uint8 image: the same floats
                assert torch.equal(plain, got)
        # p == s gives s
        assert torch.equal(wct.temporal_blend(c_d, q_d, s_d, s_d.clone(), blend, sigma, 2)[0], s_d)
    print("blend %s in %s: worst distance / bound %.3g" % (out_shape, content_shape, worst))
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. frame identities
@pytest.mark.parametrize("size", SIZES, ids=shape_id)
def test_frame_identities_against_stylize_prepared(torch, wct, size):
    H, W = size
    A, B, Cc = (sc.image(seed, H, W) for seed in (1, 2, 3))
    want = {k: wct.stylize_prepared(x, alpha=0.6).clone() for k, x in (("A", A), ("B", B), ("C", Cc))}
    # (a) the first frame and the frame after reset
    clip = wct.clip(H, W, rate=0.25, cut=0.5, blend=0.6)
    assert torch.equal(clip.stylize(A, alpha=0.6), want["A"])
    clip.stylize(B, alpha=0.6)
    clip.reset()
    assert torch.equal(clip.stylize(Cc, alpha=0.6), want["C"])
    clip.close()
    # (b) rate 1, blend 0: every frame; the uint8 image is to_u8 of the float one
    clip = wct.clip(H, W, rate=1.0, cut=INF, blend=0.0)
    for k, x in (("A", A), ("B", B), ("C", Cc), ("A", A)):
        got, hwc = clip.stylize(x, alpha=0.6, u8=True, round_mode=1)
        assert torch.equal(got, want[k]), k
        assert torch.equal(hwc, wct.to_u8(got, 1))
    clip.close()
    # (c) cut = 0 with differing frames: every frame is a cut
    clip = wct.clip(H, W, rate=0.25, cut=0.0, blend=0.6)
    for k, x in (("A", A), ("B", B), ("C", Cc)):
        assert torch.equal(clip.stylize(x, alpha=0.6), want[k]), k
    assert int(clip.export(5)[2][1]) == 1
    clip.close()
    # (d) the same frame four times
    clip = wct.clip(H, W, rate=0.25, cut=INF, blend=0.6)
    for i in range(4):
        assert torch.equal(clip.stylize(A, alpha=0.6), want["A"]), i
    flags = clip.export(5)[2]
    assert [int(v) for v in flags.cpu()] == [4, 0]
    clip.close()
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 4. the blend half
def test_blend_half_is_the_composition_of_public_calls(torch, wct):
    """rate = 1: the cascade is wct_stylize_prepared's, so frame t = wct_temporal_blend(content_t, content_{t-1}, prepared(content_t), out_{t-1})."""
    H, W, Ho, Wo = 100, 135, 96, 128
    base = sc.image(5, H, W)
    frames = [base, (base + 0.02 * (sc.image(6, H, W) - 0.5)).clamp(0, 1), (base + 0.05 * (sc.image(7, H, W) - 0.5)).clamp(0, 1)]
    clip = wct.clip(H, W, rate=1.0, cut=INF, blend=0.6, sigma=0.05, radius=2)
    prev_c = prev_o = None
    moved = 0.0
    for t, x in enumerate(frames):
        got = clip.stylize(x, alpha=0.6).clone()
        sty = wct.stylize_prepared(x, alpha=0.6).clone()
        want = sty if t == 0 else wct.temporal_blend(x, prev_c, sty, prev_o, 0.6, 0.05, 2)
        assert torch.equal(got, want), t
        if t:
            moved = max(moved, float((got - sty).abs().max()))
        prev_c, prev_o = x[:, :, :Ho, :Wo].contiguous(), got
    clip.close()
    assert moved > 1e-3            # the blend did something
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 5. the track half
def test_track_half_against_the_split_composition(torch, wct):
    """blend = 0, rate = 0.25, cut = +inf; frames A and B = 0.5 A' + 0.25.  The output for B against content_encode -> numpy track with the sums
    kept from A -> content_solve -> content_decode per level, within 5e-4 max|ref| (the split-vs-fused bound of tests/test_sharded_gpu.py);
    the same comparison at rate = 1 (paths that exist without this feature) meets the bound too, and prepared(B) is at least ten bounds
    away from the expectation: the test cannot pass without the smoothing."""
    H, W, rate, alpha = 96, 128, 0.25, 0.6
    A = sc.image(21, H, W)
    B = 0.5 * sc.image(22, H, W) + 0.25

    def composition(x, kept, rate):
        cur, sums = x, {}
        for level in (5, 4, 3, 2, 1):
            h, w, s, ss = wct.content_encode(level, cur)
            s, ss = s.cpu().numpy(), ss.cpu().numpy()
            sums[level] = (s, ss)
            if kept is not None:
                s, ss = O.track(kept[level][0], s, rate, False), O.track(kept[level][1], ss, rate, False)
                sums[level] = (s, ss)
            M, b = wct.content_solve(level, float(h * w), torch.from_numpy(s), torch.from_numpy(ss), alpha)
            cur = wct.content_decode(level, M, b, int(cur.shape[2]), int(cur.shape[3]))
        return cur.clone(), sums

    _, kept = composition(A, None, rate)
    raw5 = {}
    for k, x in (("A", A), ("B", B)):
        _, _, s, ss = wct.content_encode(5, x)
        raw5[k] = (s.cpu().numpy(), ss.cpu().numpy())
    expected, _ = composition(B, kept, rate)
    plain_split, _ = composition(B, None, 1.0)
    prepared_b = wct.stylize_prepared(B, alpha=alpha).clone()

    clip = wct.clip(H, W, rate=rate, cut=INF, blend=0.0)
    clip.stylize(A, alpha=alpha)
    got = clip.stylize(B, alpha=alpha).clone()
    s5, ss5, flags = clip.export(5)
    clip.close()
    assert [int(v) for v in flags.cpu()] == [2, 0]
    assert same_bits(s5.cpu().numpy(), O.track(raw5["A"][0], raw5["B"][0], rate, False))
    assert same_bits(ss5.cpu().numpy(), O.track(raw5["A"][1], raw5["B"][1], rate, False))

    bound = 5e-4 * float(expected.abs().max())
    d_track = float((got - expected).abs().max())
    d_plain = float((prepared_b - plain_split).abs().max())
    d_apart = float((prepared_b - expected).abs().max())
    print("track half: fused vs split %.3g, rate-1 yardstick %.3g, bound %.3g, prepared(B) vs expected %.3g" % (d_track, d_plain, bound, d_apart))
    assert d_plain <= 5e-4 * float(plain_split.abs().max())
    assert d_track <= bound
    assert d_apart >= 10 * bound
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. graph
def test_one_captured_frame_is_replayed_for_successive_frames():
    """One wct_stylize_clip captured into a HIP graph, replayed for three frames with the content rewritten in place, against three
    direct calls on a second clip.  In a fresh process: a failed capture can leave the runtime in capture mode."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
from tests import state_cases as sc
wct = sc.make_engine("16x")
wct.style_prepare(sc.image(90, 84, 108))
H, W = 100, 135
base = sc.image(1, H, W)
frames = [base, (base + 0.02 * (sc.image(2, H, W) - 0.5)).clamp(0, 1), sc.image(3, H, W)]     # a first frame, a still scene, a cut
direct = wct.clip(H, W, rate=0.25, cut=0.5, blend=0.6)
wants = [direct.stylize(x, alpha=0.6).clone() for x in frames]
cuts = []
torch.cuda.synchronize()
allocs = wct.debug_get("ws_allocs")
clip = wct.clip(H, W, rate=0.25, cut=0.5, blend=0.6)
c = frames[0].clone()
out = torch.empty((1, 3, 96, 128), device="cuda")
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    clip.stylize(c, alpha=0.6, out=out)
for t, x in enumerate(frames):
    c.copy_(x)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, wants[t]), "replay %%d differs" %% t
    cuts.append(int(clip.export(5)[2][1]))
assert cuts[:2] == [1, 0], cuts                                                  # the third is the data's business: the decision is the device's
assert not torch.equal(wants[1], wct.stylize_prepared(frames[1], alpha=0.6))      # the second frame was smoothed
assert wct.debug_get("ws_allocs") == allocs
assert wct.saturation_count() == 0
print("GRAPH_OK")
""" % (REPO, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- 7. isolation
def test_clip_and_context_do_not_see_each_other(torch):
    H, W = 100, 135
    style = sc.image(90, *STYLE)
    base = sc.image(31, H, W)
    frames = [base, (base + 0.02 * (sc.image(32, H, W) - 0.5)).clamp(0, 1), (base + 0.04 * (sc.image(33, H, W) - 0.5)).clamp(0, 1)]
    other, small = sc.image(34, 160, 208), sc.image(35, 48, 64)

    quiet = sc.make_engine("16x")                     # the clip alone
    quiet.style_prepare(style)
    clip = quiet.clip(H, W)
    wants = [clip.stylize(x, alpha=0.6).clone() for x in frames]
    clip.close()
    fresh = sc.make_engine("16x")                     # the other calls alone, and the profile of a plain prepared call
    want_other = fresh.stylize(other, style, alpha=0.6).clone()
    want_small = fresh.resample(small, (96, 128), "bicubic").clone()
    fresh.style_prepare(style)
    fresh.profile(True)
    fresh.profile_reset()
    fresh.stylize_prepared(frames[0], alpha=0.6)
    plain_before = {r["name"] for r in fresh.profile_read()}
    fresh.profile(False)

    busy = sc.make_engine("16x")
    busy.style_prepare(style)
    clip = busy.clip(H, W)
    for t, x in enumerate(frames):
        assert torch.equal(clip.stylize(x, alpha=0.6), wants[t]), t
        assert torch.equal(busy.stylize(other, style, alpha=0.6), want_other)      # the same style: the prepared slots are rewritten with the same bits
        assert torch.equal(busy.resample(small, (96, 128), "bicubic"), want_small)
    allocs = busy.debug_get("ws_allocs")
    busy.profile(True)
    busy.profile_reset()
    clip.stylize(frames[2], alpha=0.6)
    with_clip = {r["name"] for r in busy.profile_read()}
    busy.profile_reset()
    busy.stylize_prepared(frames[0], alpha=0.6)
    plain_after = {r["name"] for r in busy.profile_read()}
    busy.profile(False)
    assert busy.debug_get("ws_allocs") == allocs
    clip.close()
    assert {"clip_track", "temporal_blend", "clip_store"} <= with_clip and with_clip - {"clip_track", "temporal_blend", "clip_store"} == plain_before
    assert plain_after == plain_before and "clip_track" not in plain_after
    assert busy.saturation_count() == 0 and quiet.saturation_count() == 0 and fresh.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_name_the_entry_and_write_nothing(torch, wct):
    H, W = 96, 128
    clip = wct.clip(H, W)
    x = sc.image(41, H, W)
    out = torch.full((1, 3, H, W), -3.0, device="cuda")
    with pytest.raises(ValueError, match="wct_stylize_clip"):                       # a frame of another size
        clip.stylize(sc.image(42, 112, 128), out=out)
    buf = torch.rand(3 * H * W + 64, device="cuda")
    with pytest.raises(ValueError, match="wct_stylize_clip.*overlaps"):             # out over the content
        clip.stylize(buf[:3 * H * W].view(1, 3, H, W), out=buf[64:64 + 3 * H * W])
    other = sc.make_engine("16x")
    other.style_prepare(sc.image(90, *STYLE))
    ho, wo = ctypes.c_int(), ctypes.c_int()
    other._stream()
    rc = other._lib.wct_stylize_clip(other._ctx, clip._handle(), x.data_ptr(), H, W, 0.6, out.data_ptr(), None, 0, byref(ho), byref(wo))
    assert rc == _lib.WCT_ERR_INVALID and "wct_stylize_clip" in other._lib.wct_last_error(other._ctx).decode()      # a clip of another context
    bare = sc.make_engine("16x")                                                    # no style statistics
    bare_clip = bare.clip(H, W)
    with pytest.raises(_lib.WctError) as e:
        bare_clip.stylize(x, out=out)
    assert e.value.code == _lib.WCT_ERR_STATE and "wct_stylize_clip" in str(e.value)
    bare_clip.close()
    wide = sc.make_engine("wide")                                                   # --mode original: refused, documented
    wide.style_prepare(sc.image(90, *STYLE))
    wide_clip = wide.clip(H, W)
    with pytest.raises(_lib.WctError) as e:
        wide_clip.stylize(x, out=out)
    assert e.value.code == _lib.WCT_ERR_STATE and "wide" in str(e.value)
    wide_clip.close()
    for bad in (dict(rate=0.0), dict(rate=1.5), dict(cut=-1.0), dict(cut=float("nan")), dict(blend=1.0), dict(sigma=0.0), dict(radius=9)):
        with pytest.raises(ValueError, match="wct_clip_create"):
            wct.clip(H, W, **bad)
    with pytest.raises(ValueError, match="wct_clip_create"):
        wct.clip(31, 128)
    s = sc.image(43, H, W)
    with pytest.raises(ValueError, match="wct_temporal_blend"):
        wct.temporal_blend(x, x.clone(), s, s.clone(), 0.6, 0.05, 9)
    with pytest.raises(ValueError, match="wct_temporal_blend.*overlaps"):
        wct.temporal_blend(x, x.clone(), s, s.clone(), 0.6, 0.05, 2, out=s.view(-1))
    torch.cuda.synchronize()
    assert bool((out == -3.0).all())                                                # nothing was written by any refused call
    assert torch.equal(clip.stylize(x, alpha=0.6), wct.stylize_prepared(x, alpha=0.6))      # and the clip is still at its first frame
    clip.close()
    assert wct.saturation_count() == 0
