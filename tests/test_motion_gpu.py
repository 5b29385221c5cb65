"""Motion compensation on the device (include/wct_hip_motion.h): the luma pyramid and the block-matched field against numpy bit for bit,
the compensated blend against video mode's blend of gathered images bit for bit (and against fp64 inside video mode's bound), and
wct_stylize_clip with motion attached against the compositions of public calls written out here, with its graph, allocation, isolation
and refusal behaviour."""
import subprocess
import sys
from ctypes import byref

import numpy as np
import pytest

from tests import motion_oracle as M
from tests import state_cases as sc
from tests import video_oracle as V
from tests.conftest import PKG, REPO
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu
STYLE = (84, 108)
SIZES = [(96, 128), (100, 135)]          # the second is cropped to 96 x 128 by the cascade, with strides that differ
INF = float("inf")
SHIFT = (5, -9)


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


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------- 1. luma pyramid
LUMA_SHAPES = [((5, 7), (9, 11)), ((37, 51), (37, 51)), ((96, 128), (96, 128))]


@pytest.mark.parametrize("window,shape", LUMA_SHAPES, ids=shape_id)
def test_luma_pyramid_against_numpy(torch, wct, window, shape):
    """Levels 1 and 4 -- 3 where the window is too small for 4 (5 x 7: 2^3 > 5) -- of a window inside a larger image and of whole images;
    odd sizes at every level; one image with values the conversion has to clamp."""
    Ho, Wo = window
    img = V.image(shape, 21)
    wild = img.copy()
    for i, v in enumerate((np.nan, np.inf, -np.inf, -0.3, 1.7)):
        wild[i % 3, (2 * i) % Ho, (3 * i + 1) % Wo] = v
    top = 4 if min(Ho, Wo) >= 8 else 3
    for x in (img, wild):
        for levels in (1, top):
            want = M.pyramid(x, levels, Ho, Wo)
            got = wct.motion_luma(dev(torch, x), levels, Ho, Wo)
            assert len(got) == levels
            for k in range(levels):
                assert np.array_equal(got[k].cpu().numpy(), want[k]), (levels, k)
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 2. the field
def unrelated(shape, content_shape, seeds):
    return V.image(content_shape, seeds[0]), V.image(shape, seeds[1])


def four_greys(shape, seed):
    g = np.floor(V.image(shape, seed).mean(0) * 8.0) % 4 / 3.0            # 4 grey levels in bands: ties everywhere
    return np.ascontiguousarray(np.broadcast_to(g.astype(np.float32), (3,) + tuple(shape)))


# (H, W, shift, levels, range) of tests/test_motion_cpu.py TRANSLATIONS: the two the device runs
DEVICE_TRANSLATIONS = ((96, 112, (5, -9), 3, 4), (64, 64, (3, 2), 2, 2))


def field_cases():
    out = []
    for H, W, shift, levels, rng in DEVICE_TRANSLATIONS:                                                 # (a)
        out.append(("translated-%dx%d" % (H, W), lambda H=H, W=W, shift=shift: M.translated_pair(H, W, shift), [(levels, rng, 4)], (H, W, shift)))
    out.append(("unrelated-37x51", lambda: unrelated((37, 51), (41, 60), (1, 2)), [(1, 7, 4), (3, 2, 0), (4, 0, 255)], None))      # (b)
    out.append(("unrelated-40x72", lambda: unrelated((40, 72), (40, 72), (3, 4)), [(1, 0, 255), (3, 7, 4), (4, 2, 0)], None))
    out.append(("greys-48x48", lambda: (four_greys((48, 48), 5), four_greys((48, 48), 6)), [(1, 7, 0), (3, 0, 4), (4, 2, 255), (4, 7, 0)], None))   # (c)
    out.append(("one-block", lambda: unrelated((8, 8), (8, 8), (7, 8)), [(1, 7, 4), (4, 4, 4)], None))                              # (d)
    return out


FIELD_CASES = field_cases()


@pytest.mark.parametrize("name,make,params,translation", FIELD_CASES, ids=[c[0] for c in FIELD_CASES])
def test_field_against_numpy(torch, wct, name, make, params, translation):
    """(a) translated pairs, where the oracle's rule also claims the shift itself; (b) unrelated frames with clipped blocks, odd pyramid
    sizes and the parent clamp (37 x 51: grids 5 x 7, 3 x 4, 2 x 2, 1 x 1), one inside a larger content; (c) four grey levels: ties
    everywhere, the index order decides; (d) a single block, with a 1 x 1 top level.  Every levels / range / penalty value on (b) and (c)."""
    cur, prev = make()
    for levels, rng, penalty in params:
        want = M.estimate(cur, prev, levels, rng, penalty)
        got = wct.motion_estimate(dev(torch, cur), dev(torch, prev), levels, rng, penalty).cpu().numpy()
        assert got.dtype == np.int16 and got.shape == want.shape
        assert np.array_equal(got, want), (name, levels, rng, penalty, int((got != want).any(-1).sum()))
        if translation:
            M.assert_translation(got, *translation, levels)
    if name.startswith("greys"):
        assert len(np.unique(M.luma(cur))) == 4
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 3. the blend
BLEND_SHAPES = [((17, 25), (20, 30)), ((96, 128), (96, 128)), ((V.TILE_H + 1, V.TILE_W + 5), (V.TILE_H + 1, V.TILE_W + 5))]


def gather_t(torch, q, mv):
    """q' of the header on the device with torch indexing: rows and columns clamped, the vector of block (y >> 3, x >> 3)."""
    Ho, Wo = int(q.shape[-2]), int(q.shape[-1])
    y = torch.arange(Ho, device=q.device)[:, None].expand(Ho, Wo)
    x = torch.arange(Wo, device=q.device)[None, :].expand(Ho, Wo)
    v = mv.long()[y >> 3, x >> 3]
    return q[..., (y + v[..., 0]).clamp(0, Ho - 1), (x + v[..., 1]).clamp(0, Wo - 1)].contiguous()


def admissible_field(rng, Ho, Wo, reach=12):
    nby, nbx = M.grid(Ho, Wo)
    mv = np.zeros((nby, nbx, 2), np.int16)
    for by in range(nby):
        for bx in range(nbx):
            y0, x0 = 8 * by, 8 * bx
            bh, bw = min(8, Ho - y0), min(8, Wo - x0)
            mv[by, bx] = (rng.integers(max(-reach, -y0), min(reach, Ho - y0 - bh) + 1), rng.integers(max(-reach, -x0), min(reach, Wo - x0 - bw) + 1))
    return mv


@pytest.mark.parametrize("out_shape,content_shape", BLEND_SHAPES, ids=shape_id)
def test_blend_with_a_field(torch, wct, out_shape, content_shape):
    Ho, Wo = out_shape
    blend, sigma, radius = 0.6, 0.05, 2
    rng = np.random.default_rng(Ho)
    cur = V.image(content_shape, 11)
    prev = (cur[:, :Ho, :Wo] + 0.03 * (V.image(out_shape, 12) - 0.5)).astype(np.float32)
    s, p = V.image(out_shape, 13), V.image(out_shape, 14)
    c_d, q_d, s_d, p_d = (dev(torch, a) for a in (cur, prev, s, p))
    plain, plain_u8 = wct.temporal_blend(c_d, q_d, s_d, p_d, blend, sigma, radius, u8=True, round_mode=1)
    zero = torch.zeros(M.grid(Ho, Wo) + (2,), device="cuda", dtype=torch.int16)
    for mv in (None, zero):                                             # no field and the zero field: video mode's blend bit for bit
        got, hwc = wct.motion_blend(c_d, q_d, s_d, p_d, mv, blend, sigma, radius, u8=True, round_mode=1)
        assert torch.equal(got, plain) and torch.equal(hwc, plain_u8)
    far = (300 * rng.choice([-1, 1], size=M.grid(Ho, Wo) + (2,))).astype(np.int16)
    moved = 0.0
    for mv_h in (admissible_field(rng, Ho, Wo), far):
        mv = dev(torch, mv_h)
        q2, p2 = gather_t(torch, q_d, mv), gather_t(torch, p_d, mv)
        assert np.array_equal(q2.cpu().numpy(), M.gather(prev, mv_h))       # the torch gather is the oracle's
        want = wct.temporal_blend(c_d, q2, s_d, p2, blend, sigma, radius).clone()
        for round_mode in (0, 1):
            got, hwc = wct.motion_blend(c_d, q_d, s_d, p_d, mv, blend, sigma, radius, u8=True, round_mode=round_mode)
            assert torch.equal(got, want), round_mode
            assert torch.equal(hwc, wct.to_u8(got, round_mode)), round_mode
        ref = V.blend(cur, M.gather(prev, mv_h), s, M.gather(p, mv_h), blend, sigma, radius)
        dist, bound = float(np.abs(got[0].cpu().numpy().astype(np.float64) - ref).max()), V.blend_bound(radius, blend, M.gather(p, mv_h), s)
        print("blend %s: field reach %d: distance / bound %.3g" % (out_shape, int(np.abs(mv_h).max()), dist / bound))
        assert dist <= bound, (dist, bound)
        moved = max(moved, float((got - plain).abs().max()))
        ones = torch.ones(1, device="cuda", dtype=torch.int32)
        assert torch.equal(wct.motion_blend(c_d, q_d, s_d, p_d, mv, blend, sigma, radius, cut_flag=ones), s_d[None])       # a cut: s itself
    assert moved > 1e-3                                                     # the field did something
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 4. the frame
def pair(torch, H, W, shift=SHIFT):
    cur, prev = M.translated_pair(H, W, shift, seed=31)
    return dev(torch, prev)[None], dev(torch, cur)[None]                    # frame 1, frame 2 = frame 1 moved by `shift`


@pytest.mark.parametrize("size", SIZES, ids=shape_id)
def test_frame_identities_with_motion_attached(torch, wct, size):
    H, W = size
    Ho, Wo = H // 16 * 16, W // 16 * 16
    A, B = pair(torch, H, W)
    Cc = sc.image(3, H, W)
    want = {k: wct.stylize_prepared(x, alpha=0.6).clone() for k, x in (("A", A), ("B", B), ("C", Cc))}
    zero = torch.zeros(M.grid(Ho, Wo) + (2,), device="cuda", dtype=torch.int16)
    # (a) the first frame and the frame after a reset: the cascade's result, a zero field
    clip = wct.clip(H, W, rate=0.25, cut=0.5, blend=0.6, motion=True)
    assert clip.motion == dict(levels=_lib.MOTION_LEVELS, range=_lib.MOTION_RANGE, penalty=_lib.MOTION_PENALTY)
    assert torch.equal(clip.stylize(A, alpha=0.6), want["A"]) and torch.equal(clip.motion_field(), zero)
    clip.stylize(B, alpha=0.6)
    clip.reset()
    assert torch.equal(clip.stylize(Cc, alpha=0.6), want["C"]) and torch.equal(clip.motion_field(), zero)
    clip.close()
    # (b) rate 1, blend 0: every frame, whatever the field
    clip = wct.clip(H, W, rate=1.0, cut=INF, blend=0.0, motion=dict(levels=3, range=4, penalty=4))
    for k, x in (("A", A), ("B", B), ("C", Cc), ("A", A)):
        got, hwc = clip.stylize(x, alpha=0.6, u8=True, round_mode=1)
        assert torch.equal(got, want[k]), k
        assert torch.equal(hwc, wct.to_u8(got, 1))
    clip.close()
    # (c) a frame fed three times: a zero field, and the output of the same clip without motion
    for params in (dict(rate=0.25, cut=INF, blend=0.6), dict(rate=0.7, cut=0.5, blend=0.3, sigma=0.1, radius=4)):
        with_m, without = wct.clip(H, W, motion=dict(levels=4, range=7, penalty=0), **params), wct.clip(H, W, **params)
        for i in range(3):
            assert torch.equal(with_m.stylize(B, alpha=0.6), without.stylize(B, alpha=0.6)), i
            assert torch.equal(with_m.motion_field(), zero), i
        with_m.close()
        without.close()
    assert wct.saturation_count() == 0


@pytest.mark.parametrize("size", SIZES, ids=shape_id)
def test_frame_two_is_the_composition_of_public_calls(torch, wct, size):
    """rate = 1: the cascade is wct_stylize_prepared's, so frame 2 = wct_motion_blend(content2, crop(content1), prepared(content2), out1,
    wct_motion_estimate(content2, crop(content1))), the exported field is that field, the field holds the pan where the oracle's rule
    claims it -- and the frame differs from the one a clip without motion makes: the test that fails without the feature."""
    H, W = size
    Ho, Wo = H // 16 * 16, W // 16 * 16
    c1, c2 = pair(torch, H, W)
    mp = dict(levels=3, range=4, penalty=4)
    clip = wct.clip(H, W, rate=1.0, cut=INF, blend=0.6, sigma=0.05, radius=2, motion=mp)
    plain = wct.clip(H, W, rate=1.0, cut=INF, blend=0.6, sigma=0.05, radius=2)
    out1 = clip.stylize(c1, alpha=0.6).clone()
    assert torch.equal(plain.stylize(c1, alpha=0.6), out1)
    got = clip.stylize(c2, alpha=0.6).clone()
    field = clip.motion_field().clone()
    plain2 = plain.stylize(c2, alpha=0.6).clone()
    crop1 = c1[:, :, :Ho, :Wo].contiguous()
    mv = wct.motion_estimate(c2, crop1, **mp)
    sty = wct.stylize_prepared(c2, alpha=0.6).clone()
    want = wct.motion_blend(c2, crop1, sty, out1, mv, 0.6, 0.05, 2)
    assert torch.equal(field, mv)
    assert np.array_equal(mv.cpu().numpy(), M.estimate(c2[0].cpu().numpy(), crop1[0].cpu().numpy(), **{"rng" if k == "range" else k: v for k, v in mp.items()}))
    assert M.assert_translation(mv.cpu().numpy(), Ho, Wo, SHIFT, mp["levels"]) == 32
    assert torch.equal(got, want)
    assert torch.equal(plain2, wct.temporal_blend(c2, crop1, sty, out1, 0.6, 0.05, 2))
    # without the field the pan leaves the blend nothing to hold on to; with it the previous output comes back
    d_plain, d_motion = float((plain2 - sty).abs().mean()), float((got - sty).abs().mean())
    print("frame 2 at %s: mean |out - stylised| without the field %.3g, with it %.3g" % (size, d_plain, d_motion))
    assert not torch.equal(got, plain2) and d_motion > 10 * d_plain
    clip.close()
    plain.close()
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 5. graph, allocation, isolation
def test_one_captured_frame_with_motion_is_replayed_for_successive_frames():
    """One wct_stylize_clip with motion attached captured into a HIP graph, replayed for three frames of a panning sequence with the content
    rewritten in place, against three direct calls on a second clip.  In a fresh process: a failed capture can leave the runtime in capture mode."""
    code = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import torch
from tests import state_cases as sc
from tests import video_oracle as V
wct = sc.make_engine("16x")
wct.style_prepare(sc.image(90, 84, 108))
H, W = 100, 135
big = V.image((H + 20, W + 20), 1)
frames = [torch.from_numpy(np.ascontiguousarray(big[None, :, 10 + 3 * t:10 + 3 * t + H, 10 - 4 * t:10 - 4 * t + W])).cuda() for t in range(3)]     # a pan of (3, -4) per frame
mp = dict(levels=3, range=4, penalty=4)
direct = wct.clip(H, W, rate=0.25, cut=0.5, blend=0.6, motion=mp)
wants, fields = [], []
for x in frames:
    wants.append(direct.stylize(x, alpha=0.6).clone())
    fields.append(direct.motion_field().clone())
torch.cuda.synchronize()
allocs = wct.debug_get("ws_allocs")
clip = wct.clip(H, W, rate=0.25, cut=0.5, blend=0.6, motion=mp)
c = frames[0].clone()
out = torch.empty((1, 3, 96, 128), device="cuda")
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    clip.stylize(c, alpha=0.6, out=out)
cuts = []
for t, x in enumerate(frames):
    c.copy_(x)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, wants[t]), "replay %%d differs" %% t
    assert torch.equal(clip.motion_field(), fields[t]), "field %%d differs" %% t
    cuts.append(int(clip.export(5)[2][1]))
assert cuts == [1, 0, 0], cuts
assert not fields[0].any() and all(bool((f.view(-1, 2) == torch.tensor([3, -4], device="cuda", dtype=torch.int16)).all(1).any()) for f in fields[1:])
assert wct.debug_get("ws_allocs") == allocs
assert wct.saturation_count() == 0
print("GRAPH_OK")
""" % (REPO, PKG)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GRAPH_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_allocation_isolation_and_reattachment(torch):
    H, W = 100, 135
    style = sc.image(90, *STYLE)
    c1, c2 = pair(torch, H, W)
    c3 = sc.image(33, H, W)
    quiet = sc.make_engine("16x")                     # a clip without motion, alone
    quiet.style_prepare(style)
    clip = quiet.clip(H, W)
    wants_plain = [clip.stylize(x, alpha=0.6).clone() for x in (c1, c2, c3)]
    clip.close()

    busy = sc.make_engine("16x")
    busy.style_prepare(style)
    moving, plain = busy.clip(H, W, motion=True), busy.clip(H, W)
    got_moving = []
    allocs = None
    for t, x in enumerate((c1, c2, c3)):
        got_moving.append(moving.stylize(x, alpha=0.6).clone())
        assert torch.equal(plain.stylize(x, alpha=0.6), wants_plain[t]), t      # the second clip does not see the first
        if t == 0:
            allocs = busy.debug_get("ws_allocs")
    assert busy.debug_get("ws_allocs") == allocs                                # nothing allocated after the first frame
    assert not torch.equal(got_moving[1], wants_plain[1])
    # the profile of a frame with motion: video mode's launches, the blend under its own name, and the estimator's
    busy.profile(True)
    busy.profile_reset()
    plain.stylize(c2, alpha=0.6)
    names_plain = {r["name"] for r in busy.profile_read()}
    busy.profile_reset()
    moving.stylize(c2, alpha=0.6)
    names_moving = {r["name"] for r in busy.profile_read()}
    busy.profile(False)
    extra = {"motion_pyramid", "motion_blend", "motion_store"} | {"motion_search%d" % k for k in range(_lib.MOTION_LEVELS)}
    assert names_moving == (names_plain - {"temporal_blend"}) | extra, names_moving ^ names_plain
    assert busy.debug_get("ws_allocs") == allocs
    # detached, the clip is a clip without motion, from a first frame on; attached again it is what it was at its first frame
    moving.detach_motion()
    assert moving.motion is None
    with pytest.raises(_lib.WctError) as e:
        moving.motion_field()
    assert e.value.code == _lib.WCT_ERR_STATE and "wct_motion_export" in str(e.value)
    for t, x in enumerate((c1, c2, c3)):
        assert torch.equal(moving.stylize(x, alpha=0.6), wants_plain[t]), t
    moving.attach_motion()
    for t, x in enumerate((c1, c2, c3)):
        assert torch.equal(moving.stylize(x, alpha=0.6), got_moving[t]), t
    moving.close()
    plain.close()
    assert busy.saturation_count() == 0 and quiet.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_name_the_entry_and_write_nothing(torch, wct):
    L, ctx = wct._lib, wct._ctx
    H, W = 96, 128
    x, q = sc.image(41, H, W), sc.image(42, H, W)
    s, p = sc.image(43, H, W), sc.image(44, H, W)
    nby, nbx = M.grid(H, W)
    mv = torch.full((nby, nbx, 2), -3, device="cuda", dtype=torch.int16)
    lum = torch.full((2 * H * W,), 77, device="cuda", dtype=torch.uint8)
    out = torch.full((1, 3, H, W), -3.0, device="cuda")
    hwc = torch.full((H, W, 3), 9, device="cuda", dtype=torch.uint8)
    good = _lib.WctMotionParams(4, 4, 4)
    wct._stream()

    def refused(rc, entry, code=_lib.WCT_ERR_INVALID):
        assert rc == code and entry in L.wct_last_error(ctx).decode(), (rc, L.wct_last_error(ctx).decode())

    # wct_motion_luma
    for args in ((None, H, W, H, W, 2, lum.data_ptr()), (x.data_ptr(), H, W, H, W, 2, None), (x.data_ptr(), H, W, 0, W, 1, lum.data_ptr()),
                 (x.data_ptr(), H, W, H + 1, W, 2, lum.data_ptr()), (x.data_ptr(), H, W, H, W + 1, 2, lum.data_ptr()), (x.data_ptr(), H, W, H, W, 0, lum.data_ptr()),
                 (x.data_ptr(), H, W, H, W, 5, lum.data_ptr()), (x.data_ptr(), H, W, 7, W, 4, lum.data_ptr()), (x.data_ptr(), H, W, H, 3, 3, lum.data_ptr()),
                 (x.data_ptr(), H, W, H, W, 2, x.data_ptr() + 64)):
        refused(L.wct_motion_luma(ctx, *args), "wct_motion_luma")
    # wct_motion_estimate
    for args in ((None, H, W, q.data_ptr(), H, W, byref(good), mv.data_ptr()), (x.data_ptr(), H, W, None, H, W, byref(good), mv.data_ptr()),
                 (x.data_ptr(), H, W, q.data_ptr(), H, W, None, mv.data_ptr()), (x.data_ptr(), H, W, q.data_ptr(), H, W, byref(good), None),
                 (x.data_ptr(), H, W, q.data_ptr(), H + 16, W, byref(good), mv.data_ptr()), (x.data_ptr(), H, W, q.data_ptr(), 0, 0, byref(good), mv.data_ptr()),
                 (x.data_ptr(), H, W, q.data_ptr(), 7, 7, byref(good), mv.data_ptr()), (x.data_ptr(), H, W, q.data_ptr(), H, W, byref(good), q.data_ptr() + 8)):
        refused(L.wct_motion_estimate(ctx, *args), "wct_motion_estimate")
    for bad in ((0, 4, 4), (5, 4, 4), (4, -1, 4), (4, 8, 4), (4, 4, -1), (4, 4, 256)):
        refused(L.wct_motion_estimate(ctx, x.data_ptr(), H, W, q.data_ptr(), H, W, byref(_lib.WctMotionParams(*bad)), mv.data_ptr()), "wct_motion_estimate")
    # wct_motion_blend: what the blend of video mode refuses, under this entry's name, and an output over the field
    with pytest.raises(ValueError, match="wct_motion_blend"):
        wct.motion_blend(x, q, s, p, mv, 0.6, 0.05, 9, out=out)
    with pytest.raises(ValueError, match="wct_motion_blend"):
        wct.motion_blend(x, q, s, p, mv, 1.0, 0.05, 2, out=out)
    with pytest.raises(ValueError, match="wct_motion_blend.*overlaps"):
        wct.motion_blend(x, q, s, p, mv, 0.6, 0.05, 2, out=s.view(-1))
    big = torch.full((3 * H * W + 64,), -3.0, device="cuda")
    mv_in = big[:nby * nbx].view(torch.int16)[:nby * nbx * 2]
    refused(L.wct_motion_blend(ctx, x.data_ptr(), H, W, q.data_ptr(), s.data_ptr(), p.data_ptr(), H, W, 0.6, 0.05, 2, None, big.data_ptr(), None, 0,
                               mv_in.data_ptr()), "wct_motion_blend")
    refused(L.wct_motion_blend(ctx, x.data_ptr(), H, W, q.data_ptr(), s.data_ptr(), p.data_ptr(), H, W, 0.6, 0.05, 2, None, out.data_ptr(), hwc.data_ptr(), 2,
                               mv.data_ptr()), "wct_motion_blend")
    refused(L.wct_motion_blend(ctx, x.data_ptr(), H, W, None, s.data_ptr(), p.data_ptr(), H, W, 0.6, 0.05, 2, None, out.data_ptr(), None, 0, mv.data_ptr()),
            "wct_motion_blend")
    # wct_motion_attach / _export
    clip = wct.clip(H, W)
    refused(L.wct_motion_attach(ctx, None, byref(good)), "wct_motion_attach")
    for bad in ((0, 4, 4), (5, 4, 4), (4, 8, 4), (4, 4, 256)):
        refused(L.wct_motion_attach(ctx, clip._handle(), byref(_lib.WctMotionParams(*bad))), "wct_motion_attach")
    refused(L.wct_motion_export(ctx, None, mv.data_ptr()), "wct_motion_export")
    refused(L.wct_motion_export(ctx, clip._handle(), mv.data_ptr()), "wct_motion_export", _lib.WCT_ERR_STATE)      # nothing attached
    with pytest.raises(ValueError, match="wct_motion_attach"):
        wct.clip(H, W, motion=dict(levels=9))
    other = sc.make_engine("16x")                                                   # a clip of another context
    other._stream()
    rc = other._lib.wct_motion_attach(other._ctx, clip._handle(), byref(good))
    assert rc == _lib.WCT_ERR_INVALID and "wct_motion_attach" in other._lib.wct_last_error(other._ctx).decode()
    rc = other._lib.wct_motion_export(other._ctx, clip._handle(), mv.data_ptr())
    assert rc == _lib.WCT_ERR_INVALID and "wct_motion_export" in other._lib.wct_last_error(other._ctx).decode()
    clip.attach_motion()
    refused(L.wct_motion_export(ctx, clip._handle(), None), "wct_motion_export")
    torch.cuda.synchronize()
    assert bool((mv == -3).all()) and bool((lum == 77).all()) and bool((out == -3.0).all()) and bool((hwc == 9).all()) and bool((big == -3.0).all())
    assert torch.equal(clip.stylize(x, alpha=0.6), wct.stylize_prepared(x, alpha=0.6))      # and the clip is still at its first frame
    clip.close()
    assert wct.saturation_count() == 0
