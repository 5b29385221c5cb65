"""Video mode and motion compensation off the shipped model, on the MI355X: model E of tests/clip_cases.py (level 4 wider than level 5, the
fused level 1, levels 5 and 3 on the map-based fold) under all three transforms, in conv mode fp32 and with the side stream off, and model D
of tests/shard_cases.py -- against fp64 and bit for bit against the frame's other statements.

  a  one tracked level (content_encode -> moments_track -> content_solve -> content_decode on one clip) per frame 1..3 and level 5..1 against
     the fp64 arm of tests/clip_cases.py: the tracked sums at wm.MOM_GATE, the level at e_gpu <= 4 e32 + 1e-4, the cut flag per frame
  b  wct_stylize_clip per engine: the identities of stylize_prepared, the exported sums of EVERY level at rate 1 against content_encode of
     the style_transfer_level chain (the check on the clip's packed per-level offsets), the blend half, the track half, the frame with motion
  c  three frames with the workspace poisoned before every frame and other calls between them
  d  stylize_scaled against tests/test_scale_gpu.compose on the model-E engines"""
import ctypes

import numpy as np
import pytest

from tests import clip_cases as CC
from tests import motion_oracle as M
from tests import shard_cases as SC
from tests import video_oracle as V
from tests import width_models as wm
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

LEVELS = CC.LEVELS
ALPHA = CC.ALPHA
INF = float("inf")
SHIFT = (5, -9)
MOTION = dict(levels=3, range=4, penalty=4)
POISON = (0xFF, 0x3C)      # tests/test_state_gpu.py: NaN in every float format / finite and plausible
# (model, transform, conv mode, side stream)
ENGINES = [("E", "wct", "f16x3", True), ("E", "ot", "f16x3", True), ("E", "adain", "f16x3", True), ("E", "wct", "fp32", True),
           ("E", "wct", "f16x3", False), ("D", "wct", "f16x3", True)]
ENGINE_IDS = ["%s-%s%s%s" % (m, t, "" if c == "f16x3" else "-" + c, "" if o else "-serial") for m, t, c, o in ENGINES]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def refs():
    """The fp64 / fp32 arms, computed once per transform and never written to."""
    return CC.reference


def make_engine(key):
    from tests.shard_engine import WidthWCT
    model, mode, conv, overlap = key
    widths, w = (CC.MODEL_E, CC.weights()) if model == "E" else (SC.MODEL_D, SC.weights("D"))
    e = WidthWCT(widths, w, transform=mode)
    if conv != "f16x3":
        e.set_conv_mode(conv)
    if not overlap:
        e.set_overlap(False)
    return e


@pytest.fixture(scope="module")
def data(torch):
    """The clip's frames and style on the device ([1, 3, H, W] / [1, 3, Hs, Ws]), and a panned pair for the frame with motion."""
    f1, f2, f3, style = (torch.from_numpy(a).cuda()[None] for a in CC.images())
    cur, prev = M.translated_pair(CC.H, CC.W, SHIFT, seed=31)
    pan = (torch.from_numpy(prev).cuda()[None], torch.from_numpy(cur).cuda()[None])          # frame 1, frame 2 = frame 1 moved by SHIFT
    return dict(f1=f1, f2=f2, f3=f3, style=style, pan=pan)


@pytest.fixture(scope="module")
def engines(torch, data):
    """One engine per ENGINES entry with the style prepared, made on first use and shared by the tests of section b and d."""
    made = {}

    def get(key):
        if key not in made:
            made[key] = make_engine(key)
            made[key].style_prepare(data["style"])
        return made[key]
    return get


def same_bits(a, b):
    """fp64 device tensors, bit for bit (NaN and the sign of zero included)."""
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def clean(eng, what):
    """tests/test_state_gpu.py clean: no f16x3 clamp was counted and the range poll reports none."""
    n = ctypes.c_ulonglong()
    assert eng.saturation_count() == 0, "%s: saturation counter %d" % (what, eng.saturation_count())
    eng._chk(eng._lib.wct_range_poll(eng._ctx, ctypes.byref(n)))
    assert n.value == 0, "%s: wct_range_poll reports %d" % (what, n.value)


# ---------------------------------------------------------------------------------------------------- a. a tracked level against fp64
@pytest.mark.parametrize("mode", CC.TRANSFORMS)
def test_tracked_level_against_fp64(torch, refs, mode):
    """One clip of a model-E engine through frames 1, 2, 3, levels 5..1, level-isolated (the input of level L is the fp64 arm's output of level
    L + 1 of that frame, rounded to fp32): content_encode, moments_track (decide at level 5) against the sums the clip kept from the
    previous frame, content_solve on the returned sums, content_decode.  Frame 1 is a first frame, frame 2 the exponential average at rate
    0.25 (at least 100 level gates from the untracked result at every level: tests/test_clip_cases_cpu.py), frame 3 a cut: the flag reads
    1, 0, 1 behind the three frames (the threshold is the geometric mean of the fp64 arm's two distances).

    Measured on the MI355X, e_gpu / e32 in units of 1e-6, levels 5 4 3 2 1 (the gate is 4 e32 + 100 in these units):
        wct    frame 1  4.31/4.88  4.64/4.18  3.11/3.44  0.64/0.55  0.59/0.53
               frame 2  4.52/4.39  3.86/4.20  3.92/3.89  0.67/0.52  0.63/0.61
               frame 3  5.00/4.55  4.34/4.31  3.08/3.17  0.65/0.46  0.48/0.59
        ot     frame 1  5.20/4.29  3.53/3.80  3.03/2.91  0.59/0.52  0.79/0.62
               frame 2  4.12/4.72  4.47/4.43  3.45/3.24  0.58/0.53  0.57/0.62
               frame 3  4.15/4.90  3.77/4.90  2.87/3.20  0.63/0.70  0.48/0.52
        adain  frame 1  5.30/4.47  3.10/3.78  2.38/2.68  0.59/0.64  0.99/0.52
               frame 2  4.01/4.23  5.00/3.84  4.67/3.79  0.87/0.64  0.90/0.49
               frame 3  4.15/5.21  3.19/7.18  4.75/3.72  0.79/0.74  0.59/0.43
    Raw and tracked moments against fp64: at most 5.8e-7 against the 1e-6 gate."""
    ref = refs(mode)
    e = make_engine(("E", mode, "f16x3", True))
    e.style_prepare(torch.from_numpy(ref.style).cuda()[None])
    clip = e.clip(CC.H, CC.W, rate=CC.RATE, cut=ref.cut_thr, blend=0.0)
    rows, worst_mom = [], 0.0
    for t in CC.FRAMES:
        row = []
        for L in LEVELS:
            r64 = ref.r64[t][L]
            x = torch.from_numpy(ref.inputs[t][L]).cuda()[None]
            h, w, s, ss = e.content_encode(L, x)
            assert (h, w) == r64.cF.shape[1:] and h * w == CC.pixels(L)
            raw = (s.cpu().numpy(), ss.cpu().numpy())
            e.moments_track(clip, L, s, ss, decide=(L == 5))
            es, ess = rel_err(s.cpu().numpy(), r64.tracked[0]), rel_err(ss.cpu().numpy().reshape(-1), r64.tracked[1].reshape(-1))
            worst_mom = max(worst_mom, es, ess, rel_err(raw[0], r64.raw[0]), rel_err(raw[1].reshape(-1), r64.raw[1].reshape(-1)))
            assert es < wm.MOM_GATE and ess < wm.MOM_GATE, "%s frame %d level %d: tracked sum %.3e sumsq %.3e" % (mode, t, L, es, ess)
            if t != 2:                                                   # a first frame and a cut: c itself, bit for bit
                assert np.array_equal(s.cpu().numpy(), raw[0]) and np.array_equal(ss.cpu().numpy(), raw[1]), (mode, t, L)
            rs, rss, flags = clip.export(L)
            assert same_bits(rs, s) and same_bits(rss, ss)               # what was committed is what was returned
            assert int(flags[1]) == int(ref.cut[t]), "%s frame %d level %d: cut flag %d" % (mode, t, L, int(flags[1]))
            Mm, b = e.content_solve(L, float(h * w), s, ss, ALPHA)
            out = e.content_decode(L, Mm, b, int(x.shape[2]), int(x.shape[3]))[0].cpu().numpy()
            assert out.shape == r64.out.shape
            e_gpu, e32 = rel_err(out, r64.out), ref.e32[t][L]
            row.append((e_gpu, e32))
            print("clip level %s frame %d level %d (C = %d): gpu %.2e fp32 arm %.2e (vs fp64), gate %.3e" % (mode, t, L, r64.cF.shape[0], e_gpu, e32, ref.gate(t, L)))
            assert e_gpu <= 4 * e32 + 1e-4, (mode, t, L, e_gpu, e32)
        flags = [int(v) for v in clip.export(5)[2].cpu()]
        assert flags == [5 * t, int(ref.cut[t])], (mode, t, flags)       # every moments_track commits and counts: five a frame
        rows.append(row)
    clip.close()
    for t, row in zip(CC.FRAMES, rows):
        print("clip table %-5s frame %d  %s" % (mode, t, "  ".join("%.2f/%.2f" % (a * 1e6, b * 1e6) for a, b in row)))
    print("clip table %s: moments against fp64 at most %.1e" % (mode, worst_mom))
    assert ref.cut == {1: True, 2: False, 3: True}
    assert e.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------- b. the one-call frame
@pytest.mark.parametrize("key", ENGINES, ids=ENGINE_IDS)
def test_frame_identities_against_stylize_prepared(torch, engines, data, key):
    """tests/test_video_gpu.py test_frame_identities_against_stylize_prepared on this engine: the first frame, the frame after reset, every
    frame at rate 1 with blend 0, every frame at cut 0, and the same frame four times equal stylize_prepared by torch.equal."""
    wct = engines(key)
    A, B, Cc = data["f1"], data["f2"], data["f3"]
    want = {k: wct.stylize_prepared(x, alpha=ALPHA).clone() for k, x in (("A", A), ("B", B), ("C", Cc))}
    assert tuple(want["A"].shape) == (1, 3, CC.HO, CC.WO) and not torch.equal(want["A"], want["B"])
    clip = wct.clip(CC.H, CC.W, rate=0.25, cut=0.5, blend=0.6)
    assert torch.equal(clip.stylize(A, alpha=ALPHA), want["A"])
    clip.stylize(B, alpha=ALPHA)
    clip.reset()
    assert torch.equal(clip.stylize(Cc, alpha=ALPHA), want["C"])
    clip.close()
    clip = wct.clip(CC.H, CC.W, rate=1.0, cut=INF, blend=0.0)
    for k, x in (("A", A), ("B", B), ("C", Cc), ("A", A)):
        got, hwc = clip.stylize(x, alpha=ALPHA, u8=True, round_mode=1)
        assert torch.equal(got, want[k]), k
        assert torch.equal(hwc, wct.to_u8(got, 1))
    clip.close()
    clip = wct.clip(CC.H, CC.W, rate=0.25, cut=0.0, blend=0.6)
    for k, x in (("A", A), ("B", B), ("C", Cc)):
        assert torch.equal(clip.stylize(x, alpha=ALPHA), want[k]), k
    assert int(clip.export(5)[2][1]) == 1
    clip.close()
    clip = wct.clip(CC.H, CC.W, rate=0.25, cut=INF, blend=0.6)
    for i in range(4):
        assert torch.equal(clip.stylize(A, alpha=ALPHA), want["A"]), i
    assert [int(v) for v in clip.export(5)[2].cpu()] == [4, 0]
    # what the tracked sums of that frame went through: the fast fold where the level's decoder allows it under wct in f16x3 mode,
    # transform_mb + fold_impl (assemble_Mb under wct) at the other levels, the ot / adain assembly under those transforms
    from tests.shard_engine import profile_counts
    wct.profile(True)
    wct.profile_reset()
    clip.stylize(A, alpha=ALPHA)
    wct.sync()
    counts = profile_counts(wct)
    wct.profile(False)
    clip.close()
    model, mode, conv, _ = key
    fast = SC.fast_fold_levels(CC.MODEL_E if model == "E" else SC.MODEL_D) if (mode, conv) == ("wct", "f16x3") else []
    assert fast == {("E", "wct", "f16x3"): [4, 2, 1], ("D", "wct", "f16x3"): [2, 1]}.get((model, mode, conv), [])
    assert counts.get("clip_track") == 5 and counts.get("temporal_blend") == 1 and counts.get("clip_store") == 1 and counts.get("fold_affine") == 5, counts
    if mode == "wct":
        assert counts.get("assemble_Mb", 0) == 5 - len(fast), (key, counts)
    assert ("ot_assemble" in counts) == (mode == "ot") and ("adain_assemble" in counts) == (mode == "adain"), sorted(counts)
    assert any(n.startswith("l1_moments_fused") for n in counts) == (model == "E" and conv == "f16x3"), sorted(counts)
    assert wct.saturation_count() == 0


def forms_of(wct, fn):
    """The kernel forms (profile names with "prof_forms" on) that fn() launches."""
    from tests.shard_engine import profile_counts
    wct.debug_set("prof_forms", 1)
    wct.profile(True)
    wct.profile_reset()
    fn()
    wct.sync()
    names = set(profile_counts(wct))
    wct.profile(False)
    wct.debug_set("prof_forms", 0)
    return names


@pytest.mark.parametrize("key", ENGINES, ids=ENGINE_IDS)
def test_exported_sums_of_every_level_at_rate_one(torch, engines, data, key):
    """rate 1, cut +inf: the tracked sums are the frame's own.  clip.export(L) of EVERY level equals, bit for bit, the sums content_encode(L, x_L)
    returns, x_L from the chain of style_transfer_level calls that stylize equals -- after the first frame and after a second one.  A
    per-level offset into the clip's packed sums taken from another level's size shows here as a neighbour's values (models E and D: level
    4 is wider than level 5)."""
    wct = engines(key)
    style = data["style"]
    clip = wct.clip(CC.H, CC.W, rate=1.0, cut=INF, blend=0.0)
    for t, x in enumerate((data["f1"], data["f2"])):
        got = clip.stylize(x, alpha=ALPHA).clone()
        exported = {L: tuple(v.clone() for v in clip.export(L)) for L in LEVELS}
        cur, bad = x, []
        for L in LEVELS:
            h, w, s, ss = wct.content_encode(L, cur)
            rs, rss, flags = exported[L]
            assert [int(v) for v in flags.cpu()] == [t + 1, 1 if t == 0 else 0]
            if not (same_bits(rs, s) and same_bits(rss, ss)):
                inp = cur
                diff = forms_of(wct, lambda: clip.stylize(x, alpha=ALPHA)) ^ forms_of(wct, lambda: [wct.content_encode(l, inp) for l in LEVELS])
                bad.append((L, rel_err(rs.cpu().numpy(), s.cpu().numpy()), rel_err(rss.cpu().numpy(), ss.cpu().numpy()), sorted(n for n in diff if "moment" in n)))
            cur = wct.style_transfer_level(L, cur, style, ALPHA)
        assert not bad, "%s frame %d: exported sums differ from content_encode (level, sum, sumsq, moment forms that differ): %s" % (key, t + 1, bad)
        assert torch.equal(cur, got) and torch.equal(got, wct.stylize(x, style, alpha=ALPHA))
    clip.close()
    assert wct.saturation_count() == 0


@pytest.mark.parametrize("key", ENGINES, ids=ENGINE_IDS)
def test_blend_half_is_the_composition_of_public_calls(torch, engines, data, key):
    """rate 1: frame t = wct_temporal_blend(content_t, crop(content_{t-1}), prepared(content_t), out_{t-1}), bit for bit."""
    wct = engines(key)
    frames = [data["f1"], data["f2"], data["f1"]]
    clip = wct.clip(CC.H, CC.W, rate=1.0, cut=INF, blend=0.6, sigma=0.05, radius=2)
    prev_c = prev_o = None
    moved = 0.0
    for t, x in enumerate(frames):
        got = clip.stylize(x, alpha=ALPHA).clone()
        sty = wct.stylize_prepared(x, alpha=ALPHA).clone()
        want = sty if t == 0 else wct.temporal_blend(x, prev_c, sty, prev_o, 0.6, 0.05, 2)
        assert torch.equal(got, want), t
        if t:
            moved = max(moved, float((got - sty).abs().max()))
        prev_c, prev_o = x[:, :, :CC.HO, :CC.WO].contiguous(), got
    clip.close()
    assert moved > 1e-3            # the blend did something
    assert wct.saturation_count() == 0


@pytest.mark.parametrize("key", ENGINES, ids=ENGINE_IDS)
def test_track_half_against_the_split_composition(torch, engines, data, key):
    """tests/test_video_gpu.py test_track_half_against_the_split_composition on this engine: blend 0, rate 0.25, cut +inf, frames A = frame 1 and
    B = frame 3 (another scene).  The output for B against content_encode -> numpy track with the sums kept from A -> content_solve ->
    content_decode per level within 5e-4 max|ref|; the same comparison at rate 1 meets the bound too; prepared(B) lies at least ten bounds
    from the expectation; level 5's exported sums are the numpy track of the raw ones bit for bit.

    Measured on the MI355X (fused vs split / rate-1 yardstick / bound / prepared(B) vs expected):
        E wct, E wct fp32, E wct serial   0 / 0 / 1.68e-3 / 2.37          E ot     0 / 0 / 1.39e-3 / 1.99
        E adain                           0 / 0 / 1.36e-3 / 2.26          D wct    0 / 0 / 2.12e-3 / 3.9
    Zero: at these widths the one-call frame and the split composition give the same image bit for bit, the fast-fold levels of E and D
    (test_frame_identities_against_stylize_prepared reads from the profile that they did fold fast) included; at the shipped widths
    (tests/test_video_gpu.py) the two differ inside the bound."""
    wct = engines(key)
    rate = 0.25
    A, B = data["f1"], data["f3"]

    def composition(x, kept, rate):
        cur, sums = x, {}
        for level in LEVELS:
            h, w, s, ss = wct.content_encode(level, cur)
            s, ss = s.cpu().numpy(), ss.cpu().numpy()
            if kept is not None:
                s, ss = V.track(kept[level][0], s, rate, False), V.track(kept[level][1], ss, rate, False)
            sums[level] = (s, ss)
            Mm, b = wct.content_solve(level, float(h * w), torch.from_numpy(s), torch.from_numpy(ss), ALPHA)
            cur = wct.content_decode(level, Mm, b, int(cur.shape[2]), int(cur.shape[3]))
        return cur.clone(), sums

    _, kept = composition(A, None, rate)
    raw5 = {}
    for k, x in (("A", A), ("B", B)):
        _, _, s, ss = wct.content_encode(5, x)
        raw5[k] = (s.cpu().numpy(), ss.cpu().numpy())
    expected, _ = composition(B, kept, rate)
    plain_split, _ = composition(B, None, 1.0)
    prepared_b = wct.stylize_prepared(B, alpha=ALPHA).clone()

    clip = wct.clip(CC.H, CC.W, rate=rate, cut=INF, blend=0.0)
    clip.stylize(A, alpha=ALPHA)
    got = clip.stylize(B, alpha=ALPHA).clone()
    s5, ss5, flags = clip.export(5)
    clip.close()
    assert [int(v) for v in flags.cpu()] == [2, 0]
    assert np.array_equal(s5.cpu().numpy().view(np.uint64), V.track(raw5["A"][0], raw5["B"][0], rate, False).view(np.uint64))
    assert np.array_equal(ss5.cpu().numpy().view(np.uint64), V.track(raw5["A"][1], raw5["B"][1], rate, False).view(np.uint64))

    bound = 5e-4 * float(expected.abs().max())
    d_track = float((got - expected).abs().max())
    d_plain = float((prepared_b - plain_split).abs().max())
    d_apart = float((prepared_b - expected).abs().max())
    print("clip track half %s: fused vs split %.3g, rate-1 yardstick %.3g, bound %.3g, prepared(B) vs expected %.3g" % (ENGINE_IDS[ENGINES.index(key)], d_track, d_plain, bound, d_apart))
    assert d_plain <= 5e-4 * float(plain_split.abs().max())
    assert d_track <= bound
    assert d_apart >= 10 * bound
    assert wct.saturation_count() == 0


def test_frame_two_with_motion_is_the_composition_of_public_calls(torch, engines, data):
    """Model E, the ot engine (tests/test_motion_gpu.py test_frame_two_is_the_composition_of_public_calls): at rate 1 frame 2 of a panned pair
    equals wct_motion_blend(content2, crop(content1), prepared(content2), out1, wct_motion_estimate(content2, crop(content1))) bit for bit,
    the exported field is that field and tests/motion_oracle.py's, and it holds the pan where the oracle's rule claims it."""
    wct = engines(("E", "ot", "f16x3", True))
    c1, c2 = data["pan"]
    clip = wct.clip(CC.H, CC.W, rate=1.0, cut=INF, blend=0.6, sigma=0.05, radius=2, motion=MOTION)
    plain = wct.clip(CC.H, CC.W, rate=1.0, cut=INF, blend=0.6, sigma=0.05, radius=2)
    out1 = clip.stylize(c1, alpha=ALPHA).clone()
    assert torch.equal(plain.stylize(c1, alpha=ALPHA), out1) and not bool(clip.motion_field().any())
    got = clip.stylize(c2, alpha=ALPHA).clone()
    field = clip.motion_field().clone()
    plain2 = plain.stylize(c2, alpha=ALPHA).clone()
    crop1 = c1[:, :, :CC.HO, :CC.WO].contiguous()
    mv = wct.motion_estimate(c2, crop1, **MOTION)
    sty = wct.stylize_prepared(c2, alpha=ALPHA).clone()
    want = wct.motion_blend(c2, crop1, sty, out1, mv, 0.6, 0.05, 2)
    assert torch.equal(field, mv)
    assert np.array_equal(mv.cpu().numpy(), M.estimate(c2[0].cpu().numpy(), crop1[0].cpu().numpy(), MOTION["levels"], MOTION["range"], MOTION["penalty"]))
    assert M.assert_translation(mv.cpu().numpy(), CC.HO, CC.WO, SHIFT, MOTION["levels"]) > 0
    assert torch.equal(got, want)
    assert torch.equal(plain2, wct.temporal_blend(c2, crop1, sty, out1, 0.6, 0.05, 2)) and not torch.equal(got, plain2)
    clip.close()
    plain.close()
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------- c. poison
@pytest.mark.parametrize("motion", [None, MOTION], ids=["plain", "motion"])
@pytest.mark.parametrize("mode", ["wct", "ot"])
def test_frames_on_a_poisoned_workspace(torch, data, mode, motion):
    """Three frames (a first frame, a tracked and blended one, a cut: the threshold between the two distances) with every scratch buffer of the context filled
    with the byte before every frame, and a stylize of 208 x 280 and a motion_estimate of another size between the frames: the same bits as on
    a quiet engine, nothing allocated after the first round, no clamp counted or polled.  The clip's state is the clip's own; what a
    frame reads of the context's workspace it has to have written itself."""
    from tests import state_cases as sc
    style = data["style"]
    frames = (data["f1"], data["f2"], data["f3"])
    other = sc.image(61, 208, 280)
    pa, pb = sc.image(62, 72, 100), sc.image(63, 64, 96)
    thr = float(np.sqrt(np.prod(CC.cut_distances())))

    quiet = make_engine(("E", mode, "f16x3", True))
    quiet.style_prepare(style)
    clip = quiet.clip(CC.H, CC.W, cut=thr, motion=motion)
    wants, fields, cuts = [], [], []
    for x in frames:
        wants.append(clip.stylize(x, alpha=ALPHA).clone())
        fields.append(clip.motion_field().clone() if motion else None)
        cuts.append(int(clip.export(5)[2][1]))
    clip.close()
    assert cuts == [1, 0, 1] and not torch.equal(wants[1], quiet.stylize_prepared(frames[1], alpha=ALPHA))      # frame 2 was smoothed
    want_other = quiet.stylize(other, style, alpha=ALPHA).clone()
    want_mv = quiet.motion_estimate(pa, pb).clone()
    clean(quiet, "quiet engine")

    busy = make_engine(("E", mode, "f16x3", True))
    busy.style_prepare(style)
    allocs = None
    for byte in POISON:
        clip = busy.clip(CC.H, CC.W, cut=thr, motion=motion)
        for t, x in enumerate(frames):
            busy.debug_set("poison", byte)
            got = clip.stylize(x, alpha=ALPHA)
            assert torch.equal(got, wants[t]), "poison 0x%02X frame %d: %.3e" % (byte, t + 1, float((got - wants[t]).abs().max()))
            if motion:
                assert torch.equal(clip.motion_field(), fields[t]), (byte, t)
            assert int(clip.export(5)[2][1]) == cuts[t]
            assert torch.equal(busy.stylize(other, style, alpha=ALPHA), want_other)       # the same style: the prepared slots are rewritten with the same bits
            assert torch.equal(busy.motion_estimate(pa, pb), want_mv)
        clip.close()
        torch.cuda.synchronize()
        if allocs is None:
            allocs = busy.debug_get("ws_allocs")
        assert busy.debug_get("ws_allocs") == allocs, "allocated after the first round"
    busy.debug_set("poison", -1)
    clean(busy, "poisoned engine")


# ---------------------------------------------------------------------------------------------------- d. scale control on model E
@pytest.mark.parametrize("mode", CC.TRANSFORMS)
def test_stylize_scaled_is_the_composition_on_model_e(torch, engines, data, mode):
    """tests/test_scale_gpu.py compose against wct_stylize_scaled at divisors (4, 4, 2, 1, 1), content 208 x 280, gain 1: bit for bit."""
    from tests import state_cases as sc
    from tests.test_scale_gpu import compose
    eng = engines(("E", mode, "f16x3", True))
    style = data["style"]
    c = sc.image(41, 208, 280)
    div = (4, 4, 2, 1, 1)
    want = compose(eng, c, lambda level: style, div, 1.0, ALPHA, 1).clone()
    got = eng.stylize_scaled(c, style, div, 1.0, alpha=ALPHA)
    assert tuple(got.shape) == (1, 3, 208, 272) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    assert not torch.equal(got, eng.stylize(c, style, alpha=ALPHA))
    eng.style_prepare(style)          # the cases of section b share this engine: its prepared slots hold the style again (the same bits)
    assert eng.saturation_count() == 0
