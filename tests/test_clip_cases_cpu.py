"""The preconditions of tests/test_clip_widths_gpu.py from the fp64 reference of tests/clip_cases.py alone: model E is what its comment says, every
tracked solve of the clip is well posed, the two scene-cut decisions are far from their threshold, and frame 2 cannot pass untracked.  No GPU."""
import subprocess
import sys

import numpy as np
import pytest

from tests import clip_cases as CC
from tests import shard_cases as SC
from tests import video_oracle as V
from tests import width_models as wm
from tests.test_shard_cases_cpu import OT_MAX_COND
from tests.test_sweep_gpu import SOLVE_MAX_COND

APART_GATES = 100          # frame 2 tracked against untracked, in level gates
DECISION_MARGIN = 1e-3     # |D - cut| / cut of both decided frames


def test_helper_imports_without_torch():
    code = "import sys; sys.path[:0] = %r; from tests import clip_cases; assert 'torch' not in sys.modules, 'torch imported'" % (sys.path[:3],)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_model_e_is_what_its_comment_says():
    E = CC.MODEL_E
    C = {L: wm.feature_channels(E, L) for L in CC.LEVELS}
    assert C[4] > C[5] and len(set(C.values())) == 4 and C[2] == C[1]          # level 4 is the widest; the packed offsets are not multiples of one size
    assert 17 <= C[1] <= 24                                                    # the fused level-1 kernels (level1.hip l1_fusable)
    assert SC.fast_fold_levels(E) == [4, 2, 1]                                 # 5 and 3 take transform_mb + fold_impl under wct too
    assert max(l.cout for L in CC.LEVELS for l in wm.encoder_layers(E, L)) <= 128          # not a wide model: wct_stylize_clip runs it
    for kind, layers in (("enc", wm.encoder_layers), ("dec", wm.decoder_layers)):
        assert all(wm.loadable(kind, layers(E, L)) for L in CC.LEVELS)
    assert (CC.HO, CC.WO) == (160, 176) and (CC.H % 16, CC.W % 16) == (4, 7) and CC.W % 4                  # cropped in both axes, scalar content loads
    assert CC.pixels(5) == 110 >= 2 * C[5] and (CC.HS >> 4) * (CC.WS >> 4) == 108 >= 2 * C[5]
    assert V.clip_bytes(CC.H, CC.W, [C[L] for L in CC.LEVELS]) > 0
    # model D, the cascade-only engine of the GPU file: level 4 wider than level 5 as well, nothing wide
    D = SC.MODEL_D
    assert wm.feature_channels(D, 4) > wm.feature_channels(D, 5) and max(D.values()) <= 128


def test_images_are_drawn_as_documented():
    f1, f2, f3, style = CC.images()
    assert f1.shape == f2.shape == f3.shape == (3, CC.H, CC.W) and style.shape == (3, CC.HS, CC.WS)
    assert all(a.dtype == np.float32 and a.flags.c_contiguous and 0.0 <= a.min() and a.max() <= 1.0 for a in (f1, f2, f3, style))
    rng = np.random.default_rng(CC.IMG_SEED)
    assert np.array_equal(wm.smooth_image(rng, CC.H, CC.W), f1)
    other = wm.smooth_image(rng, CC.H, CC.W)
    assert np.abs(f2 - (0.8 * f1.astype(np.float64) + 0.2 * other)).max() < 1e-6 and np.array_equal(wm.smooth_image(rng, CC.HS, CC.WS), style)
    assert np.array_equal(wm.smooth_image(np.random.default_rng(CC.IMG_SEED + 1), CC.H, CC.W, passes=1), f3)
    assert np.abs(f3 - f1).mean() > 4 * np.abs(f2 - f1).mean()                                                   # another scene
    D2, D3 = CC.cut_distances()
    ref = CC.reference("wct")
    assert (D2, D3) == (ref.D[2], ref.D[3]) and D3 > 3 * D2            # the cheap statement of the two distances is the reference's
    # the contrast-compressed third frame (0.5 x + 0.25) is no cut behind a tracked frame 2: its distance to the tracked sums is below D2
    r2 = ref.r64[2][5].tracked
    c3 = wm.raw_moments(wm.encode(CC.MODEL_E, CC.weights(), 5, np.float32(0.5) * f3 + np.float32(0.25), True))
    assert V.decision(CC.pixels(5), c3[0], r2[0], r2[1], 2, np.inf)[1] < D2


def level_failures(ref, mode, t, L):
    """The conditioning preconditions frame t's level L misses, as text; the figures are printed."""
    bad = []
    d = CC.conditioning(ref, t, L)
    print("clip case %s seed %d frame %d level %d: C %d (live %d / %d), n_c %d n_s %d, cond(cov_c) %.2e cond(cov_s) %.2e cond(B) %.2e"
          % (mode, ref.img_seed, t, L, d["C"], d["live_c"], d["live_s"], d["n_c"], d["n_s"], d["cond_c"], d["cond_s"], d["cond_B"]))
    if d["n_c"] < 2 * d["C"] or d["n_s"] < 2 * d["C"]:
        bad.append("frame %d level %d: %d / %d pixels for %d channels" % (t, L, d["n_c"], d["n_s"], d["C"]))
    if d["rank_c"] != d["live_c"] or d["rank_s"] != d["live_s"]:
        bad.append("frame %d level %d: rank %d / %d of %d / %d live channels" % (t, L, d["rank_c"], d["rank_s"], d["live_c"], d["live_s"]))
    if not d["cond_c"] <= SOLVE_MAX_COND:
        bad.append("frame %d level %d: cond(cov_c) %.2e" % (t, L, d["cond_c"]))
    if mode == "ot" and not d["cond_B"] <= OT_MAX_COND:
        bad.append("frame %d level %d: cond(B) %.2e" % (t, L, d["cond_B"]))
    return bad


def failures(mode, img_seed):
    """Every precondition the reference of (mode, img_seed) misses, as text; the figures are printed."""
    ref = CC.reference(mode, img_seed)
    bad = []
    if not ref.D[2] < ref.cut_thr < ref.D[3]:
        bad.append("D2 %.3g, D3 %.3g: no threshold between them" % (ref.D[2], ref.D[3]))
    for t, (cut, D) in ref.decisions().items():
        if cut != ref.cut[t] or D != ref.D[t] or abs(D - ref.cut_thr) < DECISION_MARGIN * ref.cut_thr:
            bad.append("frame %d: cut %d at D %.6g against the threshold %.6g" % (t, cut, D, ref.cut_thr))
    for t in CC.FRAMES:
        for L in CC.LEVELS:
            bad += level_failures(ref, mode, t, L)
            print("    fp32 arm %.2e" % ref.e32[t][L])
            if not np.isfinite(ref.r64[t][L].out).all() or ref.r64[t][L].out.shape != (3, CC.HO, CC.WO):
                bad.append("frame %d level %d: output %s" % (t, L, ref.r64[t][L].out.shape))
            if t == 2:
                out = ref.r64[2][L].out
                apart = float(np.abs(ref.untracked[L] - out).max() / np.abs(out).max())
                print("    tracked vs untracked %.3e = %.0f gates of %.3e" % (apart, apart / ref.gate(2, L), ref.gate(2, L)))
                if apart < APART_GATES * ref.gate(2, L):
                    bad.append("frame 2 level %d: tracked and untracked %.3e apart, %.0f gates" % (L, apart, apart / ref.gate(2, L)))
    return bad


@pytest.mark.parametrize("mode", CC.TRANSFORMS)
def test_tracked_levels_are_well_posed(mode):
    """Per frame and level, on the fp64 arm, of the TRACKED covariance (shard_cases.conditioning's figures): n >= 2 C on both sides, rank == live
    channels, cond(cov_c) <= SOLVE_MAX_COND, under ot cond(B) <= OT_MAX_COND (tests/test_shard_cases_cpu.py's reasons); both decisions at least
    1e-3 cut from the threshold; and at every level frame 2's tracked output at least 100 level gates from its untracked one, so
    tests/test_clip_widths_gpu.py section a cannot pass without the tracking."""
    bad = failures(mode, CC.IMG_SEED)
    assert not bad, "%s, img_seed %d: %s" % (mode, CC.IMG_SEED, "; ".join(bad))
    ref = CC.reference(mode)
    assert ref.cut == {1: True, 2: False, 3: True}
    # a first frame and a cut take c itself; frame 2 is the exponential average, bit for bit the three rounded operations
    for L in CC.LEVELS:
        for k in (0, 1):
            assert np.array_equal(ref.r64[1][L].tracked[k], ref.r64[1][L].raw[k]) and np.array_equal(ref.r64[3][L].tracked[k], ref.r64[3][L].raw[k])
            r, c = ref.r64[1][L].tracked[k], ref.r64[2][L].raw[k]
            assert np.array_equal(ref.r64[2][L].tracked[k], r + np.float64(CC.RATE) * (c - r))
        assert np.array_equal(ref.inputs[2][L], CC.images()[1] if L == 5 else ref.r64[2][L + 1].out.astype(np.float32))       # level-isolated


def test_img_seed_is_the_first_that_qualifies():
    """The rule next to clip_cases.IMG_SEED: every seed from FIRST_SEED up to it misses a precondition -- at the (transform, frame, level) that
    clip_cases.EARLIER_SEEDS records, from the fp64 arm as far as that level -- and the seed itself passes under all three transforms (the
    test above)."""
    assert sorted(CC.EARLIER_SEEDS) == list(range(CC.FIRST_SEED, CC.IMG_SEED))
    for seed, (mode, t, L) in sorted(CC.EARLIER_SEEDS.items()):
        bad = level_failures(CC.Reference(mode, seed, upto=(t, L)), mode, t, L)
        print("img_seed %d: %s" % (seed, bad))
        assert bad, "img_seed %d meets the preconditions of %s frame %d level %d: is clip_cases.IMG_SEED still the first?" % (seed, mode, t, L)
