"""tests/geometry_cases.py without a GPU: the case lists for three CU counts, the failure locator, and that the fp64 gate of
tests/test_geometry_gpu.py is one a correct fp32 implementation meets."""
import numpy as np
import pytest

from tests import geometry_cases as gc
from tests import width_models as wm
from tests.conftest import rel_err


@pytest.mark.parametrize("cus", [256, 64, 304])
def test_cases_exist_are_deterministic_and_bounded(cus):
    cs = gc.cases(cus)
    assert len(cs) >= 40
    assert tuple(cs) == gc._cases.__wrapped__(cus)                      # a second, uncached construction
    assert len({c.id for c in cs}) == len(cs)
    for c in cs:
        assert c.H * c.W <= gc.MAX_PIXELS and c.H >= 2 << (c.level - 1) and c.W >= 2 << (c.level - 1), c.id
        assert c.expect == gc.predict_names(c.kind, c.mode, c.level, c.H, c.W, cus, dict(c.switches)), c.id
        if c.kind == "dec":                                               # the decoded size is the image's: no row / column dropped
            assert c.H % (1 << (c.level - 1)) == 0 and c.W % (1 << (c.level - 1)) == 0, c.id
    default = {n[:-1] if n.endswith("m") and "#" in n else n for c in cs if not c.switches for n in c.expect}
    assert not [f for f in gc.FORMS if f not in default]
    switched = {n[:-1] if n.endswith("m") and "#" in n else n for c in cs if c.switches for n in c.expect}
    assert not [f for f in gc.FORMS_SWITCHED if f not in switched]
    # both sides of the multi-unit walk of the persistent kernels, with tile counts that are 0, 1 and 7 modulo the eight XCDs
    assert any(c.multi for c in cs) and any(not c.multi for c in cs)


def test_cases_for_256_cus_are_the_table():
    """The sizes and forms the launchers' thresholds give on the MI355X (256 CUs)."""
    got = {c.id: c.expect for c in gc.cases(256)}

    def has(cid, *names):
        assert cid in got, (cid, sorted(got))
        assert not [n for n in names if n not in got[cid]], (cid, got[cid])
    for level in (5, 2):
        has("enc%d-16x-489x1001" % level, "enc_head_fused<3-16-16,pool>#t8m")      # 31 x 32 = 992 < 1024 tiles of 16 rows
        has("enc%d-16x-67x95" % level, "enc_head_fused<3-16-16,pool>#t8")
        has("enc%d-16x-505x1001" % level, "enc_head_fused<3-16-16,pool>#r16m")     # exactly 1024
        has("enc%d-16x-1031x1953" % level, "enc_head_fused<3-16-16,pool>#r16m")    # 4030 tiles on 256 workgroups
    has("dec2-16x-494x510", "dec_tail_fused<16-16-3>#u8m")                         # 496 < 512
    has("dec2-16x-510x510", "dec_tail_fused<16-16-3>#u16")                         # exactly 512 = two workgroups per CU
    has("dec2-16x-526x510", "dec_tail_fused<16-16-3>#u16m")
    has("dec2-16x-1034x770", "dec_tail_fused<16-16-3>#u16m")                       # 44 x 25 = 1100 >= 1024: 24 rows, upsample form 16
    has("dec2-16x-494x510-upconv0", "dec_tail_fused<16-16-3>#t8m")
    has("dec2-16x-510x510-upconv0", "dec_tail_fused<16-16-3>#t16m")
    has("dec2-16x-1034x770-upconv0", "dec_tail_fused<16-16-3>#t24m")
    has("l11-16x-239x1001", "l1_moments_fused<3-24>", "l1_decode_fused<3-24-3>#t8m")   # 480 < 512
    has("l11-16x-251x1001", "l1_decode_fused<3-24-3>#t16m")                        # exactly 512
    has("l11-16x-523x1001", "l1_decode_fused<3-24-3>#t16m")
    has("dec3-original-956x2000", "conv3x3_f16x3<co=128>#s8")                      # feature 239 x 500: 240 < 256
    has("dec3-original-1000x2000", "conv3x3_f16x3<co=128>#t16")                    # feature 250 x 500: 256
    has("enc5-16x-1031x1889", "conv3x3_f16x3<co=64,dma>#t16", "conv3x3_f16x3<co=32,dma>#316m")    # 255 tiles at 1/4 resolution
    has("enc5-16x-1031x1953", "conv3x3_f16x3<co=64,dma>#t16m")                     # 272
    has("enc5-16x-1095x1953", "conv3x3_f16x3<co=64,dma>#t16m")                     # 288
    has("enc4-original-521x1001", "conv3x3_f16x3<co=128,dma>#t16m")                # 72 tiles x 4 groups
    tiles = {gc.sp_units(c.H // 4, c.W // 4, 64, 64, False, 256)[1] for c in gc.cases(256) if c.kind == "enc" and c.mode == "16x" and c.level == 5}
    assert {t % 8 for t in tiles if t < 256} >= {1, 7} and {t % 8 for t in tiles if t > 256} >= {0, 1, 7}, sorted(tiles)


def test_form_restatements_at_the_thresholds():
    assert gc.head_form(2160, 3840, 256) == "#r16m" and gc.head_form(96, 128, 256) == "#t8"
    assert gc.tail_form(2160, 3840, 256, True) == "#u16m" and gc.tail_form(2160, 3840, 256, False) == "#t24m"
    assert gc.l1dec_form(2160, 3840, 256) == "#t16m" and gc.l1dec_form(96, 128, 256) == "#t8"
    assert gc.f16_form(135, 240, 128, 256) == "#s8"                       # "level 5's first decoder conv: 135 x 240 x 128 -> 72 tiles"
    assert gc.sp_form(540, 960, 32, 64, False, 256) == "#t16m" and gc.sp_form(64, 64, 16, 32, False, 256) == "#316"
    assert gc.sp_units(257, 472, 64, 64, False, 256)[1:] == (255, 255, 256)


def test_locate_names_a_planted_error():
    rng = np.random.default_rng(1)
    ref = rng.standard_normal((3, 75, 100))
    got = ref + 1e-9 * rng.standard_normal(ref.shape)
    got[1, 71, 40] += 0.5                       # row 71 of 75 with 24-row tiles: tile row 3 of 4 (rows 72..74 are ragged), local row 23
    msg = gc.locate(got, ref, 32, 24)
    assert "(c, y, x) = (1, 71, 40)" in msg and "y % 24 = 23" in msg and "x % 32 = 8" in msg and "tile (row 2, column 1)" in msg
    assert "in the interior" in msg
    got = ref.copy()
    got[2, 73, 50] -= 0.25                      # the ragged last tile row
    msg = gc.locate(got, ref, 32, 24)
    assert "(2, 73, 50)" in msg and "in the last tile row;" in msg and "tile (row 3, column 1)" in msg
    assert "interior 0.000e+00" in msg and "border ring 0.000e+00" in msg
    got = ref.copy()
    got[0, 10, 99] += 0.125                     # reflected column
    msg = gc.locate(got, ref, 32, 8)
    assert "in the border ring and last tile column;" in msg and "last tile row/column 0.000e+00" in msg
    got = ref.copy()
    got[0, 73, 97] += 0.125
    assert "in the last tile row and last tile column;" in gc.locate(got, ref, 32, 24)
    got = ref.copy()
    got[:, 74, :] = 0.0                         # a dropped last image row
    msg = gc.locate(got, ref, 32, 24)
    assert "in the border ring and last tile row" in msg and "y % 24 = 2," in msg and "interior 0.000e+00" in msg


@pytest.mark.parametrize("pick", ["enc2-16x-67x95", "enc2-16x-505x1001", "dec2-16x-510x510"])
def test_fp32_oracle_meets_the_gate(oracle, weights16x, pick):
    """The gate of test_geometry_gpu.py part a is reachable: the reference's own fp32 arithmetic sits inside it at a small and at
    threshold-sized cases."""
    oracle.set_num_threads(min(16, oracle.num_threads()))
    assert oracle.num_threads() <= 16
    case = {c.id: c for c in gc.cases(256)}[pick]
    rng = np.random.default_rng(3)
    img = wm.smooth_image(rng, case.H, case.W)
    ref = wm.encode(wm.W16X, weights16x, case.level, img)
    if case.kind == "enc":
        e32 = rel_err(wm.encode(wm.W16X, weights16x, case.level, img, f64=False), ref)
    else:
        f = np.maximum(ref + 0.3 * np.abs(ref).max() * rng.standard_normal(ref.shape), 0).astype(np.float32)
        refd = wm.decode(wm.W16X, weights16x, case.level, f)
        assert refd.shape == (3, case.H, case.W)
        e32 = rel_err(wm.decode(wm.W16X, weights16x, case.level, f, f64=False), refd)
    print("geometry %s: fp32 oracle %.3e from fp64 (gate %.1e)" % (pick, e32, wm.ENC_DEC_GATE))
    assert e32 < wm.ENC_DEC_GATE
