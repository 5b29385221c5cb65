"""Motion compensation without a GPU: the public header and its bindings, wct_motion_shape (host only), the identities of the numpy
reference (tests/motion_oracle.py) -- a still frame, a pure translation, what the field does to the blend's weight -- and the command
line's --motion checks."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import motion_oracle as M
from tests import video_oracle as V
from tests.conftest import PKG, REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_motion.h")
OTHER_LISTS = ("SYMBOLS", "SYMBOLS_COLOR", "SYMBOLS_SMOOTH", "SYMBOLS_TRANSFORM", "SYMBOLS_SWAP", "SYMBOLS_SCALE", "SYMBOLS_GUIDED", "SYMBOLS_VIDEO")
# (H, W, shift, levels, range): cur(y, x) = prev(y + sy, x + sx); how many level-0 blocks the oracle's rule claims
TRANSLATIONS = (((96, 112, (5, -9), 3, 4), 32), ((128, 160, (-13, 22), 3, 7), 96), ((64, 64, (3, 2), 2, 2), 16), ((160, 128, (6, -6), 3, 2), 96))


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def test_header_and_symbol_list_agree():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r"\b(wct_motion_[a-z_0-9]+)\s*\(", text)))
    assert declared and declared == sorted(lib.SYMBOLS_MOTION)
    assert len(set(lib.SYMBOLS_MOTION)) == len(lib.SYMBOLS_MOTION)
    for other in OTHER_LISTS:
        assert not set(lib.SYMBOLS_MOTION) & set(getattr(lib, other)), other
    inc = os.path.join(REPO, "include")
    for name in os.listdir(inc):                                            # declared here and nowhere else
        if name != "wct_hip_motion.h":
            assert not set(lib.SYMBOLS_MOTION) & set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(os.path.join(inc, name)).read())), name
    for name, value in (("WCT_MOTION_BLOCK", lib.MOTION_BLOCK), ("WCT_MOTION_MAX_LEVELS", lib.MOTION_MAX_LEVELS), ("WCT_MOTION_MAX_RANGE", lib.MOTION_MAX_RANGE),
                        ("WCT_MOTION_LEVELS", lib.MOTION_LEVELS), ("WCT_MOTION_RANGE", lib.MOTION_RANGE), ("WCT_MOTION_PENALTY", lib.MOTION_PENALTY)):
        m = re.search(r"#define %s\s+(\S+)" % name, text)
        assert m and int(m.group(1)) == value, name
    assert (lib.MOTION_LEVELS, lib.MOTION_RANGE, lib.MOTION_PENALTY) == (4, 4, 4) and "a look, not a measurement" in text
    assert (M.BLOCK, M.MAX_LEVELS, M.MAX_RANGE) == (lib.MOTION_BLOCK, lib.MOTION_MAX_LEVELS, lib.MOTION_MAX_RANGE)
    assert [f[0] for f in lib.WctMotionParams._fields_] == ["levels", "range", "penalty"] and ctypes.sizeof(lib.WctMotionParams) == 12
    assert ctypes.sizeof(lib.WctClipParams) == 32                           # the clip's own parameters did not grow


def test_built_library_exports_the_motion_entries_and_hides_the_helpers():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_MOTION:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_MOTION) <= exported
    assert not [s for s in exported if "motion" in s and s not in lib.SYMBOLS_MOTION]


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_motion.c"
    src.write_text('#include "wct_hip_motion.h"\n'
                   "int main(void) { wct_motion_params p = { WCT_MOTION_LEVELS, WCT_MOTION_RANGE, WCT_MOTION_PENALTY };\n"
                   "  return (p.levels <= WCT_MOTION_MAX_LEVELS && p.range <= WCT_MOTION_MAX_RANGE && WCT_MOTION_BLOCK == 8 && sizeof(wct_motion_params) == 12) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "only_motion.o")], check=True)


def test_the_sources_are_listed_and_the_search_runs_on_packed_bytes():
    build = open(os.path.join(PKG, "build.sh")).read()
    assert re.search(r'^SRC=".*\bvideo\b.*\bmotion\b.*\bapi_video\b.*\bapi_motion\b.*"', build, re.M)
    assert "../include/wct_hip_motion.h" in build and "csrc/wct_clip.h" in build
    text = open(os.path.join(PKG, "csrc", "motion.hip")).read()
    assert "__builtin_amdgcn_sad_u8" in text and "__builtin_amdgcn_alignbyte" in text and "sat_raise(" not in text
    assert "struct wct_clip {" in open(os.path.join(PKG, "csrc", "wct_clip.h")).read()
    assert "struct wct_clip {" not in open(os.path.join(PKG, "csrc", "api_video.hip")).read()


# ---------------------------------------------------------------------------------------------------------------- host-only entries
def test_a_null_context_is_refused_by_every_entry():
    L = lib.load()
    p = lib.WctMotionParams(4, 4, 4)
    assert L.wct_motion_luma(None, None, 8, 8, 8, 8, 1, None) == lib.WCT_ERR_INVALID
    assert L.wct_motion_estimate(None, None, 8, 8, None, 8, 8, ctypes.byref(p), None) == lib.WCT_ERR_INVALID
    assert L.wct_motion_blend(None, None, 1, 1, None, None, None, 1, 1, 0.5, 0.05, 2, None, None, None, 0, None) == lib.WCT_ERR_INVALID
    assert L.wct_motion_attach(None, None, ctypes.byref(p)) == lib.WCT_ERR_INVALID
    assert L.wct_motion_attach(None, None, None) == lib.WCT_ERR_INVALID
    assert L.wct_motion_export(None, None, None) == lib.WCT_ERR_INVALID


def test_motion_shape_values_and_refusals():
    L = lib.load()
    nby, nbx = ctypes.c_int(-7), ctypes.c_int(-7)
    for (Ho, Wo), want in (((5, 7), (1, 1)), ((37, 51), (5, 7)), ((8, 8), (1, 1)), ((9, 16), (2, 2)), ((96, 128), (12, 16)), ((2160, 3840), (270, 480)),
                           ((1, 1), (1, 1))):
        assert L.wct_motion_shape(Ho, Wo, ctypes.byref(nby), ctypes.byref(nbx)) == lib.WCT_OK and (nby.value, nbx.value) == want, (Ho, Wo)
        assert M.grid(Ho, Wo) == want
    nby.value = nbx.value = -7
    for Ho, Wo, a, b in ((0, 8, nby, nbx), (8, 0, nby, nbx), (-3, 8, nby, nbx), (8, 8, None, nbx), (8, 8, nby, None)):
        assert L.wct_motion_shape(Ho, Wo, ctypes.byref(a) if a is not None else None, ctypes.byref(b) if b is not None else None) == lib.WCT_ERR_INVALID
    assert (nby.value, nbx.value) == (-7, -7)                               # untouched by every refusal


# ---------------------------------------------------------------------------------------------------------------- oracle identities
def test_luma_and_pyramid_by_hand():
    img = np.zeros((3, 2, 4), np.float32)
    img[:, 0, 0] = 1.0                                                      # white: 0.299 + 0.587 + 0.114 rounds to 1 -> 255
    img[0, 0, 1] = 1.0                                                      # red: 0.299 * 255 + 0.5 = 76.745 -> 76
    img[:, 0, 2] = (np.nan, 0.5, 0.5)                                       # NaN -> 0
    img[:, 0, 3] = (np.inf, 0.0, 0.0)                                       # +inf -> 255
    img[:, 1, 0] = -0.3
    img[:, 1, 1] = 1.7
    img[:, 1, 2] = (np.inf, -np.inf, 0.0)                                   # inf - inf: NaN -> 0
    img[1, 1, 3] = 0.5                                                      # green: 0.2935 * 255 + 0.5 = 75.3425 -> 75
    assert M.luma(img).tolist() == [[255, 76, 0, 255], [0, 255, 0, 75]]
    a = np.array([[0, 1, 255, 255, 9], [2, 3, 255, 254, 9], [7, 7, 7, 7, 9]], np.uint8)
    assert M.down(a).tolist() == [[2, 255]]                                 # (0+1+2+3+2)>>2 = 2; (1019+2)>>2 = 255; the odd row and column are dropped
    p = M.pyramid(V.image((37, 51), 3), 4)
    assert [x.shape for x in p] == [(37, 51), (18, 25), (9, 12), (4, 6)] and all(x.dtype == np.uint8 for x in p)


def test_a_frame_against_itself_gives_the_zero_field():
    for shape, levels, rng, penalty in (((40, 72), 4, 7, 0), ((37, 51), 3, 4, 4), ((48, 48), 1, 7, 0)):
        x = V.image(shape, 5)
        assert not M.estimate(x, x, levels, rng, penalty).any(), shape                    # cost 0 at index 0: nothing is smaller
    flat = np.full((3, 40, 56), 0.37, np.float32)                                         # every candidate costs 0 at penalty 0: the index decides
    assert not M.estimate(flat, flat, 4, 7, 0).any()
    assert not M.estimate(flat, flat + 0.2, 2, 3, 0).any()                                # and at a constant cost


@pytest.mark.parametrize("case,claimed", TRANSLATIONS, ids=lambda v: "x".join(str(t) for t in v[:2]) if isinstance(v, tuple) else str(v))
def test_a_pure_translation_is_found_exactly_where_the_rule_claims_it(case, claimed):
    H, W, shift, levels, rng = case
    cur, prev = M.translated_pair(H, W, shift)
    assert np.array_equal(cur[:, 20:30, 30:40], prev[:, 20 + shift[0]:30 + shift[0], 30 + shift[1]:40 + shift[1]])
    mv = M.estimate(cur, prev, levels, rng, lib.MOTION_PENALTY)
    assert mv.shape == M.grid(H, W) + (2,) and mv.dtype == np.int16
    assert M.assert_translation(mv, H, W, shift, levels) == claimed


def test_the_field_brings_the_blend_weight_back():
    (H, W, shift, levels, rng), _ = TRANSLATIONS[0]
    cur, prev = M.translated_pair(H, W, shift)
    mv = M.estimate(cur, prev, levels, rng, lib.MOTION_PENALTY)
    plain = M.weights(cur, prev, lib.CLIP_BLEND, lib.CLIP_SIGMA, lib.CLIP_RADIUS)
    moved = M.weights(cur, prev, lib.CLIP_BLEND, lib.CLIP_SIGMA, lib.CLIP_RADIUS, mv)
    assert plain.mean() < 1e-3 and moved.mean() > 0.2, (plain.mean(), moved.mean())
    assert np.array_equal(M.weights(cur, prev, 0.6, 0.05, 2, np.zeros_like(mv)), plain)    # a zero field is no field
    # the gather clamps: a field of vectors far outside the frame reads the border
    far = np.full_like(mv, 300)
    g = M.gather(prev, far)
    assert g.shape == prev.shape and np.array_equal(g, np.broadcast_to(prev[:, -1:, -1:], prev.shape))
    # and the blend of the gathered images is video mode's blend of them
    s, p = V.image((H, W), 2), V.image((H, W), 3)
    assert np.array_equal(V.blend(cur, M.gather(prev, mv), s, M.gather(p, mv), 0.6, 0.05, 2), s + moved[None] * (M.gather(p, mv).astype(np.float64) - s))


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    args = cli.build_parser().parse_args(list(argv))
    cli.checkpoint_args(args)
    return args


def test_motion_defaults_and_refusals():
    args = parse("--video", "--motion", "--mode", "16x")
    cli.check_video_args(args)
    cli.check_motion_args(args)
    assert (args.motion_levels, args.motion_range, args.motion_penalty) == (lib.MOTION_LEVELS, lib.MOTION_RANGE, lib.MOTION_PENALTY)
    args = parse("--video", "--motion", "--mode", "16x", "--motion_levels", "1", "--motion_range", "0", "--motion_penalty", "255")
    cli.check_motion_args(args)
    assert (args.motion_levels, args.motion_range, args.motion_penalty) == (1, 0, 255)
    plain = parse("--video", "--mode", "16x")                                # --video without --motion: nothing to check, nothing filled in
    cli.check_motion_args(plain)
    assert not plain.motion and plain.motion_levels is None
    cli.check_motion_args(parse("--mode", "16x"))
    for flag, value in (("--motion", None), ("--motion_levels", "2"), ("--motion_range", "3"), ("--motion_penalty", "0")):
        extra = [flag] if value is None else [flag, value]
        with pytest.raises(ValueError, match="%s does nothing without --video" % flag):
            cli.check_motion_args(parse("--mode", "16x", *extra))
        cli.check_video_args(parse("--mode", "16x", *extra))                 # the video check neither knows nor minds them
        if value is not None:
            with pytest.raises(ValueError, match="%s does nothing without --motion" % flag):
                cli.check_motion_args(parse("--video", "--mode", "16x", flag, value))
    for flag, value in (("--motion_levels", "0"), ("--motion_levels", "5"), ("--motion_range", "-1"), ("--motion_range", "8"), ("--motion_penalty", "-1"),
                        ("--motion_penalty", "256")):
        with pytest.raises(ValueError, match=flag):
            cli.check_motion_args(parse("--video", "--motion", "--mode", "16x", flag, value))


def test_check_video_args_accepts_what_it_accepted():
    args = parse("--video", "--motion", "--motion_range", "7", "--mode", "16x")
    cli.check_video_args(args)                                               # fills in its own defaults, leaves the motion flags alone
    assert (args.temporal_rate, args.temporal_blend, args.motion_range, args.motion_levels) == (lib.CLIP_RATE, lib.CLIP_BLEND, 7, None)
    with pytest.raises(ValueError, match="--temporal_rate does nothing without --video"):
        cli.check_video_args(parse("--mode", "16x", "--temporal_rate", "0.5", "--motion"))
