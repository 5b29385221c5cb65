"""Scale control without a GPU: the numpy reference (tests/scale_oracle.py) against Pillow's own float path and against its identities,
the new public header and its bindings, wct_scale_shape (host only), and the command line's --level_scale / --scale_detail / --coarse_style."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import scale_oracle as O
from tests.conftest import PKG, REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_scale.h")
FILTERS = [O.BILINEAR, O.BICUBIC]
# both directions of the issue's pairs, an enlargement, a reduction, a one-sample result and a three-sample source
PILLOW_SHAPES = [((131, 257), (16, 32)), ((16, 32), (131, 257)), ((96, 128), (208, 272)), ((208, 280), (48, 64)), ((5, 7), (1, 1)), ((1, 3), (4, 9))]


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("src,dst", PILLOW_SHAPES, ids=lambda v: "%dx%d" % v)
def test_oracle_against_pillows_float_path(src, dst, name):
    """Image.fromarray(x, "F").resize: fp64 weights and sums, ONE fp32 rounding between the passes and one at the end -- each at most
    u A max|x| of the pass's result, so 4 u A_h A_v max|x| holds both with room."""
    Image = pytest.importorskip("PIL.Image")
    flt = {O.BILINEAR: Image.BILINEAR, O.BICUBIC: Image.BICUBIC}[name]
    x = O.image(src, 7)
    want = O.resample(x, dst[0], dst[1], name)
    got = np.stack([np.asarray(Image.fromarray(x[c], "F").resize((dst[1], dst[0]), flt), np.float64) for c in range(3)])
    _, ah = O.axis_stats(src[1], dst[1], name)
    _, av = O.axis_stats(src[0], dst[0], name)
    bound = 4 * O.U * ah * av * float(np.abs(x).max())
    dist = float(np.abs(got - want).max())
    print("pillow %s %s->%s: distance %.3g, bound %.3g" % (name, src, dst, dist, bound))
    assert dist <= bound


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("n_in,n_out", [(257, 32), (32, 257), (280, 272), (280, 280), (7, 1), (3, 9), (3840, 960), (528, 1072), (2160, 32)])
def test_every_weight_row_is_a_partition_of_unity(n_in, n_out, name):
    rows = O.axis_rows(n_in, n_out, name)
    assert len(rows) == n_out
    support = O.FILTER_SUPPORT[name] * max(n_in / n_out, 1.0)
    for lo, w in rows:
        assert 0 <= lo and lo + len(w) <= n_in and 1 <= len(w) <= 2 * int(np.ceil(support)) + 1
        assert abs(float(w.sum()) - 1.0) <= 4 * len(w) * 2.0 ** -53
    los = [lo for lo, _ in rows]
    his = [lo + len(w) for lo, w in rows]
    assert los == sorted(los) and his == sorted(his)              # the kernel spans a tile's window by its first and last sample
    assert abs(float(O.axis_matrix(n_in, n_out, name).sum(1).max()) - 1.0) < 1e-13


@pytest.mark.parametrize("name", FILTERS)
def test_oracle_identities(name):
    x = O.image((21, 34), 3)
    assert np.array_equal(O.resample(x, 21, 34, name), x.astype(np.float64))            # equal sizes: weights (0, 1, 0, 0)
    flat = np.full((3, 9, 13), 0.375)
    assert np.abs(O.resample(flat, 31, 5, name) - 0.375).max() < 1e-15                  # constants survive (partition of unity)
    ramp = np.broadcast_to(np.arange(40, dtype=np.float64), (3, 6, 40))
    up = O.resample(ramp, 6, 80, name)[0, 0, 8:-8]                                      # both filters reproduce a linear ramp off the edges
    assert np.abs(up - ((np.arange(80) + 0.5) * 0.5 - 0.5)[8:-8]).max() < 1e-12
    a, b, c = (O.image(s, seed).astype(np.float64) for s, seed in (((12, 16), 4), ((12, 16), 5), ((24, 40), 6)))
    assert np.array_equal(O.merge(a, b, c, 0.0), O.resample(a, 24, 40, O.BICUBIC))
    both = O.resample(a, 24, 40, O.BICUBIC) - 0.75 * O.resample(b, 24, 40, O.BICUBIC) + 0.75 * c   # linearity: one upsampling of a difference
    assert np.abs(O.merge(a, b, c, 0.75) - both).max() < 1e-14
    assert np.abs(O.merge(b, b, c, 1.0) - c).max() < 1e-14                              # nothing changed at the coarse size: the fine content


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("src,dst", [((131, 257), (16, 32)), ((16, 32), (131, 257)), ((5, 7), (1, 1)), ((1, 3), (4, 9)), ((40, 150), (16, 64))],
                         ids=lambda v: "%dx%d" % v)
def test_a_plain_fp32_evaluation_stays_inside_the_device_bound(src, dst, name):
    x = O.image(src, 11)
    dist = float(np.abs(O.resample_f32(x, dst[0], dst[1], name).astype(np.float64) - O.resample(x, dst[0], dst[1], name)).max())
    bound = O.resample_bound(src, dst[0], dst[1], name, float(np.abs(x).max()))
    print("fp32 emulation %s %s->%s: distance %.3g, bound %.3g" % (name, src, dst, dist, bound))
    assert dist <= bound


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def declared():
    return sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"wct_ctx"})


def test_header_and_symbol_list_agree():
    assert declared() and declared() == sorted(lib.SYMBOLS_SCALE)
    others = set(lib.SYMBOLS) | set(lib.SYMBOLS_COLOR) | set(lib.SYMBOLS_SMOOTH) | set(lib.SYMBOLS_TRANSFORM) | set(lib.SYMBOLS_SWAP)
    assert not set(lib.SYMBOLS_SCALE) & others
    text = open(HEADER).read()
    for name, value in (("WCT_SCALE_MAX_DIVISOR", lib.SCALE_MAX_DIVISOR), ("WCT_SCALE_MAX_SHRINK", lib.SCALE_MAX_SHRINK),
                        ("WCT_SCALE_DETAIL", lib.SCALE_DETAIL)):
        m = re.search(r"#define %s\s+(\S+)" % name, text)
        assert m and float(m.group(1)) == float(value), name
    main = open(os.path.join(REPO, "include", "wct_hip.h")).read()
    for name, key in (("WCT_FILTER_BILINEAR", O.BILINEAR), ("WCT_FILTER_BICUBIC", O.BICUBIC)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, main).group(1)) == lib.RESIZE_FILTERS[key]


def test_built_library_exports_the_scale_entries():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_SCALE:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_SCALE) <= exported


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_scale.c"
    src.write_text('#include "wct_hip_scale.h"\n'
                   "int main(void) { return (WCT_SCALE_MAX_DIVISOR == 16 && WCT_SCALE_MAX_SHRINK == 32 && WCT_SCALE_DETAIL == 1.0 && "
                   "WCT_FILTER_BICUBIC == 1) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "only_scale.o")], check=True)


def test_the_tile_the_gpu_test_names_is_the_kernels():
    text = open(os.path.join(PKG, "csrc", "scale.hip")).read()
    m = re.search(r"SC_TILE_W = (\d+), SC_TILE_H = (\d+);", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (O.TILE_W, O.TILE_H)
    assert int(re.search(r"SC_TILE_W_NARROW = (\d+);", text).group(1)) == O.TILE_W_NARROW
    assert ".commit(" not in text and "sat_raise(" not in text           # the resampler and the merge clamp nothing
    build = open(os.path.join(PKG, "build.sh")).read()
    assert re.search(r'^SRC=".*\bscale\b.*"', build, re.M) and "../include/wct_hip_scale.h" in build


def test_scale_shape_is_the_formula_and_refuses_small_working_sizes():
    L = lib.load()
    h, w = ctypes.c_int(-1), ctypes.c_int(-1)
    for H, W in ((208, 280), (272, 300), (2160, 3840), (100, 130), (32, 32), (511, 512), (767, 33 * 16 - 1)):
        for d in range(1, lib.SCALE_MAX_DIVISOR + 1):
            want = (16 * (H // (16 * d)), 16 * (W // (16 * d)))
            h.value = w.value = -1
            rc = L.wct_scale_shape(H, W, d, ctypes.byref(h), ctypes.byref(w))
            if min(want) >= 32:
                assert rc == lib.WCT_OK and (h.value, w.value) == want, (H, W, d)
            else:
                assert rc == lib.WCT_ERR_INVALID and (h.value, w.value) == (-1, -1), (H, W, d)
    assert L.wct_scale_shape(208, 280, 4, ctypes.byref(h), ctypes.byref(w)) == lib.WCT_OK and (h.value, w.value) == (48, 64)
    assert L.wct_scale_shape(208, 280, 8, ctypes.byref(h), ctypes.byref(w)) == lib.WCT_ERR_INVALID          # 16 x 32: under 32
    for bad in ((208, 280, 0), (208, 280, 17), (0, 280, 1), (208, -1, 1)):
        assert L.wct_scale_shape(*bad, ctypes.byref(h), ctypes.byref(w)) == lib.WCT_ERR_INVALID
    assert L.wct_scale_shape(208, 280, 1, None, ctypes.byref(w)) == lib.WCT_ERR_INVALID
    from wct_hip import WCT
    assert WCT.scale_shape(272, 300, 8) == (32, 32)
    with pytest.raises(ValueError, match="scale_shape"):
        WCT.scale_shape(208, 280, 8)


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    args = cli.build_parser().parse_args(["--mode", "16x"] + list(argv))
    args.outf, args.log_mark = "out", "M"
    return args


def test_parser_accepts_the_flags_and_defaults_to_off():
    a = parse()
    assert a.level_scale is None and a.scale_detail is None and a.coarse_style is None
    cli.check_scale_args(a)
    assert a.scale_detail is None
    a = parse("--level_scale", "4,4,2,1,1")
    cli.check_scale_args(a)
    assert cli.level_scale_list(a.level_scale) == (4, 4, 2, 1, 1) and a.scale_detail == lib.SCALE_DETAIL
    a = parse("--level_scale", "8, 4,2,1,1", "--scale_detail", "0", "--coarse_style", "b.png", "--transform", "ot", "--preserve_color", "match",
              "--smooth_radius", "4", "--numpy")
    cli.check_color_args(a)
    cli.check_smooth_args(a)
    cli.check_scale_args(a)
    assert cli.level_scale_list(a.level_scale) == (8, 4, 2, 1, 1) and a.scale_detail == 0.0 and a.coarse_style == "b.png"
    cli.check_scale_args(parse("--level_scale", "1,1,1,1,1"))
    assert "not a measurement" in cli.build_parser().format_help().replace("\n", " ").replace("  ", " ")


@pytest.mark.parametrize("argv,words", [
    (["--level_scale", "4,4,2,1"], "five divisors"),
    (["--level_scale", "4,4,2,1,1,1"], "five divisors"),
    (["--level_scale", "4,4,x,1,1"], "integers"),
    (["--level_scale", "4,4,2.5,1,1"], "integers"),
    (["--level_scale", "17,4,2,1,1"], "1 .. 16"),
    (["--level_scale", "4,0,0,0,0"], "1 .. 16"),
    (["--level_scale", "2,4,2,1,1"], "must not increase"),
    (["--level_scale", "4,4,2,1,2"], "must not increase"),
    (["--level_scale", "4,4,2,2,2"], "level 1 must be 1"),
    (["--level_scale", "4,4,2,1,1", "--scale_detail", "-0.5"], "--scale_detail"),
    (["--level_scale", "4,4,2,1,1", "--scale_detail", "inf"], "--scale_detail"),
    (["--level_scale", "4,4,2,1,1", "--scale_detail", "nan"], "--scale_detail"),
    (["--level_scale", "1,1,1,1,1", "--coarse_style", "b.png"], "--coarse_style does nothing"),
    (["--scale_detail", "0.5"], "--scale_detail does nothing without --level_scale"),
    (["--coarse_style", "b.png"], "--coarse_style does nothing without --level_scale"),
])
def test_bad_values_are_refused_with_a_message(argv, words):
    with pytest.raises(ValueError) as e:
        cli.check_scale_args(parse(*argv))
    assert words in str(e.value)


@pytest.mark.parametrize("extra,name", [
    (["--synthesis"], "--synthesis"),
    (["--maskPath", "m", "--region_styles", "a.png"], "--maskPath"),
    (["--interp_styles", "a.png,b.png"], "--interp_styles"),
    (["--interp_styles", "a.png", "--weightPath", "w"], "--weightPath"),
    (["--swap_level", "3"], "--swap_level"),
])
def test_refusals_name_both_flags(extra, name):
    with pytest.raises(ValueError) as e:
        cli.check_scale_args(parse("--level_scale", "4,4,2,1,1", *extra))
    assert "--level_scale" in str(e.value) and name in str(e.value)


def test_main_refuses_before_it_creates_anything(tmp_path):
    out = tmp_path / "never"
    with pytest.raises(ValueError, match="--level_scale does not mix with --swap_level"):
        cli.main(["--mode", "16x", "--outf", str(out), "--level_scale", "4,4,2,1,1", "--swap_level", "3"])
    assert not out.exists()


def test_out_name_carries_the_scale_mark_only_with_the_flag():
    plain = parse()
    assert cli.out_name(plain, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_a+b.jpg")
    assert cli.out_name(parse("--level_scale", "4,4,2,1,1"), "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_scale=4-4-2-1-1_a+b.jpg")
    full = parse("--level_scale", "8,4,2,1,1", "--transform", "ot", "--preserve_color", "luma", "--smooth_radius", "8")
    assert cli.out_name(full, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_transform=ot_scale=8-4-2-1-1_color=luma_smooth=8_a+b.jpg")
    # every name from before the flag stays as it is
    assert cli.out_name(parse("--swap_level", "4"), "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_swap=4_a+b.jpg")
    old = parse("--transform", "adain", "--preserve_color", "match", "--smooth_radius", "3")
    assert cli.out_name(old, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_transform=adain_color=match_smooth=3_a+b.jpg")
    legacy = types.SimpleNamespace(outf="out", log_mark="M", mode="16x", alpha=1)       # a namespace from before the flag
    assert cli.out_name(legacy, "a+b.jpg") == cli.out_name(plain, "a+b.jpg")


class _FakeEngine:
    """The engine surface _scale_pair uses, with the real one's range behaviour: sync() raises on a pending clamp."""

    def __init__(self, clamps):
        self.clamps, self.pending, self.calls, self.mode = list(clamps), 0, [], "f16x3"

    def color_match(self, style, content):
        self.calls.append(("color_match", style, content))
        return "matched " + style

    def style_prepare(self, style, levels):
        self.calls.append(("style_prepare", self.mode, style, tuple(levels)))

    def stylize_scaled(self, c, s, div, gain, alpha, num_run):
        self.pending = self.clamps.pop(0)
        self.calls.append(("stylize_scaled", self.mode, c, s, tuple(div), gain, alpha, num_run))
        return "result under %s" % self.mode

    def saturation_count(self, reset=False):
        n = self.pending
        if reset:
            self.pending = 0
        return n

    def set_conv_mode(self, mode):
        self.mode = mode

    def sync(self):
        if self.pending:
            self.pending = 0
            raise OverflowError("an earlier call clamped")


@pytest.mark.parametrize("clamps,modes", [([0], ["f16x3"]), ([5, 0], ["f16x3", "fp32"])])
def test_scale_pair_recomputes_in_fp32_after_a_clamp(clamps, modes):
    eng, log = _FakeEngine(clamps), []
    args = parse("--level_scale", "4,4,2,1,1", "--alpha", "0.5", "--num_run", "2")
    cli.check_scale_args(args)
    res = cli._scale_pair(eng, args, log.append, "content", lambda: "style", lambda: None)
    runs = [c for c in eng.calls if c[0] == "stylize_scaled"]
    assert [c[1] for c in runs] == modes and res == "result under %s" % modes[-1]
    assert all(c[2:] == ("content", "style", (4, 4, 2, 1, 1), 1.0, 0.5, 2) for c in runs)
    assert eng.mode == "f16x3" and eng.pending == 0 and len(log) == len(modes) - 1
    if log:
        assert "recomputing it with exact-fp32 convolutions" in log[0]
    eng.sync()          # nothing is left pending for a later call to trip over


def test_scale_pair_prepares_the_coarse_style_on_the_reduced_levels():
    eng = _FakeEngine([0])
    args = parse("--level_scale", "4,4,2,1,1", "--coarse_style", "b.png", "--preserve_color", "match", "--scale_detail", "0.5")
    cli.check_scale_args(args)
    cli._scale_pair(eng, args, lambda m: None, "content", lambda: "A", lambda: "B")
    assert eng.calls == [("color_match", "A", "content"), ("color_match", "B", "content"),
                         ("style_prepare", "f16x3", "matched B", (5, 4, 3)), ("style_prepare", "f16x3", "matched A", (2, 1)),
                         ("stylize_scaled", "f16x3", "content", None, (4, 4, 2, 1, 1), 0.5, 1, 1)]
