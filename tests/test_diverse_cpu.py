"""Seeded style variations without a GPU: the public header and its bindings, identities of the numpy restatement
(tests/diverse_oracle.py), and the command line's --diversity / --variations / --diversity_levels."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import diverse_oracle as D
from tests import synth_oracle as S
from tests.conftest import PKG, REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_diverse.h")
OTHER_LISTS = ("SYMBOLS", "SYMBOLS_COLOR", "SYMBOLS_SMOOTH", "SYMBOLS_TRANSFORM", "SYMBOLS_SWAP", "SYMBOLS_ATTN", "SYMBOLS_SCALE", "SYMBOLS_GUIDED",
               "SYMBOLS_VIDEO", "SYMBOLS_MOTION")
DECL = r"\b(wct_[a-z_0-9]+)\s*\("


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def test_header_and_symbol_list_agree():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(DECL, text)) - {"wct_ctx"})
    assert declared and declared == sorted(lib.SYMBOLS_DIVERSE) and len(set(lib.SYMBOLS_DIVERSE)) == len(lib.SYMBOLS_DIVERSE)
    for other in OTHER_LISTS:
        assert not set(lib.SYMBOLS_DIVERSE) & set(getattr(lib, other)), other
    inc = os.path.join(REPO, "include")
    for name in os.listdir(inc):                                            # declared here and nowhere else
        if name != "wct_hip_diverse.h":
            assert not set(lib.SYMBOLS_DIVERSE) & set(re.findall(DECL, open(os.path.join(inc, name)).read())), name
    m = re.search(r"#define WCT_DIVERSE_MAX_STRENGTH\s+(\S+)", text)
    assert m and float(m.group(1)) == float(lib.DIVERSE_MAX_STRENGTH) == float(D.MAX_STRENGTH) == 8.0
    assert "0x%08X" % D.TAG_BASE in text and "composes" in text.lower() and "wct_reserve" in text     # the definition, composition, the workspace rule
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):                             # the header states the generator
        assert word in text
    assert lib.DIVERSE_LEVELS == (5,)


def test_the_sources_are_listed_and_clamp_nothing():
    build = open(os.path.join(PKG, "build.sh")).read()
    assert re.search(r'^SRC=".*\brotate\b.*\bapi_diverse\b.*"', build, re.M) and "../include/wct_hip_diverse.h" in build
    for name in ("rotate.hip", "api_diverse.hip"):
        text = open(os.path.join(PKG, "csrc", name)).read()
        assert ".commit(" not in text and "sat_raise(" not in text and "atomic" not in text
    src = open(os.path.join(PKG, "csrc", "rotate.hip")).read()
    assert "0x%08X" % D.TAG_BASE + "u" in src


def test_built_library_exports_the_entries_and_hides_the_helpers():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_DIVERSE:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_DIVERSE) <= exported
    assert not [s for s in exported if re.search(r"rotation|divers", s) and s not in lib.SYMBOLS_DIVERSE]


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_diverse.c"
    src.write_text('#include "wct_hip_diverse.h"\n'
                   "int main(void) { return (WCT_DIVERSE_MAX_STRENGTH == 8 && sizeof(&wct_rotation_make) && sizeof(&wct_style_diversify) &&\n"
                   "  sizeof(&wct_stylize_diverse)) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "only_diverse.o")], check=True)


def test_product_keeps_the_test_oracle_out():
    for rel in ("csrc/rotate.hip", "csrc/api_diverse.hip", "wct_hip/lib.py", "wct_hip/wct.py", "wct_hip/cli.py"):
        text = open(os.path.join(PKG, rel)).read()
        assert not re.search(r"import\s+diverse_oracle|from tests", text), rel


# ---------------------------------------------------------------------------------------------------------------- the oracle itself
WIDTHS = (2, 6, 8, 24, 64, 128, 144, 512)


@pytest.mark.parametrize("C", WIDTHS)
def test_oracle_skew_is_skew_bit_for_bit_and_the_rotation_is_orthogonal(C):
    for strength in (0.25, 1.0, 8.0):
        A = D.skew(C, 11, 3, 5, strength)
        assert np.array_equal(A, -A.T) and not np.diag(A).any() and np.count_nonzero(A) >= C * C - C - 2
        Z = D.rotation(C, 11, 3, 5, strength)
        e = float(np.abs(Z.T @ Z - np.eye(C)).max())
        I = np.eye(C)
        back = float(np.abs(Z @ (I + A) - (I - A)).max())
        print("C=%d strength %g: |Z^T Z - I| %.2e, |Z (I + A) - (I - A)| %.2e" % (C, strength, e, back))
        assert e < 1e-13 and back < 1e-13 * max(1.0, strength)
    assert np.array_equal(D.rotation(C, 11, 3, 5, 0.0), np.eye(C))
    assert np.array_equal(D.skew(C, 11, 3, 5, 0.0), np.zeros((C, C)))


def test_oracle_words_are_the_noise_generator_s_with_the_tag_word():
    C, seed, sid, tag = 6, (7 << 32) | 9, 4, 200
    g = D.words(C, seed, sid, tag)
    for e in (0, 5, 17, 35):
        w = S.philox4x32_10((e >> 2, 0, sid, D.TAG_BASE | tag), (seed & S.MASK, seed >> 32))
        v = int(w[e & 3])
        assert int(g[e // C, e % C]) == (v - (1 << 32) if v >= 1 << 31 else v)
    assert all(D.tag_word(t) != 0 and D.tag_word(t) >> 8 == D.TAG_BASE >> 8 for t in range(256))     # never the noise image's 0
    assert len({D.tag_word(t) for t in range(256)}) == 256
    for bad in (-1, 256):
        with pytest.raises(AssertionError):
            D.tag_word(bad)
    # the scale, in the stated order
    assert D.scale(24, 1.0) == 1.0 / (2.0 * float(np.sqrt(np.float64(16.0)))) == 0.125
    assert D.scale(6, 8.0) == 8.0 / (2.0 * 2.0)


@pytest.mark.parametrize("C", (6, 24, 64))
def test_oracle_seed_stream_and_tag_each_change_most_entries(C):
    base = D.rotation(C, 1, 0, 5, 1.0)
    for what, other in (("seed", D.rotation(C, 2, 0, 5, 1.0)), ("seed high word", D.rotation(C, 1 | (1 << 32), 0, 5, 1.0)),
                        ("stream", D.rotation(C, 1, 1, 5, 1.0)), ("tag", D.rotation(C, 1, 0, 4, 1.0))):
        changed = float((other != base).mean())
        assert changed > 0.5, (what, changed)
    assert np.array_equal(D.rotation(C, 1, 0, 5, 1.0), base)


def test_oracle_spectral_radius_and_the_condition_of_b():
    """The scale puts the spectral radius of A / strength just under 1 (semicircle law: 2 sigma sqrt(C) with sigma^2 = 2 s^2 / 3), so
    B = I - A A has its eigenvalues in [1, 1 + strength^2 rho^2]: cond(B) stays near 65 at the largest strength."""
    for C in (8, 24, 64, 128, 512):
        rho = D.spectral_radius(C, 0, 0, 5)
        A = D.skew(C, 0, 0, 5, 8.0)
        lam = np.linalg.eigvalsh(np.eye(C) - A @ A)
        print("C=%d: spectral radius of A / strength %.3f, cond(B) at strength 8 %.1f" % (C, rho, lam.max() / lam.min()))
        assert 0.4 < rho < 1.05 and lam.min() >= 1.0 - 1e-12 and lam.max() / lam.min() < 1 + 64 * 1.05 ** 2
        assert C < 24 or rho > 0.8


def test_oracle_rotated_slot_reaches_the_same_target_through_a_different_map():
    from tests import transform_oracle as O
    from tests.transform_cases import make_case
    n, s, ss, st = make_case(5, 32, 1e-2, 1e-2)
    Z = D.rotation(32, 3, 0, 5, 1.0)
    Sm, _ = O.split_stats(st)
    _, cov_c = O.mean_cov(n, s, ss)
    T0, T1 = O.T_wct(cov_c, Sm), D.T_diverse(cov_c, Sm, Z)
    assert np.abs(T1 @ cov_c @ T1.T - Sm @ Sm.T).max() < 1e-10 and np.abs(T0 @ cov_c @ T0.T - Sm @ Sm.T).max() < 1e-10
    assert np.abs(T1 - T0).max() > 0.1 * np.abs(T0).max()
    M, b = D.solve(n, s, ss, st, np.eye(32), 0.6)
    M0, b0 = O.solve("wct", n, s, ss, st, 0.6)
    assert np.array_equal(M, M0) and np.array_equal(b, b0)
    assert np.array_equal(D.rotate_stats(st, np.eye(32)), st)


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    args = cli.build_parser().parse_args(["--mode", "16x"] + list(argv))
    args.outf, args.log_mark = "out", "M"
    return args


def checked(*argv):
    a = parse(*argv)
    cli.check_synthesis_args(a)
    cli.check_diverse_args(a)
    return a


def test_parser_defaults_and_filling():
    a = parse()
    assert (a.diversity, a.variations, a.diversity_levels) == (None, None, None)
    cli.check_diverse_args(a)
    assert (a.diversity, a.variations, a.diversity_levels) == (None, None, None) and cli.select_mode(a) is None
    a = checked("--diversity", "1.5")
    assert (a.diversity, a.variations, a.diversity_levels, a.seed) == (1.5, 1, (5,), 0)
    a = checked("--diversity", "8", "--variations", "64", "--diversity_levels", "5,4,1", "--seed", str(2 ** 64 - 1))
    assert (a.diversity, a.variations, a.diversity_levels, a.seed) == (8.0, 64, (5, 4, 1), 2 ** 64 - 1)
    cli.check_diverse_args(a)                                                                  # a second look changes nothing
    assert a.diversity_levels == (5, 4, 1)
    mode = cli.select_mode(a)
    assert mode is cli.DIVERSE_MODE and mode not in cli.MODES and (mode.name, mode.noun, mode.early) == ("diverse", "image", True)
    assert mode.reason.startswith("--diversity")
    # what goes with it
    for extra in (["--alpha", "0.6", "--num_run", "2"], ["--preserve_color", "luma"], ["--smooth_radius", "4"], ["--transform", "wct"]):
        a = checked("--diversity", "1", *extra)
        assert cli.select_mode(a) is cli.DIVERSE_MODE
    a = parse("--diversity", "2", "--video", "--diversity_levels", "5,4")
    cli.check_video_args(a)
    cli.check_diverse_args(a)
    assert cli.select_mode(a).name == "video" and a.variations == 1 and a.diversity_levels == (5, 4)
    cli.check_diverse_args(parse("--diversity", "2", "--video", "--variations", "1"))


def test_every_refusal_by_message():
    for argv in (["--variations", "2"], ["--variations", "1"]):
        with pytest.raises(ValueError, match="--variations does nothing without --diversity"):
            checked(*argv)
    with pytest.raises(ValueError, match="--diversity_levels does nothing without --diversity"):
        checked("--diversity_levels", "5")
    with pytest.raises(ValueError, match="--seed needs --synthesis or --diversity"):
        checked("--seed", "3", "--variations", "2")
    for bad in ("0", "-1", "8.5", "nan", "inf"):
        with pytest.raises(ValueError, match=r"--diversity: a strength in \(0, 8\]"):
            checked("--diversity", bad)
    for bad in ("0", "65", "-3"):
        with pytest.raises(ValueError, match=r"--variations: 1 \.\. 64"):
            checked("--diversity", "1", "--variations", bad)
    for bad in ("", "0", "6", "5,5", "5,x", "4;5"):
        with pytest.raises(ValueError, match="--diversity_levels"):
            checked("--diversity", "1", "--diversity_levels", bad)
    for bad in ("-1", str(2 ** 64)):
        with pytest.raises(ValueError, match="--seed"):
            checked("--diversity", "1", "--seed", bad)
    for argv, name in ((["--transform", "ot"], "--transform ot"), (["--transform", "adain"], "--transform adain"), (["--numpy"], "--numpy"),
                       (["--synthesis"], "--synthesis"), (["--maskPath", "m", "--region_styles", "s.png"], "--maskPath"),
                       (["--interp_styles", "a.png,b.png", "--interp_weights", "1,1"], "--interp_styles"),
                       (["--interp_styles", "a.png,b.png", "--weightPath", "w"], "--interp_styles, --weightPath"), (["--swap_level", "3"], "--swap_level"),
                       (["--level_scale", "2,2,1,1,1"], "--level_scale"), (["--auto_regions", "2"], "--auto_regions"),
                       (["--preserve_color", "match"], "--preserve_color match")):
        with pytest.raises(ValueError, match="--diversity does not mix with %s" % re.escape(name)):
            checked("--diversity", "1", *argv)
    with pytest.raises(ValueError, match="--video takes one variation"):
        checked("--diversity", "1", "--video", "--variations", "2")
    with pytest.raises(ValueError, match="--diversity does not mix with --transform ot"):
        cli.main(["--mode", "16x", "--diversity", "1", "--transform", "ot", "--outf", os.path.join(os.sep, "nonexistent", "never_made")])


def test_out_names_with_and_without_the_flags():
    assert cli.out_name(parse(), "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_a+b.jpg")                          # as before
    assert cli.out_name(parse("--transform", "ot", "--preserve_color", "luma"), "a+b.jpg") == os.path.join(
        "out", "M_mode=16x_alpha=1_transform=ot_color=luma_a+b.jpg")                                                      # as before
    a = checked("--diversity", "1.5")
    assert cli.out_name(a, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_div=1.5_a+b.jpg")
    a = checked("--diversity", "2", "--variations", "3", "--preserve_color", "luma", "--smooth_radius", "4", "--alpha", "0.6")
    assert cli.out_name(a, "a+b.jpg", 2) == os.path.join("out", "M_mode=16x_alpha=0.6_div=2_color=luma_smooth=4_v2_a+b.jpg")
    assert cli.out_name(a, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=0.6_div=2_color=luma_smooth=4_a+b.jpg")


class _FakeEngine:
    def __init__(self, clamps=()):
        self.calls, self.clamps, self.passes = [], list(clamps), 0

    def style_prepare(self, s):
        self.calls.append(("prepare", s))

    def style_export(self, L):
        self.calls.append(("export", L))
        return "stats%d" % L

    def style_import(self, L, stats):
        self.calls.append(("import", L, stats))

    def style_diversify(self, strength, seed, stream_id, levels):
        self.calls.append(("diversify", strength, seed, stream_id, tuple(levels)))

    def stylize_prepared(self, c, alpha, num_run):
        self.calls.append(("stylize", c, alpha, num_run))
        return "result"

    def saturation_count(self, reset=False):
        self.passes += 1
        return 1 if self.passes in self.clamps else 0

    def set_conv_mode(self, mode):
        self.calls.append(("conv", mode))

    def sync(self):
        pass


def _drive(monkeypatch, eng, *argv):
    a = checked("--diversity", "2", "--seed", "9", "--alpha", "0.5", *argv)
    seen = []
    monkeypatch.setattr(cli, "_device_images", lambda limit: lambda path: "u8:" + os.path.basename(path))
    monkeypatch.setattr(cli, "_to_tensor", lambda wct, u8, size: "f32:" + u8)
    monkeypatch.setattr(cli, "_run_jobs", lambda args, wct, log, jobs: seen.extend(jobs) or 0.0)
    total, n = cli.run_diverse(a, eng, [("c1.png", "s1.png"), ("c2.png", "s1.png")], "content", "style", lambda s: None)
    assert n == len(seen)
    for job in seen:
        assert job.content in (os.path.join("content", "c1.png"), os.path.join("content", "c2.png"))
        assert job.stylise("C", job.before(None)) == "result"
    return [os.path.basename(j.out) for j in seen]


def test_run_diverse_prepares_once_per_pair_and_rotates_per_variation(monkeypatch):
    eng = _FakeEngine()
    names = _drive(monkeypatch, eng, "--variations", "2", "--diversity_levels", "5,2")
    assert names == ["M_mode=16x_alpha=0.5_div=2_v0_c1+s1.jpg", "M_mode=16x_alpha=0.5_div=2_v1_c1+s1.jpg",
                     "M_mode=16x_alpha=0.5_div=2_v0_c2+s1.jpg", "M_mode=16x_alpha=0.5_div=2_v1_c2+s1.jpg"]
    pair = lambda: [("prepare", "f32:u8:s1.png"), ("export", 5), ("export", 2), ("diversify", 2.0, 9, 0, (5, 2)), ("stylize", "C", 0.5, 1),
                    ("import", 5, "stats5"), ("import", 2, "stats2"), ("diversify", 2.0, 9, 1, (5, 2)), ("stylize", "C", 0.5, 1)]
    assert eng.calls == pair() + pair()


def test_run_diverse_recompute_prepares_afresh_and_keeps_nothing_of_it(monkeypatch):
    eng = _FakeEngine(clamps=[1])                    # the first pass of the first image clamps
    names = _drive(monkeypatch, eng)
    assert names == ["M_mode=16x_alpha=0.5_div=2_c1+s1.jpg", "M_mode=16x_alpha=0.5_div=2_c2+s1.jpg"]
    first = [("prepare", "f32:u8:s1.png"), ("export", 5), ("diversify", 2.0, 9, 0, (5,)), ("stylize", "C", 0.5, 1)]
    again = [("conv", "fp32"), ("prepare", "f32:u8:s1.png"), ("diversify", 2.0, 9, 0, (5,)), ("stylize", "C", 0.5, 1), ("conv", "f16x3")]
    assert eng.calls == first + again + first
