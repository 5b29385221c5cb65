"""Guided-filter smoothing without a GPU: the numpy reference (tests/smooth_oracle.py) against a brute-force box filter and three
exact identities of the filter, the new public header and its bindings, and the command line's --smooth_radius / --smooth_eps."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import color_oracle as CO
from tests import smooth_oracle as O
from tests.conftest import REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_smooth.h")


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("r", [1, 3, 9])
def test_oracle_box_mean_against_a_double_loop(r):
    x = np.random.default_rng(r).random((5, 7)) * 3 - 1
    assert np.abs(O.box_mean(x, r) - O.box_mean_brute(x, r)).max() <= 1e-14
    assert np.array_equal(O.box_count(5, 7, r), O.box_sum_axis(O.box_sum_axis(np.ones((5, 7)), r, 0), r, 1))
    if r == 9:      # larger than the image: the window is the image
        assert np.abs(O.box_mean(x, r) - x.mean()).max() <= 1e-14


SHAPES = [(33, 65, 4), (120, 90, 25)]


@pytest.mark.parametrize("H,W,r", SHAPES)
def test_oracle_constant_source_comes_back_constant(H, W, r):
    guide = CO.natural(1, H, W)
    const = np.broadcast_to(np.array([0.25, -0.125, 1.25])[:, None, None], (3, H, W))
    assert np.abs(O.guided_filter(const, guide, r, 1e-4) - const).max() <= 1e-12


@pytest.mark.parametrize("H,W,r", SHAPES)
def test_oracle_constant_guide_gives_the_box_mean_of_the_box_mean(H, W, r):
    src = CO.natural(2, H, W).astype(np.float64) * 1.5 - 0.2
    guide = np.broadcast_to(np.array([0.5, 0.25, 0.75])[:, None, None], (3, H, W))
    want = O.box_mean(O.box_mean(src, r), r)
    assert np.abs(O.guided_filter(src, guide, r, 1e-4) - want).max() <= 1e-13


@pytest.mark.parametrize("H,W,r", SHAPES)
def test_oracle_affine_function_of_the_guide_comes_back_as_eps_vanishes(H, W, r):
    guide = CO.natural(3, H, W).astype(np.float64)
    M = np.array([[0.9, 0.2, -0.1], [0.1, 0.7, 0.3], [-0.2, 0.1, 1.1]])
    src = np.einsum("ci,ihw->chw", M, guide) + np.array([0.05, -0.1, 0.2])[:, None, None]
    # a = (Sigma0 + eps Id)^-1 Sigma0 M^T exactly, so |a - M^T| <= eps |M| / lambda_min(Sigma0) per window and the result moves by at
    # most that times the guide's spread; the cancellation in Sigma0 (values <= 1, fp64) adds ~1e-15 / lambda_min
    eps = 1e-12
    mean_I = O.box_mean(guide, r)
    Sigma0 = O.box_mean(guide[:, None] * guide[None, :], r) - mean_I[:, None] * mean_I[None, :]
    lam_min = np.linalg.eigvalsh(Sigma0.transpose(2, 3, 0, 1)).min()
    spread = np.linalg.norm(guide.max((1, 2)) - guide.min((1, 2)))
    bound = (eps * np.linalg.norm(M, 2) * spread + 1e-14) / lam_min
    err = np.abs(O.guided_filter(src, guide, r, eps) - src).max()
    print("affine identity %dx%d r=%d: deviation %.2e, bound %.2e (lambda_min %.2e)" % (H, W, r, err, bound, lam_min))
    assert lam_min > 1e-7 and err <= bound <= 1e-5
    # and with a real eps the filter pulls towards the window mean: no longer the identity
    assert np.abs(O.guided_filter(src, guide, r, 1e-2) - src).max() > 1e-3


def test_oracle_reads_the_guides_top_left_window():
    src, guide = CO.natural(4, 32, 48), CO.natural(5, 37, 58)
    assert np.array_equal(O.guided_filter(src, guide, 3, 1e-4), O.guided_filter(src, guide[:, :32, :48], 3, 1e-4))
    a32 = O.guided_filter(src, guide, 3, 1e-4, ab_fp32=True)
    assert 0 < np.abs(a32 - O.guided_filter(src, guide, 3, 1e-4)).max() <= 1e-6      # what storing a, b in fp32 costs


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def declared():
    return sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"wct_ctx"})


def test_header_and_symbol_list_agree():
    assert declared() and declared() == sorted(lib.SYMBOLS_SMOOTH)
    assert not set(lib.SYMBOLS_SMOOTH) & (set(lib.SYMBOLS) | set(lib.SYMBOLS_COLOR))
    for other in ("wct_hip.h", "wct_hip_color.h"):
        text = open(os.path.join(REPO, "include", other)).read()
        assert not set(lib.SYMBOLS_SMOOTH) & set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", text)), other


def test_built_library_exports_the_smoothing_entries():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_SMOOTH:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_SMOOTH) <= exported


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_smooth.c"
    src.write_text('#include "wct_hip_smooth.h"\n'
                   "int use(wct_ctx* c, const float* p, float* q, int* n) {\n"
                   "  return wct_guided_filter(c, p, 1, 2, p, 1, 2, WCT_SMOOTH_MAX_RADIUS, WCT_SMOOTH_EPS, q, 0, 0)\n"
                   "    + wct_stylize_smooth(c, p, 32, 32, p, 32, 32, 1.0f, 1, WCT_COLOR_LUMA, 8, WCT_SMOOTH_EPS, q, n, n + 1) + WCT_OK; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_header_states_its_contract():
    text = open(HEADER).read()
    assert '#include "wct_hip_color.h"' in text and "WCT.py:120-125" in text
    for word in ("CHOLESKY", "ARE stored in fp32", "NOT clamped", "CLIPPED", "No floating-point atomics", "(Ho, Wo, r)", "ORIGINAL content"):
        assert word in text, word


def test_constants_of_the_binding_are_the_headers():
    text = open(HEADER).read()
    assert int(re.search(r"#define WCT_SMOOTH_MAX_RADIUS (\d+)", text).group(1)) == lib.SMOOTH_MAX_RADIUS >= 256
    assert float(re.search(r"#define WCT_SMOOTH_EPS (\S+)", text).group(1)) == lib.SMOOTH_EPS == O.EPS == 1e-3


def test_history_cases_cover_both_entries_and_the_base_shapes():
    from tests import test_smooth_gpu as G          # imports without a GPU
    covered = set(sym for c in G.CASES.values() for sym in c.covers)
    assert covered == set(lib.SYMBOLS_SMOOTH)
    assert set(c.size for c in G.CASES.values()) == {"small", "large"}
    base = [(1, 1, 1), (1, 2, 1), (5, 7, 9), (33, 65, 4), (64, 64, 1), (250, 333, 35), (272, 400, 16), (600, 900, 60), (600, 900, 8),
             (1100, 70, 200), (70, 1100, 200)]
    assert [s[:3] for s in G.SHAPES[:11]] == base
    assert [s[3] for s in G.SHAPES[:11]] == [1e-4] * 8 + [1e-6] + [1e-4] * 2 and G.SHAPES[6][4] == (277, 410)
    assert G.GATE == 2e-5


def test_product_keeps_the_test_oracle_out():
    pkg = os.path.join(REPO, "collaborative-distillation_amd")
    for rel in ("csrc/smooth.hip", "wct_hip/lib.py", "wct_hip/wct.py", "wct_hip/cli.py", "../include/wct_hip_smooth.h"):
        text = open(os.path.join(pkg, rel)).read()
        assert "smooth_oracle" not in text and not re.search(r"wct_oracle|liboracle|oracle/", text), rel


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_parser_flag_defaults():
    assert parse().smooth_radius == 0 and parse().smooth_eps is None
    a = parse("--smooth_radius", "8", "--smooth_eps", "1e-2")
    assert a.smooth_radius == 8 and a.smooth_eps == 1e-2
    with pytest.raises(SystemExit):
        parse("--smooth_radius", "2.5")
    with pytest.raises(SystemExit):
        parse("--smooth_radius")


def test_check_smooth_args_fills_the_default_and_refuses():
    a = parse()
    cli.check_smooth_args(a)
    assert a.smooth_radius == 0 and a.smooth_eps is None
    a = parse("--smooth_radius", "8")
    cli.check_smooth_args(a)
    assert a.smooth_eps == lib.SMOOTH_EPS
    a = parse("--smooth_radius", "8", "--smooth_eps", "1e-2", "--preserve_color", "luma", "--maskPath", "m", "--region_styles", "a.png")
    cli.check_smooth_args(a)
    assert a.smooth_eps == 1e-2
    cli.check_smooth_args(parse("--smooth_radius", "8", "--interp_styles", "a.png,b.png", "--weightPath", "w"))
    cli.check_smooth_args(parse("--smooth_radius", str(lib.SMOOTH_MAX_RADIUS), "--preserve_color", "match"))
    cli.check_smooth_args(types.SimpleNamespace(synthesis=False))          # a namespace from before the flags existed
    with pytest.raises(ValueError, match="--synthesis"):
        cli.check_smooth_args(parse("--smooth_radius", "8", "--synthesis"))
    with pytest.raises(ValueError, match="--smooth_eps does nothing without --smooth_radius"):
        cli.check_smooth_args(parse("--smooth_eps", "1e-3"))
    with pytest.raises(ValueError, match="--smooth_radius"):
        cli.check_smooth_args(parse("--smooth_radius", "-1"))
    with pytest.raises(ValueError, match="--smooth_radius"):
        cli.check_smooth_args(parse("--smooth_radius", str(lib.SMOOTH_MAX_RADIUS + 1)))
    for bad in ("0", "-1e-3", "inf", "nan"):
        with pytest.raises(ValueError, match="--smooth_eps"):
            cli.check_smooth_args(parse("--smooth_radius", "8", "--smooth_eps=" + bad))


def test_main_refuses_before_it_touches_anything(tmp_path):
    out = tmp_path / "o"
    with pytest.raises(ValueError, match="--smooth_radius does not mix with --synthesis"):
        cli.main(["--mode", "16x", "--synthesis", "--smooth_radius", "8", "--outf", str(out)])
    with pytest.raises(ValueError, match="--smooth_eps"):
        cli.main(["--mode", "16x", "--smooth_eps", "1e-3", "--outf", str(out)])
    assert not out.exists()


def test_output_names_with_and_without_the_flag():
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_b+s1.jpg")
    plain = types.SimpleNamespace(outf="o", log_mark="L", mode="16x", alpha=1)           # a namespace from before the flags existed
    assert cli.out_name(plain, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=1_b+s1.jpg")
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6", "--preserve_color", "luma")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_color=luma_b+s1.jpg")
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6", "--smooth_radius", "8")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_smooth=8_b+s1.jpg")
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--smooth_radius", "16", "--preserve_color", "match")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=1_color=match_smooth=16_b+s1.jpg")
    assert cli.region_out_name(a, "b.v2.png") == os.path.join("o", "L_mode=16x_alpha=1_color=match_smooth=16_b+regions.jpg")
    assert cli.interp_out_name(a, "b.png", blend=True) == os.path.join("o", "L_mode=16x_alpha=1_color=match_smooth=16_b+blend.jpg")
