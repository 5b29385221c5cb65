"""Colour preservation without a GPU: the algebra of the numpy reference (tests/color_oracle.py), the new public header and its
bindings, and the command line's --preserve_color."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import color_oracle as O
from tests.conftest import REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_color.h")
natural = O.natural


# ---------------------------------------------------------------------------------------------------------------- oracle algebra
def test_oracle_map_carries_the_style_covariance_onto_the_contents():
    c, s = natural(1, 40, 56), natural(2, 33, 47, cast=(0.5, 1.0, 0.9), shift=(0.3, 0.0, 0.1))
    A, t = O.solve(*O.moments(c), *O.moments(s))
    mu_c, Sc = O.cov(*O.moments(c))
    mu_s, Ss = O.cov(*O.moments(s))
    assert np.abs(A @ Ss @ A.T - Sc).max() <= 1e-10 * np.abs(Sc).max()
    assert np.abs(A @ mu_s + t - mu_c).max() <= 1e-12
    # the matched style has the content's mean and (up to eps) covariance
    m = O.match(s, c)
    mu_m, Sm = O.cov(*O.moments(m), eps=0.0)
    assert np.abs(mu_m - mu_c).max() <= 1e-10
    assert np.abs(Sm + O.EPS * A @ A.T - Sc).max() <= 1e-10 * np.abs(Sc).max()


def test_oracle_style_equal_to_content_is_the_identity():
    c = natural(3, 31, 45)
    A, t = O.solve(*O.moments(c), *O.moments(c))
    assert np.abs(A - np.eye(3)).max() <= 1e-10 and np.abs(t).max() <= 1e-10


@pytest.mark.parametrize("kind", ["grey", "constant"])
def test_oracle_degenerate_styles_stay_bounded(kind):
    c = natural(4, 36, 52)
    if kind == "grey":
        s = np.repeat(natural(5, 30, 44).mean(0, keepdims=True), 3, 0).astype(np.float32)
    else:
        s = np.broadcast_to(np.array([0.25, 0.5, 0.75], np.float32)[:, None, None], (3, 30, 44)).copy()
    A, t = O.solve(*O.moments(c), *O.moments(s))
    assert np.isfinite(A).all() and np.isfinite(t).all()
    _, Sc = O.cov(*O.moments(c), eps=0.0)
    bound = np.sqrt((np.linalg.eigvalsh(Sc).max() + O.EPS) / O.EPS)
    assert np.linalg.norm(A, 2) <= bound * (1 + 1e-9)


def test_oracle_luma_merge_keeps_chroma_and_takes_luminance():
    rng = np.random.default_rng(6)
    c = rng.random((3, 25, 33)) * 1.0
    s = rng.random((3, 16, 32)) * 3.0 - 1.0
    out = O.luma_merge(s, c)
    assert out.shape == s.shape
    assert np.abs(O.luma(out) - O.luma(s)).max() <= 1e-12          # the weights sum to 1
    d = out - c[:, :16, :32]
    assert np.abs(d[0] - d[1]).max() <= 1e-12 and np.abs(d[0] - d[2]).max() <= 1e-12
    assert abs(O.LUMA.sum() - 1.0) <= 1e-15


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def declared():
    return sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"wct_ctx"})


def test_header_and_symbol_list_agree():
    assert declared() and declared() == sorted(lib.SYMBOLS_COLOR)
    assert not set(lib.SYMBOLS_COLOR) & set(lib.SYMBOLS)
    main = open(os.path.join(REPO, "include", "wct_hip.h")).read()
    main_declared = set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", main))
    assert not set(lib.SYMBOLS_COLOR) & main_declared
    assert "wct_hip_color.h" in main              # the main header points to the new one


def test_built_library_exports_the_colour_entries():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_COLOR:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_COLOR) <= exported


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_color.c"
    src.write_text('#include "wct_hip_color.h"\n'
                   "int use(wct_ctx* c, const float* p, double* s) { return wct_color_moments(c, p, 1, 2, s, s + 3) + WCT_COLOR_MATCH + WCT_COLOR_LUMA\n"
                   "    + (WCT_COLOR_EPS > 0.0) + WCT_OK; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_header_cites_the_reference_lines_it_extends():
    text = open(HEADER).read()
    assert "util_wct.py:62-131" in text and "WCT.py:120-125" in text
    assert '#include "wct_hip.h"' in text
    for word in ("WCT_COLOR_MATCH 1", "WCT_COLOR_LUMA 2", "WCT_COLOR_EPS 1e-5", "MATCHED"):
        assert word in text, word


def test_constants_of_the_binding_are_the_headers():
    text = open(HEADER).read()
    assert int(re.search(r"#define WCT_COLOR_MATCH (\d+)", text).group(1)) == lib.COLOR_MATCH
    assert int(re.search(r"#define WCT_COLOR_LUMA (\d+)", text).group(1)) == lib.COLOR_LUMA
    assert float(re.search(r"#define WCT_COLOR_EPS (\S+)", text).group(1)) == lib.COLOR_EPS == O.EPS
    assert lib.COLOR_MODES == {"match": 1, "luma": 2, "match+luma": 3}


def test_history_cases_cover_every_colour_entry():
    from tests import test_color_gpu as G          # imports without a GPU
    covered = set(sym for c in G.CASES.values() for sym in c.covers)
    assert set(lib.SYMBOLS_COLOR) <= covered, sorted(set(lib.SYMBOLS_COLOR) - covered)
    assert covered <= set(lib.SYMBOLS_COLOR) | set(lib.SYMBOLS)
    sizes = set(c.size for c in G.CASES.values())
    assert sizes == {"small", "large"}


def test_product_keeps_the_reference_code_out():
    pkg = os.path.join(REPO, "collaborative-distillation_amd")
    for rel in ("csrc/color.hip", "wct_hip/lib.py", "wct_hip/wct.py", "wct_hip/cli.py", "../include/wct_hip_color.h"):
        text = open(os.path.join(pkg, rel)).read()
        assert "color_oracle" not in text and not re.search(r"wct_oracle|liboracle|oracle/", text), rel


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_parser_flag_defaults_and_choices():
    assert parse().preserve_color is None
    assert parse("--preserve_color", "match").preserve_color == "match"
    assert parse("--preserve_color", "luma").preserve_color == "luma"
    with pytest.raises(SystemExit):
        parse("--preserve_color", "match+luma")
    with pytest.raises(SystemExit):
        parse("--preserve_color")


def test_check_color_args_refusals():
    cli.check_color_args(parse())
    cli.check_color_args(parse("--preserve_color", "match"))
    cli.check_color_args(parse("--preserve_color", "luma"))
    cli.check_color_args(parse("--preserve_color", "luma", "--maskPath", "m", "--region_styles", "a.png"))
    cli.check_color_args(parse("--preserve_color", "luma", "--interp_styles", "a.png,b.png", "--interp_weights", "1,1"))
    cli.check_color_args(parse("--preserve_color", "luma", "--interp_styles", "a.png,b.png", "--weightPath", "w"))
    with pytest.raises(ValueError, match="--maskPath"):
        cli.check_color_args(parse("--preserve_color", "match", "--maskPath", "m", "--region_styles", "a.png"))
    with pytest.raises(ValueError, match="--interp_styles"):
        cli.check_color_args(parse("--preserve_color", "match", "--interp_styles", "a.png,b.png", "--interp_weights", "1,1"))
    for mode in ("match", "luma"):
        with pytest.raises(ValueError, match="--synthesis"):
            cli.check_color_args(parse("--preserve_color", mode, "--synthesis"))
    with pytest.raises(ValueError):
        cli.check_color_args(types.SimpleNamespace(preserve_color="chroma", synthesis=False, maskPath=None, interp_styles=None, weightPath=None))


def test_main_refuses_before_it_touches_anything(tmp_path):
    out = tmp_path / "o"
    with pytest.raises(ValueError, match="--synthesis"):
        cli.main(["--mode", "16x", "--synthesis", "--preserve_color", "luma", "--outf", str(out)])
    assert not out.exists()


def test_output_names_with_and_without_the_flag():
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_b+s1.jpg")
    plain = types.SimpleNamespace(outf="o", log_mark="L", mode="16x", alpha=1)           # a namespace from before the flag existed
    assert cli.out_name(plain, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=1_b+s1.jpg")
    for mode in ("match", "luma"):
        a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6", "--preserve_color", mode)
        assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_color=%s_b+s1.jpg" % mode)
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--preserve_color", "luma")
    assert cli.region_out_name(a, "b.v2.png") == os.path.join("o", "L_mode=16x_alpha=1_color=luma_b+regions.jpg")
    assert cli.interp_out_name(a, "b.png", blend=True) == os.path.join("o", "L_mode=16x_alpha=1_color=luma_b+blend.jpg")
