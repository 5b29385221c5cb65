"""The choice of feature transform without a GPU: the numpy reference (tests/transform_oracle.py) against the identities that define the
operators, the new public header and its bindings, and the command line's --transform."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import transform_cases as TC
from tests import transform_oracle as O
from tests.conftest import REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_transform.h")


# ---------------------------------------------------------------------------------------------------------------- oracle
def _pair(seed, C, lo_c, lo_s):
    rng = np.random.default_rng(seed)
    return O.spd(rng, C, lo_c), O.spd(rng, C, lo_s)


@pytest.mark.parametrize("C,lo_c,lo_s", [(8, 1e-2, 1e-1), (32, 1e-3, 1e-3), (64, 1e-5, 1e-4)])
def test_oracle_ot_and_wct_reach_the_style_covariance_and_ot_is_symmetric(C, lo_c, lo_s):
    cov_c, cov_s = _pair(C, C, lo_c, lo_s)
    S = O.sym_pow(cov_s, 0.5)
    for mode in ("wct", "ot"):
        T = O.T_of(mode, cov_c, S)
        assert O.rel_fro(T @ cov_c @ T.T, cov_s) < 1e-9, mode
    T = O.T_ot(cov_c, S)
    assert np.abs(T - T.T).max() <= 1e-10 * np.abs(T).max()
    assert np.linalg.eigvalsh(O.sym(T)).min() > 0                                    # the Monge map is positive definite
    Tw = O.T_wct(cov_c, S)
    assert np.abs(Tw - Tw.T).max() > 1e-3 * np.abs(Tw).max()                          # ... and WCT's map is not even symmetric
    # among the maps that reach cov_s, ot moves the content least: E |T x - x|^2 = tr((T - I) cov_c (T - I)^T)
    cost = lambda M: np.trace((M - np.eye(C)) @ cov_c @ (M - np.eye(C)).T)
    assert cost(T) < cost(Tw)


@pytest.mark.parametrize("lo_c,lo_s,gate", [(1e-2, 1e-2, 1e-9), (1e-4, 1e-5, 1e-9), (1e-5, 1e-5, 1e-9)])
def test_oracle_the_two_ot_forms_agree_on_full_rank_cases(lo_c, lo_s, gate):
    cov_c, cov_s = _pair(7, 32, lo_c, lo_s)
    S = O.sym_pow(cov_s, 0.5)
    cond = np.linalg.cond(O.ot_B(cov_c, S))
    err = O.rel_fro(O.T_ot(cov_c, S), O.T_ot_sigma_form(cov_c, cov_s))
    print("ot forms: cond(B) %.1e, S-form vs Sigma-form %.2e" % (cond, err))
    assert err < gate


def test_oracle_adain_matches_channel_statistics_and_dead_channels_map_with_one():
    rng = np.random.default_rng(3)
    dead = (2, 5)
    cov_c, cov_s = O.spd(rng, 16, 1e-2, dead), O.spd(rng, 16, 1e-2, dead)
    S = O.sym_pow(cov_s, 0.5)
    T = O.T_adain(cov_c, S)
    assert np.count_nonzero(T - np.diag(np.diag(T))) == 0
    out_var = np.diag(T @ cov_c @ T)
    live = [i for i in range(16) if i not in dead]
    assert np.allclose(out_var[live] + O.ADAIN_EPS * np.diag(T)[live] ** 2, np.diag(cov_s)[live] + O.ADAIN_EPS, rtol=1e-12)
    assert np.array_equal(np.diag(T)[list(dead)], np.ones(2))


def test_oracle_singular_B_any_null_space_treatment_acts_alike_on_the_support():
    """The header's argument: B v = 0 means (S v) is orthogonal to range(cov_c) -- adding ANY multiple of the null projector of B to
    B^(-1/2) changes T only off the content's support."""
    rng = np.random.default_rng(11)
    C = 24
    cov_c, cov_s = O.spd(rng, C, 1e-2, rank=15), O.spd(rng, C, 1e-2)
    S = O.sym_pow(cov_s, 0.5)
    B = O.ot_B(cov_c, S)
    lam, V = np.linalg.eigh(B)
    N = V[:, lam <= 1e-12 * lam.max()]
    assert N.shape[1] == C - 15
    R = O.sym_pow(cov_c, 0.5)
    assert np.abs(R @ S @ N).max() < 1e-7
    T0, T1 = O.T_ot(cov_c, S), S @ (O.sym_pow(B, -0.5) + 1e3 * N @ N.T) @ S
    assert O.rel_fro(T1, T0) > 1 and O.rel_fro(T1 @ R, T0 @ R) < 1e-6


def test_oracle_raw_moment_round_trip_and_alpha_blend():
    rng = np.random.default_rng(5)
    cov_c, cov_s = _pair(5, 12, 1e-2, 1e-2)
    mu_c, mu_s = rng.random(12), rng.random(12)
    S = O.sym_pow(cov_s, 0.5)
    n, s, ss = O.raw(500, mu_c, cov_c)
    for mode in O.MODES:
        M1, b1 = O.solve(mode, n, s, ss, O.stats(S, mu_s), 1.0)
        Ma, ba = O.solve(mode, n, s, ss, O.stats(S, mu_s), 0.6)
        assert np.allclose(Ma, 0.6 * M1 + 0.4 * np.eye(12), atol=1e-13) and np.allclose(ba, 0.6 * b1, atol=1e-13)
        assert np.allclose(M1 @ mu_c + b1, mu_s, atol=1e-10)          # the content mean lands on the style mean


# ---------------------------------------------------------------------------------------------------------------- the width sweep's cases
def test_width_table_reaches_the_branches_it_names():
    """tests/transform_cases.py: every width even and <= 512, the front end its name claims (solve.hip ns_pad), ragged tiles and k-tails
    in every class, and the dead channels where the table says they are."""
    assert list(TC.WIDTHS) == sorted(TC.WIDTHS) and all(C % 2 == 0 and 2 <= C <= 512 for C in TC.WIDTHS)
    for C, fe in TC.WIDTHS.items():
        Cp = TC.ns_pad(C)
        assert {"lds32": Cp == 32, "lds64": Cp == 64, "plain96": Cp == 96, "single128": Cp == 128, "deflated": C > 128}[fe], (C, fe, Cp)
        a, z = TC.dead_tail(C)
        assert a % 16 == 0 and a < z == C - 1 and z - a < 16 and a // 16 == TC.tiles(C) - 1
    for fe, cs in TC.FRONT_ENDS.items():
        assert any(TC.k_tail(C) for C in cs) and any(C % 16 for C in cs), fe
    assert sorted({TC.ns_pad(C) for C in TC.FRONT_ENDS["deflated"]}) == [192, 256, 320, 448, 512]      # wide<4> and wide<8>
    assert sorted({TC.tiles(C) for C in TC.WIDTHS}) == [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 17, 25, 32]
    assert len(TC.CASES) == 2 * len(TC.WIDTHS) + len(TC.RANK_WIDTHS)
    assert len({TC.seed_of(n) for n in TC.CASES}) == len(TC.CASES)


@pytest.mark.parametrize("name", list(TC.CASES))
def test_width_case_is_what_the_table_says(name):
    """The reference alone: cond(B) on the live block within the solver's gates (gate_for of the GPU test cannot trip), the intended
    rank, and -- where the content has full rank on its live channels -- the textbook form of the ot map against S B^(-1/2) S."""
    spec = TC.CASES[name]
    C = spec["C"]
    n, s, ss, st = TC.build(name)
    d = TC.describe(n, s, ss, st)
    print("%s: cond(B) %.2e rank %d live %d rank_c %d" % (name, d["cond"], d["rank"], d["live"], d["rank_c"]))
    assert d["cond"] <= 1e10
    dead = spec.get("dead_c", ())
    if "rank_c" in spec:
        assert n == C - 11 and d["live"] == C and d["rank_c"] == spec["rank_c"] == d["rank"] == C - 12      # singular by rank, not by dead channels
        return                                                                        # (the textbook form needs cov_c^(-1/2): not the same operator here)
    assert d["live"] == C - len(dead) == d["rank"] == d["rank_c"]
    assert d["cond"] <= 1e6                                                           # the 1e-8 gate
    live = [i for i in range(C) if i not in dead]
    _, cov_c = O.mean_cov(n, s, ss)
    S, _ = O.split_stats(st)
    ix = np.ix_(live, live)
    T = O.T_ot(cov_c, S)
    assert np.count_nonzero(T[list(dead), :]) == 0 and np.count_nonzero(T[:, list(dead)]) == 0
    err = O.rel_fro(T[ix], O.T_ot_sigma_form(cov_c[ix], (S @ S)[ix]))
    assert err < 1e-9, (name, err)


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def declared():
    return sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"wct_ctx"})


def test_header_and_symbol_list_agree():
    assert declared() and declared() == sorted(lib.SYMBOLS_TRANSFORM)
    assert not set(lib.SYMBOLS_TRANSFORM) & (set(lib.SYMBOLS) | set(lib.SYMBOLS_COLOR) | set(lib.SYMBOLS_SMOOTH))
    for other in ("wct_hip.h", "wct_hip_color.h", "wct_hip_smooth.h"):
        text = open(os.path.join(REPO, "include", other)).read()
        assert not set(lib.SYMBOLS_TRANSFORM) & set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", text)), other


def test_built_library_exports_the_transform_entries():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_TRANSFORM:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_TRANSFORM) <= exported


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_transform.c"
    src.write_text('#include "wct_hip_transform.h"\n'
                   "int use(wct_ctx* c, const double* p, double* q, int* n) {\n"
                   "  return wct_set_transform(c, WCT_TRANSFORM_OT) + wct_get_transform(c, n)\n"
                   "    + wct_transform_solve(c, WCT_TRANSFORM_ADAIN, 32, 100.0, p, p, p, WCT_ADAIN_EPS, q, q, n) + WCT_TRANSFORM_WCT + WCT_OK; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_constants_of_the_binding_are_the_headers():
    text = open(HEADER).read()
    for name, value in (("WCT", lib.TRANSFORM_WCT), ("OT", lib.TRANSFORM_OT), ("ADAIN", lib.TRANSFORM_ADAIN)):
        assert int(re.search(r"#define WCT_TRANSFORM_%s (\d+)" % name, text).group(1)) == value == lib.TRANSFORMS[name.lower()]
    assert float(re.search(r"#define WCT_ADAIN_EPS (\S+)", text).group(1)) == lib.ADAIN_EPS == O.ADAIN_EPS == 1e-5
    assert sorted(lib.TRANSFORMS) == sorted(O.MODES)
    assert '#include "wct_hip.h"' in text


def test_product_keeps_the_test_oracle_out():
    pkg = os.path.join(REPO, "collaborative-distillation_amd")
    for rel in ("csrc/transform.hip", "wct_hip/lib.py", "wct_hip/wct.py", "wct_hip/cli.py", "../include/wct_hip_transform.h"):
        text = open(os.path.join(pkg, rel)).read()
        assert "transform_oracle" not in text and not re.search(r"wct_oracle|liboracle|oracle/", text), rel


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_parser_and_names():
    assert parse().transform == "wct"
    assert parse("--transform", "ot").transform == "ot" and parse("--transform", "adain").transform == "adain"
    with pytest.raises(SystemExit):
        parse("--transform", "cholesky")
    base = ["--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6"]
    assert cli.out_name(parse(*base), "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_b+s1.jpg")                    # unchanged
    assert cli.out_name(parse(*base, "--transform", "wct"), "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_b+s1.jpg")
    assert cli.out_name(parse(*base, "--transform", "ot"), "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_transform=ot_b+s1.jpg")
    a = parse(*base, "--transform", "adain", "--preserve_color", "luma", "--smooth_radius", "4")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_transform=adain_color=luma_smooth=4_b+s1.jpg")


def test_check_transform_args():
    for t in ("wct", "ot", "adain"):
        cli.check_transform_args(parse("--transform", t))
        cli.check_transform_args(parse("--transform", t, "--pipeline", "0", "--synthesis"))
        cli.check_transform_args(parse("--transform", t, "--interp_styles", "a.png,b.png", "--interp_weights", "1,2", "--preserve_color", "luma"))
    cli.check_transform_args(parse("--numpy", "--maskPath", "m", "--region_styles", "a.png"))      # wct: everything as before
    for t in ("ot", "adain"):
        for extra, word in ((["--numpy"], "--numpy"), (["--maskPath", "m", "--region_styles", "a.png"], "--maskPath"),
                            (["--interp_styles", "a.png", "--weightPath", "w"], "--weightPath")):
            with pytest.raises(ValueError, match=word):
                cli.check_transform_args(parse("--transform", t, *extra))
    a = parse()
    a.transform = "monge"
    with pytest.raises(ValueError, match="--transform"):
        cli.check_transform_args(a)
