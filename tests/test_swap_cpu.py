"""Patch swap without a GPU: identities of the numpy reference (tests/swap_oracle.py), the new public header and its bindings, and the
command line's --swap_level / --swap_match."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import swap_oracle as O
from tests.conftest import REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_swap.h")


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("hs,ws,C,oy,ox,h,w", [(12, 14, 8, 2, 3, 7, 9), (21, 18, 4, 1, 1, 19, 16), (9, 40, 12, 5, 30, 3, 3)])
def test_oracle_a_crop_matches_every_patch_to_its_origin(hs, ws, C, oy, ox, h, w):
    K = np.random.default_rng(hs).standard_normal((hs, ws, C)).astype(np.float32)
    Q = K[oy:oy + h, ox:ox + w]
    m = O.match(Q, K)
    qy, qx = np.divmod(np.arange((h - 2) * (w - 2)), w - 2)
    assert np.array_equal(m.idx, (qy + oy) * (ws - 2) + qx + ox)
    assert np.allclose(m.best, m.qnorm, rtol=1e-12) and (m.gap > 1e-2 * m.qnorm).all()


def test_oracle_scores_against_a_double_loop():
    rng = np.random.default_rng(3)
    Q, K = rng.standard_normal((4, 5, 4)), rng.standard_normal((5, 4, 4))
    S = O.scores(Q, K)
    for qy in range(2):
        for qx in range(3):
            for ky in range(3):
                for kx in range(2):
                    a, b = Q[qy:qy + 3, qx:qx + 3], K[ky:ky + 3, kx:kx + 3]
                    assert abs(S[qy * 3 + qx, ky * 2 + kx] - (a * b).sum() / np.sqrt((b * b).sum() + O.EPS)) < 1e-13


def test_oracle_lowest_index_wins_among_equal_patches():
    block = np.random.default_rng(1).standard_normal((5, 6, 4))
    K = np.tile(block, (5, 3, 1))[:21, :18]
    rep = O.lowest_duplicate(K)
    ky, kx = np.divmod(np.arange(19 * 16), 16)
    assert np.array_equal(rep, (ky % 5) * 16 + kx % 6)


@pytest.mark.parametrize("h,w,C", [(3, 3, 4), (3, 9, 8), (8, 7, 4)])
def test_oracle_assembling_the_identity_mapping_returns_v(h, w, C):
    V = np.random.default_rng(h * w).standard_normal((h, w, C))
    idx = np.arange((h - 2) * (w - 2))
    assert np.abs(O.assemble(idx, h, w, V) - V).max() <= 1e-15
    base = np.random.default_rng(5).standard_normal((h, w, C))
    assert np.array_equal(O.assemble(idx, h, w, V, base, 0.0), base)
    assert np.abs(O.assemble(idx, h, w, V, base, 0.25) - (0.25 * V + 0.75 * base)).max() <= 1e-15


def test_oracle_assemble_against_a_double_loop_in_fp32_order():
    rng = np.random.default_rng(11)
    h, w, hs, ws, C = 5, 6, 6, 5, 4
    V = rng.standard_normal((hs, ws, C)).astype(np.float32)
    base = rng.standard_normal((h, w, C)).astype(np.float32)
    idx = rng.integers(0, (hs - 2) * (ws - 2), (h - 2) * (w - 2))
    want = np.zeros((h, w, C), np.float32)
    a = np.float32(0.6)
    for y in range(h):
        for x in range(w):
            s, n = np.zeros(C, np.float32), 0
            for qy in range(max(0, y - 2), min(h - 3, y) + 1):
                for qx in range(max(0, x - 2), min(w - 3, x) + 1):
                    ky, kx = divmod(int(idx[qy * (w - 2) + qx]), ws - 2)
                    s = s + V[ky + y - qy, kx + x - qx]
                    n += 1
            want[y, x] = a * (s / np.float32(n)) + (np.float32(1) - a) * base[y, x]
    assert np.array_equal(O.assemble(idx, h, w, V, base, 0.6, dtype=np.float32), want)


def test_oracle_whitened_features_are_white():
    x = np.random.default_rng(2).random((9, 11, 6)) @ (np.eye(6) + 0.3 * np.random.default_rng(3).random((6, 6)))
    y = O.whiten(x).reshape(-1, 6)
    assert np.abs(y.mean(0)).max() < 1e-12 and np.abs(np.cov(y.T) - np.eye(6)).max() < 1e-10


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def declared():
    return sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"wct_ctx"})


def test_header_and_symbol_list_agree():
    assert declared() and declared() == sorted(lib.SYMBOLS_SWAP)
    assert not set(lib.SYMBOLS_SWAP) & (set(lib.SYMBOLS) | set(lib.SYMBOLS_COLOR) | set(lib.SYMBOLS_SMOOTH) | set(lib.SYMBOLS_TRANSFORM))
    text = open(HEADER).read()
    for name, value in (("WCT_SWAP_EPS", lib.SWAP_EPS), ("WCT_SWAP_WHITENED", lib.SWAP_WHITENED), ("WCT_SWAP_RAW", lib.SWAP_RAW),
                        ("WCT_SWAP_KEY_CHUNK", lib.SWAP_KEY_CHUNK)):
        m = re.search(r"#define %s\s+(\S+)" % name, text)
        assert m and float(m.group(1)) == float(value), name
    assert lib.SWAP_MATCHES == {"whitened": lib.SWAP_WHITENED, "raw": lib.SWAP_RAW} and lib.SWAP_EPS == O.EPS


def test_built_library_exports_the_swap_entries():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_SWAP:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_SWAP) <= exported


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_swap.c"
    src.write_text('#include "wct_hip_swap.h"\n'
                   "int main(void) { return (WCT_SWAP_WHITENED == 0 && WCT_SWAP_RAW == 1 && WCT_SWAP_KEY_CHUNK > 0 && WCT_SWAP_EPS > 0) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "only_swap.o")], check=True)


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    args = cli.build_parser().parse_args(["--mode", "16x"] + list(argv))
    args.outf, args.log_mark = "out", "M"
    return args


def test_parser_accepts_the_flags_and_defaults_to_off():
    a = parse()
    assert a.swap_level is None and a.swap_match is None
    cli.check_swap_args(a)
    assert a.swap_match is None
    for level in lib.SWAP_LEVELS:
        a = parse("--swap_level", str(level))
        cli.check_swap_args(a)
        assert a.swap_level == level and a.swap_match == "whitened"
    a = parse("--swap_level", "3", "--swap_match", "raw", "--preserve_color", "luma", "--smooth_radius", "4", "--transform", "ot")
    cli.check_swap_args(a)
    assert (a.swap_level, a.swap_match) == (3, "raw")
    for bad in (["--swap_level", "1"], ["--swap_level", "6"], ["--swap_match", "cosine", "--swap_level", "3"]):
        with pytest.raises(SystemExit):
            parse(*bad)
    with pytest.raises(ValueError, match="--swap_match does nothing without --swap_level"):
        cli.check_swap_args(parse("--swap_match", "raw"))
    with pytest.raises(ValueError, match="--swap_level"):
        cli.check_swap_args(types.SimpleNamespace(swap_level=1, swap_match=None))


@pytest.mark.parametrize("extra,name", [
    (["--synthesis"], "--synthesis"),
    (["--maskPath", "m", "--region_styles", "a.png"], "--maskPath"),
    (["--interp_styles", "a.png,b.png"], "--interp_styles"),
    (["--interp_styles", "a.png", "--weightPath", "w"], "--weightPath"),
    (["--numpy"], "--numpy"),
    (["--preserve_color", "match"], "--preserve_color match"),
])
def test_refusals_name_both_flags(extra, name):
    a = parse("--swap_level", "4", *extra)
    with pytest.raises(ValueError) as e:
        cli.check_swap_args(a)
    assert "--swap_level" in str(e.value) and name in str(e.value)


def test_main_refuses_before_it_creates_anything(tmp_path):
    out = tmp_path / "never"
    with pytest.raises(ValueError, match="--swap_level does not mix with --numpy"):
        cli.main(["--mode", "16x", "--outf", str(out), "--swap_level", "3", "--numpy"])
    assert not out.exists()


def test_out_name_carries_the_swap_mark_after_the_transform_mark():
    plain = parse()
    assert cli.out_name(plain, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_a+b.jpg")
    assert cli.out_name(parse("--swap_level", "4"), "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_swap=4_a+b.jpg")
    full = parse("--swap_level", "3", "--transform", "ot", "--preserve_color", "luma", "--smooth_radius", "8")
    assert cli.out_name(full, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_transform=ot_swap=3_color=luma_smooth=8_a+b.jpg")
    legacy = types.SimpleNamespace(outf="out", log_mark="M", mode="16x", alpha=1)       # a namespace from before the flag
    assert cli.out_name(legacy, "a+b.jpg") == cli.out_name(plain, "a+b.jpg")


class _FakeEngine:
    """The engine surface _swap_pair uses, with the real one's range behaviour: sync() raises on a pending clamp."""

    def __init__(self, clamps):
        self.clamps, self.pending, self.calls, self.mode = list(clamps), 0, [], "f16x3"

    def stylize_swap(self, c, s, level, match, alpha, num_run):
        self.pending = self.clamps.pop(0)
        self.calls.append((self.mode, c, s, level, match, alpha, num_run))
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


@pytest.mark.parametrize("clamps,modes,warnings", [([0], ["f16x3"], 0), ([5, 0], ["f16x3", "fp32"], 1), ([5, 2], ["f16x3", "fp32"], 2)])
def test_swap_pair_recomputes_in_fp32_and_reports_a_clamp_inside_the_match(clamps, modes, warnings):
    """A clamp under f16x3 convolutions -> one recompute under fp32 convolutions; a clamp that survives it sits in the match (which stays
    f16x3): it is logged, acknowledged, and the pair's result is still returned -- never an exception that drops the pair."""
    eng, log, styles = _FakeEngine(clamps), [], []
    args = parse("--swap_level", "3", "--swap_match", "raw", "--alpha", "0.5", "--num_run", "2")
    res = cli._swap_pair(eng, args, log.append, "content", lambda: styles.append(len(styles)) or "style%d" % len(styles))
    assert [c[0] for c in eng.calls] == modes and res == "result under %s" % modes[-1]
    assert all(c[1:] == ("content", "style%d" % (i + 1), 3, "raw", 0.5, 2) for i, c in enumerate(eng.calls))
    assert eng.mode == "f16x3" and eng.pending == 0 and len(log) == warnings
    if warnings:
        assert "recomputing it with exact-fp32 convolutions" in log[0]
    if warnings == 2:
        assert "inside the patch match" in log[1] and "clamped" in log[1]
    eng.sync()          # nothing is left pending for a later call to trip over
