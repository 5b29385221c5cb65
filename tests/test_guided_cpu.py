"""Region-to-region transfer without a GPU: the new public header against its bindings, the numpy definitions (tests/guided_oracle.py)
against the region oracle and against k-means' own invariants, and the command line's --styleMaskPath / --auto_regions."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import guided_oracle as G
from tests import region_oracle
from tests.conftest import PKG, REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_guided.h")


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def declared():
    return sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"wct_ctx"})


def test_header_and_symbol_list_agree():
    assert declared() and declared() == sorted(lib.SYMBOLS_GUIDED)
    others = (set(lib.SYMBOLS) | set(lib.SYMBOLS_COLOR) | set(lib.SYMBOLS_SMOOTH) | set(lib.SYMBOLS_TRANSFORM) | set(lib.SYMBOLS_SWAP)
              | set(lib.SYMBOLS_SCALE))
    assert not set(lib.SYMBOLS_GUIDED) & others
    main = open(os.path.join(REPO, "include", "wct_hip.h")).read()
    assert not any(re.search(r"\b%s\s*\(" % s, main) for s in lib.SYMBOLS_GUIDED)
    text = open(HEADER).read()
    for name, value in (("WCT_GUIDED_MAX_REGIONS", lib.GUIDED_MAX_REGIONS), ("WCT_GUIDED_MAX_STYLES", lib.GUIDED_MAX_STYLES),
                        ("WCT_KMEANS_MAX_K", lib.KMEANS_MAX_K), ("WCT_KMEANS_MAX_ITERS", lib.KMEANS_MAX_ITERS),
                        ("WCT_KMEANS_DEAD_VARIANCE", lib.KMEANS_DEAD_VARIANCE)):
        m = re.search(r"#define %s\s+(\S+)" % name, text)
        assert m and float(m.group(1)) == float(value), name
    assert lib.KMEANS_DEAD_VARIANCE == G.DEAD_VARIANCE


def test_built_library_exports_the_guided_entries():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_GUIDED:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_GUIDED) <= exported


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_guided.c"
    src.write_text('#include "wct_hip_guided.h"\n'
                   "int main(void) { return (WCT_GUIDED_MAX_REGIONS == 8 && WCT_GUIDED_MAX_STYLES == 8 && WCT_KMEANS_MAX_K == 8) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "only_guided.o")], check=True)


def test_the_new_kernels_are_listed_and_clamp_nothing():
    text = open(os.path.join(PKG, "csrc", "cluster.hip")).read()
    assert ".commit(" not in text and "sat_raise(" not in text
    build = open(os.path.join(PKG, "build.sh")).read()
    assert re.search(r'^SRC=".*\bcluster\b.*"', build, re.M) and "../include/wct_hip_guided.h" in build
    names = {}
    for f in os.listdir(os.path.join(PKG, "csrc")):
        for k in re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(PKG, "csrc", f)).read()):
            names.setdefault(k, set()).add(f)
    mine = [k for k, fs in names.items() if "cluster.hip" in fs]
    assert len(mine) >= 6 and all(names[k] == {"cluster.hip"} for k in mine)       # kernel names are unique across csrc/


# ---------------------------------------------------------------------------------------------------------------- guided oracle
def _smooth(rng, shape, passes=2):
    x = rng.random(shape, dtype=np.float32)
    for _ in range(passes):
        x = (x + np.roll(x, 1, -1) + np.roll(x, 1, -2) + np.roll(x, -1, -1) + np.roll(x, -1, -2)) / 5
    return np.ascontiguousarray(x, np.float32)


def test_guided_oracle_without_maps_is_the_region_oracle(oracle, weights16x):
    rng = np.random.default_rng(5)
    mods = oracle.Modules("16x", weights16x)
    c = _smooth(rng, (3, 64, 80))
    styles = [_smooth(rng, (3, 48, 64)), rng.random((3, 48, 40), dtype=np.float32)]
    lab = np.zeros((64, 80), np.uint8)
    lab[:, 40:] = 1
    lab[:8] = 255
    ref = region_oracle.stylize_regions(mods, c, styles, lab, [1.0, 0.6])
    assert np.array_equal(G.stylize_guided(mods, c, styles, lab, None, None, [1.0, 0.6]), ref)
    assert np.array_equal(G.stylize_guided(mods, c, styles, lab, [None, None], [0, 1], [1.0, 0.6]), ref)
    # a map that selects every style pixel for its region is no restriction; one that selects fewer than 2 leaves the region alone
    full = [np.zeros((48, 64), np.uint8), np.ones((48, 40), np.uint8)]
    assert np.array_equal(G.stylize_guided(mods, c, styles, lab, full, [0, 1], [1.0, 0.6]), ref)
    none = [np.full((48, 64), 255, np.uint8), np.ones((48, 40), np.uint8)]
    lone = lab.copy()
    lone[lab == 0] = 255
    assert np.array_equal(G.stylize_guided(mods, c, styles, lab, none, [0, 1], [1.0, 0.6]), region_oracle.stylize_regions(mods, c, styles, lone, [1.0, 0.6]))
    half = [np.zeros((48, 64), np.uint8), np.ones((48, 40), np.uint8)]
    half[0][:, 32:] = 255
    got = G.stylize_guided(mods, c, styles, lab, half, [0, 1], [1.0, 0.6])
    assert not np.array_equal(got, ref) and np.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------------------- k-means oracle
@pytest.mark.parametrize("C,K,h,w", [(4, 2, 29, 33), (20, 3, 37, 53), (64, 8, 37, 53), (132, 5, 31, 41)])
def test_kmeans_oracle_cost_never_increases(C, K, h, w):
    f = G.cluster_features(K, h, w, C, 100 * C + K)
    sh, sc = G.standardisation_of(f)
    assert sc[1] == 0 and (sc[np.arange(C) != 1] > 0).all()                        # the dead channel, and only it
    z = G.zmap(f, sh, sc)
    assert z.dtype == np.float32 and np.array_equal(z[:, 1], np.zeros(h * w, np.float32))
    cent, idx, costs, unclear, margins = G.lloyd(z, K, 10)
    assert len(set(idx.tolist())) == K and min(margins) > 0
    assert all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:])), costs
    assert max(unclear) <= 0.01 * h * w
    lab = G.assign(z, cent)[0]
    assert lab.max() < K and np.array_equal(G.expand(lab.reshape(h, w), 1, h, w), lab.reshape(h, w))


def test_kmeans_oracle_empty_and_duplicate_clusters():
    f = G.cluster_features(3, 23, 31, 20, 9)
    sh, sc = G.standardisation_of(f)
    z = G.zmap(f, sh, sc)
    cent = G.seed(z, 3)[0]
    far = np.vstack([cent, np.full((1, 20), 1e3)])
    lab, n, s, cost, nxt, _ = G.assign(z, far)
    assert n[3] == 0 and np.array_equal(nxt[3], far[3]) and (lab < 3).all() and n.sum() == z.shape[0]
    dup = np.vstack([cent[:2], cent[1:2], cent[2:]])
    lab, n, *_ = G.assign(z, dup)
    assert n[2] == 0 and n[1] > 0                                                   # ties go to the lowest k
    lab2 = G.assign(z, cent)[0]
    assert np.array_equal(np.where(lab == 3, 2, lab), lab2)


def test_expand_clamps_at_the_ragged_edge():
    lab = np.arange(12, dtype=np.uint8).reshape(3, 4)
    out = G.expand(lab, 3, 14, 19)                                                  # s = 4: rows 12, 13 and columns 16..18 repeat the last cell
    assert out.shape == (14, 19) and out[13, 18] == 11 and out[12, 0] == 8 and out[0, 16] == 3 and out[5, 9] == 6


# ---------------------------------------------------------------------------------------------------------------- command line
def _args(*argv):
    return cli.build_parser().parse_args(list(argv))


def _check_all(args):
    cli.check_region_args(args)
    cli.check_interp_args(args)
    cli.check_synthesis_args(args)
    cli.check_color_args(args)
    cli.check_smooth_args(args)
    cli.check_transform_args(args)
    cli.check_swap_args(args)
    cli.check_scale_args(args)
    cli.check_auto_args(args)


def test_auto_regions_arguments(tmp_path):
    a = _args("--auto_regions", "3")
    _check_all(a)
    assert (a.auto_level, a.auto_iters) == (4, 10)
    a.outf, a.log_mark = str(tmp_path), "m"
    assert "_auto=3_" in cli.out_name(a, "x+y.jpg") and "_auto" not in cli.out_name(_args(), "x+y.jpg")
    a = _args("--auto_regions", "8", "--auto_level", "2", "--auto_iters", "64", "--preserve_color", "luma", "--smooth_radius", "4")
    _check_all(a)
    assert (a.auto_level, a.auto_iters) == (2, 64)
    for bad, word in ((("--auto_regions", "1"), "2..8"), (("--auto_regions", "9"), "2..8"), (("--auto_regions", "3", "--auto_iters", "0"), "1..64"),
                      (("--auto_regions", "3", "--auto_iters", "65"), "1..64"), (("--auto_level", "3"), "--auto_regions"), (("--auto_iters", "3"), "--auto_regions")):
        with pytest.raises(ValueError, match=re.escape(word)):
            _check_all(_args(*bad))
    clashes = [(("--maskPath", "m", "--region_styles", "a.jpg"), "--maskPath"), (("--interp_styles", "a.jpg,b.jpg"), "--interp_styles"),
               (("--synthesis",), "--synthesis"), (("--swap_level", "3"), "--swap_level"), (("--level_scale", "2,2,1,1,1"), "--level_scale"),
               (("--transform", "ot"), "--transform ot"), (("--transform", "adain"), "--transform adain"), (("--preserve_color", "match"), "match")]
    for extra, word in clashes:
        with pytest.raises(ValueError, match=re.escape(word)):
            cli.check_auto_args(_args("--auto_regions", "3", *extra))
    a = _args("--auto_regions", "3")
    a.weightPath = "w"
    with pytest.raises(ValueError, match="--weightPath"):
        cli.check_auto_args(a)


def test_style_mask_path_lookup(tmp_path):
    from PIL import Image
    d = tmp_path / "smasks"
    d.mkdir()
    Image.fromarray(np.zeros((5, 7), np.uint8), "L").save(str(d / "sky.png"))
    assert cli.style_mask_path(str(d), "/some/where/sky.v2.jpg") == str(d / "sky.png")       # X = the text before the first dot
    assert cli.style_mask_path(str(d), "houses.jpg") is None                                # no file: the style is used whole
    assert cli.style_mask_path(None, "sky.jpg") is None
    assert cli.load_mask(str(d / "sky.png"), (5, 7)).shape == (5, 7)
    with pytest.raises(ValueError, match="not resampled"):
        cli.load_mask(str(d / "sky.png"), (6, 7))
    with pytest.raises(ValueError, match="--maskPath"):
        cli.check_region_args(_args("--styleMaskPath", str(d)))
    with pytest.raises(ValueError, match="not a folder"):
        cli.check_region_args(_args("--maskPath", "m", "--region_styles", "a.jpg", "--styleMaskPath", str(d / "nope")))
    cli.check_region_args(_args("--maskPath", "m", "--region_styles", "a.jpg", "--styleMaskPath", str(d)))
