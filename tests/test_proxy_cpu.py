"""Proxy mode without a GPU: the numpy reference (tests/proxy_oracle.py) against the identities of its definition, the conditioning that
keeps the GPU tests' absolute gates meaningful, the new public header and its bindings, and the command line's --proxy_scale."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import color_oracle as CO
from tests import proxy_oracle as O
from tests.conftest import REPO
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_bgrid.h")


# ---------------------------------------------------------------------------------------------------------------- oracle
@pytest.mark.parametrize("h,w,gz,gh,gw", [(1, 1, 1, 1, 1), (3, 5, 3, 4, 6), (40, 56, 8, 3, 4), (37, 53, 32, 1, 7)])
def test_oracle_weights_sum_to_one_and_totals_survive_the_blur(h, w, gz, gh, gw):
    img = CO.natural(h + w, h, w)
    ws = O.weights(img, gz, gh, gw)
    assert len(ws) == 8
    total = sum(wt for _, wt in ws)
    assert np.abs(total - 1.0).max() <= 4e-16 and all((wt >= 0).all() and (wt <= 1).all() for _, wt in ws)
    assert all(((idx >= 0) & (idx < gz * gh * gw)).all() for idx, _ in ws)
    Gv, Rv = O.sums(img, CO.natural(h * w, h, w), gz, gh, gw)
    assert abs(Gv[..., 3, 3].sum() - h * w) <= 1e-12 * h * w            # the weights of all pixels
    for times in (1, 4):
        for S in (Gv, Rv):
            B = O.blur(S, times)
            assert B.shape == S.shape
            assert np.abs(B.sum((0, 1, 2)) - S.sum((0, 1, 2))).max() <= 1e-12 * max(1.0, np.abs(S.sum((0, 1, 2))).max())
    assert np.array_equal(O.blur(Gv, 0), Gv)


def test_oracle_shape():
    assert O.shape(64, 96) == (5, 7) and O.shape(65, 97) == (6, 8) and O.shape(1, 1, 16) == (2, 2) and O.shape(40, 56, 8) == (6, 8)
    assert O.shape(255 * 16, 16)[0] == O.MAX_XY == lib.BGRID_MAX_XY and O.MAX_Z == lib.BGRID_MAX_Z


def test_oracle_vertex_no_pixel_reaches_gets_the_global_map():
    from tests import test_proxy_gpu as G          # imports without a GPU
    h, w, gz, gh, gw, narrow, eps, smooth = G.EMPTY_BINS
    assert (gz, smooth, narrow) == (8, 0, True)
    cl, sl = G.fit_pair(h, w, narrow=True)
    g = O.guide(cl)
    assert 0.4 - 1e-9 <= g.min() and g.max() <= 0.6 + 1e-9
    A, Ag, _, _ = O.fit(cl, sl, gz, gh, gw, eps, smooth, details=True)
    Gv, _ = O.sums(cl, sl, gz, gh, gw)
    reached = Gv[..., 3, 3] > 0
    assert not reached[[0, 1, 6, 7]].any() and reached[3:5].any() and 0 < reached.sum() < reached.size
    assert np.abs(A[~reached] - Ag).max() <= 1e-13
    assert np.abs(A[reached] - Ag).max() > 1e-3


def test_oracle_one_vertex_is_the_global_ridge_fit():
    cl, sl = CO.natural(1, 32, 32).astype(np.float64), CO.natural(2, 32, 32).astype(np.float64)
    for eps in (1e-2, 1e-4):
        A, Ag, _, lam = O.fit(cl, sl, 1, 1, 1, eps, 4, details=True)
        assert lam == eps * 32 * 32
        v = np.concatenate([cl, np.ones((1, 32, 32))]).reshape(4, -1)
        # lambda regularises towards Ag, which is itself the ridge fit: (G + l I) A = R + l Ag  with  (G + l I) Ag = R  gives
        # A = Ag + l (G + l I)^-1 Ag -- the closed form of the definition's two steps
        G, R = v @ v.T, v @ sl.reshape(3, -1).T
        ridge = np.linalg.solve(G + lam * np.eye(4), R)
        want = ridge + lam * np.linalg.solve(G + lam * np.eye(4), ridge)
        assert np.abs(Ag - ridge.T).max() <= 1e-12 and np.abs(A[0, 0, 0] - want.T).max() <= 1e-12


def test_oracle_affine_result_comes_back_as_eps_vanishes():
    """sl an exact affine function of cl: every local fit is that function, and so is the slice of any full image."""
    M = np.array([[0.9, 0.2, -0.1, 0.05], [0.1, 0.7, 0.3, -0.1], [-0.2, 0.1, 1.1, 0.2]])
    cl = CO.natural(3, 40, 56).astype(np.float64)
    sl = np.einsum("ca,ahw->chw", M[:, :3], cl) + M[:, 3][:, None, None]
    c = CO.natural(4, 97, 131).astype(np.float64)
    want = np.einsum("ca,ahw->chw", M[:, :3], c) + M[:, 3][:, None, None]
    errs = []
    for eps in (1e-2, 1e-6, 1e-10):
        errs.append(float(np.abs(O.slice_(O.fit(cl, sl, 8, 4, 5, eps, 1), c) - want).max()))
    print("affine identity, eps 1e-2 / 1e-6 / 1e-10: deviation %.2e / %.2e / %.2e" % tuple(errs))
    assert errs[0] > errs[1] > errs[2] and errs[2] <= 1e-6
    # and rounding the grid to fp32 moves the sliced image by about one rounding of its coefficients
    A = O.fit(cl, CO.natural(5, 40, 56), 8, 4, 5)
    moved = float(np.abs(O.slice_(A.astype(np.float32), c) - O.slice_(A, c)).max())
    assert 0 < moved <= 4 * 2.0 ** -24 * max(1.0, np.abs(A).max()) * 4


def test_gated_cases_are_well_conditioned():
    """What keeps the GPU tests' absolute gates meaningful: every fit case has max |A| <= 4 and cond(Gv + lambda I) <= 1e6, so the fp64
    solve error (about cond * 2^-53) is far below the 2^-24 of the single rounding."""
    from tests import test_proxy_gpu as G
    assert len(G.FIT_CASES) == 6 * len(G.FIT_SHAPES) and set(c[6:] for c in G.FIT_CASES) == {(e, s) for e in (1e-2, 1e-4) for s in (0, 1, 4)}
    issue = [(1, 1, 1, 1, 1), (32, 32, 1, 1, 1), (3, 5, 3, 4, 6), (32, 48, 2, 2, 2), (40, 56, 8, 3, 4), (64, 96, 16, 5, 7), (70, 90, 32, 6, 7)]
    assert [s[:5] for s in G.FIT_SHAPES[:7]] == issue
    R = lib.BGRID_FIT_ROWS
    assert {s[0] for s in G.FIT_SHAPES if s[3] <= 2} >= {R - 1, R, R + 1}, "one row below, at and above the fit's row chunk"
    assert G.EMPTY_BINS in G.FIT_CASES and G.GATE == 2e-5 and G.ULP == 2.0 ** -23
    worst_a = worst_c = 0.0
    for h, w, gz, gh, gw, narrow, eps, smooth in G.FIT_CASES:
        cl, sl = G.fit_pair(h, w, narrow)
        A, _, cond, _ = O.fit(cl, sl, gz, gh, gw, eps, smooth, details=True)
        worst_a, worst_c = max(worst_a, float(np.abs(A).max())), max(worst_c, cond)
        assert np.abs(A).max() <= 4.0 and cond <= 1e6, (h, w, gz, gh, gw, narrow, eps, smooth, np.abs(A).max(), cond)
    print("fit cases: worst max |A| = %.3f, worst cond = %.3e" % (worst_a, worst_c))
    T = (lib.BGRID_TILE_H, lib.BGRID_TILE_W)
    sizes = {(H, W) for _, H, W in G.SLICE_CASES}
    assert sizes >= {(1, 1), (37, 53), (130, 257), (8, 8), (T[0] - 1, T[1] - 1), T, (T[0] + 1, T[1] + 1)}
    assert G.GRIDS["fine"][2:] == (4, 9, 9) and 4 * 9 * 9 > lib.BGRID_LDS_VERTICES >= 4 * 8 * 9


# ---------------------------------------------------------------------------------------------------------------- the edge cases
def test_edge_fit_cases_are_well_conditioned():
    """The condition of test_gated_cases_are_well_conditioned for every case of tests/proxy_edge_cases.py.  If an image or a seed ever
    breaks it, the case changes, never the bound."""
    from tests import proxy_edge_cases as E
    assert len(E.EDGE_FIT_CASES) == 6 * len(E.EDGE_FIT_SHAPES) and set(c[6:] for c in E.EDGE_FIT_CASES) == {(e, s) for e in (1e-2, 1e-4) for s in (0, 1, 4)}
    assert len(set(E.EDGE_FIT_CASES)) == len(E.EDGE_FIT_CASES)
    assert set(E.POISON_CASES) | set(E.UNREACHED) <= set(E.EDGE_FIT_CASES)
    worst_a, worst_c = (0.0, None), (0.0, None)
    for case in E.EDGE_FIT_CASES:
        _, _, A, _, cond = E.fit_reference(*case)
        a = float(np.abs(A).max())
        worst_a, worst_c = max(worst_a, (a, case)), max(worst_c, (cond, case))
        assert np.isfinite(A).all() and a <= 4.0 and cond <= 1e6, (case, a, cond)
    print("edge fit cases: worst max |A| = %.3f at %s, worst cond = %.3e at %s" % (worst_a[0], E.fit_id(worst_a[1]), worst_c[0], E.fit_id(worst_c[1])))


def test_wide_images_leave_the_unit_range_and_reach_both_ends_of_the_guide():
    from tests import proxy_edge_cases as E
    wide = [E.fit_images(h, w, kind)[0] for h, w, _, _, _, kind, _ in E.EDGE_FIT_SHAPES if kind == "wide"] + \
           [E.slice_image(H, W, kind) for _, _, _, H, W, kind, _ in E.EDGE_SLICE_CASES if kind == "wide"]
    assert len(wide) == 7
    big = [c for c in wide if c[0].size >= 4]
    assert len(big) == 6
    for c in big:
        g = O.guide(c)
        assert c.dtype == np.float32 and (g == 0.0).any() and (g == 1.0).any() and c.min() < 0.0 < 1.0 < c.max(), (c.shape, c.min(), c.max())
        assert [float(v) for v in c.reshape(3, -1)[0, :4]] == [0.0, 1.0, 2.0, -0.5]
        raw = O.LUMA @ c.reshape(3, -1).astype(np.float64)
        assert c[0].size < 100 or (raw < 0.0).sum() >= 10 and (raw > 1.0).sum() >= 10, "tens of pixels beyond either end besides the planted ones"
        print("wide %dx%d: content in [%.3f, %.3f], %d pixels with guide 0, %d with guide 1" % (c.shape[1:] + (c.min(), c.max(), (g == 0).sum(), (g == 1).sum())))
    assert all(np.isfinite(E.fit_images(h, w, kind)[1]).all() for h, w, _, _, _, kind, _ in E.EDGE_FIT_SHAPES), "the tone curve of a clipped content"
    # and no image gated before these reaches either end: tests/test_proxy_gpu.py's fit and slice images
    from tests import test_proxy_gpu as G
    for img in [G.fit_pair(h, w, narrow)[0] for h, w, _, _, _, narrow, _ in G.FIT_SHAPES] + [G.full_image(H, W) for _, H, W in G.SLICE_CASES]:
        g = O.guide(img)
        assert 0.0 < g.min() and g.max() < 1.0


def test_edge_cases_reach_the_branches_they_name():
    """Every count from the header's rule (tests/proxy_edge_cases.py: the oracle's tent, the header's constants), none from the product."""
    from tests import proxy_edge_cases as E
    src = open(os.path.join(REPO, "collaborative-distillation_amd", "csrc", "bgrid.hip")).read()
    assert "constexpr int BG_WX = %d;" % E.TABLE in src and "constexpr int BG_SLAB = %d;" % E.SLAB in src, "the two constants the header does not name"
    assert (E.ROWS, E.TW, E.TH, E.CAP) == (64, 128, 8, 320)
    shapes = [s[:5] for s in E.EDGE_FIT_SHAPES]
    assert len(set(s[:6] for s in E.EDGE_FIT_SHAPES)) == len(shapes)
    # column supports.  A support that is the whole row cannot be cut more generously: its width is exact.
    widths = {s: E.support_widths(s[1], s[4]) for s in shapes}
    whole = {max(ws) for s, ws in widths.items() if max(ws) == s[1]}
    assert {63, 64, 65, 128, E.TABLE, E.TABLE + 1, 300, 600} <= whole
    assert widths[(3, 600, 2, 1, 3)] == [300, 600, 300] and widths[(3, 500, 2, 1, 3)] == [250, 500, 250]
    mixed = [s for s, ws in widths.items() if min(ws) + 2 <= E.TABLE < max(ws) and s[1] > E.TABLE]
    assert (3, 500, 2, 1, 3) in mixed, "tabulated and untabulated vertices in one launch"
    assert widths[(100, 1, 2, 3, 1)] == [1] and widths[(2, 1024, 1, 1, 2)] == [1024, 1024]
    # row chunks: an outer vertex with fewer chunks than an inner one, however generously the support is cut
    chunks = {s: E.row_chunks(s[0], s[3]) for s in shapes}
    assert chunks[(200, 7, 2, 3, 2)] == [(2, 2), (4, 4), (2, 2)]
    assert [c[0] for c in chunks[(193, 5, 3, 4, 1)]] == [1, 3, 3, 1] and [c[1] for c in chunks[(193, 5, 3, 4, 1)]] == [2, 3, 3, 2]
    spans = E.vertex_spans(193, 4)
    assert spans[2][0] % E.ROWS != 0 or spans[3][0] % E.ROWS != 0, "a support starts inside a chunk of the image's rows"
    ragged = [s for s, c in chunks.items() if len(c) >= 3 and max(c[0][1], c[-1][1]) < max(lo for lo, _ in c[1:-1])]
    assert (200, 7, 2, 3, 2) in ragged and (193, 5, 3, 4, 1) in ragged
    # the totals
    counts = [E.slabs(*s[2:]) for s in shapes]
    assert counts.count(64) >= 2 and counts.count(65) == 2 and counts.count(67) == 2 and max(counts) == 67
    # ... and a lane's second step adds something: vertex (k, j, i) is number (k gh + j) gw + i, so the slabs past the 64th of a grid
    # with many bins are its brightest bins, which the images of fit_pair leave empty; the two grids of two bins put weight there
    assert [E.weight_past_slab(24, 24, *g, "fit") for g in ((5, 29, 113), (32, 23, 23))] == [0.0, 0.0]
    assert E.weight_past_slab(24, 24, 2, 91, 91, "fit") > 1.0 and E.weight_past_slab(24, 24, 2, 92, 92, "fit") > 10.0
    assert 5 * 29 * 113 == 64 * E.SLAB + 1 and E.slabs(32, 2, 256) == 64 and (32, 40, 32, 2, 256) in shapes and (20, 12, 1, 256, 3) in shapes
    for case in E.UNREACHED:
        _, _, A, Ag, _ = E.fit_reference(*case)
        Gv, _ = O.sums(*E.fit_images(*case[:2], case[5]), *case[2:5])
        reached = Gv[..., 3, 3] != 0.0
        assert case[7] == 0 and 0 < reached.sum() < reached.size / 2 and np.abs(A[~reached] - Ag).max() <= 1e-13 and np.abs(A[reached] - Ag).max() > 1e-3
    # the slice
    cases = [c[:6] for c in E.EDGE_SLICE_CASES]
    assert len(set(cases)) == len(cases) == 18
    assert set(E.MIXED + E.AT_CAP + E.OVER_CAP + E.BITWISE + [E.NONFINITE]) <= set(cases)
    foot = {c: E.tile_footprints(*c[:5]) for c in cases}
    for c, f in foot.items():
        assert len(f) == -(-c[3] // E.TH) * -(-c[4] // E.TW) and min(f) >= c[0] and max(f) <= c[0] * c[1] * c[2], c
    assert foot[(4, 2, 100, 8, 130, "full")] == [792, 24]
    f = foot[(4, 20, 100, 17, 258, "full")]
    assert len(f) == 9 and sum(n > E.CAP for n in f) == 6 and sum(n <= E.CAP for n in f) == 3
    both = [c for c, f in foot.items() if min(f) <= E.CAP < max(f)]
    assert set(E.MIXED) <= set(both) and len(E.MIXED) >= 2        # the largest x axis over three tiles mixes the paths too
    assert all(foot[c] == [E.CAP] for c in E.AT_CAP) and foot[E.OVER_CAP[0]] == [E.CAP + 1] and foot[E.OVER_CAP[1]] == [330]
    assert len(foot[(8, 5, 7, 1, 1000, "full")]) == 8 and len(foot[(8, 5, 7, 1000, 1, "full")]) == 125
    for axis in range(3):
        assert any(c[axis] == 1 and all(c[a] > 1 for a in range(3) if a != axis) for c in cases), axis
    assert (1, 1, 1) in {c[:3] for c in cases} and {32} <= {c[0] for c in cases} and {256} <= {c[1] for c in cases} & {c[2] for c in cases}
    assert {c[4] % 4 for c in cases} >= {1, 2} and any(c[4] < 4 and c[4] > 1 for c in cases)
    grid = E.random_grid(8, 5, 7)
    assert grid.dtype == np.float32 and -0.3 <= grid.min() < -0.25 and 0.65 < grid.max() < 0.7


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def declared():
    return sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"wct_ctx"})


def test_header_and_symbol_list_agree():
    assert declared() and declared() == sorted(lib.SYMBOLS_BGRID)
    others = set(lib.SYMBOLS) | set(lib.SYMBOLS_COLOR) | set(lib.SYMBOLS_SMOOTH) | set(lib.SYMBOLS_SCALE)
    assert not set(lib.SYMBOLS_BGRID) & others
    for other in ("wct_hip.h", "wct_hip_color.h", "wct_hip_smooth.h", "wct_hip_scale.h"):
        text = open(os.path.join(REPO, "include", other)).read()
        assert not set(lib.SYMBOLS_BGRID) & set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", text)), other


def test_built_library_exports_the_proxy_entries():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_BGRID:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_BGRID) <= exported
    assert not [s for s in exported if "bgrid" in s and s not in lib.SYMBOLS_BGRID], "the launchers stay inside the library"


def test_bgrid_shape_is_host_only_and_the_oracles():
    import ctypes
    L = lib.load()
    gh, gw = ctypes.c_int(), ctypes.c_int()
    for h, w, cell in ((64, 96, 16), (65, 97, 16), (1, 1, 16), (40, 56, 8), (255 * 16, 3, 16), (540, 960, 16)):
        assert L.wct_bgrid_shape(h, w, cell, ctypes.byref(gh), ctypes.byref(gw)) == lib.WCT_OK
        assert (gh.value, gw.value) == O.shape(h, w, cell)
    for h, w, cell in ((0, 1, 16), (1, 0, 16), (1, 1, 0), (255 * 16 + 1, 1, 16), (1, 4096, 16)):
        assert L.wct_bgrid_shape(h, w, cell, ctypes.byref(gh), ctypes.byref(gw)) == lib.WCT_ERR_INVALID
    assert L.wct_bgrid_shape(8, 8, 16, None, ctypes.byref(gw)) == lib.WCT_ERR_INVALID


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_bgrid.c"
    src.write_text('#include "wct_hip_bgrid.h"\n'
                   "int use(wct_ctx* c, const float* p, float* q, uint8_t* b, int* n) {\n"
                   "  return wct_bgrid_shape(64, 96, WCT_BGRID_CELL, n, n + 1)\n"
                   "    + wct_bgrid_fit(c, p, p, 64, 96, WCT_BGRID_BINS, 5, 7, WCT_BGRID_EPS, WCT_BGRID_SMOOTH, q)\n"
                   "    + wct_bgrid_slice(c, p, WCT_BGRID_MAX_Z, WCT_BGRID_MAX_XY, 7, p, 128, 192, 0, b, 1)\n"
                   "    + wct_stylize_proxy(c, p, 128, 192, p, 32, 32, 1.0f, 1, WCT_SCALE_MAX_DIVISOR, WCT_BGRID_CELL, WCT_BGRID_BINS, WCT_BGRID_EPS,\n"
                   "                        WCT_BGRID_SMOOTH, q, 0, 0) + WCT_OK; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(REPO, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_header_states_its_contract():
    text = open(HEADER).read()
    assert '#include "wct_hip_scale.h"' in text and "Bilateral Guided Upsampling" in text
    for word in ("CHOLESKY", "rounded ONCE", "NOT clamped", "No floating-point atomics", "THE SLICE INTERPOLATES IN FP64", "out_planar == content is ALLOWED",
                 "a look, not a measurement", "0.299 R + 0.587 G + 0.114 B", "ws_allocs", "Bit-identical to that composition"):
        assert word in text, word


def test_constants_of_the_binding_are_the_headers():
    text = open(HEADER).read()
    val = lambda name: re.search(r"#define %s (\S+)" % name, text).group(1)
    assert (int(val("WCT_BGRID_MAX_XY")), int(val("WCT_BGRID_MAX_Z")), int(val("WCT_BGRID_MAX_SMOOTH"))) == \
        (lib.BGRID_MAX_XY, lib.BGRID_MAX_Z, lib.BGRID_MAX_SMOOTH) == (256, 32, 4)
    assert (int(val("WCT_BGRID_FIT_ROWS")), int(val("WCT_BGRID_TILE_W")), int(val("WCT_BGRID_TILE_H")), int(val("WCT_BGRID_LDS_VERTICES"))) == \
        (lib.BGRID_FIT_ROWS, lib.BGRID_TILE_W, lib.BGRID_TILE_H, lib.BGRID_LDS_VERTICES)
    assert (int(val("WCT_BGRID_CELL")), int(val("WCT_BGRID_BINS")), float(val("WCT_BGRID_EPS")), int(val("WCT_BGRID_SMOOTH"))) == \
        (lib.BGRID_CELL, lib.BGRID_BINS, lib.BGRID_EPS, lib.BGRID_SMOOTH) == (O.CELL, O.BINS, O.EPS, O.SMOOTH) == (16, 8, 1e-2, 1)
    assert lib.BGRID_LDS_VERTICES * 48 <= 64 * 1024, "the staged footprint fits the LDS of a workgroup"


def test_history_cases_cover_the_entries():
    from tests import test_proxy_gpu as G
    covered = set(sym for c in G.CASES.values() for sym in c.covers)
    assert covered == set(lib.SYMBOLS_BGRID)
    assert set(c.size for c in G.CASES.values()) == {"small", "large"}


def test_product_keeps_the_test_oracle_out():
    pkg = os.path.join(REPO, "collaborative-distillation_amd")
    for rel in ("csrc/bgrid.hip", "csrc/api_bgrid.hip", "wct_hip/lib.py", "wct_hip/wct.py", "wct_hip/cli.py", "../include/wct_hip_bgrid.h"):
        text = open(os.path.join(pkg, rel)).read()
        assert "proxy_oracle" not in text and not re.search(r"wct_oracle|liboracle|oracle/", text), rel


def test_build_lists_the_new_sources():
    text = open(os.path.join(REPO, "collaborative-distillation_amd", "build.sh")).read()
    src = re.search(r'^SRC="([^"]*)"', text, re.M).group(1).split()
    assert "bgrid" in src and "api_bgrid" in src and "../include/wct_hip_bgrid.h" in re.search(r'^HDR="([^"]*)"', text, re.M).group(1).split()


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    return cli.build_parser().parse_args(list(argv))


def test_parser_flag_defaults():
    a = parse()
    assert a.proxy_scale is None and a.proxy_cell is None and a.proxy_bins is None and a.proxy_eps is None and a.proxy_smooth is None
    a = parse("--proxy_scale", "4", "--proxy_cell", "8", "--proxy_bins", "16", "--proxy_eps", "1e-3", "--proxy_smooth", "2")
    assert (a.proxy_scale, a.proxy_cell, a.proxy_bins, a.proxy_eps, a.proxy_smooth) == (4, 8, 16, 1e-3, 2)
    with pytest.raises(SystemExit):
        parse("--proxy_scale", "2.5")
    with pytest.raises(SystemExit):
        parse("--proxy_scale")


def test_select_mode_looks_at_the_proxy_behind_the_table():
    assert cli.select_mode(parse()) is None
    assert cli.select_mode(parse("--proxy_scale", "2")) is cli.PROXY_MODE
    assert cli.PROXY_MODE not in cli.MODES and cli.PROXY_MODE.name == "proxy" and cli.PROXY_MODE.run is cli.run_proxy
    assert cli.PROXY_MODE.early and cli.PROXY_MODE.noun == "pair" and "serial loop" in cli.PROXY_MODE.reason
    assert cli.select_mode(parse("--diversity", "1")) is cli.DIVERSE_MODE
    assert cli.select_mode(parse("--proxy_scale", "2", "--level_scale", "2,2,1,1,1")).name == "scale"      # the table first (check_proxy_args refuses the mix)


def test_check_proxy_args_fills_the_defaults_and_refuses():
    a = parse()
    cli.check_proxy_args(a)
    assert a.proxy_scale is None and a.proxy_cell is None
    cli.check_proxy_args(types.SimpleNamespace(synthesis=False))          # a namespace from before the flags existed
    a = parse("--proxy_scale", "2")
    cli.check_proxy_args(a)
    assert (a.proxy_cell, a.proxy_bins, a.proxy_eps, a.proxy_smooth) == (lib.BGRID_CELL, lib.BGRID_BINS, lib.BGRID_EPS, lib.BGRID_SMOOTH)
    a = parse("--proxy_scale", "16", "--proxy_cell", "4", "--proxy_bins", "32", "--proxy_eps", "1e-4", "--proxy_smooth", "0", "--alpha", "0.6",
              "--num_run", "2", "--transform", "ot", "--content_size", "512", "--style_size", "256", "--round", "1")
    cli.check_proxy_args(a)
    assert (a.proxy_cell, a.proxy_bins, a.proxy_eps, a.proxy_smooth) == (4, 32, 1e-4, 0)
    for flag in ("--proxy_cell", "--proxy_bins", "--proxy_eps", "--proxy_smooth"):
        with pytest.raises(ValueError, match="%s does nothing without --proxy_scale" % flag):
            cli.check_proxy_args(parse(flag, "2"))
    for bad in ("0", "17", "-2"):
        with pytest.raises(ValueError, match="--proxy_scale"):
            cli.check_proxy_args(parse("--proxy_scale=" + bad))
    for flag, bads in (("--proxy_cell", ("0", "-1")), ("--proxy_bins", ("0", "33")), ("--proxy_eps", ("0", "-1e-3", "inf", "nan")),
                       ("--proxy_smooth", ("-1", "5"))):
        for bad in bads:
            with pytest.raises(ValueError, match=flag):
                cli.check_proxy_args(parse("--proxy_scale", "2", "%s=%s" % (flag, bad)))
    clashes = [(("--synthesis",), "--synthesis"), (("--maskPath", "m"), "--maskPath"), (("--interp_styles", "a.png,b.png"), "--interp_styles"),
               (("--weightPath", "w"), "--weightPath"), (("--video",), "--video"), (("--swap_level", "3"), "--swap_level"),
               (("--level_scale", "2,2,1,1,1"), "--level_scale"), (("--auto_regions", "3"), "--auto_regions"), (("--diversity", "1"), "--diversity"),
               (("--preserve_color", "luma"), "--preserve_color"), (("--preserve_color", "match"), "--preserve_color"),
               (("--smooth_radius", "8"), "--smooth_radius")]
    for extra, name in clashes:
        with pytest.raises(ValueError, match="--proxy_scale does not mix with .*%s" % name):
            cli.check_proxy_args(parse("--proxy_scale", "2", *extra))


def test_main_refuses_before_it_touches_anything(tmp_path):
    out = tmp_path / "o"
    with pytest.raises(ValueError, match="--proxy_scale does not mix with --smooth_radius"):
        cli.main(["--mode", "16x", "--proxy_scale", "2", "--smooth_radius", "8", "--outf", str(out)])
    with pytest.raises(ValueError, match="--proxy_bins does nothing without --proxy_scale"):
        cli.main(["--mode", "16x", "--proxy_bins", "4", "--outf", str(out)])
    assert not out.exists()


def test_output_names_with_and_without_the_flag():
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_b+s1.jpg")
    plain = types.SimpleNamespace(outf="o", log_mark="L", mode="16x", alpha=1)           # a namespace from before the flags existed
    assert cli.out_name(plain, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=1_b+s1.jpg")
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--alpha", "0.6", "--proxy_scale", "2")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=0.6_proxy=2_b+s1.jpg")
    a = parse("--mode", "16x", "--outf", "o", "--log_mark", "L", "--proxy_scale", "8", "--transform", "ot")
    assert cli.out_name(a, "b+s1.jpg") == os.path.join("o", "L_mode=16x_alpha=1_transform=ot_proxy=8_b+s1.jpg")
