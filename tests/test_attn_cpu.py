"""Attention statistics without a GPU: the public header and its bindings, identities of the numpy reference (tests/attn_oracle.py), the
command line's --swap_match attention / --swap_temp, the input condition of the GPU level tests, and the launch plan and the edge cases of
tests/test_attn_edges_gpu.py (tests/attn_cases.py): the plan against the source, and that every planted case separates a wrong kernel."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import attn_cases as AC
from tests import attn_oracle as A
from tests import sweep_cases
from tests import width_models as wm
from tests.conftest import PKG, REPO
from tests.test_attn_gpu import FLOOR_MEAN, FLOOR_VAR
from wct_hip import cli, lib

HEADER = os.path.join(REPO, "include", "wct_hip_attn.h")
OTHER_LISTS = ("SYMBOLS", "SYMBOLS_COLOR", "SYMBOLS_SMOOTH", "SYMBOLS_TRANSFORM", "SYMBOLS_SWAP", "SYMBOLS_SCALE", "SYMBOLS_GUIDED", "SYMBOLS_VIDEO",
               "SYMBOLS_MOTION")


# ---------------------------------------------------------------------------------------------------------------- header and bindings
def test_header_and_symbol_list_agree():
    text = open(HEADER).read()
    declared = sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", text)) - {"wct_ctx"})
    assert declared and declared == sorted(lib.SYMBOLS_ATTN) and len(set(lib.SYMBOLS_ATTN)) == len(lib.SYMBOLS_ATTN)
    for other in OTHER_LISTS:
        assert not set(lib.SYMBOLS_ATTN) & set(getattr(lib, other)), other
    inc = os.path.join(REPO, "include")
    for name in os.listdir(inc):                                            # declared here and nowhere else
        if name != "wct_hip_attn.h":
            assert not set(lib.SYMBOLS_ATTN) & set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", open(os.path.join(inc, name)).read())), name
    main_header = open(os.path.join(inc, "wct_hip.h")).read()
    assert "attn" not in main_header and not [s for s in lib.SYMBOLS if "attn" in s]     # wct_hip.h and lib.SYMBOLS are as they were
    for name, value in (("WCT_ATTN_EPS", lib.ATTN_EPS), ("WCT_ATTN_MAX_TEMP", lib.ATTN_MAX_TEMP), ("WCT_ATTN_STANDARD", lib.ATTN_STANDARD),
                        ("WCT_ATTN_WHITENED", lib.ATTN_WHITENED), ("WCT_ATTN_QUERY_TILE", lib.ATTN_QUERY_TILE),
                        ("WCT_ATTN_KEY_TILE", lib.ATTN_KEY_TILE), ("WCT_ATTN_QUERY_CHUNK", lib.ATTN_QUERY_CHUNK)):
        m = re.search(r"#define %s\s+(\S+)" % name, text)
        assert m and float(m.group(1)) == float(value), name
    assert lib.ATTN_MATCHES == {"attention": lib.ATTN_STANDARD, "attention_whitened": lib.ATTN_WHITENED}
    assert tuple(lib.ATTN_MATCHES) == cli.ATTN_MATCH_NAMES and not set(lib.ATTN_MATCHES) & set(lib.SWAP_MATCHES)
    assert (A.EPS, A.ADAIN_EPS, A.MAX_TEMP) == (lib.ATTN_EPS, lib.ADAIN_EPS, lib.ATTN_MAX_TEMP)
    assert (A.STANDARD, A.WHITENED) == (lib.ATTN_STANDARD, lib.ATTN_WHITENED)


def test_the_tile_constants_of_the_tests_are_the_kernel_s():
    src = open(os.path.join(PKG, "csrc", "attn.hip")).read()
    m = re.search(r"constexpr int AT_QT = (\d+), AT_KT = (\d+), AT_CS = (\d+)", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (AC.QUERY_TILE, AC.KEY_TILE) == (lib.ATTN_QUERY_TILE, lib.ATTN_KEY_TILE)
    assert int(m.group(3)) == 128                                            # the value slab: C = 512 runs four
    h, w, hs, ws, _ = AC.STATS_SHAPES[-1]
    assert h * w % AC.QUERY_TILE == 1 and h * w > AC.QUERY_TILE and hs * ws % AC.KEY_TILE == 1 and hs * ws > AC.KEY_TILE
    # the range contract: nothing here clamps or raises the flag, and nothing synchronises lanes in software
    assert ".commit(" not in src and "sat_raise(" not in src and "atomic" not in src.replace("no atomics", "")
    build = open(os.path.join(PKG, "build.sh")).read()
    assert re.search(r'^SRC=".*\bswap attn\b.*\bapi_swap api_attn\b.*"', build, re.M) and "../include/wct_hip_attn.h" in build


def test_built_library_exports_the_attn_entries_and_hides_the_helpers():
    import __graft_entry__ as g
    g.build()
    L = lib.load()
    for s in lib.SYMBOLS_ATTN:
        assert hasattr(L, s), s
    out = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(lib.SYMBOLS_ATTN) <= exported
    assert not [s for s in exported if "attn" in s and s not in lib.SYMBOLS_ATTN]


def test_header_is_c99_clean_on_its_own(tmp_path):
    src = tmp_path / "only_attn.c"
    src.write_text('#include "wct_hip_attn.h"\n'
                   "int main(void) { return (WCT_ATTN_STANDARD == 0 && WCT_ATTN_WHITENED == 1 && WCT_ATTN_MAX_TEMP == 32 && WCT_ATTN_EPS > 0 &&\n"
                   "  WCT_ATTN_QUERY_CHUNK % WCT_ATTN_QUERY_TILE == 0 && WCT_ATTN_KEY_TILE == 32) ? 0 : 1; }\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), "-c", str(src), "-o",
                    str(tmp_path / "only_attn.o")], check=True)


# ---------------------------------------------------------------------------------------------------------------- oracle identities
@pytest.mark.parametrize("h,w,hs,ws,C", AC.STATS_SHAPES[:3])
def test_oracle_tau_zero_is_adain_with_the_population_variance(h, w, hs, ws, C):
    cF, sF = A.relu_map(1, h, w, C), A.relu_map(2, hs, ws, C)
    for domain in (A.STANDARD, A.WHITENED):
        csF, m, v = A.level_feature(cF, sF, domain, 0.0, 1.0)
        nk = hs * ws
        vs = np.asarray(sF, np.float64).reshape(-1, C).var(0, ddof=1)
        assert np.abs(m).max() < 1e-12
        assert np.abs(v - (nk - 1) / nk * vs / (vs + A.ADAIN_EPS)).max() < 1e-12
        # i.e. the content's standardised map with the style's mean and POPULATION deviation (+ eps (Nk - 1) / Nk ... exactly as the header says)
        mu_s, sig_s = A.moments(sF)
        want = sig_s * np.sqrt((nk - 1) / nk * vs / (vs + A.ADAIN_EPS)) * A.standardise(cF) + mu_s
        assert np.abs(csF - want).max() < 1e-10


def test_oracle_a_key_equal_to_the_query_takes_all_the_weight_as_tau_grows():
    sF = A.relu_map(3, 9, 8, 12)
    khat, sstd = A.project(sF, A.STANDARD)
    k, v = khat.reshape(-1, 12), sstd.reshape(-1, 12)
    picks = np.array([5, 17, 40])
    last = None
    for tau in (8.0, 32.0, 256.0, 4096.0):
        Aw = A.weights(k[picks], k, tau)
        own = Aw[np.arange(3), picks]
        assert last is None or (own >= last).all()
        last = own
    assert (last > 1 - 1e-9).all()
    m, var = A.stats(k[picks], k, v, 4096.0)
    assert np.abs(m - v[picks]).max() < 1e-6 and var.max() < 1e-6          # the 1 x 1 nearest-feature swap


def test_oracle_is_invariant_to_the_order_of_the_keys():
    q, k, v = AC.stats_inputs(7, 9, 5, 6, 8)
    perm = np.random.default_rng(4).permutation(k.shape[0])
    for tau in AC.TAUS:
        m0, v0 = A.stats(q, k, v, tau)
        m1, v1 = A.stats(q, k[perm], v[perm], tau)
        assert np.abs(m0 - m1).max() < 1e-12 and np.abs(v0 - v1).max() < 1e-12


def test_oracle_apply_emulation_is_the_fp64_formula_to_fp32_rounding():
    rng = np.random.default_rng(5)
    n, C = 33, 12
    m, z, x = (rng.standard_normal((n, C)).astype(np.float32) for _ in range(3))
    v = rng.random((n, C)).astype(np.float32)
    mu, sg = rng.standard_normal(C), rng.random(C) + 0.5
    for alpha in (1.0, 0.6):
        got = A.apply_f32_emulation(m, v, z, x, mu, sg, alpha)
        want = A.apply(m, v, z, x, mu, sg, alpha)
        assert got.dtype == np.float32 and np.abs(got - want).max() < 2e-6 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------------------- the input condition
def test_the_input_condition_on_random_maps_as_stated():
    """ReLU-like random maps at the three non-degenerate shapes: min var is above the floor for tau <= 4 -- the regime in which results may be
    compared through the sqrt; beyond it (tau = 16, 32) results are compared on (mean, var) only, whatever min var is.  The fp32 arm's
    distance from fp64 on the mean is printed (about 1e-6 of max |V| at every tau on these maps)."""
    for h, w, hs, ws, C in AC.CONDITION_SHAPES:
        q, k, v = AC.stats_inputs(h, w, hs, ws, C)
        vmax = np.abs(v).max()
        for tau in (0.0, 4.0, 16.0, 32.0):
            m64, v64 = A.stats(q, k, v, tau)
            m32, _ = A.stats(q, k, v, tau, np.float32)
            print("C=%d tau=%g: e32(mean) %.2e, min var %.2e" % (C, tau, np.abs(m32 - m64).max() / vmax, v64.min()))
            if tau <= 4:
                assert v64.min() >= AC.MIN_VAR, (C, tau, v64.min())


@pytest.mark.parametrize("model,level,domain", AC.LEVEL_CASES)
def test_the_gpu_level_cases_meet_the_input_condition(model, level, domain):
    """Every (model, level, domain) tests/test_attn_gpu.py runs through wct_attn_level: the fp64 oracle's min var over all queries and the
    style's live channels is at least 1e-4.  Below it sqrt(var) turns a 1e-7 error of var into 3e-4 of the output and the comparison would
    no longer measure the kernel.  A case that fails this is a failure HERE, never a skip there."""
    _, sF = AC.level_features(model, level)
    _, _, var = AC.level_reference(model, level, domain)
    live = A.live_channels(sF)
    assert live.any()
    print("%s level %d domain %d: min var over %d live channels %.3e" % (model, level, domain, int(live.sum()), var[:, live].min()))
    assert var[:, live].min() >= AC.MIN_VAR


@pytest.mark.parametrize("model,level,domain", AC.EDGE_LEVEL_CASES)
def test_the_gpu_edge_level_cases_meet_the_input_condition(model, level, domain):
    """The same statement for the level cases of tests/test_attn_edges_gpu.py (E8): level 3 at C = 256 and at C = 132.  The stand-in model
    is one wct_load_module takes, every module of it."""
    widths = AC.ALL_LEVEL_MODELS[model][0]
    for lv in (1, 2, 3, 4, 5):
        assert wm.loadable("enc", wm.encoder_layers(widths, lv)) and wm.loadable("dec", wm.decoder_layers(widths, lv)), (model, lv)
    cF, sF = AC.level_features(model, level)
    assert cF.shape[-1] == widths[3] == {"wide": 256, "w132": 132}[model]
    _, _, var = AC.level_reference(model, level, domain)
    live = A.live_channels(sF)
    assert live.any()
    print("%s level %d domain %d: min var over %d live channels %.3e" % (model, level, domain, int(live.sum()), var[:, live].min()))
    assert var[:, live].min() >= AC.MIN_VAR


# ---------------------------------------------------------------------------------------------------------------- the launch plan and the edge cases
def gates(e32):
    """The gate of wct_attn_stats (tests/test_attn_gpu.py) for a case whose fp32 arm is at e32 = (mean, var)."""
    return 4 * e32[0] + FLOOR_MEAN, 4 * e32[1] + FLOOR_VAR


def test_the_plan_constants_are_the_kernel_s():
    src = open(os.path.join(PKG, "csrc", "attn.hip")).read()
    api = open(os.path.join(PKG, "csrc", "api_attn.hip")).read()
    header = open(HEADER).read()
    m = re.search(r"constexpr int AT_QT = (\d+), AT_KT = (\d+), AT_CS = (\d+)", src)
    assert m and int(m.group(3)) == AC.VALUE_SLAB
    m = re.search(r"#define WCT_ATTN_QUERY_CHUNK\s+(\d+)", header)
    assert m and int(m.group(1)) == AC.QUERY_CHUNK == lib.ATTN_QUERY_CHUNK and AC.QUERY_CHUNK % AC.QUERY_TILE == 0
    assert "ctx->attn_query_chunk > 0 ? ctx->attn_query_chunk : WCT_ATTN_QUERY_CHUNK" in api
    assert '"%s"' % AC.PROFILE_NAME in api and '"l%d.s%u", nlaunch, slabs' in src
    # the expressions `plan` restates
    for text in ("(C + AT_CS - 1) / AT_CS", "(e - b + AT_QT - 1) / AT_QT", "((long)Nk + AT_KT - 1) / AT_KT", "const int nct = (slabC + 15) >> 4;",
                 "const int nks = cleft >= 128 ? 4 : (cleft + 31) >> 5;", "if (c + 4 < C) b ="):
        assert text in src, text
    m = re.search(r"constexpr int AW_PIX = (\d+);", src)
    assert m and int(m.group(1)) == AC.WHITEN_PIX
    assert AC.WIDTHS == sweep_cases.WIDTHS and len(AC.WIDTHS) == 128


def test_the_plan_on_worked_cases():
    P = AC.plan
    assert P(65, 33, 4) == AC.Plan(1, 1, (2,), 2, 1, 1, True, "l1.s1")
    assert P(64, 32, 128) == AC.Plan(1, 1, (1,), 1, 8, 4, False, "l1.s1")
    assert P(65, 33, 132) == AC.Plan(1, 2, (2,), 2, 1, 1, True, "l1.s2")
    assert P(2, 2, 256) == AC.Plan(1, 2, (1,), 1, 8, 4, False, "l1.s2")
    assert P(70, 129, 360) == AC.Plan(1, 3, (2,), 5, 7, 4, False, "l1.s3")          # 104 channels left: 6.5 value tiles, 3.25 score steps
    assert P(70, 129, 388) == AC.Plan(1, 4, (2,), 5, 1, 1, True, "l1.s4")
    assert P(AC.SPLIT_NQ, 33, 132) == AC.Plan(2, 2, (512, 2), 2, 1, 1, True, "l2.s2")
    assert P(AC.SPLIT_NQ, 33, 4).form == "l2.s1" and P(AC.QUERY_CHUNK, 33, 4).form == "l1.s1"
    assert P(203, 378, 36, chunk=50) == AC.Plan(5, 1, (1, 1, 1, 1, 1), 12, 3, 2, True, "l5.s1")
    assert AC.profile_name(65, 33, 512) == "attn_stats<f16x3>:l1.s4"


def test_the_case_lists_reach_every_tail_class():
    """(nct of the last slab, nks of the last chunk, half-live last group): 16 classes over the 128 widths.  The bands of E1 hold every
    width; the planted list of E2 must be shown to hold every class, in one slab and in several."""
    every = {AC.tail_class(C) for C in AC.WIDTHS}
    assert len(every) == 16 and every == {(n, (n + 1) // 2, h) for n in range(1, 9) for h in (False, True)}
    assert sorted(C for b in sweep_cases.BANDS for C in b) == list(AC.WIDTHS)
    assert {AC.tail_class(C) for C in AC.PLANT_WIDTHS} == every
    assert {AC.tail_class(C) for C in AC.PLANT_WIDTHS if C > 128} == every
    named = (4, 8, 12, 20, 28, 36, 100, 124, 132, 136, 156, 252, 256, 260, 264, 380, 388, 508, 512)
    assert AC.PLANT_WIDTHS[:len(named)] == named and len(set(AC.PLANT_WIDTHS)) == len(AC.PLANT_WIDTHS)
    assert {AC.plan(2, 2, C).slabs for C in AC.ROLL_WIDTHS} == {2, 3, 4} and all(r % 4 == 0 for r in AC.ROLLS)
    assert AC.plants(4) == {"last4": 0} and AC.plants(12) == {"last4": 8, "hi_half": 4} and AC.plants(136) == {"last4": 132, "chunk_first": 128}
    assert AC.plants(132) == {"last4": 128, "hi_half": 124} and AC.plants(260) == {"last4": 256, "hi_half": 252}
    assert AC.plants(264) == {"last4": 260, "chunk_first": 256}


@pytest.mark.parametrize("C", AC.PLANT_WIDTHS)
def test_e2_the_planted_group_decides(C):
    """Zeroing the planted group in k^ moves the fp64 mean by at least 0.1 max |V|: a staging that drops, zero-fills or misplaces those four
    channels cannot pass a gate of 5e-6."""
    q0, k0, v0 = AC.edge_inputs(C)
    for name, c0 in AC.plants(C).items():
        q, k, v = AC.planted_inputs(C, c0)
        assert q.dtype == np.float32 and np.abs((q.astype(np.float64) ** 2).sum(1) - 1).max() < 1e-6 and np.array_equal(v, v0)
        share = (k.astype(np.float64)[:, c0:c0 + 4] ** 2).sum(1)
        (m64, _), e32, vmax = AC.reference(q, k, v, AC.PLANT_TAU)
        cut = np.array(k)
        cut[:, c0:c0 + 4] = 0
        moved = np.abs(A.stats(q, cut, v, AC.PLANT_TAU)[0] - m64).max() / vmax
        print("E2 C=%d %s (channels %d..%d): median share of |k^|^2 %.2f, zeroing moves the mean by %.3f max|V|; gate %.2e / %.2e"
              % (C, name, c0, c0 + 3, np.median(share), moved, *gates(e32)))
        assert moved >= 0.1, (C, name, moved)


def test_e4_the_standardised_key_subsets_have_the_header_s_tau_zero_statistics():
    for C in AC.BORDER_WIDTHS:
        for Nk in AC.BORDER_NK:
            v, want = AC.border_standardised(C, Nk)
            q, k, _ = AC.border_inputs(C, 65, Nk)
            m64, v64 = A.stats(q, k, v, 0.0)
            vmax = np.abs(v).max()
            assert np.abs(m64).max() / vmax < 1e-7 and np.abs(v64 - want).max() / vmax ** 2 < 1e-6, (C, Nk)      # V rounded to fp32 once


@pytest.mark.parametrize("C", AC.RUN_WIDTHS)
def test_e5_the_key_orders_drive_the_running_maximum(C):
    """Ascending: every query's per-tile maximum strictly increases over all five tiles; descending (and "own"): never after tile 0.  In
    "own" every key but the first is at least 1.69 tau below it: P' = 2^15 e^(-54) rounds to 0 in f16 (smallest subnormal 6e-8)."""
    for order in AC.RUN_ORDERS:
        q, k, v = AC.running_inputs(C, order)
        assert q.shape == (AC.RUN_NQ, C) and k.shape == v.shape == (AC.RUN_NK, C) and AC.plan(AC.RUN_NQ, AC.RUN_NK, C).key_tiles == 5
        assert np.abs((k.astype(np.float64) ** 2).sum(1) - 1).max() < 1e-6
        tm = AC.tile_maxima(q, k, AC.RUN_TAU)
        assert tm.shape == (AC.RUN_NQ, 5)
        if order.endswith("up"):
            assert (np.diff(tm, axis=1) > 0).all(), order
            print("E5 C=%d %s: smallest / largest step of a tile maximum %.3f / %.3f" % (C, order, np.diff(tm, axis=1).min(), np.diff(tm, axis=1).max()))
        else:
            assert (tm[:, 1:] < tm[:, :1]).all(), order
    sets = [sorted(map(bytes, AC.running_inputs(C, o)[1])) for o in ("up", "down", "own")]
    assert sets[0] == sets[1] == sets[2], "one key set in three orders"
    q, k, v = AC.running_inputs(C, "own")
    s = AC.RUN_TAU * (q.astype(np.float64) @ k.astype(np.float64).T)
    assert (s[:, 1:].max(1) - s[:, 0] <= -1.69 * AC.RUN_TAU).all() and 2.0 ** 15 * np.exp(-1.69 * AC.RUN_TAU) < 2.0 ** -25
    m64, v64 = A.stats(q, k, v, AC.RUN_TAU)
    assert np.abs(m64 - v[0]).max() < 1e-12 and v64.max() < 1e-12
    drop = np.exp(s[:, 1:] - s[:, :1]).sum(1).max()
    assert drop <= AC.RUN_NK * 2.0 ** -40                                      # the header's bound on the weight mass a conversion may drop


def test_e5_the_online_walk_is_the_oracle_and_its_mutants_are_not():
    """online_stats is attn_oracle.stats to 1e-12.  The walk that never rescales differs from fp64 by at least 100 gates on the ascending
    orders; the walk that counts the pad keys of the last tile differs by at least 100 gates on E4's Nk = 33 at tau = 0 (where a pad key
    has the weight of a key; at tau = 32 its score 0 lies 10 and more below the maximum)."""
    for C in AC.RUN_WIDTHS:
        for order in AC.RUN_ORDERS:
            q, k, v = AC.running_inputs(C, order)
            (m64, v64), e32, vmax = AC.reference(q, k, v, AC.RUN_TAU)
            gm, gv = gates(e32)
            m, var = AC.online_stats(q, k, v, AC.RUN_TAU)
            assert np.abs(m - m64).max() < 1e-12 and np.abs(var - v64).max() < 1e-12
            m, var = AC.online_stats(q, k, v, AC.RUN_TAU, rescale=False)
            dm, dv = np.abs(m - m64).max() / vmax, np.abs(var - v64).max() / vmax ** 2
            print("E5 C=%d %s: never rescaling is off by %.2e / %.2e (gates %.2e / %.2e)" % (C, order, dm, dv, gm, gv))
            if order.endswith("up"):
                assert dm >= 100 * gm and dv >= 100 * gv, (C, order, dm, dv)
            else:
                assert dm < 1e-12 and dv < 1e-12                              # nothing to rescale: why the ascending orders are needed
    for C in AC.BORDER_WIDTHS:
        q, k, v = AC.border_inputs(C, 65, 33)
        (m64, v64), e32, vmax = AC.reference(q, k, v, 0.0)
        gm, gv = gates(e32)
        m, var = AC.online_stats(q, k, v, 0.0)
        assert np.abs(m - m64).max() < 1e-12 and np.abs(var - v64).max() < 1e-12
        m, var = AC.online_stats(q, k, v, 0.0, count_pad=True)
        dm, dv = np.abs(m - m64).max() / vmax, np.abs(var - v64).max() / vmax ** 2
        print("E4 C=%d Nk=33 tau=0: counting the 31 pad keys is off by %.2e / %.2e (gates %.2e / %.2e)" % (C, dm, dv, gm, gv))
        assert dm >= 100 * gm and dv >= 100 * gv, (C, dm, dv)


#: 2^-53 cond moves cov^(-1/2) by a tenth of the 1e-8 solve gate at cond = 9e6 (tests/test_sweep_gpu.py SOLVE_MAX_COND): far inside the 1e-6
#: of the projection, so a map below it is held to the ordinary gate and one above it would be replaced here
WHITEN_MAX_COND = 1e-9 / 2.0 ** -53


@pytest.mark.parametrize("C", AC.WHITEN_WIDTHS)
def test_e7_the_whitened_maps_are_well_conditioned(C):
    f = AC.whiten_map(C)
    n = f.shape[0] * f.shape[1]
    assert n == 2 * C + 3 and n % AC.WHITEN_PIX != 0
    lam = np.linalg.eigvalsh(np.cov(np.asarray(f, np.float64).reshape(n, C).T))
    print("E7 C=%d: %d positions, cond(cov) = %.3e" % (C, n, lam[-1] / lam[0]))
    assert lam[0] > 0 and lam[-1] / lam[0] <= WHITEN_MAX_COND
    u64, _ = A.project(f, A.WHITENED)
    assert np.isfinite(u64).all() and np.abs((u64 ** 2).sum(-1) - 1).max() < 1e-9


# ---------------------------------------------------------------------------------------------------------------- command line
def parse(*argv):
    args = cli.build_parser().parse_args(["--mode", "16x"] + list(argv))
    args.outf, args.log_mark = "out", "M"
    return args


def test_parser_accepts_the_attention_matches_and_the_temperature():
    a = parse()
    assert a.swap_temp is None
    cli.check_swap_args(a)
    for match in cli.ATTN_MATCH_NAMES:
        a = parse("--swap_level", "3", "--swap_match", match)
        cli.check_swap_args(a)
        assert (a.swap_level, a.swap_match, a.swap_temp) == (3, match, lib.ATTN_TEMP) and lib.ATTN_TEMP == 8
        a = parse("--swap_level", "4", "--swap_match", match, "--swap_temp", "0")
        cli.check_swap_args(a)
        assert a.swap_temp == 0.0
        a = parse("--swap_level", "4", "--swap_match", match, "--swap_temp", "32", "--transform", "adain", "--preserve_color", "luma")
        cli.check_swap_args(a)
        assert a.swap_temp == 32.0
    for bad in ("-1", "32.5", "nan", "inf"):
        with pytest.raises(ValueError, match="--swap_temp"):
            cli.check_swap_args(parse("--swap_level", "3", "--swap_match", "attention", "--swap_temp", bad))
    for argv in (["--swap_temp", "4"], ["--swap_level", "3", "--swap_temp", "4"], ["--swap_level", "3", "--swap_match", "raw", "--swap_temp", "4"]):
        with pytest.raises(ValueError, match="--swap_temp needs"):
            cli.check_swap_args(parse(*argv))
    with pytest.raises(ValueError, match="--swap_match does nothing without --swap_level"):
        cli.check_swap_args(parse("--swap_match", "attention"))
    with pytest.raises(ValueError, match="--swap_level does not mix with --numpy"):
        cli.check_swap_args(parse("--swap_level", "3", "--swap_match", "attention", "--numpy"))


def test_attention_is_not_a_mode_of_its_own_and_the_names_carry_the_match():
    assert [m.name for m in cli.MODES].count("swap") == 1 and not [m.name for m in cli.MODES if "attn" in m.name or "attention" in m.name]
    a = parse("--swap_level", "3", "--swap_match", "attention")
    cli.check_swap_args(a)
    assert cli.out_name(a, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_swap=3_attention=8_a+b.jpg")
    a = parse("--swap_level", "4", "--swap_match", "attention_whitened", "--swap_temp", "2.5", "--transform", "ot")
    cli.check_swap_args(a)
    assert cli.out_name(a, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_transform=ot_swap=4_attention_whitened=2.5_a+b.jpg")
    plain = parse("--swap_level", "4")
    cli.check_swap_args(plain)
    assert cli.out_name(plain, "a+b.jpg") == os.path.join("out", "M_mode=16x_alpha=1_swap=4_a+b.jpg")        # as before


class _FakeEngine:
    def __init__(self):
        self.calls = []

    def stylize_attn(self, c, s, level, match, tau, alpha, num_run):
        self.calls.append(("attn", c, s, level, match, tau, alpha, num_run))
        return "attn result"

    def stylize_swap(self, c, s, level, match, alpha, num_run):
        self.calls.append(("swap", c, s, level, match, alpha, num_run))
        return "swap result"

    def saturation_count(self, reset=False):
        return 0

    def set_conv_mode(self, mode):
        raise AssertionError("no recompute without a clamp")

    def sync(self):
        pass


def test_swap_pair_routes_an_attention_match_to_stylize_attn():
    eng, log = _FakeEngine(), []
    a = parse("--swap_level", "3", "--swap_match", "attention_whitened", "--swap_temp", "6", "--alpha", "0.5", "--num_run", "2")
    cli.check_swap_args(a)
    assert cli._swap_pair(eng, a, log.append, "content", lambda: "style") == "attn result"
    b = parse("--swap_level", "3", "--swap_match", "raw", "--alpha", "0.5")
    cli.check_swap_args(b)
    assert cli._swap_pair(eng, b, log.append, "content", lambda: "style") == "swap result"
    assert eng.calls == [("attn", "content", "style", 3, "attention_whitened", 6.0, 0.5, 2), ("swap", "content", "style", 3, "raw", 0.5, 1)] and not log
