"""Seeded style variations on the device (include/wct_hip_diverse.h) against the numpy fp64 restatement (tests/diverse_oracle.py): the
rotation, the rotated slot, the map made from it, the cascade under both fold arms, the refusals and video mode.

Gates, taken from the project: GATE_WELL = 1e-8, the solver's gate for well-conditioned matrices (tests/test_transform_gpu.py,
tests/test_hip_parity.py); the cascade gate e_gpu <= 4 e32 + 1e-4 against the fp64 arm (tests/test_widths_gpu.py); and the forward bound
of a length-C fp64 dot product, C 2^-53 |S| |Z| per side, for the slot's GEMM against numpy's.  Every measured distance is printed."""
import numpy as np
import pytest

from tests import diverse_oracle as D
from tests import state_cases as sc
from tests import transform_oracle as O
from tests.conftest import rel_err
from tests.transform_cases import make_case
from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

GATE_WELL = 1e-8
WIDTHS = (2, 6, 24, 64, 128, 144, 512)          # one tile with a k-tail; the LDS front ends; the single-workgroup limit; the deflated iteration
STRENGTHS = (0.25, 1.0, 8.0)
SEED, STREAM, TAG = (5 << 32) | 77, 3, 5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    return sc.make_engine("16x")


@pytest.fixture(scope="module")
def other(torch):
    """A second context with a past of its own."""
    e = sc.make_engine("16x")
    e.stylize(sc.image(7, 72, 88), sc.image(8, 66, 70))
    return e


def t64(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float64)).cuda()


def npy(x):
    return x.detach().cpu().numpy()


def slots(e, levels=(5, 4, 3, 2, 1)):
    return {L: npy(e.style_export(L)) for L in levels}


def same_slots(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[L], b[L]) for L in a)


# ------------------------------------------------------------------------------------------------ 1. wct_rotation_make
@pytest.mark.parametrize("C", WIDTHS)
def test_rotation_against_the_oracle(torch, eng, other, C):
    for strength in STRENGTHS:
        Z, A = eng.rotation(C, strength, SEED, STREAM, TAG, want_skew=True)
        Z, A = npy(Z), npy(A)
        assert np.array_equal(A, D.skew(C, SEED, STREAM, TAG, strength)), (C, strength)
        e_z = rel_err(Z, D.rotation(C, SEED, STREAM, TAG, strength))
        e_o = float(np.abs(Z.T @ Z - np.eye(C)).max())
        print("rotation C=%d strength %g: Z vs oracle %.2e, |Z^T Z - I| %.2e (gate %.0e)" % (C, strength, e_z, e_o, GATE_WELL))
        assert e_z < GATE_WELL and e_o < GATE_WELL, (C, strength, e_z, e_o)
        again = npy(eng.rotation(C, strength, SEED, STREAM, TAG))
        elsewhere = npy(other.rotation(C, strength, SEED, STREAM, TAG))
        assert np.array_equal(again, Z) and np.array_equal(elsewhere, Z), (C, strength)
    Z, A = eng.rotation(C, 0.0, SEED, STREAM, TAG, want_skew=True)
    assert np.array_equal(npy(Z), np.eye(C)) and not npy(A).any()
    if C >= 6:
        assert (npy(eng.rotation(C, 1.0, SEED, STREAM + 1, TAG)) != npy(eng.rotation(C, 1.0, SEED, STREAM, TAG))).mean() > 0.5


def test_rotation_refusals_leave_the_buffers_untouched(torch, eng):
    L, ctx = eng._lib, eng._ctx
    Z = torch.full((514 * 514,), 7.25, dtype=torch.float64, device="cuda")
    A = torch.full((514 * 514,), 7.25, dtype=torch.float64, device="cuda")
    eng._stream()
    call = lambda C, tag, strength, z=Z, a=A: L.wct_rotation_make(ctx, C, SEED, STREAM, tag, strength, z.data_ptr() if z is not None else None,
                                                                   a.data_ptr() if a is not None else None)
    for C in (0, 1, 31, 514, -2):
        assert call(C, TAG, 1.0) == _lib.WCT_ERR_INVALID, C
    assert call(32, 256, 1.0) == _lib.WCT_ERR_INVALID
    for strength in (-1.0, -1e-300, float("nan"), 8.5, float("inf")):
        assert call(32, TAG, strength) == _lib.WCT_ERR_INVALID and b"strength" in L.wct_last_error(ctx), strength
    assert call(32, TAG, 1.0, None) == _lib.WCT_ERR_INVALID
    assert call(32, TAG, 1.0, Z, Z[512:]) == _lib.WCT_ERR_INVALID and b"overlaps" in L.wct_last_error(ctx)
    torch.cuda.synchronize()
    assert bool((Z == 7.25).all()) and bool((A == 7.25).all())
    assert call(32, TAG, 8.0) == _lib.WCT_OK and call(32, 255, 0.0, Z, None) == _lib.WCT_OK
    torch.cuda.synchronize()
    assert bool((Z[32 * 32:] == 7.25).all()) and bool((A[32 * 32:] == 7.25).all()) and bool(torch.isfinite(A[:32 * 32]).all())
    for bad in (dict(strength=9), dict(strength=-0.5), dict(tag=256), dict(C=7), dict(seed=1 << 64), dict(stream_id=1 << 32)):
        with pytest.raises(ValueError):
            eng.rotation(**dict(dict(C=8, strength=1.0), **bad))


# ------------------------------------------------------------------------------------------------ 2. the slot
def test_the_slot_is_post_multiplied_and_the_mark_follows_it(torch, golden):
    g = golden("g4_cascade.npz")
    e = sc.make_engine("16x")
    style = t64(torch, g["a.style"]).float()[None]
    e.style_prepare(style)
    before = slots(e)
    e.style_diversify(1.0, SEED, STREAM, levels=(5, 2))
    after = slots(e)
    u = 2.0 ** -53

    def check(was, now, L, seed, what):
        C = sc.channels(e, L)
        S0, mu0 = O.split_stats(was)
        S1, mu1 = O.split_stats(now)
        Z = npy(e.rotation(C, 1.0, seed, STREAM, L))
        assert np.array_equal(mu1, mu0), (what, L)
        slack = 2 * C * u * (np.abs(S0) @ np.abs(Z))
        d = np.abs(S1 - S0 @ Z)
        e_cov = rel_err(S1 @ S1.T, S0 @ S0.T)
        print("slot %s level %d: max |S' - S Z| %.2e (largest bound %.2e), S'S'^T vs SS^T %.2e, |S' - S| / |S| %.2f"
              % (what, L, d.max(), slack.max(), e_cov, np.abs(S1 - S0).max() / np.abs(S0).max()))
        assert (d <= slack).all(), (what, L, float((d - slack).max()))
        assert e_cov < GATE_WELL, (what, L, e_cov)
        assert np.abs(S1 - S0).max() > 0.05 * np.abs(S0).max(), (what, L)            # it did move

    for L in (4, 3, 1):
        assert np.array_equal(after[L], before[L]), L
    for L in (5, 2):
        check(before[L], after[L], L, SEED, "first")
    # composition: a second call rotates what the first one left
    e.style_diversify(1.0, SEED + 1, STREAM, levels=(5, 2))
    twice = slots(e)
    for L in (5, 2):
        check(after[L], twice[L], L, SEED + 1, "second")
        assert not np.array_equal(twice[L], after[L])
    # strength 0: bit-identical
    e.style_diversify(0.0, SEED, STREAM, levels=(5, 4, 3, 2, 1))
    assert same_slots(slots(e), twice)
    # the mark: ot / adain are refused while a slot is rotated, whatever rewrites the slot clears it
    for mode in ("ot", "adain"):
        with pytest.raises(_lib.WctError) as err:
            e.set_transform(mode)
        assert err.value.code == _lib.WCT_ERR_STATE and "rotated" in str(err.value)
    assert e.transform_mode == "wct"
    e.style_prepare(style, levels=(5,))
    with pytest.raises(_lib.WctError):
        e.set_transform("ot")                       # level 2 is still rotated
    e.style_import(2, t64(torch, before[2]))
    e.set_transform("ot")
    assert e.transform_mode == "ot"
    e.set_transform("wct")
    assert np.array_equal(npy(e.style_export(5)), before[5]) and np.array_equal(npy(e.style_export(2)), before[2])
    e.style_diversify(0.0, SEED, STREAM, levels=(5,))          # Z = I sets no mark
    e.set_transform("adain")
    e.set_transform("wct")
    assert e.saturation_count() == 0


# ------------------------------------------------------------------------------------------------ 3. the map
@pytest.mark.parametrize("C", (32, 64, 128, 256))
def test_the_map_of_a_rotated_slot_against_the_oracle(torch, eng, C):
    """Rotated statistics into wct_transform_solve("wct"): assemble_row_kernel reads S as it is (rows times cov_c^(-1/2)), nothing is
    transposed or symmetrised.  cond(cov_c) = 1e2: the solver's gate for well-conditioned matrices."""
    n, s, ss, st = make_case(4000 + C, C, 1e-2, 1e-2)
    Z = npy(eng.rotation(C, 1.0, SEED, STREAM, TAG))
    rot = D.rotate_stats(st, Z)
    mu_c, cov_c = O.mean_cov(n, s, ss)
    Sm, _ = O.split_stats(st)
    R = O.sym_pow(cov_c, 0.5)
    for alpha in (1.0, 0.6):
        M, b = eng.transform_solve("wct", n, t64(torch, s), t64(torch, ss), t64(torch, rot), alpha=alpha)
        M, b = npy(M), npy(b)
        Mr, br = D.solve(n, s, ss, st, Z, alpha)
        e_map, e_mean = rel_err(M @ R, Mr @ R), rel_err(M @ mu_c + b, Mr @ mu_c + br)
        M0, _ = O.solve("wct", n, s, ss, st, alpha)
        moved = rel_err(M @ R, M0 @ R)
        print("map C=%d alpha %.1f: M R %.2e, M mu + b %.2e (gate %.0e); distance from the unrotated map %.2f" % (C, alpha, e_map, e_mean, GATE_WELL, moved))
        assert e_map < GATE_WELL and e_mean < GATE_WELL, (C, alpha, e_map, e_mean)
        assert moved > 0.1
        if alpha == 1.0:                             # the feature's claim: the same target covariance through a different map
            e_cov = rel_err((M @ R) @ (M @ R).T, Sm @ Sm.T)
            print("map C=%d: (M R)(M R)^T vs cov_s %.2e" % (C, e_cov))
            assert e_cov < GATE_WELL, (C, e_cov)


# ------------------------------------------------------------------------------------------------ 4. the cascade
def test_stylize_diverse_is_the_three_public_calls(torch, eng, other):
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(31, H, W), sc.image(32, Hs, Ws)
    got = eng.stylize_diverse(c, s, 1.0, SEED, STREAM, levels=(5, 3, 1), alpha=0.8, num_run=2).clone()
    other.style_prepare(s)
    other.style_diversify(1.0, SEED, STREAM, levels=(5, 3, 1))
    want = other.stylize_prepared(c, alpha=0.8, num_run=2).clone()
    assert torch.equal(got, want)
    assert torch.equal(eng.stylize_diverse(c, s, 1.0, SEED, STREAM, levels=(5, 3, 1), alpha=0.8, num_run=2), got)       # the same arguments, the same bits
    plain = eng.stylize(c, s, alpha=0.8, num_run=2).clone()
    sid = eng.stylize_diverse(c, s, 1.0, SEED, STREAM + 1, levels=(5, 3, 1), alpha=0.8, num_run=2).clone()
    seed = eng.stylize_diverse(c, s, 1.0, SEED + 1, STREAM, levels=(5, 3, 1), alpha=0.8, num_run=2).clone()
    zero = eng.stylize_diverse(c, s, 0.0, SEED, STREAM, levels=(5, 3, 1), alpha=0.8, num_run=2).clone()
    d = lambda a, b: float((a - b).abs().max())
    print("cascade: |diverse - plain| %.3f, |stream 3 - stream 4| %.3f, |seed - seed + 1| %.3f (images in [0, 1])" % (d(got, plain), d(got, sid), d(got, seed)))
    assert d(got, plain) > 1e-2 and d(got, sid) > 1e-2 and d(got, seed) > 1e-2
    eng.style_prepare(s)
    assert torch.equal(zero, eng.stylize_prepared(c, alpha=0.8, num_run=2))                   # strength 0: the undiversified cascade
    assert eng.saturation_count() == 0 and other.saturation_count() == 0


@pytest.mark.parametrize("alpha", (0.6, 1.0))
@pytest.mark.parametrize("fastfold", (1, 0), ids=("fast fold", "Mb fold"))
def test_level_isolated_cascade_against_the_fp64_arm(torch, oracle, weights16x, golden, fastfold, alpha):
    """One rotated level at a time, levels 5, 2 and 1 (the fused level-1 path), on the g4 pair.  The cascade against prepared statistics is
    the one entry that reads a rotated slot on the fast-fold path, and it runs all five levels; the level under test is isolated by
    giving every arm the SAME other levels: the input of level L is the engine's own chain of the levels above it (the cascade is that
    chain bit for bit, asserted here), level L itself is the oracle's T = S Z cov_c^(-1/2) in fp64 and in fp32, and the engine's levels
    below L finish both arms.  Gate: e_gpu <= 4 e32 + 1e-4 on the final image."""
    g = golden("g4_cascade.npz")
    c, s = g["b.content"], g["b.style"]
    arms = {p: oracle.Modules("16x", weights16x, precision=p) for p in ("fp64", "fp32")}
    e = sc.make_engine("16x")
    e.debug_set("fastfold", fastfold)
    S, C0 = t64(torch, s).float()[None], t64(torch, c).float()[None]

    def chain(img, levels):
        for L in levels:
            img = e.style_transfer_level(L, img, S, alpha)
        return img

    def level(mods, L, img, Z):
        f64 = mods.precision == "fp64"
        dt = np.float64 if f64 else np.float32
        cF, sF = mods.encode(L, np.asarray(img, dt)), mods.encode(L, np.asarray(s, dt))
        return mods.decode(L, D.transform_features(cF, sF, Z, alpha).astype(dt))          # fp64 statistics in both arms, like the reference

    e.style_prepare(S)
    plain = e.stylize_prepared(C0, alpha=alpha).clone()
    assert torch.equal(plain, chain(C0, (5, 4, 3, 2, 1)))
    for L in (5, 2, 1):
        e.profile_reset(); e.profile(True)
        e.style_prepare(S)
        e.style_diversify(1.0, SEED, STREAM, levels=(L,))
        got = e.stylize_prepared(C0, alpha=alpha).clone()
        e.profile(False)
        names = {r["name"] for r in e.profile_read()}                      # the arm is the one the case names
        assert ("assemble_Mb" in names) == (fastfold == 0) and ("fold_style" in names) == (fastfold == 1), names
        assert {"rotation_make", "rotation_apply"} <= names, names
        Z = npy(e.rotation(sc.channels(e, L), 1.0, SEED, STREAM, L))
        x = chain(C0, [k for k in (5, 4, 3, 2, 1) if k > L])
        below = [k for k in (5, 4, 3, 2, 1) if k < L]
        ref = {}
        for p in ("fp64", "fp32"):
            y = level(arms[p], L, npy(x)[0], Z).astype(np.float32)
            ref[p] = npy(chain(t64(torch, y).float()[None], below))[0]
        e_gpu, e32 = rel_err(npy(got)[0], ref["fp64"]), rel_err(ref["fp32"], ref["fp64"])
        moved = rel_err(npy(got)[0], npy(plain)[0])
        print("cascade fastfold %d alpha %.1f level %d: gpu %.2e fp32 arm %.2e (vs fp64), gate %.2e; distance from the undiversified result %.3f"
              % (fastfold, alpha, L, e_gpu, e32, 4 * e32 + 1e-4, moved))
        assert e_gpu <= 4 * e32 + 1e-4, (fastfold, alpha, L, e_gpu, e32)
        assert moved > 1e-2, (L, moved)
    assert e.saturation_count() == 0


# ------------------------------------------------------------------------------------------------ 5. refusals and state
def test_refusals_come_before_anything_is_written(torch):
    H, W, Hs, Ws = sc.SIZES["small"]
    c, s = sc.image(41, H, W), sc.image(42, Hs, Ws)
    e = sc.make_engine("16x")
    L, ctx = e._lib, e._ctx
    e.style_prepare(s, levels=(5, 4))
    want = slots(e, (5, 4))
    out = torch.full((3, H, W), 7.25, device="cuda")
    # a masked level without a prepared slot: nothing is written, level 5 (looked at first) included
    with pytest.raises(_lib.WctError) as err:
        e.style_diversify(1.0, SEED, STREAM, levels=(5, 3))
    assert err.value.code == _lib.WCT_ERR_STATE and "level 3" in str(err.value)
    assert same_slots(slots(e, (5, 4)), want)
    # an empty mask, a bit outside levels 1..5
    e._stream()
    for mask in (0, 1, 1 << 6, (1 << 5) | (1 << 7), 0x80000000):
        assert L.wct_style_diversify(ctx, mask, 1.0, SEED, STREAM) == _lib.WCT_ERR_INVALID and b"mask" in L.wct_last_error(ctx), mask
        assert L.wct_stylize_diverse(ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, mask, 1.0, SEED, STREAM, 1.0, 1, out.data_ptr(), None, None) == _lib.WCT_ERR_INVALID
    # a bad strength
    for strength in (-1.0, float("nan"), 8.5):
        assert L.wct_style_diversify(ctx, 1 << 5, strength, SEED, STREAM) == _lib.WCT_ERR_INVALID and b"strength" in L.wct_last_error(ctx), strength
        assert L.wct_stylize_diverse(ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, 1 << 5, strength, SEED, STREAM, 1.0, 1, out.data_ptr(), None,
                                     None) == _lib.WCT_ERR_INVALID
    assert L.wct_stylize_diverse(ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, 1 << 5, 1.0, SEED, STREAM, 1.0, 0, out.data_ptr(), None, None) == _lib.WCT_ERR_INVALID
    assert same_slots(slots(e, (5, 4)), want)
    for bad in (dict(levels=()), dict(levels=(0,)), dict(levels=(6,)), dict(strength=9.0), dict(strength=float("nan")), dict(seed=-1)):
        with pytest.raises(ValueError):
            e.style_diversify(**dict(dict(strength=1.0), **bad))
    # a non-wct mode
    for mode in ("ot", "adain"):
        e.set_transform(mode)
        with pytest.raises(ValueError, match="wct transform only"):
            e.style_diversify(1.0, SEED, STREAM, levels=(5,))
        with pytest.raises(ValueError, match="wct transform only"):
            e.stylize_diverse(c, s, 1.0, SEED, STREAM, out=out)
        assert same_slots(slots(e, (5, 4)), want)
    e.set_transform("wct")
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())
    # and the call still works afterwards; the workspace is allocated once per width
    e.style_diversify(1.0, SEED, STREAM, levels=(5, 4))
    assert not np.array_equal(npy(e.style_export(5)), want[5])
    allocs = e.debug_get("ws_allocs")
    e.style_prepare(s, levels=(5, 4))
    e.style_diversify(2.0, SEED + 1, STREAM, levels=(5, 4))
    e.rotation(128, 1.0)
    assert e.debug_get("ws_allocs") == allocs
    assert e.saturation_count() == 0


def test_reserve_and_the_workspace_plan_do_not_move(torch):
    H, W, Hs, Ws = sc.SIZES["small"]
    e, fresh = sc.make_engine("16x"), sc.make_engine("16x")
    plan = sc.workspace_bytes(fresh, H, W, Hs, Ws)
    e.style_prepare(sc.image(42, Hs, Ws))
    e.style_diversify(1.0, SEED, STREAM, levels=(5, 4, 3, 2, 1))
    assert sc.workspace_bytes(e, H, W, Hs, Ws) == plan


def test_cli_writes_one_file_per_variation(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    import os
    from wct_hip import cli
    rng = np.random.default_rng(1)
    c, s = tmp_path / "content", tmp_path / "style"
    c.mkdir(); s.mkdir()
    Image.fromarray(rng.integers(0, 256, size=(64, 80, 3), dtype=np.uint8)).save(c / "c1.png")
    Image.fromarray(rng.integers(0, 256, size=(56, 40, 3), dtype=np.uint8)).save(s / "st.png")
    base = ["--mode", "16x", "--contentPath", str(c), "--stylePath", str(s), "--log_mark", "T", "--alpha", "0.6"]
    data = {}
    for tag, extra in (("plain", ["--pipeline", "0"]), ("div", ["--diversity", "1", "--variations", "2", "--seed", "4", "--diversity_levels", "5,4"]),
                       ("again", ["--diversity", "1", "--variations", "2", "--seed", "4", "--diversity_levels", "5,4", "--pipeline", "0"]),
                       ("one", ["--diversity", "1", "--seed", "4", "--diversity_levels", "5,4"])):
        o = tmp_path / tag
        assert cli.main(base + ["--outf", str(o)] + extra) == 0
        data[tag] = {f: (o / f).read_bytes() for f in sorted(os.listdir(o)) if f.endswith(".jpg")}
    assert list(data["plain"]) == ["T_mode=16x_alpha=0.6_c1+st.jpg"]
    assert list(data["div"]) == ["T_mode=16x_alpha=0.6_div=1_v0_c1+st.jpg", "T_mode=16x_alpha=0.6_div=1_v1_c1+st.jpg"]
    v0, v1 = data["div"].values()
    assert v0 != v1 and v0 != data["plain"]["T_mode=16x_alpha=0.6_c1+st.jpg"]
    assert data["again"] == data["div"]                                                        # the seed decides, not the run
    assert data["one"] == {"T_mode=16x_alpha=0.6_div=1_c1+st.jpg": v0}                       # variation 0 is stream id 0


# ------------------------------------------------------------------------------------------------ 6. video
def test_a_clip_reads_the_diversified_style(torch):
    H, W = 48, 64
    e = sc.make_engine("16x")
    e.style_prepare(sc.image(52, 80, 96))
    frames = [sc.image(53, H, W), sc.image(54, H, W)]
    plain = e.stylize_prepared(frames[0], alpha=0.6).clone()
    e.style_diversify(1.0, SEED, STREAM, levels=(5, 4))
    for x in frames:
        want = e.stylize_prepared(x, alpha=0.6).clone()
        clip = e.clip(H, W, rate=0.25, cut=0.5, blend=0.6)
        try:
            assert torch.equal(clip.stylize(x, alpha=0.6), want)
        finally:
            clip.close()
    assert not torch.equal(e.stylize_prepared(frames[0], alpha=0.6), plain)
    assert e.saturation_count() == 0
