"""The column-sharded cascade off the shipped models, on the MI355X: custom widths (tests/width_models.py A, B, C; tests/shard_cases.py D), all three transforms,
against fp64 and bit for bit against its other statements.  Every rank is a thread of this process (tools/sharded_standins.py).

  a  one sharded level (wct_level_sharded over the in-process transport) per rank window against the fp64 arm of tests/shard_cases.py:
     per-rank raw moments of the owned window at wm.MOM_GATE, the joined owned columns at e_gpu <= 4 e32 + 1e-4
  b  a strip fed own +- LEVEL_HALO[L] reproduces the untiled level bit for bit on its owned columns, at these widths
  c  the library's cascade (wct_stylize_sharded) == the Python orchestration bit for bit, == itself with a synchronisation around every
     collective, within the sharded tests' tolerance of the untiled frame
  d  WCT_SHARD_FAST_FOLD in jobs whose levels mix the fast and the map-based fold
  e  one context through jobs of two geometries: the per-level packed buffers follow the job

What each level ran is read back from the profile names."""
import numpy as np
import pytest

from tests import shard_cases as SC
from tests import width_models as wm
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

LEVELS = SC.LEVELS
ALPHA = SC.ALPHA
UNTILED_GATE = {"A": 5e-4, "B": 5e-4, "C": 2e-3, "D": 5e-4}      # tests/test_sharded_gpu.py: the sharded tests' 5e-4, the wide-model gate of test_c_cascade_mode_original


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def refs():
    """The fp64 / fp32 arms, computed once per (model, transform) and never written to."""
    return SC.reference


def engine(model, mode="wct", profile=False):
    from tests.shard_engine import WidthWCT
    e = WidthWCT(SC.widths_of(model), SC.weights(model), transform=mode)
    if profile:
        e.profile(True)
        e.profile_reset()
    return e


def images(torch, model, passes=2):
    c, s = SC.case_images(model, passes)
    return torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda()


def l1_path(names):
    """"fused" | "layerwise" | "mixed": which level-1 kernels a profile shows."""
    fused = any(n.startswith("l1_moments_fused") or n.startswith("l1_decode_fused") for n in names)
    layerwise = "moments" in names
    return "mixed" if fused and layerwise else "fused" if fused else "layerwise" if layerwise else "none"


L1_PATH = {"A": "layerwise", "B": "fused", "C": "layerwise", "D": "layerwise"}          # level-1 widths 28, 20, 48, 28: the fused kernels cover 17..24


# ---------------------------------------------------------------------------------------------------- a. one sharded level against fp64
@pytest.mark.parametrize("world", SC.WORLDS)
@pytest.mark.parametrize("mode", SC.TRANSFORMS)
@pytest.mark.parametrize("model", sorted(SC.CASES))
def test_sharded_level_against_fp64(torch, refs, model, mode, world):
    """Levels 5..1, level-isolated (the fp64 arm's previous output, rounded to fp32, is every rank's input).  Per rank:
    content_encode(L, strip, f0, f1) against the fp64 raw moments of the same window; then level_sharded(L, strip own +- LEVEL_HALO[L], f0, f1,
    n_total, alpha) with the all-reduce between the rank threads.  The joined owned columns against the fp64 arm.

    Measured on the MI355X, e_gpu / e32 in units of 1e-6, levels 5 4 3 2 1 (three ranks; two ranks give the same figures, the strips
    being bit-exact -- section b):
        A wct    2.22/2.65  5.05/4.85  1.03/0.78  1.21/0.83  0.73/0.45      B wct    4.79/5.11  10.5/13.2  4.91/10.7  1.61/1.49  0.23/0.34
        A ot     2.68/2.16  6.50/4.35  0.99/0.94  1.72/1.06  0.80/0.70      B ot     5.51/5.21  9.67/16.9  7.53/5.60  1.72/0.92  0.27/0.40
        A adain  2.33/2.23  4.45/4.49  0.79/0.82  1.15/1.13  1.29/0.60      B adain  4.75/4.86  5.16/6.30  3.29/7.44  0.79/0.97  0.33/0.64
    Rank-summed moments: at most 4.8e-7 against the 1e-6 gate."""
    from tests.shard_engine import profile_counts, run_rank_threads
    ref = refs(model, mode)
    c = SC.CASES[model]
    wins = SC.content_windows(c["W"], world, "exchange")          # exchange mode: every level gets exactly its own margin
    style = torch.from_numpy(SC.case_images(model)[1]).cuda()
    inputs = {L: torch.from_numpy(ref.inputs[L]).cuda() for L in LEVELS}

    def rank_job(r, group):
        e = engine(model, mode)
        e.comm_attach_collectives(*group.c_transport(), world, r)
        e.style_prepare(style)
        got = {}
        for L in LEVELS:
            p, sh = wins[L][r], L - 1
            img = inputs[L]
            assert int(img.shape[2]) == p.Wc
            strip = img[:, :, p.lo:p.hi].contiguous()
            if L == 1:
                e.profile(True)
                e.profile_reset()
            h, w, s, ss = e.content_encode(L, strip, p.f0, p.f1)
            n_total = float((int(img.shape[1]) >> sh) * p.wf)
            out = e.level_sharded(L, strip, p.f0, p.f1, n_total, ALPHA)
            own1 = min(p.own[1], (p.Wc >> sh) << sh)
            got[L] = (h, w, s.cpu().numpy(), ss.cpu().numpy(), out[0, :, :, p.own[0] - p.lo:own1 - p.lo].cpu().numpy())
        e.sync()
        names = set(profile_counts(e))
        return got, names, e.saturation_count()

    outs, groups = run_rank_threads(world, rank_job)
    for L in LEVELS:
        r64, sh = ref.r64[L], L - 1
        whole_s, whole_ss = wm.raw_moments(r64.cF)
        acc_s, acc_ss = 0, 0
        for r in range(world):
            p = wins[L][r]
            h, w, s, ss, _ = outs[r][0][L]
            assert (h, w) == (r64.cF.shape[1], (p.hi - p.lo) >> sh), (L, r)
            rs, rss = wm.raw_moments(r64.cF, p.g0, p.g0 + p.n)
            es, ess = rel_err(s, rs), rel_err(ss, rss)
            assert es < wm.MOM_GATE and ess < wm.MOM_GATE, "%s %s world %d level %d rank %d window [%d, %d): sum %.3e sumsq %.3e" % (model, mode, world, L, r, p.g0, p.g0 + p.n, es, ess)
            acc_s, acc_ss = acc_s + s, acc_ss + ss
        es, ess = rel_err(acc_s, whole_s), rel_err(acc_ss, whole_ss)
        assert es < wm.MOM_GATE and ess < wm.MOM_GATE, (model, mode, world, L, es, ess)
        joined = np.concatenate([outs[r][0][L][4] for r in range(world)], axis=2)
        assert joined.shape == r64.out.shape, (L, joined.shape, r64.out.shape)
        e_gpu, e32 = rel_err(joined, r64.out), ref.e32[L]
        print("shard level %s %s world %d level %d (C = %d): gpu %.2e fp32 arm %.2e (vs fp64); rank-sum moments %.1e / %.1e"
              % (model, mode, world, L, r64.cF.shape[0], e_gpu, e32, es, ess))
        assert e_gpu <= 4 * e32 + 1e-4, (model, mode, world, L, e_gpu, e32)
    for r in range(world):
        assert l1_path(outs[r][1]) == L1_PATH[model], (model, r, sorted(outs[r][1]))
        assert outs[r][2] == 0
    assert all(g.calls == {"all_reduce": 5, "broadcast": 0, "p2p": 0} for g in groups)


# ---------------------------------------------------------------------------------------------------- b. strip exactness at custom widths
@pytest.mark.parametrize("model", ["A", "B", "C"])
def test_strip_halos_exact_at_custom_widths(torch, model):
    """tests/test_sharded_gpu.py test_strip_halos_exact_with_level_margins with these models at W = 541 in three strips (an edge strip, an
    interior one that is cropped on both sides, a last one that floor pooling shrinks): with the same (M, b) a strip fed own +-
    LEVEL_HALO[L] columns equals the untiled level on its owned columns bit for bit."""
    from tests.shard_engine import profile_counts
    from wct_hip.sharded import LEVEL_HALO, ext_bounds, strip_bounds
    wct = engine(model)
    wct.debug_set("prof_forms", 1)
    content, style = images(torch, model)
    content = content[None]
    W, world = int(content.shape[-1]), 3
    bad = []
    for L in LEVELS:
        sh = L - 1
        sF = wct.encode(L, style, layout="nhwc")
        wct.profile(True)
        wct.profile_reset()
        cF = wct.encode(L, content, layout="nhwc")
        nc, sc_, ssc = wct.moments(cF)
        M, b = wct.solve(nc, sc_, ssc, *wct.moments(sF))
        full = wct.decode_affine(L, cF, M, b)
        wct.sync()
        forms_full = set(profile_counts(wct))
        Wn = (W >> sh) << sh
        for own in strip_bounds(W, world):
            lo, hi = ext_bounds(own, W, LEVEL_HALO[L])
            wct.profile_reset()
            f = wct.encode(L, content[..., lo:hi].contiguous(), layout="nhwc")
            o = wct.decode_affine(L, f, M, b)
            wct.sync()
            a, e = own[0], min(Wn, own[1])
            if not torch.equal(o[..., a - lo:e - lo], full[..., a:e]):
                forms = set(profile_counts(wct))
                bad.append((L, own, float((o[..., a - lo:e - lo] - full[..., a:e]).abs().max()), sorted(forms ^ forms_full)))
    assert not bad, "%s: strips differ from the untiled level (level, own, max |diff|, kernel forms that differ): %s" % (model, bad)
    assert wct.saturation_count() == 0


# ---------------------------------------------------------------------------------------------------- c. the library's cascade
WCT_JOBS = [(3, "exchange", "strips", False), (3, "exchange", "owner", True), (3, "recompute", "replicate", False), (2, "recompute", "strips", False)]
OTHER_JOBS = [(3, "exchange", "owner", True), (3, "exchange", "strips", False), (2, "recompute", "owner", False)]
# model D (level 4 wider than level 5) in the arrangement whose per-level packed buffers are live at the same time: the style strips'
D_JOBS = [(3, "exchange", "strips", False), (2, "recompute", "strips", False)]
CASCADE_CASES = [(m, "wct") + j for m in ("A", "B", "C") for j in WCT_JOBS] + [(m, t) + j for m in ("A", "B") for t in ("ot", "adain") for j in OTHER_JOBS] \
    + [("D", "wct") + j for j in D_JOBS]


def expected_calls(world, halo_mode, smode, bmap):
    """Collectives per rank and frame (tests/test_sharded_gpu.py test_device_buffer_collectives_are_checked)."""
    if smode == "owner":
        bc = (5 + sum(1 for L in LEVELS if (5 - L) % world != 0)) if bmap else 5
    else:
        bc = 5 if bmap else 0
    return {"all_reduce": 5, "broadcast": bc, "p2p": 4 if halo_mode == "exchange" else 0}


@pytest.mark.parametrize("model,mode,world,halo_mode,smode,bmap", CASCADE_CASES)
def test_c_cascade_at_custom_widths(torch, model, mode, world, halo_mode, smode, bmap):
    from tests.shard_engine import profile_counts
    from tools import sharded_standins as standins
    content, style = images(torch, model)
    H, W = int(content.shape[1]), int(content.shape[2])
    made = []

    def make(profile=False):
        made.append(engine(model, mode, profile))
        return made[-1]
    kw = dict(halo_mode=halo_mode, broadcast_map=bmap, style_mode=smode, alpha=ALPHA)
    want, groups_py = standins.run_in_process(world, make, content, style, **kw)
    got, groups_c = standins.run_in_process(world, make, content, style, c_cascade=True, **kw)
    assert tuple(got.shape) == tuple(want.shape) == (1, 3, H // 16 * 16, W // 16 * 16)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert [g.calls for g in groups_c] == [g.calls for g in groups_py] == [expected_calls(world, halo_mode, smode, bmap)] * world
    del made[:]
    synced, _ = standins.run_in_process(world, lambda: make(True), content, style, c_cascade=True, sync_every=True, **kw)
    assert torch.equal(got, synced)
    for e in made:
        names = set(profile_counts(e))
        # (the whole frame's names: "moments" is levels 5..2's as well, so only the fused kernels tell level 1's path here)
        assert any(n.startswith("l1_") and "fused" in n for n in names) == (L1_PATH[model] == "fused"), (model, sorted(names))
        assert e.saturation_count() == 0
        if e is made[0]:          # rank 0 solves in every arrangement (with a broadcast map it alone)
            assert ("ot_assemble" in names) == (mode == "ot") and ("adain_assemble" in names) == (mode == "adain"), sorted(names)
    ref = engine(model, mode).stylize(content, style, alpha=ALPHA)
    err = rel_err(got.cpu().numpy(), ref.cpu().numpy())
    print("shard cascade %s %s world %d %s %s bmap %d: vs untiled %.2e" % (model, mode, world, halo_mode, smode, bmap, err))
    assert tuple(got.shape) == tuple(ref.shape) and err < UNTILED_GATE[model], err


# ---------------------------------------------------------------------------------------------------- d. mixed folds
@pytest.mark.parametrize("model,world,halo_mode,smode", [("A", 3, "exchange", "owner"), ("B", 2, "recompute", "strips")])
def test_fast_fold_in_jobs_that_mix_fold_forms(torch, model, world, halo_mode, smode):
    """WCT_SHARD_FAST_FOLD where only some levels can take it (A: levels 2 and 1, B: levels 3 and 1): reproducible bit for bit, within the 1e-4 of
    test_c_cascade_fast_fold of the default form, and both arms ran in the one job -- assemble_Mb (the map-based arm's (M, b)) once per
    level that cannot fold fast, the decoder's first conv folded at all five.  Under ot the flag changes nothing."""
    from tests.shard_engine import profile_counts
    from tools import sharded_standins as standins
    content, style = images(torch, model)
    fast_levels = SC.fast_fold_levels(wm.MODELS[model])
    assert 0 < len(fast_levels) < 5
    made = []

    def make(mode="wct"):
        made.append(engine(model, mode, profile=True))
        return made[-1]
    kw = dict(halo_mode=halo_mode, style_mode=smode, alpha=ALPHA, c_cascade=True)
    base, _ = standins.run_in_process(world, make, content, style, **kw)
    for e in made:
        counts = profile_counts(e)
        assert counts.get("assemble_Mb") == 5 and counts.get("fold_affine") == 5, counts
    del made[:]
    fast, _ = standins.run_in_process(world, make, content, style, fast_fold=True, **kw)
    for e in made:
        counts = profile_counts(e)
        assert counts.get("assemble_Mb") == 5 - len(fast_levels) and counts.get("fold_affine") == 5, (model, counts)
    again, _ = standins.run_in_process(world, make, content, style, fast_fold=True, **kw)
    assert torch.equal(fast, again)
    err = rel_err(fast.cpu().numpy(), base.cpu().numpy())
    print("shard fast fold %s world %d: fast vs (M, b) form %.2e" % (model, world, err))
    assert err < 1e-4
    assert all(e.saturation_count() == 0 for e in made)
    ot_base, _ = standins.run_in_process(world, lambda: make("ot"), content, style, **kw)
    ot_fast, _ = standins.run_in_process(world, lambda: make("ot"), content, style, fast_fold=True, **kw)
    assert torch.equal(ot_fast, ot_base) and not torch.equal(ot_base, base)


# ---------------------------------------------------------------------------------------------------- e. sized-per-level buffers
def test_one_context_through_two_geometries(torch):
    """The packed all-reduce buffers, the (M, b) broadcast buffer and the statistics buffer are sized and laid out per job from each
    level's C; the strip buffers from the job's geometry.  Three contexts (the ranks) run a three-rank job, a two-rank job of another
    size and arrangement, and both again: every frame equals the one of fresh contexts bit for bit (tests/state_cases.py's claim)."""
    from tools import sharded_standins as standins
    model = "A"
    content, style = images(torch, model)
    jobs = [dict(world=3, c=content, s=style, kw=dict(halo_mode="exchange", style_mode="strips")),
            dict(world=2, c=content[:, :88, :389].contiguous(), s=style[:, :150, :200].contiguous(),
                 kw=dict(halo_mode="recompute", style_mode="owner", broadcast_map=True))]
    fresh = [standins.run_in_process(j["world"], lambda: engine(model), j["c"], j["s"], c_cascade=True, alpha=ALPHA, **j["kw"])[0] for j in jobs]
    assert fresh[0].shape != fresh[1].shape
    pool = [engine(model) for _ in range(3)]
    for k in (0, 1, 0, 1):
        j = jobs[k]
        for e in pool:
            if e.has_comm:
                e.comm_destroy()
        it = iter(pool)
        got, _ = standins.run_in_process(j["world"], lambda: next(it), j["c"], j["s"], c_cascade=True, alpha=ALPHA, **j["kw"])
        assert torch.equal(got, fresh[k]), "job %d on used contexts differs from fresh ones: %.3e" % (k, float((got - fresh[k]).abs().max()))
    assert all(e.saturation_count() == 0 for e in pool)
