"""The size-selected convolution kernel forms on the MI355X, at the sizes of tests/geometry_cases.py: large enough to cross every
launcher's threshold, with ragged right / bottom tiles, odd sizes under the floor pooling and tile counts that divide unevenly over
the eight XCDs.

a. every case against the fp64 restatement (tests/width_models.py) at the gate of the width tests, in both conv modes, with the
   launcher's choice read back from the profile names (wct_debug_set("prof_forms", 1)) and held against the Python restatement of the
   launchers -- so a case that no longer reaches its form fails instead of passing on another kernel;
b. what the sources call "the same arithmetic per pixel" / "bit-identical", bit for bit: each forced form (WCT_TAIL_TH, WCT_L1DEC_TH,
   WCT_HEAD_TH / WCT_HEAD_ROLES, WCT_F16_SMALL, WCT_SP3; honoured under WCT_DEBUG only, read once per process) in a child process of its
   own, sha256 of the outputs compared across the arms;
c. every form of geometry_cases.FORMS is reached by the default switches.

Failures of (a) are reported through geometry_cases.locate: worst pixel, its place in its tile, worst error per region."""
import json
import os
import re
import subprocess
import sys
import time
import types

import numpy as np
import pytest

from tests import geometry_cases as gc
from tests import width_models as wm
from tests.conftest import PKG, REPO, rel_err
from wct_hip import model_zoo

pytestmark = pytest.mark.gpu

ENC_DEC_GATE = wm.ENC_DEC_GATE
MOM_GATE = wm.MOM_GATE


def _device_cus():
    """CU count of device 0 (what conv_f16_dev.h num_cus() reads); 256 where there is no device (collection on a CPU box)."""
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        pass
    return 256


CUS = _device_cus()
CASES = gc.cases(CUS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from oracle import wct_oracle
    wct_oracle.set_num_threads(min(16, wct_oracle.num_threads()))
    return torch


@pytest.fixture(scope="module")
def weights(weights16x):
    cache = {"16x": weights16x}

    def get(mode):
        if mode not in cache:
            cache[mode] = model_zoo.synth_weights("original", 7)
        return cache[mode]
    return get


@pytest.fixture(scope="module")
def engines(torch_cuda, weights):
    """mode -> WCT with profiling and the form suffixes on"""
    from wct_hip import WCT
    cache = {}

    def get(mode):
        if mode not in cache:
            w = WCT(types.SimpleNamespace(mode=mode, alpha=1.0), weights=weights(mode))
            w.profile(True)
            w.debug_set("prof_forms", 1)
            cache[mode] = w
        return cache[mode]
    yield get
    cache.clear()


def _tile_h(case):
    """tile height of the case's last size-selected launch (the one that writes the result)"""
    m = re.search(r"#.(\d+)m?$", [n for n in case.expect if "#" in n][-1])
    return int(m.group(1))


def _names(wct):
    return {e["name"] for e in wct.profile_read()}


def _check_names(case, mode, names):
    if mode == 1:
        missing = [n for n in case.expect if n not in names]
        assert not missing, "%s: expected launches %s did not run; ran %s" % (case.id, missing, sorted(names))
        if case.multi:
            assert any("#" in n and n.endswith("m") for n in names), "%s: no launch walked more than one unit; ran %s" % (case.id, sorted(names))
    else:
        bad = [n for n in names if "f16x3" in n or "fused" in n or n.startswith("l1_") or "#" in n]
        assert not bad and any(n.startswith("conv3x3_f32") for n in names), "%s: conv mode 0 ran %s" % (case.id, sorted(names))


def _run_modes(case, wct, run):
    """run(mode) in conv mode 1 then 0 with the case's switches set, profile names checked per mode; no clamp on the way"""
    for k, v in case.switches:
        wct.debug_set(k, v)
    try:
        for mode in (1, 0):
            wct.set_conv_mode("f16x3" if mode else "fp32")
            wct.profile_reset()
            run(mode)
            _check_names(case, mode, _names(wct))
    finally:
        wct.set_conv_mode("f16x3")
        for k, _ in case.switches:
            wct.debug_set(k, 1)
    assert wct.saturation_count() == 0


def _seed(case):
    return (case.level * 1000003 + case.H * 4099 + case.W) % (2 ** 31)


# ---------------------------------------------------------------------------------------------------- a. every case against fp64
@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "enc"], ids=lambda c: c.id)
def test_encoder_case_vs_fp64(torch_cuda, engines, weights, case):
    torch, wct, w, widths = torch_cuda, engines(case.mode), weights(case.mode), gc.WIDTHS[case.mode]
    img = wm.smooth_image(np.random.default_rng(_seed(case)), case.H, case.W)
    ref = wm.encode(widths, w, case.level, img)
    e32 = rel_err(wm.encode(widths, w, case.level, img, f64=False), ref)
    gate = max(ENC_DEC_GATE, 4 * e32)
    x = torch.from_numpy(img).cuda()

    def run(mode):
        got = wct.encode(case.level, x)[0].cpu().numpy()
        assert got.shape == ref.shape
        err = rel_err(got, ref)
        print("geometry %s mode %d: %.3e (fp32 arm %.3e, gate %.1e) %s" % (case.id, mode, err, e32, gate, " ".join(n for n in case.expect if "#" in n)))
        assert err < gate, "%s mode %d: %s" % (case.id, mode, gc.locate(got, ref, gc.FTW, gc.SPH))
    _run_modes(case, wct, run)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "dec"], ids=lambda c: c.id)
def test_decoder_case_vs_fp64(torch_cuda, engines, weights, case):
    torch, wct, w, widths = torch_cuda, engines(case.mode), weights(case.mode), gc.WIDTHS[case.mode]
    rng = np.random.default_rng(_seed(case))
    # a well-spread feature of the level's shape: the fp64 feature of an image of the decoded size plus a positive perturbation
    enc = wm.encode(widths, w, case.level, wm.smooth_image(rng, case.H, case.W))
    f = np.maximum(enc + 0.3 * np.abs(enc).max() * rng.standard_normal(enc.shape), 0).astype(np.float32)
    ref = wm.decode(widths, w, case.level, f)
    assert ref.shape == (3, case.H, case.W)
    e32 = rel_err(wm.decode(widths, w, case.level, f, f64=False), ref)
    gate = max(ENC_DEC_GATE, 4 * e32)
    x = torch.from_numpy(f)[None].cuda()
    th = _tile_h(case)

    def run(mode):
        got = wct.decode(case.level, x)[0].cpu().numpy()
        assert got.shape == ref.shape
        err = rel_err(got, ref)
        print("geometry %s mode %d: %.3e (fp32 arm %.3e, gate %.1e) %s" % (case.id, mode, err, e32, gate, " ".join(n for n in case.expect if "#" in n)))
        assert err < gate, "%s mode %d: %s" % (case.id, mode, gc.locate(got, ref, gc.FTW, th))
    _run_modes(case, wct, run)


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "l1"], ids=lambda c: c.id)
def test_level1_case_vs_fp64(torch_cuda, engines, weights, case):
    """wct_content_encode (fused level-1 moments, whole map and an interior column window that is not 32-aligned) and
    wct_content_decode (fused level-1 decode) with a random well-conditioned (M, b), as test_level1_width_vs_fp64 does."""
    torch, wct, w, widths = torch_cuda, engines(case.mode), weights(case.mode), gc.WIDTHS[case.mode]
    rng = np.random.default_rng(_seed(case))
    H, W, C = case.H, case.W, widths["l1"]
    img = wm.smooth_image(rng, H, W)
    F = wm.encode(widths, w, 1, img)
    x0 = W // 3 + (5 if (W // 3) % 32 == 0 else 0)
    x1 = x0 + min(301, W // 3)
    x1 += 7 if x1 % 32 == 0 else 0
    assert x0 % 32 and x1 % 32 and x1 < W
    M = np.eye(C) + 0.1 * rng.standard_normal((C, C)) / np.sqrt(C)
    b = rng.standard_normal(C) * 0.1 * np.abs(F).max()
    ref = wm.decode_affine(widths, w, 1, F, M, b)
    e32 = rel_err(wm.decode_affine(widths, w, 1, F, M, b, f64=False), ref)
    gate = max(ENC_DEC_GATE, 4 * e32)
    x, Md, bd = torch.from_numpy(img).cuda(), torch.from_numpy(M).cuda(), torch.from_numpy(b).cuda()
    th = _tile_h(case)

    def run(mode):
        got_f = wct.encode(1, x)[0].cpu().numpy()
        assert rel_err(got_f, F) < ENC_DEC_GATE, "%s mode %d relu1_1: %s" % (case.id, mode, gc.locate(got_f, F, gc.FTW, 8))
        for win in ((x0, x1), (0, -1)):              # the whole map last: wct_content_decode closes that pair
            _, _, s, ss = wct.content_encode(1, x, *win)
            rs, rss = wm.raw_moments(F, win[0], None if win[1] < 0 else win[1])
            es, ess = rel_err(s.cpu().numpy(), rs), rel_err(ss.cpu().numpy(), rss)
            print("geometry %s mode %d window %s: sum %.3e sumsq %.3e (gate %.1e)" % (case.id, mode, win, es, ess, MOM_GATE))
            assert es < MOM_GATE and ess < MOM_GATE, (case.id, mode, win, es, ess)
        got = wct.content_decode(1, Md, bd, H, W)[0].cpu().numpy()
        err = rel_err(got, ref)
        print("geometry %s mode %d: %.3e (fp32 arm %.3e, gate %.1e) %s" % (case.id, mode, err, e32, gate, " ".join(n for n in case.expect if "#" in n)))
        assert err < gate, "%s mode %d: %s" % (case.id, mode, gc.locate(got, ref, gc.FTW, th))
    _run_modes(case, wct, run)


# ---------------------------------------------------------------------------------------------------- b. tile-shape independence
# One child process per arm: the WCT_* switches are read once per process.  `jobs` below name what a child computes; it prints one
# "<tag> <sha256>" line per output and one "names <profile names>" line.
_CHILD = r"""
import hashlib, json, os, sys, types
sys.path[:0] = [%r, %r]
import torch
from wct_hip import WCT, model_zoo
job, sizes = sys.argv[1], json.loads(sys.argv[2])
g = torch.Generator(device="cuda").manual_seed(11)
def rand(*shape, dtype=torch.float32):
    return torch.rand(shape, device="cuda", generator=g, dtype=dtype)
def engine(mode):
    w = model_zoo.load_npz_weights(os.path.join(%r, "weights", "16x.npz")) if mode == "16x" else model_zoo.synth_weights("original", 7)
    e = WCT(types.SimpleNamespace(mode=mode, alpha=1.0), weights=w)
    e.profile(True)
    e.debug_set("prof_forms", 1)
    return e
def out(tag, t):
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t).all()), tag
    print(tag, hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest())
names, e = set(), None
for spec in sizes:
    mode, op, level, a, b = spec[:5]
    if e is None or e.mode != mode:
        e = engine(mode)
    for upconv in spec[5:] or [1]:
        e.debug_set("upconv", upconv)
        tag = "%%s-%%s%%d-%%dx%%d-upconv%%d" %% (mode, op, level, a, b, upconv)
        if op == "enc":
            out(tag, e.encode(level, rand(1, 3, a, b)))
        elif op == "dec":
            out(tag, e.decode(level, rand(1, model_zoo.feature_channels(mode, level), a, b)))
        else:
            C = model_zoo.feature_channels(mode, 1)
            x = rand(1, 3, a, b)
            M = torch.eye(C, device="cuda", dtype=torch.float64) + 0.1 * (rand(C, C, dtype=torch.float64) - 0.5)
            _, _, s, ss = e.content_encode(1, x)
            out(tag + "-sum", s), out(tag + "-sumsq", ss)
            out(tag, e.content_decode(1, M, rand(C, dtype=torch.float64), a, b))
        names |= {r["name"] for r in e.profile_read()}
    assert e.saturation_count() == 0
print("names", json.dumps(sorted(names)))
""" % (REPO, PKG, PKG)

# per-child time limits (s): about five times the slowest arm of each job on the MI355X box (tail 3.1 s, l1dec 2.5 s, head 3.2 s,
# f16small 3.9 s, sp3 2.3 s; python + torch start-up, first-use code loading and allocation make up nearly all of it, box-to-box
# spread is ~10 %), rounded up to 5 s
_JOB_TIMEOUT = {"tail": 20, "l1dec": 15, "head": 20, "f16small": 20, "sp3": 15}


def _child(job, sizes, env, tmp_path):
    script = tmp_path / "geometry_child.py"
    if not script.exists():
        script.write_text(_CHILD)
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, str(script), job, json.dumps(sizes)], env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=_JOB_TIMEOUT[job])
    except subprocess.TimeoutExpired:
        pytest.exit("geometry child %s %s ran into its %d s limit: nothing more is started on this GPU" % (job, env, _JOB_TIMEOUT[job]), returncode=3)
    dt = time.time() - t0
    if r.returncode < 0 or r.returncode in (134, 139):      # killed by a signal (abort, segmentation fault): a GPU fault until shown otherwise
        pytest.exit("geometry child %s %s died with %d: nothing more is started on this GPU\n%s" % (job, env, r.returncode, r.stderr[-3000:]), returncode=3)
    assert r.returncode == 0, "child %s %s exited %d:\n%s" % (job, env, r.returncode, r.stderr[-3000:])
    lines = [ln.split(" ", 1) for ln in r.stdout.splitlines() if " " in ln]
    digests = {k: v for k, v in lines if k != "names"}
    names = set(json.loads(dict(lines)["names"]))
    print("geometry child %s %s: %.1f s (limit %d s), %d digests" % (job, {k: v for k, v in env.items() if k != "WCT_DEBUG"}, dt, _JOB_TIMEOUT[job], len(digests)))
    return digests, names


def _arms_agree(job, sizes, arms, tmp_path, must_run):
    """arms: [(env, forms)]: each child, one after another (its return code asserted before the next starts, nothing retried), must run a
    launch of `must_run` with each of its forced forms; every output digest must be the same in all arms."""
    results = []
    for env, forms in arms:
        digests, names = _child(job, sizes, dict(env, WCT_DEBUG="1") if env else {}, tmp_path)
        for form in forms:
            assert any(n.startswith(must_run) and re.search("#%s(m?)$" % re.escape(form), n) for n in names), \
                "%s %s: no %s launch took form %s; ran %s" % (job, env, must_run, form, sorted(names))
        results.append((env, digests))
    env0, d0 = results[0]
    assert d0, job
    for env, d in results[1:]:
        assert d.keys() == d0.keys()
        diff = sorted(k for k in d0 if d[k] != d0[k])
        assert not diff, "%s: outputs %s differ between %s and %s" % (job, diff, env0, env)


def _case_size(kind, mode, level, pick, **switches):
    """(H, W) of the pick-th case of that kind / mode / level (the thresholds' sizes for this device)"""
    sw = tuple(sorted(switches.items()))
    return [(c.H, c.W) for c in CASES if (c.kind, c.mode, c.level, c.switches) == (kind, mode, level, sw)][pick]


def test_tail_tile_height_does_not_change_a_bit(torch_cuda, tmp_path):
    """launch_dec_tail: "results do not depend on the tile shape (same arithmetic per pixel)" -- tile heights 8 / 16 / 24 of the upsample
    form (dec_tail_up_kernel) and of the nine-tap form (dec_tail_kernel) on the ragged threshold sizes and a small one."""
    sizes = [["16x", "dec", 2, H // 2, W // 2, 1, 0] for H, W in (_case_size("dec", "16x", 2, 0), _case_size("dec", "16x", 2, 3), (38, 46))]
    sizes.append(["16x", "dec", 3, *(v // 4 for v in _case_size("dec", "16x", 3, 0)), 1, 0])
    _arms_agree("tail", sizes, [({"WCT_TAIL_TH": str(th)}, ("u%d" % th, "t%d" % th)) for th in (8, 16, 24)], tmp_path, "dec_tail_fused")


def test_level1_decode_tile_height_does_not_change_a_bit(torch_cuda, tmp_path):
    """launch_l1_decode: "results do not depend on the tile shape" -- 32 x 8 against 32 x 16 tiles."""
    sizes = [["16x", "l1", 1, H, W] for H, W in (_case_size("l1", "16x", 1, 0), _case_size("l1", "16x", 1, 2), (29, 45))]
    _arms_agree("l1dec", sizes, [({"WCT_L1DEC_TH": str(th)}, ("t%d" % th,)) for th in (8, 16)], tmp_path, "l1_decode_fused")


def test_head_form_does_not_change_a_bit(torch_cuda, tmp_path):
    """launch_enc_head: the two-role head (default at these sizes), enc_head_kernel<8>, enc_head_kernel<24> and whatever WCT_HEAD_ROLES=0
    selects share their per-pixel device functions ("bit-identical results", conv3x3_f16.hip) -- encoders 5 and 2 (SP16 and fp32
    outputs behind the head) at the threshold size, the 2 MP one and a small one."""
    hw = [_case_size("enc", "16x", 5, 2), (1031, 1953), (67, 95)]
    sizes = [["16x", "enc", level, H, W] for H, W in hw for level in (5, 2)]
    arms = [({}, ("r16", "t8")), ({"WCT_HEAD_TH": "8"}, ("t8",)), ({"WCT_HEAD_TH": "24"}, ("t24",)), ({"WCT_HEAD_ROLES": "0"}, ("t8",))]
    _arms_agree("head", sizes, arms, tmp_path, "enc_head_fused")


def test_small_map_form_does_not_change_a_bit(torch_cuda, tmp_path):
    """launch_conv3x3_f16: the small-map form (32 x 8 tiles, cout groups of 64) is "the same arithmetic per output (bit-identical)" as
    the 32 x 16 form -- the first conv of the 16x d5 and of --mode original's d3 (at the size just below the threshold)."""
    H, W = _case_size("dec", "original", 3, 0)
    sizes = [["16x", "dec", 5, 33, 50], ["16x", "dec", 5, 67, 120], ["original", "dec", 3, H // 4, W // 4]]
    _arms_agree("f16small", sizes, [({"WCT_F16_SMALL": "1"}, ("s8",)), ({"WCT_F16_SMALL": "0"}, ("t16",))], tmp_path, "conv3x3_f16x3<co=128>")


def test_three_stage_sp_kernel_does_not_change_a_bit(torch_cuda, tmp_path):
    """conv3x3_sp.hip: conv3x3_sp3_kernel has "same tiles, same MFMA order, same epilogue" as the two-stage kernel (WCT_SP3=0): "results
    are bit-identical" -- the 32-cout layers of e3 (plain and pooled; many units per workgroup at 2 MP) and of d3 in its nine-tap form."""
    sizes = [["16x", "enc", 3, 1031, 1953], ["16x", "enc", 3, 67, 95], ["16x", "dec", 3, 61, 63, 0], ["16x", "dec", 3, 259, 193, 0]]
    _arms_agree("sp3", sizes, [({"WCT_SP3": "1"}, ("316",)), ({"WCT_SP3": "0"}, ("t16",))], tmp_path, "conv3x3_f16x3<co=32,")


# ---------------------------------------------------------------------------------------------------- c. forms reachable by default
def test_default_switches_reach_every_form(torch_cuda, engines):
    """Over the default-switch cases, the launches must cover geometry_cases.FORMS: a threshold change that orphans a kernel form shows
    up here.  (No reference: the calls run on random inputs; what they compute is part a's business.)"""
    torch = torch_cuda
    g = torch.Generator(device="cuda").manual_seed(5)
    seen = set()
    for case in CASES:
        if case.switches:
            continue
        wct = engines(case.mode)
        wct.profile_reset()
        if case.kind == "enc":
            wct.encode(case.level, torch.rand((1, 3, case.H, case.W), device="cuda", generator=g))
        elif case.kind == "dec":
            C = model_zoo.feature_channels(case.mode, case.level)
            wct.decode(case.level, torch.rand((1, C, case.H >> (case.level - 1), case.W >> (case.level - 1)), device="cuda", generator=g))
        else:
            C = model_zoo.feature_channels(case.mode, 1)
            wct.content_encode(1, torch.rand((1, 3, case.H, case.W), device="cuda", generator=g))
            wct.content_decode(1, torch.eye(C, device="cuda", dtype=torch.float64), torch.zeros(C, device="cuda", dtype=torch.float64), case.H, case.W)
        seen |= {n[:-1] if n.endswith("m") and "#" in n else n for n in _names(wct)}
        assert wct.saturation_count() == 0
    missing = [f for f in gc.FORMS if f not in seen]
    assert not missing, "forms no default-switch case reaches on %d CUs: %s; reached %s" % (CUS, missing, sorted(n for n in seen if "#" in n))
