"""What motion compensation costs on the device (include/wct_hip_motion.h), written to profiles/motion_timing.txt, at 3840 x 2160 with the
command line's defaults (levels 4, range 4, penalty 4; blend 0.6, sigma 0.05, radius 2):

  1. the launches of one frame's estimate and blend, event-timed one by one through the library's profiler: luma / pyramid, every search
     level, the compensated blend -- against video mode's plain blend on the same frames;
  2. wct_stylize_clip per frame with and without motion attached, on two alternating frames that are a 7-pixel pan of each other;
  3. with --baseline_lib, wct_stylize_clip of ANOTHER build of the library (the parent commit's, which has no motion entries) on the same
     frames, the two builds alternating in fresh processes on the same device: video mode without motion must cost the same in both.

    python tools/experiments/motion_timing.py [--baseline_lib /path/to/parent/libwct_hip.so] [--rounds 3] [--out profiles/motion_timing.txt]

Times are device events around `--steps` back-to-back calls after `--warmup` calls (tools/experiments/video_timing.py's method)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

H, W, HS, WS, PAN = 2160, 3840, 1024, 1024, 7
MOTION_ENTRIES = ("wct_motion_shape", "wct_motion_luma", "wct_motion_estimate", "wct_motion_blend", "wct_motion_attach", "wct_motion_export")
FAMILIES = ("motion_pyramid", "motion_search3", "motion_search2", "motion_search1", "motion_search0", "motion_blend", "motion_store", "temporal_blend",
            "clip_track", "clip_store")


def worker(steps, warmup):
    """One process, one build (WCT_LIB_PATH): every timing this build can give, as one JSON line."""
    old = bool(os.environ.get("MOTION_TIMING_OLD_BUILD"))
    if old:
        # a build from before this feature lacks its entries; the binding sets their argument types at load time -- hand it placeholders
        class Tolerant(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if name in MOTION_ENTRIES:
                        return types.SimpleNamespace()
                    raise
        ctypes.CDLL = Tolerant
    import torch
    from wct_hip import WCT, model_zoo
    assert torch.cuda.is_available(), "motion_timing.py measures on the MI355X: no GPU, no numbers"
    w = model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz"))
    wct = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=w)
    g = torch.Generator().manual_seed(5)
    big = torch.rand((1, 3, H, W + PAN), generator=g).cuda()
    for _ in range(2):                                                   # smooth enough for a block to have something to match
        big = torch.nn.functional.avg_pool2d(big, 5, stride=1, padding=2)
    frames = (big[..., :W].contiguous(), big[..., PAN:].contiguous())    # a pan of 7 pixels, there and back
    del big
    style = torch.rand((1, 3, HS, WS), generator=g).cuda()
    wct.style_prepare(style)
    out = torch.empty((1, 3, H, W), device="cuda")

    def timed(fn, n):
        for i in range(warmup):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def families(clip):
        wct.profile(True)
        wct.profile_reset()
        for i in range(4):
            clip.stylize(frames[i & 1], alpha=0.6, out=out.view(-1))
        fam = {r["name"]: r["ms"] / 4 for r in wct.profile_read() if r["name"] in FAMILIES}
        wct.profile(False)
        return fam

    res = {"old": old}
    res["prepared_ms"] = timed(lambda i: wct.stylize_prepared(frames[i & 1], alpha=0.6, out=out.view(-1)), steps)
    plain = wct.clip(H, W, cut=float("inf"))
    res["clip_ms"] = timed(lambda i: plain.stylize(frames[i & 1], alpha=0.6, out=out.view(-1)), steps)
    res["clip_families"] = families(plain)
    plain.close()
    if not old:
        moving = wct.clip(H, W, cut=float("inf"), motion=True)
        res["motion_ms"] = timed(lambda i: moving.stylize(frames[i & 1], alpha=0.6, out=out.view(-1)), steps)
        res["motion_families"] = families(moving)
        mv = moving.motion_field()
        res["pan_blocks"] = float((mv.view(-1, 2).abs() == torch.tensor([0, PAN], device="cuda", dtype=torch.int16)).all(1).float().mean())
        moving.close()
        mv = wct.motion_estimate(frames[1], frames[0])
        res["estimate_ms"] = timed(lambda i: wct.motion_estimate(frames[i & 1], frames[1 - (i & 1)], out=mv.view(-1)), 2 * steps)
        plain = wct.clip(H, W, cut=float("inf"))
        res["clip_after_ms"] = timed(lambda i: plain.stylize(frames[i & 1], alpha=0.6, out=out.view(-1)), steps)
        plain.close()
    assert wct.saturation_count() == 0
    print("MOTION_TIMING " + json.dumps(res))


def run_worker(lib_path, old, steps, warmup):
    env = dict(os.environ)
    if lib_path:
        env["WCT_LIB_PATH"] = lib_path
    if old:
        env["MOTION_TIMING_OLD_BUILD"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(steps), "--warmup", str(warmup)], env=env,
                       capture_output=True, text=True, timeout=900)
    for line in r.stdout.splitlines():
        if line.startswith("MOTION_TIMING "):
            return json.loads(line[len("MOTION_TIMING "):])
    raise RuntimeError("worker failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--baseline_lib", default=None, help="libwct_hip.so of the commit to compare with (built from its tree)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motion_timing.txt"))
    args = ap.parse_args()
    if args.worker:
        worker(args.steps, args.warmup)
        return
    new, old = [], []
    for _ in range(args.rounds):
        if args.baseline_lib:
            old.append(run_worker(args.baseline_lib, True, args.steps, args.warmup))
        new.append(run_worker(None, False, args.steps, args.warmup))
    med = lambda rows, k: sorted(r[k] for r in rows)[len(rows) // 2]
    span = lambda rows, k: "%.3f (%.3f .. %.3f)" % (med(rows, k), min(r[k] for r in rows), max(r[k] for r in rows))

    def fam_med(rows, key):
        acc = {}
        for r in rows:
            for k, v in r[key].items():
                acc.setdefault(k, []).append(v)
        return {k: sorted(v)[len(v) // 2] for k, v in acc.items()}

    px = float(H) * W
    lines = ["motion compensation at %d x %d (16x model, style %d x %d prepared once; levels 4, range 4, penalty 4), two frames a %d-pixel pan apart,"
             % (W, H, WS, HS, PAN), "%d processes per build, %d timed calls each; ms: median (min .. max)" % (args.rounds, args.steps), ""]
    fm, fp = fam_med(new, "motion_families"), fam_med(new, "clip_families")
    est = sum(v for k, v in fm.items() if k.startswith("motion_pyramid") or k.startswith("motion_search"))
    lines += ["1. the launches of one frame (event-timed one by one, launches serialised by the profiler)"]
    for k in FAMILIES[:7]:
        if k in fm:
            lines += ["   %-16s %.4f" % (k, fm[k])]
    lines += ["   the estimate (pyramid + searches) %.4f;  video mode's plain blend on the same frames %.4f;  the compensated blend / the plain one %.2f"
              % (est, fp.get("temporal_blend", float("nan")), fm.get("motion_blend", float("nan")) / fp.get("temporal_blend", float("nan"))),
              "   pyramid: %.0f MB read, %.0f MB written -> %.0f GB/s" % (12 * px / 1e6, 4 * px / 3e6, (12 + 4.0 / 3) * px / 1e6 / fm.get("motion_pyramid", float("nan"))),
              "   wct_motion_estimate standalone (two pyramids + searches) %s" % span(new, "estimate_ms"),
              "   blocks of the last field that hold the pan exactly: %.1f %%" % (100 * med(new, "pan_blocks")), ""]
    lines += ["2. wct_stylize_clip per frame",
              "   this build: wct_stylize_prepared                  %s" % span(new, "prepared_ms"),
              "   this build: wct_stylize_clip without motion       %s" % span(new, "clip_ms"),
              "   this build: wct_stylize_clip with motion          %s   (+%.3f)" % (span(new, "motion_ms"), med(new, "motion_ms") - med(new, "clip_ms")),
              "   this build: wct_stylize_clip without motion again %s" % span(new, "clip_after_ms")]
    if old:
        lines += ["   baseline build: wct_stylize_prepared              %s" % span(old, "prepared_ms"),
                  "   baseline build: wct_stylize_clip                  %s   (this build without motion / baseline: %.4f)"
                  % (span(old, "clip_ms"), med(new, "clip_ms") / med(old, "clip_ms"))]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
