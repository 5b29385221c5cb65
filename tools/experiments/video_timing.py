"""What video mode costs on the device (include/wct_hip_video.h), written to profiles/video_timing.txt:

  1. wct_temporal_blend at 3840 x 2160, radius 2, against wct_luma_merge at the same size scaled by the bytes moved (the blend reads
     four images and writes one, the merge reads two and writes one: 5 / 3), with and without the fused uint8 image, and on a cut.
  2. wct_stylize_clip per frame against wct_stylize_prepared -- and, with --baseline_lib, against wct_stylize_prepared of ANOTHER build of
     the library (the parent commit's), the two builds alternating in fresh processes on the same device: a plain prepared call
     must cost the same in both.

    python tools/experiments/video_timing.py [--baseline_lib /path/to/parent/libwct_hip.so] [--rounds 3] [--out profiles/video_timing.txt]

Times are device events around `--steps` back-to-back calls after `--warmup` calls; the frames alternate between two images so that the
blend really blends."""
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

H, W, HS, WS = 2160, 3840, 1024, 1024
VIDEO_ENTRIES = ("wct_clip_bytes", "wct_clip_create", "wct_clip_destroy", "wct_clip_reset", "wct_clip_export", "wct_moments_track",
                 "wct_temporal_blend", "wct_stylize_clip")


def worker(steps, warmup):
    """One process, one build (WCT_LIB_PATH): every timing this build can give, as one JSON line."""
    if os.environ.get("VIDEO_TIMING_OLD_BUILD"):
        # a build from before video mode lacks its entries; the binding sets their argument types at load time -- hand it placeholders
        class Tolerant(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if name in VIDEO_ENTRIES:
                        return types.SimpleNamespace()
                    raise
        ctypes.CDLL = Tolerant
    import torch
    from wct_hip import WCT, model_zoo
    assert torch.cuda.is_available(), "video_timing.py measures on the MI355X: no GPU, no numbers"
    w = model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz"))
    wct = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=w)
    has_video = hasattr(wct._lib, "wct_stylize_clip") and not os.environ.get("VIDEO_TIMING_OLD_BUILD")
    g = torch.Generator().manual_seed(5)
    a = torch.rand((1, 3, H, W), generator=g).cuda()
    b = (a + 0.02 * (torch.rand((1, 3, H, W), generator=g).cuda() - 0.5)).clamp(0, 1)
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

    res = {"has_video": has_video}
    frames = (a, b)
    res["prepared_ms"] = timed(lambda i: wct.stylize_prepared(frames[i & 1], alpha=0.6, out=out.view(-1)), steps)
    sty = wct.stylize_prepared(a, alpha=0.6).clone()
    merged = torch.empty_like(sty)
    res["luma_merge_ms"] = timed(lambda i: wct.luma_merge(sty, a, out=merged.view(-1)), 4 * steps)
    if has_video:
        prev_o, blended = sty.clone(), torch.empty_like(sty)
        one = torch.ones(1, device="cuda", dtype=torch.int32)
        res["blend_ms"] = timed(lambda i: wct.temporal_blend(b, a, sty, prev_o, 0.6, 0.05, 2, out=blended.view(-1)), 4 * steps)
        res["blend_r8_ms"] = timed(lambda i: wct.temporal_blend(b, a, sty, prev_o, 0.6, 0.05, 8, out=blended.view(-1)), 4 * steps)
        res["blend_r0_ms"] = timed(lambda i: wct.temporal_blend(b, a, sty, prev_o, 0.6, 0.05, 0, out=blended.view(-1)), 4 * steps)
        res["blend_u8_ms"] = timed(lambda i: wct.temporal_blend(b, a, sty, prev_o, 0.6, 0.05, 2, out=blended.view(-1), u8=True), 4 * steps)
        res["blend_cut_ms"] = timed(lambda i: wct.temporal_blend(b, a, sty, prev_o, 0.6, 0.05, 2, cut_flag=one, out=blended.view(-1)), 4 * steps)
        clip = wct.clip(H, W, rate=0.25, cut=float("inf"), blend=0.6)
        res["clip_ms"] = timed(lambda i: clip.stylize(frames[i & 1], alpha=0.6, out=blended.view(-1)), steps)
        wct.profile(True)
        wct.profile_reset()
        for i in range(4):
            clip.stylize(frames[i & 1], alpha=0.6, out=blended.view(-1))
        fam = {r["name"]: r["ms"] / 4 for r in wct.profile_read() if r["name"] in ("clip_track", "temporal_blend", "clip_store")}
        wct.profile(False)
        res["families_ms_per_frame"] = fam
        clip.close()
        res["prepared_after_ms"] = timed(lambda i: wct.stylize_prepared(frames[i & 1], alpha=0.6, out=out.view(-1)), steps)
    assert wct.saturation_count() == 0
    print("VIDEO_TIMING " + json.dumps(res))


def run_worker(lib_path, old, steps, warmup):
    env = dict(os.environ)
    if lib_path:
        env["WCT_LIB_PATH"] = lib_path
    if old:
        env["VIDEO_TIMING_OLD_BUILD"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(steps), "--warmup", str(warmup)], env=env,
                       capture_output=True, text=True, timeout=900)
    for line in r.stdout.splitlines():
        if line.startswith("VIDEO_TIMING "):
            return json.loads(line[len("VIDEO_TIMING "):])
    raise RuntimeError("worker failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--baseline_lib", default=None, help="libwct_hip.so of the commit to compare with (built from its tree)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "video_timing.txt"))
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
    mb = 12.0 * H * W / 1e6                     # one planar fp32 image
    lines = ["video mode at %d x %d (16x model, style %d x %d prepared once), %d processes per build, %d timed calls each; ms: median (min .. max)"
             % (W, H, WS, HS, args.rounds, args.steps), ""]
    lm, bl = med(new, "luma_merge_ms"), med(new, "blend_ms")
    lines += ["1. wct_temporal_blend against wct_luma_merge",
              "   wct_luma_merge (2 images read, 1 written = %.0f MB)      %s   -> %.0f GB/s" % (3 * mb, span(new, "luma_merge_ms"), 3 * mb / lm),
              "   wct_temporal_blend radius 2 (4 read, 1 written = %.0f MB)  %s   -> %.0f GB/s" % (5 * mb, span(new, "blend_ms"), 5 * mb / bl),
              "   ratio to luma_merge x 5/3: %.2f   (expected at most 1.5: halo re-reads and the exponential)" % (bl / (lm * 5 / 3)),
              "   radius 0 %s    radius 8 %s    radius 2 + uint8 image %s    on a cut (1 read, 1 written) %s"
              % (span(new, "blend_r0_ms"), span(new, "blend_r8_ms"), span(new, "blend_u8_ms"), span(new, "blend_cut_ms")), ""]
    lines += ["2. wct_stylize_clip per frame against wct_stylize_prepared",
              "   this build: wct_stylize_prepared            %s" % span(new, "prepared_ms"),
              "   this build: wct_stylize_clip                %s   (+%.3f)" % (span(new, "clip_ms"), med(new, "clip_ms") - med(new, "prepared_ms")),
              "   this build: wct_stylize_prepared afterwards %s" % span(new, "prepared_after_ms")]
    fam = {}
    for r in new:
        for k, v in r["families_ms_per_frame"].items():
            fam.setdefault(k, []).append(v)
    lines += ["   profile families per frame (event-timed, launches serialised by the profiler): " +
              ", ".join("%s %.3f" % (k, sorted(v)[len(v) // 2]) for k, v in sorted(fam.items()))]
    if old:
        lines += ["   baseline build: wct_stylize_prepared        %s   (this build / baseline: %.4f)"
                  % (span(old, "prepared_ms"), med(new, "prepared_ms") / med(old, "prepared_ms")),
                  "   baseline build: wct_luma_merge              %s" % span(old, "luma_merge_ms")]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
