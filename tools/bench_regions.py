"""Cost of spatial control: wct_stylize against wct_stylize_regions on the config-2 frame (3840 x 2160 content, 2048 x 2048 style, 16x),
interleaved in one process.  Cases: K = 1 (uniform labels), K = 2 (left / right halves), K = 4 (thresholded smooth-noise blobs).
Per case the median of --frames frames, each synchronised on its own, with the device clock read beside it; then one profiled frame
per case (the library's own per-kernel timing, wct_profile_*) for the new kernels, with the algorithmic GB/s of moments_labeled and
apply_labeled, and wct_moments on the same level-1 map for comparison.  Prints one JSON line.

    python tools/bench_regions.py [--frames 10]
"""
import argparse
import glob
import json
import os
import statistics
import sys
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def sclk_file():
    for pat in ("/sys/class/drm/card[0-9]*/device/hwmon/hwmon*/freq1_input",):
        g = sorted(glob.glob(pat))
        if len(g) == 1:
            return g[0]
    return None


def read_mhz(f):
    try:
        return int(open(f).read().split()[0]) * 1e-6 if f else None
    except Exception:     # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    from PIL import Image
    from wct_hip import WCT, model_zoo
    w = model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz"))
    wct = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=w)
    gold = os.path.join(REPO, "tests", "golden")

    def img(name):
        x = np.asarray(Image.open(os.path.join(gold, name)).convert("RGB"), np.float32) / 255
        return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))).cuda()

    c, s = img("g11_uhd_content_3840x2160.jpg"), img("g11_style_2048x2048.jpg")
    H, W = int(c.shape[1]), int(c.shape[2])
    g = torch.Generator(device="cuda").manual_seed(5)
    s2 = torch.rand((3, 1024, 1024), device="cuda", generator=g)
    noise = torch.nn.functional.avg_pool2d(torch.rand((1, 1, H, W), device="cuda", generator=g), 63, 1, 31, count_include_pad=False)
    noise = torch.nn.functional.avg_pool2d(noise, 63, 1, 31, count_include_pad=False)[0, 0]
    q = torch.quantile(noise.flatten()[::97].float(), torch.tensor([0.25, 0.5, 0.75], device="cuda"))
    blobs = (noise > q[0]).to(torch.uint8) + (noise > q[1]).to(torch.uint8) + (noise > q[2]).to(torch.uint8)
    halves = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    halves[:, W // 2:] = 1
    cases = {
        "K1_uniform": ([s], torch.zeros((H, W), dtype=torch.uint8, device="cuda"), [1.0]),
        "K2_halves": ([s, s2], halves, [1.0, 0.6]),
        "K4_blobs": ([s, s2, s, s2], blobs, [1.0, 0.6, 0.8, 1.0]),
    }
    out = torch.empty((3, H, W), device="cuda")
    runs = {"stylize": lambda: wct.stylize(c, s, 1.0, out=out)}
    for name, (st, lab, al) in cases.items():
        runs[name] = (lambda st=st, lab=lab, al=al: wct.stylize_regions(c, st, lab, al, out=out))
    f = sclk_file()
    times = {k: [] for k in runs}
    clocks = {k: [] for k in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(a.warmup + a.frames):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
                clocks[k].append(read_mhz(f))
    res = {"frame": "%dx%d content, %dx%d style, 16x" % (W, H, int(s.shape[2]), int(s.shape[1])), "frames": a.frames}
    base = statistics.median(times["stylize"])
    for k in runs:
        m = statistics.median(times[k])
        cl = [x for x in clocks[k] if x]
        res[k] = {"ms_median": round(m, 3), "ms_min": round(min(times[k]), 3), "x_stylize": round(m / base, 3),
                  "sclk_MHz_median": round(statistics.median(cl), 0) if cl else None}
    # per-kernel times from the library's profiler: one frame per case
    prof = {}
    for k in cases:
        wct.profile(True)
        wct.profile_reset()
        runs[k]()
        torch.cuda.synchronize()
        rows = wct.profile_read()
        wct.profile(False)
        sel = {}
        for r in rows:
            if r["name"] in ("moments_labeled", "apply_labeled", "labels_levels", "moments", "matfun_invsqrt", "matfun_sqrt", "assemble_Mb"):
                sel[r["name"]] = {"ms": round(r["ms"], 3), "launches": r["launches"]}
                if r["name"] in ("moments_labeled", "apply_labeled") and r["ms"] > 0:
                    sel[r["name"]]["GBps"] = round(r["bytes"] / r["ms"] * 1e-6, 0)
        sel["all_kernels_ms"] = round(sum(r["ms"] for r in rows), 3)
        prof[k] = sel
    res["profile"] = prof
    # moments_labeled (K = 2, halves) against wct_moments on the same level-1 map (relu1_1, 24 channels)
    feat = wct.encode(1, c[None], layout="nhwc")
    lab1 = halves[: feat.shape[1], : feat.shape[2]].contiguous()
    cmp = {}
    for name, fn in (("wct_moments", lambda: wct.moments(feat)), ("moments_labeled_K2", lambda: wct.moments_labeled(feat, lab1, 2))):
        ts = []
        for i in range(a.warmup + a.frames):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        cmp[name] = round(statistics.median(ts), 3)
    cmp["ratio"] = round(cmp["moments_labeled_K2"] / cmp["wct_moments"], 3)
    res["level1_moments_ms"] = cmp
    res["range_count"] = wct.saturation_count()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
