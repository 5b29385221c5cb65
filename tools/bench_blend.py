"""Cost of style interpolation and per-pixel style weights on the config-2 frame (3840 x 2160 content, 2048 x 2048 styles, 16x), interleaved
in one process with the single-style calls they extend.  Cases: wct_stylize_interp at K = 2 and K = 4 (against wct_stylize);
wct_style_blend of K = 2 cached stat sets + wct_stylize_prepared (against wct_stylize_prepared); wct_stylize_blend at K = 2 with a
horizontal gradient and at K = 4 with feathered blobs (against wct_stylize).  Per case the median of --frames frames, each synchronised
on its own, with the device clock read beside it; then one profiled frame per case (the library's own per-kernel timing, wct_profile_*)
with the algorithmic GB/s of moments_weighted and apply_mixed, and wct_moments on the same level-1 map for comparison.  Prints one JSON
line.

    python tools/bench_blend.py [--frames 10]
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
    # four 2048^2 styles: the style image, its mirror images and its transpose (same cost, different statistics)
    st4 = [s, torch.flip(s, [2]).contiguous(), torch.flip(s, [1]).contiguous(), s.transpose(1, 2).contiguous()]
    ramp = torch.linspace(0, 1, W, device="cuda")[None, :].expand(H, W)
    gradient = torch.stack([1 - ramp, ramp]).contiguous()
    noise = torch.rand((4, 1, H // 8, W // 8), device="cuda", generator=g)
    for _ in range(3):
        noise = torch.nn.functional.avg_pool2d(noise, 9, 1, 4, count_include_pad=False)
    noise = torch.nn.functional.interpolate(noise, size=(H, W), mode="bilinear", align_corners=False)[:, 0] ** 6
    blobs = (noise / noise.sum(0, keepdim=True)).contiguous()            # four feathered blobs summing to 1
    out = torch.empty((3, H, W), device="cuda")
    stats = []
    for x in st4[:2]:
        wct.style_prepare(x)
        stats.append({L: wct.style_export(L).clone() for L in (1, 2, 3, 4, 5)})
    wct.style_prepare(s)
    single = {L: wct.style_export(L).clone() for L in (1, 2, 3, 4, 5)}

    def prepared_single():
        for L in (1, 2, 3, 4, 5):
            wct.style_import(L, single[L])
        wct.stylize_prepared(c, 1.0, out=out)

    def prepared_blend():
        wct.style_blend(stats, [0.4, 0.6])
        wct.stylize_prepared(c, 1.0, out=out)

    runs = {
        "stylize": lambda: wct.stylize(c, s, 1.0, out=out),
        "interp_K2": lambda: wct.stylize_interp(c, st4[:2], [0.4, 0.6], 1.0, out=out),
        "interp_K4": lambda: wct.stylize_interp(c, st4, [0.1, 0.2, 0.3, 0.4], 1.0, out=out),
        "prepared": prepared_single,
        "style_blend_prepared_K2": prepared_blend,
        "blend_K2_gradient": lambda: wct.stylize_blend(c, st4[:2], gradient, [1.0, 0.6], out=out),
        "blend_K4_blobs": lambda: wct.stylize_blend(c, st4, blobs, [1.0, 0.6, 0.8, 1.0], out=out),
    }
    base_of = {k: "prepared" if k.startswith("style_blend") or k == "prepared" else "stylize" for k in runs}
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
    res = {"frame": "%dx%d content, %dx%d styles, 16x" % (W, H, int(s.shape[2]), int(s.shape[1])), "frames": a.frames}
    for k in runs:
        m = statistics.median(times[k])
        base = statistics.median(times[base_of[k]])
        cl = [x for x in clocks[k] if x]
        res[k] = {"ms_median": round(m, 3), "ms_min": round(min(times[k]), 3), "x_" + base_of[k]: round(m / base, 3),
                  "sclk_MHz_median": round(statistics.median(cl), 0) if cl else None}
    # per-kernel times from the library's profiler: one frame per case
    prof = {}
    for k in runs:
        if k in ("stylize", "prepared"):
            continue
        wct.profile(True)
        wct.profile_reset()
        runs[k]()
        torch.cuda.synchronize()
        rows = wct.profile_read()
        wct.profile(False)
        sel = {}
        for r in rows:
            if r["name"] in ("moments_weighted", "apply_mixed", "weights_levels", "stats_blend", "moments", "matfun_invsqrt", "matfun_sqrt", "assemble_Mb"):
                sel[r["name"]] = {"ms": round(r["ms"], 3), "launches": r["launches"]}
                if r["name"] in ("moments_weighted", "apply_mixed", "weights_levels") and r["ms"] > 0:
                    sel[r["name"]]["GBps"] = round(r["bytes"] / r["ms"] * 1e-6, 0)
        sel["all_kernels_ms"] = round(sum(r["ms"] for r in rows), 3)
        prof[k] = sel
    res["profile"] = prof
    # moments_weighted (K = 2, gradient) against wct_moments on the same level-1 map (relu1_1, 24 channels)
    feat = wct.encode(1, c[None], layout="nhwc")
    g1 = gradient[:, : feat.shape[1], : feat.shape[2]].contiguous()
    cmp = {}
    for name, fn in (("wct_moments", lambda: wct.moments(feat)), ("moments_weighted_K2", lambda: wct.moments_weighted(feat, g1))):
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
    cmp["ratio"] = round(cmp["moments_weighted_K2"] / cmp["wct_moments"], 3)
    res["level1_moments_ms"] = cmp
    res["range_count"] = wct.saturation_count()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
