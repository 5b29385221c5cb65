"""Cost of texture synthesis on the config-2 frame (3840 x 2160 output, 2048 x 2048 texture, 16x): the noise kernel on its own, and
wct_synthesize beside wct_stylize of the same shapes (content = the same noise, already in memory), alternating the two in one process.
Per case the median of --frames frames, each synchronised on its own; wct_stylize is timed TWICE per round (stylize_a, stylize_b) so
that the spread between two runs of the same code is measured by the same loop.  The noise kernel: --reps back-to-back launches
between two events (an upper bound: it is the host's enqueue rate where that is slower than the kernel), and the library's own
per-launch event timing (wct_profile_*: the events' own cost included), against its floor of 3 H W x 4 bytes written once and against a
plain fill of the same buffer timed the same way; the kernel's own duration comes from a rocprofv3 kernel trace of --noise-only.  Prints one JSON line.

    python tools/bench_synthesis.py [--frames 20] [--noise-only]

--noise-only runs just the noise launches: the process to put under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
for p in (REPO, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_TBPS = 8.0     # MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--noise-only", action="store_true")
    a = ap.parse_args()
    import torch
    from wct_hip import WCT, model_zoo
    w = model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz"))
    wct = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=w)
    H, W = 2160, 3840
    buf = torch.empty((3, H, W), device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nbytes = 12.0 * H * W
    res = {"frame": "%dx%d output, 2048x2048 texture, 16x" % (W, H), "noise_bytes": nbytes, "noise_floor_us": round(nbytes / (HBM_PEAK_TBPS * 1e12) * 1e6, 2)}

    # the noise kernel: back-to-back launches
    for _ in range(10):
        wct.noise(H, W, seed=1, out=buf)
    batches = []
    for b in range(5):
        torch.cuda.synchronize()
        e0.record()
        for i in range(a.reps):
            wct.noise(H, W, seed=b * a.reps + i, out=buf)
        e1.record()
        torch.cuda.synchronize()
        batches.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    us = statistics.median(batches)
    res["noise_us_back_to_back"] = {"median": round(us, 2), "min": round(min(batches), 2), "max": round(max(batches), 2), "reps": a.reps,
                                    "TBps": round(nbytes / us * 1e-6, 2), "of_hbm_peak": round(nbytes / us * 1e-6 / HBM_PEAK_TBPS, 3)}
    # a plain fill of the same buffer in the same loop: what writing 3 H W floats costs on this device when nothing is computed
    fills = []
    for b in range(5):
        torch.cuda.synchronize()
        e0.record()
        for i in range(a.reps):
            buf.fill_(0.5)
        e1.record()
        torch.cuda.synchronize()
        fills.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    res["fill_us_back_to_back"] = {"median": round(statistics.median(fills), 2), "min": round(min(fills), 2), "max": round(max(fills), 2)}
    if a.noise_only:
        print(json.dumps(res))
        return
    wct.profile(True)
    wct.profile_reset()
    for i in range(50):
        wct.noise(H, W, seed=i, out=buf)
    torch.cuda.synchronize()
    for r in wct.profile_read():
        if r["name"].startswith("noise_uniform"):
            res["noise_us_profile_events"] = {"mean": round(r["ms"] / r["launches"] * 1e3, 2), "launches": r["launches"]}
    wct.profile(False)

    # synthesize beside stylize of the same shapes
    from PIL import Image
    t = np.asarray(Image.open(os.path.join(REPO, "tests", "golden", "g11_style_2048x2048.jpg")).convert("RGB"), np.float32) / 255
    t = torch.from_numpy(np.ascontiguousarray(t.transpose(2, 0, 1))).cuda()
    content = wct.noise(H, W, seed=7).clone()
    out = torch.empty((3, H, W), device="cuda")
    runs = {
        "stylize_a": lambda: wct.stylize(content, t, 1.0, out=out),
        "synthesize": lambda: wct.synthesize(t, H, W, seed=7, out=out),
        "stylize_b": lambda: wct.stylize(content, t, 1.0, out=out),
    }
    assert torch.equal(wct.synthesize(t, H, W, seed=7).clone(), wct.stylize(content, t, 1.0))
    times = {k: [] for k in runs}
    for i in range(a.warmup + a.frames):
        for k, fn in runs.items():
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
    for k in runs:
        q = statistics.quantiles(times[k], n=4)
        res[k] = {"ms_median": round(statistics.median(times[k]), 4), "ms_min": round(min(times[k]), 4), "ms_iqr": round(q[2] - q[0], 4)}
    base = (res["stylize_a"]["ms_median"] + res["stylize_b"]["ms_median"]) / 2
    res["synthesize_minus_stylize_us"] = round((res["synthesize"]["ms_median"] - base) * 1e3, 1)
    res["stylize_a_minus_b_us"] = round((res["stylize_a"]["ms_median"] - res["stylize_b"]["ms_median"]) * 1e3, 1)
    # paired: each round's synthesize against the mean of the two stylize frames around it
    paired = [(s - (x + y) / 2) * 1e3 for s, x, y in zip(times["synthesize"], times["stylize_a"], times["stylize_b"])]
    res["paired_difference_us"] = {"median": round(statistics.median(paired), 1), "iqr": round(statistics.quantiles(paired, n=4)[2] - statistics.quantiles(paired, n=4)[0], 1)}
    res["frames"] = a.frames
    res["range_count"] = wct.saturation_count()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
