"""Measurements for DESIGN.md's colour section (tools/bench_color.py <leg>).  Three legs, chosen by argv[1]:
  summarise <kernel_trace.csv> <log of the kernels leg>   per-launch medians of a rocprofv3 kernel trace of the kernels leg, by position in
            the round (the trace's --stats file merges launches of one kernel name: both moment sizes, both merge outputs, all copies)
  kernels   every colour kernel at the benchmark's sizes after a warm-up, with torch device copies of the same byte counts, 20 rounds
            (run under rocprofv3 --kernel-trace --stats); prints the algorithmic bytes per launch as JSON
  frames    stylize_color in each mode against stylize on the same frame, alternating, medians of synchronised frames
"""
import json
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
sys.path[:0] = [REPO, PKG]

if sys.argv[1] == "summarise":
    import csv
    import re
    log = [l for l in open(sys.argv[3]) if l.startswith("BYTES ")][-1]
    meta = json.loads(log[6:])
    rows = sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Start_Timestamp"]))
    mine = ("color_moments_kernel", "color_moments_final_kernel", "color_solve_kernel", "color_apply_kernel", "luma_merge_kernel", "copyBuffer")
    rows = [r for r in rows if any(m in r["Kernel_Name"] for m in mine)]
    # one round: moments content (stage 1 + final), moments style (2), solve, apply, merge planar, merge u8, then the copies
    names = ["color_moments_content stage1", "color_moments_content final", "color_moments_style stage1", "color_moments_style final", "color_solve",
             "color_apply_style", "luma_merge_planar", "luma_merge_u8"] + ["copy " + k for k in meta["copy_bytes_moved"]]
    per = len(names)
    tail = rows[-per * meta["rounds"]:]
    assert len(tail) == per * meta["rounds"], (len(rows), per)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {}
    for i, n in enumerate(names):
        sel = tail[i::per]
        kn = set(re.search(r"(\w+_kernel|copyBuffer)", r["Kernel_Name"]).group(1) for r in sel)
        assert len(kn) == 1, (n, kn)
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sel]
        out[n] = {"kernel": kn.pop(), "us_median": round(med(d), 2), "us_min": round(min(d), 2), "us_max": round(max(d), 2), "launches": len(d)}
    ab = meta["algorithmic_bytes"]
    for k in ("content", "style"):
        us = out["color_moments_%s stage1" % k]["us_median"] + out["color_moments_%s final" % k]["us_median"]
        out["color_moments_%s" % k] = {"us_median_both_stages": round(us, 2), "algorithmic_bytes": ab["color_moments_" + k], "TB_per_s": round(ab["color_moments_" + k] / us / 1e6, 3)}
    for k in ("color_apply_style", "luma_merge_planar", "luma_merge_u8"):
        out[k].update(algorithmic_bytes=ab[k], TB_per_s=round(ab[k] / out[k]["us_median"] / 1e6, 3))
    for k, v in meta["copy_bytes_moved"].items():
        out["copy " + k].update(bytes_moved=v, TB_per_s=round(v / out["copy " + k]["us_median"] / 1e6, 3))
    print(json.dumps({"content": [2160, 3840], "style": [2048, 2048], "rounds": meta["rounds"], "warmup_rounds": meta["warmup"], "per_position": out}, indent=1))
    sys.exit(0)

import torch  # noqa: E402
from wct_hip import WCT, model_zoo  # noqa: E402

H, W, Hs, Ws = 2160, 3840, 2048, 2048
w = model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz"))
wct = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=w)
g = torch.Generator(device="cuda").manual_seed(1)
c = torch.rand((1, 3, H, W), device="cuda", generator=g)
s = torch.rand((1, 3, Hs, Ws), device="cuda", generator=g)
leg = sys.argv[1]

if leg == "kernels":
    sty = torch.rand((1, 3, H, W), device="cuda", generator=g)
    nc, sc_, ssc = wct.color_moments(c)
    ns, ss_, sss = wct.color_moments(s)
    A, t = wct.color_solve(nc, sc_, ssc, ns, ss_, sss)
    out_s = torch.empty_like(s)
    out_p = torch.empty_like(c)
    out_b = torch.empty((H, W, 3), device="cuda", dtype=torch.uint8)
    # yardsticks: device copies moving the same bytes (read + write) as each kernel's algorithmic bytes
    px_c, px_s = H * W, Hs * Ws
    byt = {"color_moments_content": 12 * px_c, "color_moments_style": 12 * px_s, "color_apply_style": 24 * px_s,
           "luma_merge_planar": 36 * px_c, "luma_merge_u8": 27 * px_c, "color_solve": 36 * 8}
    cp = {k: (torch.empty(v // 2, device="cuda", dtype=torch.uint8), torch.empty(v // 2, device="cuda", dtype=torch.uint8)) for k, v in byt.items() if v > 1000}

    def round_():
        wct.color_moments(c)
        wct.color_moments(s)
        wct.color_solve(nc, sc_, ssc, ns, ss_, sss)
        wct.color_apply(s, A, t, out=out_s.view(-1))
        wct.luma_merge(sty, c, out=out_p.view(-1))
        wct.luma_merge(sty, c, out=out_b.view(-1), u8=True)
        for k, (a, b) in cp.items():
            b.copy_(a)
    for _ in range(3):
        round_()
    torch.cuda.synchronize()
    for _ in range(20):
        round_()
    torch.cuda.synchronize()
    print("BYTES " + json.dumps({"algorithmic_bytes": byt, "copy_bytes_moved": {k: 2 * a.numel() for k, (a, b) in cp.items()},
                                 "order_per_round": ["color_moments content", "color_moments style", "color_solve", "color_apply style",
                                                     "luma_merge planar", "luma_merge u8"] + ["copy " + k for k in cp], "rounds": 20, "warmup": 3}))
else:
    out = torch.empty((3, H, W), device="cuda")

    def frame(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    plain = lambda: wct.stylize(c, s, out=out)
    legs = {"plain_again": plain, "match": lambda: wct.stylize_color(c, s, "match", out=out), "luma": lambda: wct.stylize_color(c, s, "luma", out=out),
            "match+luma": lambda: wct.stylize_color(c, s, "match+luma", out=out)}
    for fn in [plain] + list(legs.values()):
        for _ in range(3):
            fn()
    res = {}
    med = lambda v: sorted(v)[len(v) // 2]
    for name, fn in legs.items():
        a, b = [], []
        for _ in range(15):
            a.append(frame(plain))
            b.append(frame(fn))
        res[name] = {"stylize_ms_median": round(med(a), 4), "leg_ms_median": round(med(b), 4), "difference_ms": round(med(b) - med(a), 4),
                     "stylize_ms_min_max": [round(min(a), 4), round(max(a), 4)], "leg_ms_min_max": [round(min(b), 4), round(max(b), 4)]}
    assert wct.saturation_count() == 0
    print("FRAMES " + json.dumps({"content": [H, W], "style": [Hs, Ws], "frames_each": 15, "legs": res}))
