"""Measurements for DESIGN.md's region-to-region section (tools/bench_guided.py [out.json]): a 3840 x 2160 content, a 2048 x 2048 style,
--mode 16x.
  frames   wct_feature_regions at levels 2 and 4 (K = 8, 10 iterations), wct_stylize_guided (K = 3, one mapped style), wct_stylize_regions
           with three whole styles, and wct_stylize twice (the second against the first is the noise floor): interleaved in one process,
           each frame synchronised on its own, median of 15, min, max
  assign   the profile families of the k-means passes inside wct_feature_regions (an event pair around each launch group, 5 calls): ms
           per pass and the achieved GB/s of the assign pass on the bytes it reads from HBM (the map once)
The result is one JSON document on stdout and, with argv[1], in that file."""
import ctypes
import json
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
sys.path[:0] = [REPO, PKG]

import torch  # noqa: E402

H, W, HS, WS = 2160, 3840, 2048, 2048
RUNS = 15


def profile_all(eng):
    from wct_hip import lib
    n = ctypes.c_int()
    eng._chk(eng._lib.wct_profile_read(eng._ctx, None, 0, ctypes.byref(n)))
    buf = (lib.WctProfEntry * max(n.value, 1))()
    eng._chk(eng._lib.wct_profile_read(eng._ctx, buf, n.value, ctypes.byref(n)))
    return [buf[i] for i in range(n.value)]


def main():
    from wct_hip import WCT, model_zoo
    eng = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))
    g = torch.Generator().manual_seed(5)
    c, s = torch.rand((1, 3, H, W), generator=g).cuda(), torch.rand((1, 3, HS, WS), generator=g).cuda()
    s2, s3 = torch.rand((1, 3, HS, WS), generator=g).cuda(), torch.rand((1, 3, HS, WS), generator=g).cuda()
    out = torch.empty((3, H, W), device="cuda")
    lab = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    lab[:, W // 3:] = 1
    lab[H // 2:, 2 * W // 3:] = 2
    slab = torch.zeros((HS, WS), dtype=torch.uint8, device="cuda")
    slab[:, WS // 3:] = 1
    slab[HS // 2:, 2 * WS // 3:] = 2
    legs = [
        ("stylize", lambda: eng.stylize(c, s, out=out)),
        ("stylize_again", lambda: eng.stylize(c, s, out=out)),
        ("stylize_regions_3_styles", lambda: eng.stylize_regions(c, [s, s2, s3], lab, 1.0, out=out)),
        ("stylize_guided_1_mapped_style", lambda: eng.stylize_guided(c, [s], lab, [slab], [0, 0, 0], 1.0, out=out)),
        ("feature_regions_level2", lambda: eng.feature_regions(c, s, 8, 2, 10)),
        ("feature_regions_level4", lambda: eng.feature_regions(c, s, 8, 4, 10)),
    ]
    for _ in range(2):
        for _, fn in legs:
            fn()
    torch.cuda.synchronize()
    t_end = time.time() + 2.0                                               # settle the clocks on the workload itself
    while time.time() < t_end:
        legs[0][1]()
        torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for _ in range(RUNS):
        for name, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    frames = {}
    for name, v in ms.items():
        v.sort()
        frames[name] = {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}
    assign = {}
    for level in (2, 4):
        eng.profile(True)
        eng.profile_reset()
        for _ in range(5):
            eng.feature_regions(c, s, 8, level, 10)
        torch.cuda.synchronize()
        recs = profile_all(eng)
        eng.profile(False)
        C, hs, ws = eng.feature_shape(level, HS, WS)
        fams = {}
        for r in recs:
            name = r.name.decode()
            if name.startswith("kmeans"):
                fams[name] = {"launch_groups_per_call": r.launches / 5, "ms_per_group": round(r.ms / r.launches, 4),
                              "bytes_per_group": int(r.bytes / r.launches), "GBps": round(r.bytes / r.ms / 1e6, 1)}
        assign["level%d" % level] = {"C": C, "style_map": [hs, ws], "families": fams}
    assert eng.saturation_count() == 0
    doc = {"content": [H, W], "style": [HS, WS], "mode": "16x", "runs": RUNS, "frames": frames,
           "noise_floor_ms": round(abs(frames["stylize"]["ms_median"] - frames["stylize_again"]["ms_median"]), 3), "kmeans": assign,
           "note": "kmeans_assign groups are the assign kernel plus its two small reductions; the family mixes the 11 style-map passes with the one content-map pass"}
    text = json.dumps(doc, indent=1)
    print(text, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
