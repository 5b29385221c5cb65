"""A/B of the feature transforms on the 4K frame of BASELINE.json configs[1] (3840x2160 content, 2048x2048 style, --mode 16x):
ms per frame of wct, ot and adain from ONE build on ONE box, interleaved (round r times wct, ot, adain in turn, so drift of the box
hits all three alike), for wct_stylize_prepared (cached style) and wct_stylize (style side included).  A plain HIP-event loop:
warm-up, then the median of --rounds frames per mode.  Then, per mode, one profiled frame: the per-kernel ms of the transform's own
families (wct_profile_read) and, per level, info[0] of the content-side solve on THAT frame's features (wct_transform_solve on the
level-isolated content of the cascade), with the count of solves that fell into the Jacobi net (info[0] >= 100).

    python tools/experiments/ab_transform.py [--rounds 12] [--warmup 3] [--out profiles/transform_modes_4k.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "collaborative-distillation_amd")]

H, W, HS, WS = 2160, 3840, 2048, 2048
MODES = ("wct", "ot", "adain")
FAMILIES = ("ot_sandwich", "ot_assemble", "adain_assemble", "matfun_invsqrt", "matfun_sqrt", "assemble_Mb", "fold_affine", "fold_style")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "transform_modes_4k.json"))
    a = ap.parse_args()
    import torch
    from wct_hip import WCT
    g = torch.Generator().manual_seed(4)
    c = torch.rand((1, 3, H, W), generator=g).cuda()
    s = torch.rand((1, 3, HS, WS), generator=g).cuda()
    eng = {m: WCT(types.SimpleNamespace(mode="16x", alpha=1.0, transform=m)) for m in MODES}
    out = {m: torch.empty((3, H, W), device="cuda") for m in MODES}
    res = {"frame": "%dx%d content, %dx%d style, --mode 16x, alpha 1" % (W, H, WS, HS), "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for entry in ("stylize_prepared", "stylize"):
        for m in MODES:
            eng[m].style_prepare(s)
        run = (lambda m: eng[m].stylize_prepared(c, out=out[m])) if entry == "stylize_prepared" else (lambda m: eng[m].stylize(c, s, out=out[m]))
        for _ in range(a.warmup):
            for m in MODES:
                run(m)
        torch.cuda.synchronize()
        ms = {m: [] for m in MODES}
        for _ in range(a.rounds):
            for m in MODES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(m)
                e1.record()
                e1.synchronize()
                ms[m].append(e0.elapsed_time(e1))
        res[entry] = {m: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for m, v in ms.items()}
    res["kernels_ms_per_frame"], res["solve_info_per_level"], res["jacobi_solves"] = {}, {}, {}
    for m in MODES:
        e = eng[m]
        e.profile(True)
        e.profile_reset()
        e.stylize(c, s, out=out[m])
        e.sync()
        res["kernels_ms_per_frame"][m] = {p["name"]: {"ms": p["ms"], "launches": p["launches"]} for p in e.profile_read() if p["name"].split("#")[0] in FAMILIES}
        e.profile(False)
        # the solves of that frame, level by level: the content of level L is the output of level L + 1
        infos, img = {}, c
        for L in (5, 4, 3, 2, 1):
            n, sm, ssq = e.moments(e.encode(L, img, layout="nhwc"))
            _, _, info = e.transform_solve(m, n, sm, ssq, e.style_export(L), want_info=True)
            infos["level%d" % L] = info[0]
            img = e.style_transfer_level(L, img, s)
        res["solve_info_per_level"][m] = infos
        res["jacobi_solves"][m] = sum(1 for v in infos.values() if v >= 100)
    print(json.dumps(res, indent=1))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
