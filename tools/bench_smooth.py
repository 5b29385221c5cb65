"""Measurements for DESIGN.md's smoothing section (tools/bench_smooth.py <leg>).  Three legs, chosen by argv[1]:
  kernels   wct_guided_filter at 3840 x 2160 with r = 16 and r = 64, planar and uint8 output, after a warm-up; torch device copies that
            move each kernel's algorithmic bytes; and the same filter composed from torch fp32 ops (summed-area boxes, adjugate solve), for
            time only -- 10 rounds (run under rocprofv3 --kernel-trace --stats, no counters).  Prints the byte counts as JSON, and the
            error of both arms against the numpy fp64 oracle (tests/smooth_oracle.py) at 600 x 900
  summarise <kernel_trace.csv> <log of the kernels leg>   per-launch medians of that trace by position in the round (the --stats file
            merges launches of one kernel name: both radii, both outputs, all copies)
  frames    stylize_smooth (r = 16, r = 64) against stylize on the same frame, alternating, medians of synchronised frames
"""
import json
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
sys.path[:0] = [REPO, PKG]

RADII = (16, 64)
KERNELS = ("vert<1>", "horiz<1>", "vert<2>", "horiz<2>")
# algorithmic bytes per pixel: every window sample once (its second, leaving read is 2r + 1 rows or columns behind the first)
BYTES_PX = {"vert<1>": 24 + 168, "horiz<1>": 168 + 48, "vert<2>": 48 + 96, "horiz<2> planar": 96 + 12 + 12, "horiz<2> u8": 96 + 12 + 3}

if sys.argv[1] == "summarise":
    import csv
    import re
    meta = json.loads([l for l in open(sys.argv[3]) if l.startswith("BYTES ")][-1][6:])
    errs = json.loads([l for l in open(sys.argv[3]) if l.startswith("ERRORS ")][-1][7:])
    rows = sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Start_Timestamp"]))

    def kind(r):
        m = re.search(r"smooth_(vert|horiz)_kernel<(\d)>", r["Kernel_Name"])
        return "%s<%s>" % m.groups() if m else "copy" if "copyBuffer" in r["Kernel_Name"] else "torch"
    # a round: 16 smoothing launches (r = 16 planar, r = 16 uint8, r = 64 planar, r = 64 uint8), the copies, then the torch arm
    rounds, cur = [], None
    for r in rows:
        k = kind(r)
        if k not in ("copy", "torch") and (cur is None or cur["torch"]):
            cur = {"mine": [], "copy": [], "torch": []}
            rounds.append(cur)
        if cur is not None:
            cur["torch" if k == "torch" else "copy" if k == "copy" else "mine"].append((k, r))
    ncopy = len(meta["copy_bytes_moved"])
    rounds = [c for c in rounds if len(c["mine"]) == 16 and len(c["copy"]) == ncopy][-meta["rounds"]:]
    assert len(rounds) == meta["rounds"], len(rounds)
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    med = lambda v: sorted(v)[len(v) // 2]
    stat = lambda d: {"us_median": round(med(d), 2), "us_min": round(min(d), 2), "us_max": round(max(d), 2), "launches": len(d)}
    px = meta["pixels"]
    out = {}
    for i in range(16):
        radius, form, kn = RADII[i // 8], ("planar", "u8")[(i // 4) % 2], KERNELS[i % 4]
        assert all(c["mine"][i][0] == kn for c in rounds), (i, kn)
        key = kn + (" " + form if kn == "horiz<2>" else "")
        out["r=%d %s %s" % (radius, form, kn)] = dict(stat([us(c["mine"][i][1]) for c in rounds]), algorithmic_bytes=BYTES_PX[key] * px,
                                                      copy_of=key)
    for j, key in enumerate(meta["copy_bytes_moved"]):
        out["copy " + key] = dict(stat([us(c["copy"][j][1]) for c in rounds]), bytes_moved=meta["copy_bytes_moved"][key])
        out["copy " + key]["TB_per_s"] = round(out["copy " + key]["bytes_moved"] / out["copy " + key]["us_median"] / 1e6, 3)
    for k, v in out.items():
        if "copy_of" in v:
            v["TB_per_s"] = round(v["algorithmic_bytes"] / v["us_median"] / 1e6, 3)
            v["copy_us_over_kernel_us"] = round(out["copy " + v["copy_of"]]["us_median"] / v["us_median"], 3)
    whole = {}
    for radius in RADII:
        for form in ("planar", "u8"):
            tot = [sum(us(c["mine"][i][1]) for i in range(16) if RADII[i // 8] == radius and ("planar", "u8")[(i // 4) % 2] == form) for c in rounds]
            cp = sum(out["copy " + (kn + (" " + form if kn == "horiz<2>" else ""))]["us_median"] for kn in KERNELS)
            whole["r=%d %s" % (radius, form)] = dict(stat(tot), copies_us=round(cp, 2), copies_over_filter=round(cp / med(tot), 3))
    torch_arm = {"kernel_us_sum": stat([sum(us(r) for _, r in c["torch"]) for c in rounds]),
                 "first_start_to_last_end_us": stat([(int(c["torch"][-1][1]["End_Timestamp"]) - int(c["torch"][0][1]["Start_Timestamp"])) / 1e3 for c in rounds]),
                 "launches_per_round": len(rounds[0]["torch"]), "radius": meta["torch_radius"]}
    print(json.dumps({"image": meta["image"], "eps": meta["eps"], "rounds": meta["rounds"], "warmup_rounds": meta["warmup"], "per_position": out,
                      "whole_filter": whole, "torch_fp32_composition": torch_arm, "errors_vs_fp64_oracle_600x900": errs}, indent=1))
    sys.exit(0)

import torch  # noqa: E402
from wct_hip import WCT, model_zoo  # noqa: E402

H, W, Hs, Ws, EPS = 2160, 3840, 2048, 2048, 1e-3
w = model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz"))
wct = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=w)
g = torch.Generator(device="cuda").manual_seed(1)
c = torch.rand((1, 3, H, W), device="cuda", generator=g)
leg = sys.argv[1]


def torch_box(x, r):
    """Clipped-window box MEAN of [C, H, W] by fp32 summed areas: the framework composition the library is measured against."""
    for dim in (1, 2):
        n = x.shape[dim]
        cs = torch.cat([torch.zeros_like(x.narrow(dim, 0, 1)), torch.cumsum(x, dim)], dim)
        i = torch.arange(n, device=x.device)
        x = cs.index_select(dim, torch.clamp(i + r, max=n - 1) + 1) - cs.index_select(dim, torch.clamp(i - r, min=0))
    i, j = torch.arange(x.shape[1], device=x.device), torch.arange(x.shape[2], device=x.device)
    ny = torch.clamp(i + r, max=x.shape[1] - 1) - torch.clamp(i - r, min=0) + 1
    nx = torch.clamp(j + r, max=x.shape[2] - 1) - torch.clamp(j - r, min=0) + 1
    return x / (ny[:, None] * nx[None, :]).to(x.dtype)


def torch_guided(p, I, r, eps):
    """The colour-guide filter from torch ops in the dtype of its inputs ([3, H, W]); the 3 x 3 solve by the adjugate."""
    iu = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    m = torch_box(torch.cat([I, p, torch.stack([I[a] * I[b] for a, b in iu]), torch.stack([I[a] * p[b] for a in range(3) for b in range(3)])]), r)
    mI, mp = m[0:3], m[3:6]
    s = {ab: m[6 + k] - mI[ab[0]] * mI[ab[1]] + (eps if ab[0] == ab[1] else 0.0) for k, ab in enumerate(iu)}
    s00, s01, s02, s11, s12, s22 = (s[ab] for ab in iu)
    cov = (m[12:21] - (mI[:, None] * mp[None, :]).reshape(9, *mI.shape[1:])).view(3, 3, *mI.shape[1:])
    c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
    c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
    det = s00 * c00 + s01 * c01 + s02 * c02
    inv = torch.stack([torch.stack([c00, c01, c02]), torch.stack([c01, c11, c12]), torch.stack([c02, c12, c22])]) / det
    a = torch.einsum("ijhw,jchw->ichw", inv, cov)
    b = mp - torch.einsum("ichw,ihw->chw", a, mI)
    mab = torch_box(torch.cat([a.reshape(9, *mI.shape[1:]), b]), r)
    return torch.einsum("ichw,ihw->chw", mab[:9].view(3, 3, *mI.shape[1:]), I) + mab[9:]


if leg == "kernels":
    import numpy as np
    from tests import smooth_oracle as O
    from tests import test_smooth_gpu as G
    errs = {}
    for r, eps in ((8, 1e-6), (60, 1e-4)):      # two shapes of the accuracy test's table: the error of both arms against the fp64 oracle
        src, guide, ref = G.reference(600, 900, r, eps, None)
        ts, tg = torch.from_numpy(src).cuda(), torch.from_numpy(guide).cuda()
        lib_out = wct.guided_filter(ts, tg, r, eps).cpu().numpy()[0].astype(np.float64)
        t_out = torch_guided(ts, tg, r, eps).cpu().numpy().astype(np.float64)
        errs["r=%d eps=%g" % (r, eps)] = {"wct_guided_filter": float(np.abs(lib_out - ref).max()), "torch_fp32_composition": float(np.abs(t_out - ref).max())}
    print("ERRORS " + json.dumps(errs))
    sty = torch.rand((3, H, W), device="cuda", generator=g) * 1.5 - 0.2
    out_p = torch.empty((3, H, W), device="cuda")
    out_b = torch.empty((H, W, 3), device="cuda", dtype=torch.uint8)
    px = H * W
    cp = {k: (torch.empty(v * px // 2, device="cuda", dtype=torch.uint8), torch.empty(v * px // 2, device="cuda", dtype=torch.uint8)) for k, v in BYTES_PX.items()}

    def round_():
        for r in RADII:
            wct.guided_filter(sty, c, r, EPS, out=out_p.view(-1))
            wct.guided_filter(sty, c, r, EPS, out=out_b.view(-1), u8=True)
        for k, (a, b) in cp.items():
            b.copy_(a)
        torch_guided(sty, c[0], RADII[0], EPS)
    for _ in range(2):
        round_()
    torch.cuda.synchronize()
    for _ in range(10):
        round_()
    torch.cuda.synchronize()
    print("BYTES " + json.dumps({"image": [H, W], "pixels": px, "eps": EPS, "radii": RADII, "bytes_per_pixel": BYTES_PX, "torch_radius": RADII[0],
                                 "copy_bytes_moved": {k: 2 * a.numel() for k, (a, b) in cp.items()}, "rounds": 10, "warmup": 2}))
else:
    s = torch.rand((1, 3, Hs, Ws), device="cuda", generator=g)
    out = torch.empty((3, H, W), device="cuda")

    def frame(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    plain = lambda: wct.stylize(c, s, out=out)
    legs = {"plain_again": plain}
    for r in RADII:
        legs["smooth r=%d" % r] = lambda r=r: wct.stylize_smooth(c, s, r, EPS, out=out)
    legs["smooth r=%d luma" % RADII[0]] = lambda: wct.stylize_smooth(c, s, RADII[0], EPS, color="luma", out=out)
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
    print("FRAMES " + json.dumps({"content": [H, W], "style": [Hs, Ws], "eps": EPS, "frames_each": 15, "legs": res}))
