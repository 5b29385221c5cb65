"""Measurements for DESIGN.md's proxy-mode section (tools/bench_proxy.py [out.jsonl]), under the shipped 16x model:
  1  a device copy of a 3840 x 2160 planar fp32 image (24 B per pixel of traffic): the box's copy bandwidth, what the slice's floor is
     measured against;
  2  for a 3840 x 2160 content, a 2048 x 2048 style and D in 2, 4, 8 (cell, bins, eps, smooth at the command line's defaults):
     wct_bgrid_fit of the reduced pair, wct_bgrid_slice of the full content into planar fp32 and into uint8, wct_stylize_proxy, and
     wct_stylize of the same pair at full size -- what the mode replaces;
  3  one 10240 x 4096 content at D = 4 (no full-size cascade beside it).
Every figure is a host clock around calls that end in a synchronisation of the context's streams, warm, the median of RUNS runs with
the smallest and the largest beside it, the arms of a comparison interleaved run by run, and the device clock read before and after
(bench.py's Telemetry).  Every result is one JSON line on stdout and, with argv[1], appended to that file.  For the kernels' own times
run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_proxy.py`."""
import json
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
sys.path[:0] = [REPO, PKG]

import torch  # noqa: E402

CONTENT, STYLE, WIDE = (2160, 3840), (2048, 2048), (4096, 10240)
DIVISORS = (2, 4, 8)
RUNS, WARM = 11, 2


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(line + "\n")


def wall_ms(eng, fn):
    eng.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    eng.sync()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(name, ms):
    ms = sorted(ms)
    return {name + "_ms_median": round(ms[len(ms) // 2], 3), name + "_ms_min": round(ms[0], 3), name + "_ms_max": round(ms[-1], 3)}


def interleaved(eng, arms):
    """{name: [ms] * RUNS} of the callables in `arms`, run in turn, WARM unrecorded rounds first."""
    out = {k: [] for k in arms}
    for r in range(WARM + RUNS):
        for k, fn in arms.items():
            ms = wall_ms(eng, fn)
            if r >= WARM:
                out[k].append(ms)
    return out


def photo_like(g, shape):
    """A content with a photograph's statistics where they matter here: luminance that varies smoothly across the frame (the fit's z waves
    skip the passes none of whose pixels reach their bin) under fine texture -- noise of a 1/32 grid brought up bicubically, plus 5 % noise."""
    H, W = shape
    low = torch.rand((1, 3, H // 32 + 2, W // 32 + 2), generator=g).cuda()
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    return (0.9 * x + 0.05 * torch.rand((1, 3, H, W), generator=g).cuda()).clamp_(0, 1).contiguous()


def proxy_arms(eng, lib, content, style, D, with_cascade):
    """The arms of one (content, divisor): the parts on their own, the composed call and -- with_cascade -- the full-size cascade."""
    H, W = int(content.shape[2]), int(content.shape[3])
    h, w = eng.scale_shape(H, W, D)
    gh, gw = eng.bgrid_shape(h, w, lib.BGRID_CELL)
    cl = eng.resample(content, (h, w), "bicubic")
    sl = eng.stylize(cl, style).clone()
    grid = eng.bgrid_fit(cl, sl, lib.BGRID_BINS, gh, gw)
    out = torch.empty(3 * H * W, device="cuda")
    out8 = torch.empty(3 * H * W, device="cuda", dtype=torch.uint8)
    gout = torch.empty_like(grid)
    arms = {
        "fit": lambda: eng.bgrid_fit(cl, sl, lib.BGRID_BINS, gh, gw, out=gout.view(-1)),
        "slice_planar": lambda: eng.bgrid_slice(grid, content, out=out),
        "slice_u8": lambda: eng.bgrid_slice(grid, content, out=out8, u8=True),
        "stylize_proxy": lambda: eng.stylize_proxy(content, style, D, out=out),
        "stylize_proxy_u8": lambda: eng.stylize_proxy(content, style, D, out=out8, u8=True),
        "stylize_reduced": lambda: eng.stylize(cl, style),
    }
    if with_cascade:
        full = torch.empty((3, H, W), device="cuda")
        arms["stylize_full"] = lambda: eng.stylize(content, style, out=full)
    return arms, {"content": [H, W], "divisor": D, "working_size": [h, w], "grid_zyx": [lib.BGRID_BINS, gh, gw]}


def main():
    from bench import Telemetry
    from wct_hip import WCT, lib, model_zoo
    eng = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))
    tele = Telemetry(0)
    g = torch.Generator().manual_seed(5)
    content = photo_like(g, CONTENT)
    style = torch.rand((1, 3) + STYLE, generator=g).cuda()
    sclk0 = tele.read_sclk()

    dst = torch.empty_like(content)
    t = interleaved(eng, {"copy": lambda: dst.copy_(content)})
    npix = CONTENT[0] * CONTENT[1]
    copy_ms = sorted(t["copy"])[len(t["copy"]) // 2]
    copy_gbs = 24.0 * npix / copy_ms / 1e6
    rec = {"what": "device copy of a planar fp32 image", "content": list(CONTENT), "bytes_per_pixel": 24, "runs": RUNS, "GB_per_s": round(copy_gbs, 1)}
    rec.update(summary("copy", t["copy"]))
    emit(rec)
    del dst

    for D in DIVISORS:
        arms, rec = proxy_arms(eng, lib, content, style, D, True)
        t = interleaved(eng, arms)
        rec.update({"what": "proxy mode of a 3840x2160 pair", "style": list(STYLE), "runs": RUNS, "content_kind": "photo_like"})
        for k, ms in t.items():
            rec.update(summary(k, ms))
        for k, bpp in (("slice_planar", 24.0), ("slice_u8", 15.0)):
            rec[k + "_fraction_of_floor"] = round(bpp * npix / copy_gbs / 1e6 / rec[k + "_ms_median"], 3)      # floor time at the copy's bandwidth / measured
        rec["sclk_MHz_before_after"] = [sclk0, tele.read_sclk()]
        emit(rec)

    del content
    wide = photo_like(g, WIDE)
    arms, rec = proxy_arms(eng, lib, wide, style, 4, False)
    t = interleaved(eng, arms)
    rec.update({"what": "proxy mode of a 10240x4096 content", "style": list(STYLE), "runs": RUNS})
    for k, ms in t.items():
        rec.update(summary(k, ms))
    wpix = WIDE[0] * WIDE[1]
    for k, bpp in (("slice_planar", 24.0), ("slice_u8", 15.0)):
        rec[k + "_fraction_of_floor"] = round(bpp * wpix / copy_gbs / 1e6 / rec[k + "_ms_median"], 3)
    rec["sclk_MHz_before_after"] = [sclk0, tele.read_sclk()]
    emit(rec)
    assert eng.saturation_count() == 0


if __name__ == "__main__":
    main()
