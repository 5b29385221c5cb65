"""Measurements for DESIGN.md's scale-control section (tools/bench_scale.py [out.jsonl]): a 3840 x 2160 content, a 2048 x 2048 style,
--mode 16x, divisors (4, 4, 2, 1, 1), detail gain 1.
  families   every profile family of the resampler and the merge inside wct_stylize_scaled (an event pair around each, 10 calls): ms per
             launch as wct_profile_read reports it -- the pair's own cost included, which at these lengths is most of it
  ops        the four operations those families are made of at this size, each through its public C entry 20 times back to back
             between two events: ms, the achieved GB/s on its algorithmic bytes, and beside it a device-to-device hipMemcpyAsync
             that moves the SAME traffic (half the bytes, read once and written once) timed the same way in the same process
  frame      wct_stylize_scaled beside wct_stylize, interleaved, each frame synchronised on its own: median of 20, min, max
The device's clock and power during the timed part come from bench.py's Telemetry.  Every result is one JSON line on stdout and, with
argv[1], appended to that file."""
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
DIV, GAIN = (4, 4, 2, 1, 1), 1.0
FAMILIES = ("resample<", "pyramid_merge")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(line + "\n")


def hip_runtime():
    """The libamdhip64 this process already runs on (torch's), by its mapped path."""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return ctypes.CDLL(ln.split()[-1])
    raise RuntimeError("no libamdhip64 is mapped")


def copy_ms(hip, nbytes, runs=20):
    """ms of one device-to-device hipMemcpyAsync of nbytes: `runs` in a row between two events, after one warm-up."""
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.fill_(7)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    go = lambda: hip.hipMemcpyAsync(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src.data_ptr()), ctypes.c_size_t(nbytes), 3, st)   # noqa: E731
    assert go() == 0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(runs):
        assert go() == 0
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / runs


def profile_all(eng):
    from wct_hip import lib
    n = ctypes.c_int()
    eng._chk(eng._lib.wct_profile_read(eng._ctx, None, 0, ctypes.byref(n)))
    buf = (lib.WctProfEntry * max(n.value, 1))()
    eng._chk(eng._lib.wct_profile_read(eng._ctx, buf, n.value, ctypes.byref(n)))
    return [buf[i] for i in range(n.value)]


def main():
    import bench
    from wct_hip import WCT, model_zoo
    eng = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))
    g = torch.Generator().manual_seed(5)
    c, s = torch.rand((1, 3, H, W), generator=g).cuda(), torch.rand((1, 3, HS, WS), generator=g).cuda()
    out = torch.empty((3, H, W), device="cuda")
    plain = lambda: eng.stylize(c, s, out=out)                              # noqa: E731
    scaled = lambda: eng.stylize_scaled(c, s, DIV, GAIN, out=out)           # noqa: E731
    for _ in range(3):
        plain()
        scaled()
    torch.cuda.synchronize()
    tele = bench.Telemetry(0)
    tele.start()
    t_end = time.time() + 2.0                                               # settle the clocks on the workload itself
    while time.time() < t_end:
        scaled()
        torch.cuda.synchronize()

    ms = {"stylize": [], "stylize_scaled": []}
    for _ in range(20):
        for name, fn in (("stylize", plain), ("stylize_scaled", scaled)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    frame = {}
    for name, v in ms.items():
        v.sort()
        frame[name] = {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}

    eng.profile(True)
    eng.profile_reset()
    for _ in range(10):
        scaled()
    torch.cuda.synchronize()
    recs = profile_all(eng)
    eng.profile(False)
    hip = hip_runtime()
    fams = [{"family": r.name.decode(), "launches_per_call": r.launches / 10, "bytes_per_launch": int(r.bytes / r.launches),
             "ms_per_launch": round(r.ms / r.launches, 4)} for r in recs if r.name.decode().startswith(FAMILIES)]
    ops = []
    sizes = {d: eng.scale_shape(H, W, d) for d in (4, 2, 1)}
    F = {d: eng.resample(c, sizes[d], "bicubic") for d in (4, 2)}
    F[1] = c
    L, ctx, P = eng._lib, eng._ctx, lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for name, call, nbytes in [
            ("resample<bicubic,down> %dx%d -> %dx%d" % ((H, W) + sizes[d]),
             (lambda d=d: L.wct_resample_planar(ctx, P(c), H, W, P(out), sizes[d][0], sizes[d][1], 1)), 12 * (H * W + sizes[d][0] * sizes[d][1]))
            for d in (4, 2)] + [
            ("pyramid_merge %dx%d -> %dx%d" % (sizes[a] + sizes[b]),
             (lambda a=a, b=b: L.wct_pyramid_merge(ctx, P(F[a]), P(F[a]), sizes[a][0], sizes[a][1], P(F[b]), sizes[b][0], sizes[b][1], GAIN, P(out))),
             12 * (2 * sizes[a][0] * sizes[a][1] + 2 * sizes[b][0] * sizes[b][1])) for a, b in ((4, 2), (2, 1))]:
        eng._stream()
        assert call() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            assert call() == 0
        e1.record()
        e1.synchronize()
        ms_op = e0.elapsed_time(e1) / 20
        cms = copy_ms(hip, nbytes // 2)
        ops.append({"op": name, "bytes": nbytes, "ms": round(ms_op, 4), "GBps": round(nbytes / ms_op / 1e6, 1), "copy_same_traffic_ms": round(cms, 4),
                    "copy_GBps": round(nbytes / cms / 1e6, 1), "share_of_copy_rate": round(cms / ms_op, 3)})
    telemetry = tele.stop()
    assert eng.saturation_count() == 0
    emit({"leg": "frame", "content": [H, W], "style": [HS, WS], "divisors": DIV, "detail_gain": GAIN, "runs": 20,
          "frame": frame, "ratio_scaled_over_plain": round(frame["stylize_scaled"]["ms_median"] / frame["stylize"]["ms_median"], 3),
          "telemetry": telemetry})
    emit({"leg": "families", "calls": 10, "families": fams})
    emit({"leg": "ops", "runs": 20, "ops": ops, "ms_per_cascade": round(sum(o["ms"] for o in ops), 4)})


if __name__ == "__main__":
    main()
