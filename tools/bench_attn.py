"""Measurements for DESIGN.md's attention-statistics section (tools/bench_attn.py [out.jsonl]): wct_attn_stats and wct_attn_level at levels
5, 4 and 3 of a 3840 x 2160 content with a 2048 x 2048 style under the shipped 16x model,
  L5  135 x 240 queries x 128 x 128 keys, C = 128        L4  270 x 480 x 256 x 256, C = 128        L3  540 x 960 x 512 x 512, C = 64
against a chunked torch fp32 evaluation of the same statistics on the same GPU (scores, softmax, P V and P V^2 per block of queries
whose score block stays under 1 GiB), the two arms interleaved run by run, medians of event timings.  TFLOP/s counts the f16 products
the kernel actually issues: per (query, key) pair 3 split terms over the 32-channel steps of the scores and 2 x 3 over the 16-channel
tiles of the two value operands.  Every result is one JSON line on stdout and, with argv[1], appended to that file."""
import json
import os
import sys
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
sys.path[:0] = [REPO, PKG]

import torch  # noqa: E402

CONTENT, STYLE, TAU = (2160, 3840), (2048, 2048), 8.0
LEVELS = {5: (135, 240, 128, 128, 128), 4: (270, 480, 256, 256, 128), 3: (540, 960, 512, 512, 64)}      # h, w, hs, ws, C
RUNS = {5: 7, 4: 5, 3: 3}


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "a") as f:
            f.write(line + "\n")


def issued_flops(C, nq, nk):
    per_pair = 0.0
    for s in range((C + 127) // 128):
        sc = min(C - 128 * s, 128)
        per_pair += 3.0 * ((C + 31) // 32 * 32) + 6.0 * ((sc + 15) // 16 * 16)
    return 2.0 * per_pair * nq * nk


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def median(ms):
    return sorted(ms)[len(ms) // 2]


def torch_stats(q, k, v, tau):
    nq, nk = q.shape[0], k.shape[0]
    chunk = max(1, (1 << 28) // nk)
    kt, v2 = k.t().contiguous(), v * v
    mean, var = torch.empty_like(q), torch.empty_like(q)
    for i in range(0, nq, chunk):
        p = torch.softmax(tau * (q[i:i + chunk] @ kt), dim=1)
        m = p @ v
        mean[i:i + chunk] = m
        var[i:i + chunk] = (p @ v2 - m * m).clamp_min_(0)
    return mean, var


def main():
    from wct_hip import WCT, model_zoo
    torch.backends.cuda.matmul.allow_tf32 = False
    eng = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))
    g = torch.Generator().manual_seed(5)
    content = torch.rand((1, 3) + CONTENT, generator=g).cuda()
    style = torch.rand((1, 3) + STYLE, generator=g).cuda()
    for level in (5, 4, 3):
        h, w, hs, ws, C = LEVELS[level]
        cF, sF = eng.encode(level, content, layout="nhwc"), eng.encode(level, style, layout="nhwc")
        assert tuple(cF.shape) == (1, h, w, C) and tuple(sF.shape) == (1, hs, ws, C), (cF.shape, sF.shape)
        qhat = eng.attn_project(cF, "attention", want_std=False).reshape(-1, C)
        khat, sstd = (t.reshape(-1, C) for t in eng.attn_project(sF, "attention"))
        del cF, sF
        nq, nk = h * w, hs * ws
        ours = lambda: eng.attn_stats(qhat, khat, sstd, TAU)
        theirs = lambda: torch_stats(qhat, khat, sstd, TAU)
        (m0, v0), (m1, v1) = ours(), theirs()                   # warm-up of both arms, and how far apart they are
        torch.cuda.synchronize()
        diff = (float((m0 - m1).abs().max() / sstd.abs().max()), float((v0 - v1).abs().max() / sstd.abs().max() ** 2))
        del m0, v0, m1, v1
        a, b = [], []
        for _ in range(RUNS[level]):
            a.append(event_ms(ours))
            b.append(event_ms(theirs))
        lv = [event_ms(lambda: eng.attn_level(level, content, style, "attention", TAU)) for _ in range(1 + RUNS[level])][1:]
        fl = issued_flops(C, nq, nk)
        emit({"level": level, "queries": nq, "keys": nk, "C": C, "tau": TAU, "runs": RUNS[level],
              "attn_stats_ms_median": round(median(a), 2), "attn_stats_ms_min": round(min(a), 2), "attn_stats_ms_max": round(max(a), 2),
              "tflops_issued_products": round(fl / median(a) / 1e9, 1),
              "torch_fp32_chunked_ms_median": round(median(b), 2), "torch_ms_min": round(min(b), 2), "torch_ms_max": round(max(b), 2),
              "ratio_torch_over_attn_stats": round(median(b) / median(a), 3),
              "max_diff_mean_rel": diff[0], "max_diff_var_rel": diff[1],
              "attn_level_ms_median": round(median(lv), 2), "attn_level_ms_min": round(min(lv), 2), "attn_level_ms_max": round(max(lv), 2)})
        del qhat, khat, sstd
        torch.cuda.empty_cache()
    assert eng.saturation_count() == 0


if __name__ == "__main__":
    main()
