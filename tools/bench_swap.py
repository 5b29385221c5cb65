"""Measurements for DESIGN.md's patch-swap section (tools/bench_swap.py <leg> [out.jsonl]).  Two legs, chosen by argv[1]:
  match      wct_patch_match alone, timed with events: one warm-up, then the median of 10 runs, at
               A   relu4_1 of a 1920 x 1080 content (135 x 240 x 128) against relu4_1 of a 512 x 512 style (64 x 64)
               B4  relu3_1 of a 960 x 540 content (135 x 240 x 64) against relu3_1 of a 1024 x 1024 style (256 x 256): B at a quarter of
                   each edge, the largest of these shapes whose score matrix (8.2 GB) the yardstick can hold
               B   relu3_1 of a 3840 x 2160 content (540 x 960 x 64) against relu3_1 of a 2048 x 2048 style (512 x 512)
             with the achieved TFLOP/s counting the three f16 products (6 * 9C * Nq * Nk flop) and the time of one key-chunk launch
  yardstick  how the method is usually run, on the same GPU: torch conv2d with the (normalised) style patches as filters + argmax over
             the materialised score matrix, fp32, at A and B4; also checks that both arms choose the same patches
Every result is one JSON line on stdout and, with argv[2], appended to that file."""
import json
import os
import sys
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
sys.path[:0] = [REPO, PKG]

import torch  # noqa: E402

SHAPES = {"A": (135, 240, 64, 64, 128), "B4": (135, 240, 256, 256, 64), "B": (540, 960, 512, 512, 64)}      # h, w, hs, ws, C
RUNS = 10


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            f.write(line + "\n")


def maps(name):
    h, w, hs, ws, C = SHAPES[name]
    g = torch.Generator().manual_seed(len(name) + h)
    # whitened features are O(1) and centred
    return torch.randn((1, h, w, C), generator=g).cuda(), torch.randn((1, hs, ws, C), generator=g).cuda()


def timed(fn, runs):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms


def flops(name):
    h, w, hs, ws, C = SHAPES[name]
    return 6.0 * 9 * C * (h - 2) * (w - 2) * (hs - 2) * (ws - 2)


def leg_match():
    from wct_hip import WCT, lib, model_zoo
    eng = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))
    for name in ("A", "B4", "B"):
        h, w, hs, ws, C = SHAPES[name]
        q, k = maps(name)
        t0 = time.time()
        eng.patch_match(q, k)
        torch.cuda.synchronize()
        first = time.time() - t0
        ms = timed(lambda: eng.patch_match(q, k), RUNS)
        nk = (hs - 2) * (ws - 2)
        launches = (nk + lib.SWAP_KEY_CHUNK - 1) // lib.SWAP_KEY_CHUNK
        med = ms[len(ms) // 2]
        emit({"leg": "match", "shape": name, "h": h, "w": w, "hs": hs, "ws": ws, "C": C, "queries": (h - 2) * (w - 2), "keys": nk, "runs": RUNS,
              "first_call_s": round(first, 3), "ms_median": round(med, 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
              "tflops_3_products": round(flops(name) / med / 1e9, 1), "key_chunk": lib.SWAP_KEY_CHUNK, "chunk_launches": launches,
              "ms_per_chunk_launch": round(med / launches, 3)})
    assert eng.saturation_count() == 0


def leg_yardstick():
    from wct_hip import WCT, model_zoo
    import torch.nn.functional as F
    eng = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))
    for name in ("A", "B4"):
        h, w, hs, ws, C = SHAPES[name]
        q, k = maps(name)
        qn = q.permute(0, 3, 1, 2).contiguous()                                              # [1, C, h, w]
        pk = F.unfold(k.permute(0, 3, 1, 2), 3)[0].t().reshape(-1, C, 3, 3)                  # [Nk, C, 3, 3], key index = ky (ws - 2) + kx
        filt = (pk / pk.flatten(1).norm(dim=1).clamp_min(1e-6)[:, None, None, None]).contiguous()

        def run():
            return F.conv2d(qn, filt).argmax(1)

        t0 = time.time()
        ref = run().reshape(-1)
        torch.cuda.synchronize()
        first = time.time() - t0
        ms = timed(run, RUNS)
        med = ms[len(ms) // 2]
        mine = eng.patch_match(q, k).long()
        my_ms = timed(lambda: eng.patch_match(q, k), RUNS)
        my_med = my_ms[len(my_ms) // 2]
        emit({"leg": "yardstick", "shape": name, "arm": "torch conv2d (fp32) + argmax", "score_matrix_GB": round(4.0 * (h - 2) * (w - 2) * pk.shape[0] / 1e9, 2),
              "first_call_s": round(first, 3), "runs": RUNS, "ms_median": round(med, 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
              "tflops_fp32_products": round(flops(name) / 3 / med / 1e9, 1), "wct_patch_match_ms_median": round(my_med, 3),
              "ratio_yardstick_over_patch_match": round(med / my_med, 3), "indices_that_differ": int((ref != mine).sum()), "queries": int(ref.numel())})
        del filt, pk, qn
        torch.cuda.empty_cache()


if __name__ == "__main__":
    {"match": leg_match, "yardstick": leg_yardstick}[sys.argv[1]]()
