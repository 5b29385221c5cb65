"""Measurements for DESIGN.md's device-JPEG section (tools/bench_jpeg.py [out.jsonl] [--no-folder]), under the shipped 16x model, at
3840 x 2160:
  1  a device copy of the uint8 image (2 x 24.9 MB of traffic): the box's copy bandwidth, what the encoder's traffic is set against;
  2  for a stylised sample frame, a smooth ramp and uniform noise at quality 75: wct_jpeg_blocks, wct_jpeg_pack and wct_jpeg_encode
     (device events around each call, warm, the median of RUNS with the smallest and the largest beside it, the arms interleaved), the
     file's size, the bytes each entry has to move, and Pillow's encode of the same array on one thread in the same process;
  3  the folder run: N 4K pairs, `--pipeline 3 --io_threads 8`, with and without --device_jpeg, in turn, ROUNDS times each -- without
     the flag the loop is the one the parent commit ran.
The device clock is read before and after (bench.py's Telemetry).  Every result is one JSON line on stdout and, with a file argument,
appended to that file.  For the kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_jpeg.py --no-folder`."""
import io
import json
import os
import sys
import tempfile
import time
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "collaborative-distillation_amd")
sys.path[:0] = [REPO, PKG]

import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 2160, 3840
QUALITY = 75
RUNS, WARM = 11, 3
PAIRS, ROUNDS = 32, 3
OUT = next((a for a in sys.argv[1:] if not a.startswith("--")), None)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def interleaved(arms):
    out = {k: [] for k in arms}
    for r in range(WARM + RUNS):
        for k, fn in arms.items():
            ms = event_ms(fn)
            if r >= WARM:
                out[k].append(ms)
    return out


def summary(name, ms):
    ms = sorted(ms)
    return {name + "_ms_median": round(ms[len(ms) // 2], 4), name + "_ms_min": round(ms[0], 4), name + "_ms_max": round(ms[-1], 4)}


def photo_like(g, h, w):
    low = torch.rand((1, 3, h // 32 + 2, w // 32 + 2), generator=g)
    x = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)
    return (0.9 * x + 0.05 * torch.rand((1, 3, h, w), generator=g)).clamp_(0, 1).contiguous()


def pillow_ms(a):
    from PIL import Image
    ms = []
    for _ in range(5):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        Image.fromarray(a).save(buf, format="JPEG", quality=QUALITY)
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2], buf.getvalue()


def folder_run(tele):
    from PIL import Image
    from wct_hip import cli
    g = torch.Generator().manual_seed(11)
    with tempfile.TemporaryDirectory() as root:
        cdir, sdir = os.path.join(root, "content"), os.path.join(root, "style")
        os.makedirs(cdir)
        os.makedirs(sdir)
        for i in range(PAIRS):
            a = (photo_like(g, H, W)[0].permute(1, 2, 0) * 255).to(torch.uint8).numpy()
            Image.fromarray(a).save(os.path.join(cdir, "c%02d.jpg" % i), quality=90)
        Image.fromarray((torch.rand((512, 512, 3), generator=g) * 255).to(torch.uint8).numpy()).save(os.path.join(sdir, "s.png"))
        walls = {"host": [], "device": []}
        files = {}
        for r in range(ROUNDS + 1):              # round 0 warms both arms (code objects, the page cache)
            for arm in ("host", "device"):
                out = os.path.join(root, "out_%s_%d" % (arm, r))
                argv = ["--mode", "16x", "--contentPath", cdir, "--stylePath", sdir, "--outf", out, "--pipeline", "3", "--io_threads", "8"]
                t0 = time.perf_counter()
                assert cli.main(argv + (["--device_jpeg"] if arm == "device" else [])) == 0
                if r:
                    walls[arm].append((time.perf_counter() - t0) * 1e3 / PAIRS)
                files[arm] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f.endswith(".jpg")}
        rec = {"what": "folder run, wall time per pair (engine start-up included)", "pairs": PAIRS, "size": [H, W], "pipeline": 3, "io_threads": 8,
               "rounds": ROUNDS, "outputs_byte_identical": files["host"] == files["device"] and len(files["host"]) == PAIRS,
               "cpus": len(os.sched_getaffinity(0)), "sclk_MHz_after": tele.read_sclk()}
        rec.update(summary("host_encode_per_pair", walls["host"]))
        rec.update(summary("device_jpeg_per_pair", walls["device"]))
        emit(rec)


def main():
    from bench import Telemetry
    from wct_hip import WCT, model_zoo
    eng = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))
    tele = Telemetry(0)
    sclk0 = tele.read_sclk()
    g = torch.Generator().manual_seed(5)

    src = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g).cuda()
    dst = torch.empty_like(src)
    t = interleaved({"copy": lambda: dst.copy_(src)})
    copy_ms = sorted(t["copy"])[len(t["copy"]) // 2]
    copy_gbs = 2.0 * src.numel() / copy_ms / 1e6
    rec = {"what": "device copy of a uint8 image", "size": [H, W], "bytes_moved": 2 * src.numel(), "runs": RUNS, "GB_per_s": round(copy_gbs, 1)}
    rec.update(summary("copy", t["copy"]))
    emit(rec)

    stylised = eng.to_u8(eng.stylize(photo_like(g, H, W).cuda(), torch.rand((1, 3, 512, 512), generator=g).cuda()))
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([(yy * 5 + xx * 3) // 64 % 256, (xx * 7) // 64 % 256, (yy * 11 / 64 + 40 * np.sin(xx / 300.0)) % 256], -1).astype(np.uint8)
    images = {"stylised": stylised, "ramp": torch.from_numpy(ramp).cuda(), "noise": src}
    nb = eng.jpeg_num_blocks(H, W)
    out = torch.empty(eng.jpeg_bound(H, W), dtype=torch.uint8, device="cuda")
    length = torch.zeros(1, dtype=torch.int64, device="cuda")
    for name, x in images.items():
        coef = eng.jpeg_blocks(x, QUALITY)
        arms = {"blocks": lambda: eng.jpeg_blocks(x, QUALITY),
                "pack": lambda: eng.jpeg_pack(coef, H, W, out=out, length=length),
                "encode": lambda: eng.jpeg_encode_async(x, QUALITY, out=out, length=length)}
        t = interleaved(arms)
        n = int(length.item())
        host_ms, ref = pillow_ms(x.cpu().numpy())
        same = out[:n].cpu().numpy().tobytes() == ref
        # what has to move: blocks reads the image and writes the coefficients; pack reads them twice (count, pack), writes the stream,
        # reads it twice (count, scatter) and writes the file
        moved = {"blocks": 3 * H * W + 128 * nb, "pack": 2 * 128 * nb + 4 * n}
        moved["encode"] = moved["blocks"] + moved["pack"]
        rec = {"what": "device JPEG encode", "image": name, "size": [H, W], "quality": QUALITY, "runs": RUNS, "file_bytes": n,
               "equals_pillow": same, "pillow_one_thread_ms": round(host_ms, 2), "copy_GB_per_s": round(copy_gbs, 1)}
        for k, ms in t.items():
            rec.update(summary(k, ms))
            rec[k + "_bytes_moved"] = moved[k]
            rec[k + "_floor_ms_at_copy_bandwidth"] = round(moved[k] / copy_gbs / 1e6, 4)
        rec["d2h_bytes_image_over_file"] = round(3.0 * H * W / n, 2)
        rec["sclk_MHz_before_after"] = [sclk0, tele.read_sclk()]
        emit(rec)
        assert same, "the device file differs from Pillow's"
    assert eng.saturation_count() == 0
    if "--no-folder" not in sys.argv:
        folder_run(tele)


if __name__ == "__main__":
    main()
