"""Measurements for DESIGN.md's device-decode section (tools/bench_jdec.py [out.jsonl] [--no-folder]), under the shipped 16x model:
  1  for the 3840 x 2160 content fixture and its re-encodings at quality 30 / 95: wct_jdec_coefficients, wct_jdec_pixels and
     wct_jdec_decode (device events around each call, warm, the median of RUNS with the smallest and the largest beside it, the arms
     interleaved), the status, whether the pixels are Pillow's, Pillow's decode of the same bytes on one thread in the same process, and
     the bytes that cross PCIe with and without the flag;
  2  the folder run: N 4K pairs, `--pipeline 3 --io_threads 8`, with and without --device_decode, in turn, ROUNDS times each -- without
     the flag the loop is the one the parent commit ran.
The rounds a file needs are a property of the file: tools/jdec_sync_survey.py reports them without a GPU.  The device clock is read
before and after (bench.py's Telemetry).  Every result is one JSON line on stdout and, with a file argument, appended to that file."""
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
from PIL import Image  # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "g11_uhd_content_3840x2160.jpg")
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


def pillow_ms(data):
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        a = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2], a


def folder_run(tele, fixture):
    from wct_hip import cli
    g = torch.Generator().manual_seed(11)
    with tempfile.TemporaryDirectory() as root:
        cdir, sdir = os.path.join(root, "content"), os.path.join(root, "style")
        os.makedirs(cdir)
        os.makedirs(sdir)
        for i in range(PAIRS):      # the photograph, shifted per file so that no two files are the same
            Image.fromarray(np.roll(fixture, (37 * i, 53 * i), (0, 1))).save(os.path.join(cdir, "c%02d.jpg" % i), quality=90)
        Image.fromarray((torch.rand((512, 512, 3), generator=g) * 255).to(torch.uint8).numpy()).save(os.path.join(sdir, "s.png"))
        walls = {"host": [], "device": []}
        files, notes = {}, 0
        for r in range(ROUNDS + 1):              # round 0 warms both arms (code objects, the page cache)
            for arm in ("host", "device"):
                out = os.path.join(root, "out_%s_%d" % (arm, r))
                argv = ["--mode", "16x", "--contentPath", cdir, "--stylePath", sdir, "--outf", out, "--pipeline", "3", "--io_threads", "8"]
                t0 = time.perf_counter()
                assert cli.main(argv + (["--device_decode"] if arm == "device" else [])) == 0
                if r:
                    walls[arm].append((time.perf_counter() - t0) * 1e3 / PAIRS)
                files[arm] = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out)) if f.endswith(".jpg")}
                notes += sum(open(os.path.join(out, f)).read().count("--device_decode:") for f in os.listdir(out) if f.startswith("log_"))
        rec = {"what": "folder run, wall time per pair (engine start-up included)", "pairs": PAIRS, "size": list(fixture.shape[:2]), "pipeline": 3,
               "io_threads": 8, "rounds": ROUNDS, "outputs_byte_identical": files["host"] == files["device"] and len(files["host"]) == PAIRS,
               "files_that_fell_back_to_pillow": notes, "cpus": len(os.sched_getaffinity(0)), "sclk_MHz_after": tele.read_sclk()}
        rec.update(summary("host_decode_per_pair", walls["host"]))
        rec.update(summary("device_decode_per_pair", walls["device"]))
        emit(rec)


def main():
    from bench import Telemetry
    from wct_hip import WCT, lib, model_zoo
    eng = WCT(types.SimpleNamespace(mode="16x", alpha=1.0), weights=model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz")))
    tele = Telemetry(0)
    sclk0 = tele.read_sclk()
    original = open(FIXTURE, "rb").read()
    fixture = np.asarray(Image.open(io.BytesIO(original)).convert("RGB"))
    files = {"fixture": original}
    for q in (30, 95):
        buf = io.BytesIO()
        Image.fromarray(fixture).save(buf, format="JPEG", quality=q)
        files["q%d" % q] = buf.getvalue()
    for name, data in files.items():
        info = eng.jdec_parse(data)
        assert info is not None, name
        H, W = int(info.H), int(info.W)
        scan = torch.from_numpy(np.frombuffer(data, np.uint8, int(info.scan_length), int(info.scan_offset)).copy()).cuda()
        out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        coef, st = eng.jdec_coefficients(scan, info)
        arms = {"coefficients": lambda: eng.jdec_coefficients(scan, info),
                "pixels": lambda: eng.jdec_pixels(coef, info),
                "decode": lambda: eng.jdec_decode_async(scan, info, out=out, status=status)}
        t = interleaved(arms)
        host_ms, ref = pillow_ms(data)
        same = bool((out.cpu().numpy() == ref).all())
        smallest = next((r for r in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32) if int(eng.jdec_coefficients(scan, info, r)[1].item()) == lib.JDEC_STATUS_OK), None)
        rec = {"what": "device JPEG decode", "file": name, "size": [H, W], "file_bytes": len(data), "runs": RUNS, "status": int(status.item()),
               "equals_pillow": same, "smallest_rounds_that_end_ok": smallest, "default_rounds": lib.JDEC_ROUNDS, "launches": lib.JDEC_LAUNCHES,
               "pillow_one_thread_ms": round(host_ms, 2), "h2d_bytes_without_flag": 3 * H * W, "h2d_bytes_with_flag": int(info.scan_length),
               "h2d_bytes_image_over_segment": round(3.0 * H * W / int(info.scan_length), 2), "sclk_MHz_before_after": [sclk0, tele.read_sclk()]}
        for k, ms in t.items():
            rec.update(summary(k, ms))
        emit(rec)
        assert same and int(status.item()) == lib.JDEC_STATUS_OK, "the device pixels differ from Pillow's"
    if "--no-folder" not in sys.argv:
        folder_run(tele, fixture)


if __name__ == "__main__":
    main()
