"""The synchronisation survey behind WCT_JDEC_ROUNDS (tools/jdec_sync_survey.py [out.json]): for the 3840 x 2160 content fixture, the
2048 x 2048 style fixture and their re-encodings at quality 30 / 75 / 95, the smallest `rounds` at which the schedule of
include/wct_hip_jdec.h (restated by tests/jdec_oracle.py, no GPU) ends with every stored state in place, and the rounds each launch
runs at the default.  The property is the file's, not the machine's.  One JSON record per file on stdout; with a file argument, the
list as one document."""
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "collaborative-distillation_amd")]

from PIL import Image  # noqa: E402

from tests import jdec_oracle as jd  # noqa: E402

FIXTURES = ("g11_uhd_content_3840x2160.jpg", "g11_style_2048x2048.jpg")
LADDER = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 128, 256)


def files():
    for name in FIXTURES:
        data = open(os.path.join(REPO, "tests", "golden", name), "rb").read()
        yield name, data
        img = Image.open(io.BytesIO(data)).convert("RGB")
        for q in (30, 75, 95):
            buf = io.BytesIO()
            img.save(buf, format="JPEG", quality=q)
            yield "%s@q%d" % (name, q), buf.getvalue()


def main():
    out = []
    for name, data in files():
        t0 = time.time()
        d = jd.decoder(data)
        need = next((r for r in LADDER if d.schedule(r)[0]), None)
        synced, used = d.schedule(jd.ROUNDS)
        rec = {"file": name, "bytes": len(data), "subsequences": d.nsub, "workgroups": -(-d.nsub // jd.SYNC_THREADS), "launches": jd.LAUNCHES,
               "smallest_rounds_on_ladder": need, "ladder": list(LADDER), "default_rounds": jd.ROUNDS, "ok_at_default": synced,
               "rounds_run_per_launch_at_default": used, "seconds": round(time.time() - t0, 1)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
