"""The device JPEG decoder without a GPU: the oracle (tests/jdec_oracle.py) against Pillow pixel for pixel, the host-only parser
wct_jdec_parse against the oracle's and under the host sanitizers, its refusals, the schedule's restatement, and the edge cases' claims."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest

from tests import jdec_cases as jc
from tests import jdec_oracle as jd
from tests import jpeg_oracle as jo
from tests.conftest import PKG, REPO
from wct_hip import lib as _lib


@pytest.mark.parametrize("case", jc.CASES, ids=jc.case_id)
def test_oracle_equals_pillow_and_the_parser_the_oracle(case):
    from wct_hip import WCT
    data = jc.case_bytes(case)
    px, status = jd.decode(data)
    assert status == jd.OK
    assert np.array_equal(px, jd.pillow_pixels(data))
    f, info = jd.parse(data), WCT.jdec_parse(data)
    assert info is not None
    for name in ("H", "W", "ncomp", "restart_interval", "scan_offset", "scan_length"):
        assert getattr(info, name) == f[name], name
    for name in ("hs", "vs", "tq", "td", "ta"):
        assert list(getattr(info, name))[:f["ncomp"]] == f[name][:f["ncomp"]], name
    for name in ("qt", "dc_counts", "dc_vals", "ac_counts", "ac_vals"):
        assert np.array_equal(np.ctypeslib.as_array(getattr(info, name)), f[name]), name
    assert WCT.jdec_num_blocks(info) == jd.geometry(f)["blocks"]


def test_cases_cover_the_variants_and_the_qualities():
    assert len(jc.CASES) == 99 and len(set(jc.CASES)) == 99
    assert {c[4] for c in jc.CASES} >= {1, 100}
    infos = [jd.parse(jc.case_bytes(c)) for c in jc.CASES]
    assert {(f["ncomp"], f["hs"][0], f["vs"][0]) for f in infos} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert any(f["restart_interval"] for f in infos)
    assert any(not np.array_equal(f["ac_counts"][0], jo.AC_Y[0]) for f in infos), "an optimised Huffman table"


def refused(data):
    from wct_hip import WCT
    with pytest.raises(jd.Unsupported):
        jd.parse(data)
    return WCT.jdec_parse(data) is None


def test_parser_refuses_by_name():
    from PIL import Image
    a = jo.make_image(24, 40, "smooth")
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", progressive=True)
    assert refused(buf.getvalue()), "progressive"
    buf = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(buf, format="JPEG")
    assert refused(buf.getvalue()), "CMYK"
    good = jc.save(a, 75, subsampling=2)
    assert not refused_quietly(good)
    adobe = good[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + good[2:]
    assert refused(adobe), "an Adobe APP14 segment"
    comment = good[:2] + b"\xff\xfe\x00\x05abc" + good[2:]
    assert not refused_quietly(comment), "COM segments are skipped"
    assert refused(good.replace(b"\xff\xc0\x00\x11\x08", b"\xff\xc1\x00\x11\x08")), "extended sequential"
    assert refused(good.replace(b"\xff\xc0\x00\x11\x08", b"\xff\xc0\x00\x11\x0c")), "12 bit"
    assert refused(good[:-2] + b"\xff\xda" + good[-2:]), "something other than EOI behind the scan"
    sof = good.index(b"\xff\xc0")
    assert refused(good[:sof + 11] + b"\x41" + good[sof + 12:]), "4 x 1 sampling"
    # components named 'R', 'G', 'B' and no JFIF segment: libjpeg reads RGB, without the colour conversion
    sos = good.index(b"\xff\xda")
    assert good[2:4] == b"\xff\xe0" and good[6:11] == b"JFIF\0" and (good[sof + 10], good[sof + 13], good[sof + 16]) == (1, 2, 3)
    named = bytearray(good)
    for k, c in enumerate(b"RGB"):
        named[sof + 10 + 3 * k] = named[sos + 5 + 2 * k] = c
    named = bytes(named)
    assert not refused_quietly(named), "with its JFIF segment the file is YCbCr whatever the ids"
    app0 = 4 + (good[4] << 8 | good[5])
    assert refused(named[:2] + named[app0:]), "R, G, B without JFIF"
    assert not refused_quietly(good[:2] + good[app0:]), "ids 1, 2, 3 without JFIF are YCbCr"
    assert np.array_equal(jd.decode(good[:2] + good[app0:])[0], jd.pillow_pixels(good[:2] + good[app0:]))
    assert not np.array_equal(jd.pillow_pixels(named[:2] + named[app0:]), jd.pillow_pixels(good)), "Pillow does read that file as RGB"


def refused_quietly(data):
    from wct_hip import WCT
    return WCT.jdec_parse(data) is None


def test_every_truncation_is_refused_and_writes_nothing():
    data = jc.case_bytes((9, 7, "noise", "420opt", 30))
    L = _lib.load()
    for n in range(len(data)):
        info = _lib.WctJdecInfo()
        ctypes.memset(ctypes.byref(info), 0xA5, ctypes.sizeof(info))
        assert L.wct_jdec_parse(data[:n], n, ctypes.byref(info)) == _lib.JDEC_UNSUPPORTED, n
        assert bytes(info) == b"\xa5" * ctypes.sizeof(info), n
        with pytest.raises(jd.Unsupported):
            jd.parse(data[:n])
    assert L.wct_jdec_parse(None, 4, ctypes.byref(_lib.WctJdecInfo())) == _lib.WCT_ERR_INVALID
    assert L.wct_jdec_parse(data, len(data), None) == _lib.WCT_ERR_INVALID
    # no context: the device entries refuse before they touch anything
    assert L.wct_jdec_coefficients(None, 1, None, 0, 16, 4) == _lib.WCT_ERR_INVALID
    assert L.wct_jdec_pixels(None, 16, None, 1) == _lib.WCT_ERR_INVALID
    assert L.wct_jdec_decode(None, 1, None, 0, 1, 4) == _lib.WCT_ERR_INVALID


def test_parser_under_the_host_sanitizers(tmp_path):
    """tests/jdec_parse_main.cpp, its own main, built with the sanitizers and run as a child: every prefix and every single-byte
    corruption of three small files.  The sanitizers' runtimes are linked statically, so the program asks nothing of the order in
    which the environment loads libraries and runs in whatever environment the suite has.  Skipped only where a trivial main does not
    link and run with the flags."""
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    (tmp_path / "t.cpp").write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + flags + [str(tmp_path / "t.cpp"), "-o", str(tmp_path / "t")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "t")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot link or run a trivial main with -fsanitize=address,undefined and the static runtimes")
    exe = tmp_path / "jdec_parse_main"
    r = subprocess.run(["g++"] + flags + [os.path.join(REPO, "tests", "jdec_parse_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    names = []
    for i, case in enumerate([(9, 7, "noise", "420opt", 30), (1, 1, "noise", "grey", 50), (18, 34, "noise", "422opt-rb1", 90)]):
        names.append(str(tmp_path / ("f%d.jpg" % i)))
        open(names[-1], "wb").write(jc.case_bytes(case))
    r = subprocess.run([str(exe)] + names, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.split("\n")[:3]
    # every prefix is refused; a corrupted table entry or scan byte is still a file
    assert len(lines) == 3 and all(int(l.split()[2]) >= os.path.getsize(n) and int(l.split()[1]) > 0 for l, n in zip(lines, names)), r.stdout


def test_header_symbol_list_and_library_agree():
    text = open(os.path.join(REPO, "include", "wct_hip_jdec.h")).read()
    declared = sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", text)) - {"wct_ctx"})
    assert declared == sorted(_lib.SYMBOLS_JDEC)
    others = [getattr(_lib, n) for n in dir(_lib) if n.startswith("SYMBOLS") and n != "SYMBOLS_JDEC"]
    assert not set(_lib.SYMBOLS_JDEC) & {s for o in others for s in o}
    L = _lib.load()
    assert all(hasattr(L, s) for s in _lib.SYMBOLS_JDEC)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(_lib.SYMBOLS_JDEC) <= exported
    assert not [s for s in exported if "jdec" in s.lower() and s not in _lib.SYMBOLS_JDEC], "the launchers and kernels stay inside the library"
    for name in ("UNSUPPORTED", "SUBSEQ_BITS", "SYNC_THREADS", "LAUNCHES", "ROUNDS", "MAX_ROUNDS", "CHUNK", "SCAN_CHUNK", "DC_TILE", "MAX_DIM"):
        m = re.search(r"#define WCT_JDEC_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(_lib, "JDEC_" + name), name
    for name, value in (("OK", jd.OK), ("UNSYNC", jd.UNSYNC), ("CORRUPT", jd.CORRUPT)):
        m = re.search(r"#define WCT_JDEC_STATUS_%s (\d+)u" % name, text)
        assert m and int(m.group(1)) == value == getattr(_lib, "JDEC_STATUS_" + name)
    assert (jd.SUBSEQ_BITS, jd.SYNC_THREADS, jd.LAUNCHES, jd.ROUNDS) == (_lib.JDEC_SUBSEQ_BITS, _lib.JDEC_SYNC_THREADS, _lib.JDEC_LAUNCHES, _lib.JDEC_ROUNDS)
    assert ctypes.sizeof(_lib.WctJdecInfo) == 960
    assert "jdec" in open(os.path.join(PKG, "build.sh")).read()


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------

# The synchronisation study's table: S = 1024 bits, whole-stream Jacobi rounds to the fixpoint; per file the subsequences, the wrong exit
# states after the initial guesses and after each round (as far as the study lists them), and the rounds to the fixpoint.  `same`: the
# file is rebuilt here bit for bit (the subsequence count proves it); the photograph rows are a 640 x 480 crop of the 4K fixture whose
# window the study does not name, so those are rows of another picture of the same scene.
STUDY = [
    ("crop-q75-420", lambda: jc.photo_crop(75), False, 451, [163, 81, 36, 16, 9, 4, 2, 1], 8),
    ("crop-q30-420", lambda: jc.photo_crop(30), False, 231, [70, 16, 2], 3),
    ("crop-q95-444-opt", lambda: jc.photo_crop(95, subsampling=0, optimize=True), False, 1184, [5], 1),
    ("smooth-320-opt", jc.smooth_opt, True, 206, [132, 90, 65, 46], 17),
    ("noise-128-q100-420", jc.noise_q100, True, 252, [246, 238, 233], 104),
    ("flat-320-opt", lambda: jc.flat(True), True, 5, [4, 3, 2, 1], 4),
    ("flat-320-standard", jc.flat_standard, True, 13, [12, 11, 10], 12),
]


@pytest.mark.parametrize("row", STUDY, ids=lambda r: r[0])
def test_schedule_simulation_reproduces_the_study(row):
    """Tolerances, and where they come from.  The study counted a state wrong by its own bookkeeping; this oracle's definition differs
    in two places that can move a count by a subsequence or two -- bits at or beyond an anchor read as 1 and no symbol crosses one (the
    stream's end is an anchor), and a state is (p, b, z) compared whole.  So on a rebuilt file: the subsequence count exact, every listed
    wrong count within 2, the rounds exact for the flat and noise files (there the round count is the length of a chain, which no
    bookkeeping changes) and within 3 for the smooth file (17 listed, its tail of one or two stragglers is what the definition moves).
    On the photograph rows, another crop window: subsequences within 6 %, rounds within 1, the first wrong count within a third, and
    the decay the study shows -- each round leaves at most 0.6 of the wrong states while 8 or more are left."""
    name, make, same, nsub, listed, rounds = row
    d = jd.decoder(make())
    wrong = d.jacobi()
    print(name, "subsequences", d.nsub, "wrong per round", wrong, "rounds", len(wrong) - 1)
    assert wrong[-1] == 0 and all(b <= a for a, b in zip(wrong, wrong[1:]))
    if same:
        assert d.nsub == nsub
        assert all(abs(a - b) <= 2 for a, b in zip(wrong, listed)), (wrong[:len(listed)], listed)
        assert abs(len(wrong) - 1 - rounds) <= (3 if name == "smooth-320-opt" else 0), (len(wrong) - 1, rounds)
    else:
        assert abs(d.nsub - nsub) <= 0.06 * nsub, (d.nsub, nsub)
        assert abs(len(wrong) - 1 - rounds) <= 1, (len(wrong) - 1, rounds)
        assert abs(wrong[0] - listed[0]) <= listed[0] / 3 + 1, (wrong[0], listed[0])
        assert all(b <= 0.6 * a for a, b in zip(wrong, wrong[1:]) if a >= 8), wrong


def heals(d):
    """Per round of the whole-stream Jacobi iteration: (states that became right, those of them whose predecessor was still wrong)."""
    wrong = d.jacobi(sets=True)
    return [(before - after, {i for i in before - after if i - 1 in before}) for before, after in zip(wrong, wrong[1:])]


@pytest.mark.parametrize("make", [jc.flat_standard, lambda: jc.flat(True)], ids=["flat-standard", "flat-opt"])
def test_flat_colour_propagates_strictly_one_subsequence_a_round(make):
    """Nothing synchronises by itself: one wrong run behind the true start, eaten from its head, exactly one state a round."""
    d = jd.decoder(make())
    assert d.jacobi() == list(range(d.nsub - 1, -1, -1))
    assert all(len(h) == 1 and not lucky for h, lucky in heals(d))


def test_noise_propagates_one_subsequence_a_round():
    """Noise at quality 100: a state becomes right in the round after its predecessor did.  The exceptions are lucky alignments of a
    guess in the first rounds (a guess is one draw among the 6 x 64 block states, and the stream has 252 of them), so: none in the
    second half of the rounds, and under one heal in twenty overall.  The COUNT of wrong states still falls by more than one a round
    while several wrong runs are eaten at once, which is what the study's 246, 238, 233 shows: the rounds to the fixpoint are the
    longest run's length, 104 of 252 subsequences, where the photograph's runs are at most 8 of 435 long."""
    noise = heals(jd.decoder(jc.noise_q100()))
    assert len(noise) == 104
    assert not any(lucky for h, lucky in noise[len(noise) // 2:])
    assert sum(len(lucky) for h, lucky in noise) * 20 < sum(len(h) for h, lucky in noise)
    assert len(heals(jd.decoder(jc.photo_crop()))) <= 9


def test_photo_crop_ends_ok_at_the_default_and_unsync_at_one_round():
    d = jd.decoder(jc.photo_crop())
    assert d.schedule(jd.ROUNDS)[0] and not d.schedule(1)[0]
    assert d.status(1) == jd.UNSYNC and d.status(jd.ROUNDS) == jd.OK


def test_survey_record_is_the_tools_and_bounds_the_defaults():
    import json
    recs = json.load(open(os.path.join(REPO, "profiles", "jdec_sync_survey.json")))
    assert len(recs) == 8 and all(r["ok_at_default"] and r["default_rounds"] == jd.ROUNDS and r["launches"] == jd.LAUNCHES for r in recs)
    assert jd.ROUNDS >= 2 * max(max(r["rounds_run_per_launch_at_default"]) for r in recs)
    assert jd.ROUNDS >= 2 * max(r["smallest_rounds_on_ladder"] for r in recs)
    # launches that still changed something: those that ran more than the one round that finds nothing to do
    assert jd.LAUNCHES >= 2 * max(sum(1 for u in r["rounds_run_per_launch_at_default"] if u > 1) for r in recs)


@pytest.mark.parametrize("name", sorted(jc.EDGES))
def test_every_gpu_case_synchronises_within_half_the_default(name):
    assert jd.decoder(jc.EDGES[name]()).schedule(jd.ROUNDS // 2)[0]


def test_every_listed_case_synchronises_within_half_the_default():
    for case in jc.CASES:
        assert jd.decoder(jc.case_bytes(case)).schedule(jd.ROUNDS // 2)[0], jc.case_id(case)


def symbols(d):
    """(start, end) of every step of sequential decoding."""
    st = (0, 0, 0)
    while st[0] < d.total:
        nxt = d.decode(st, st[0] + 1)[0]
        yield st[0], nxt[0]
        st = nxt


def test_edge_cases_are_where_they_claim():
    S = jd.SUBSEQ_BITS
    short = jd.decoder(jc.EDGES["short"]())
    assert 0 < short.total < S and short.nsub == 1
    exact = jd.decoder(jc.exact())
    assert exact.total % S == 0 and exact.nsub >= 2
    anchored = jd.decoder(jc.anchor_edge())
    on_edge = [a for a in anchored.anchors[:-1] if a % S == 0]
    # the byte in front of such an anchor ends in pad bits: a 1 at the bottom that is not part of seven ones
    assert any(anchored.stream[a // 8 - 1] & 1 for a in on_edge), "pad bits are the last bits of a subsequence"
    sat = jd.decoder(jc.saturated())
    assert any(e - s >= 26 and s // S != (e - 1) // S for s, e in symbols(sat)), "a symbol of >= 26 bits across a subsequence boundary"


def test_the_large_case_spans_three_workgroups_and_two_steps_of_every_scan():
    data = jc.large()
    f = jd.parse(data)
    g = jd.geometry(f)
    stream, anchors, ok = jd.unstuff(data[f["scan_offset"]:f["scan_offset"] + f["scan_length"]], 0)
    nsub = -(-anchors[-1] // jd.SUBSEQ_BITS)
    assert nsub > 2 * _lib.JDEC_SYNC_THREADS and nsub > _lib.JDEC_SCAN_CHUNK
    assert f["scan_length"] > _lib.JDEC_CHUNK * _lib.JDEC_SCAN_CHUNK
    assert g["mcus"] > _lib.JDEC_DC_TILE * _lib.JDEC_SCAN_CHUNK


def test_cli_default_is_off():
    from wct_hip import cli
    assert cli.build_parser().parse_args([]).device_decode is False
    assert cli.build_parser().parse_args(["--device_decode"]).device_decode is True
    assert cli._DEVICE_DECODER is None
    assert cli.is_jpeg_file("a.JPG") and cli.is_jpeg_file("b.jpeg") and not cli.is_jpeg_file("c.png")
