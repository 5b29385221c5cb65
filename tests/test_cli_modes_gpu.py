"""wct_hip/cli.py end to end for the modes no other file drives through cli.main: --weightPath, --auto_regions and --video (with and
without --motion), and a clamp injected into a mode of the shared serial loop (--interp_styles).  Every file cli.main writes is compared
byte for byte with a file made here from the public WCT calls the loop is documented to make, saved through the same Pillow call."""
import os
import types

import numpy as np
import pytest

from wct_hip import lib as _lib

pytestmark = pytest.mark.gpu

ALPHA = 0.8


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "-m gpu tests need the MI355X"
    return t


@pytest.fixture(scope="module")
def ref(torch):
    """The engine the expected pictures are made with (its own context: nothing cli.main does touches it)."""
    from wct_hip import WCT
    return WCT(types.SimpleNamespace(mode="16x", alpha=ALPHA))


def blocky(rng, h, w):
    """4 x 4 blocks plus noise (the images of test_swap_gpu.py): features that are not degenerate."""
    img = rng.random(((h + 3) // 4, (w + 3) // 4, 3)).repeat(4, 0).repeat(4, 1)[:h, :w] * 0.8 + rng.random((h, w, 3)) * 0.2
    return (img * 255).astype(np.uint8)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """content/: two 100 x 132 images; style/: 90 x 84 and 64 x 72; frames/: three 100 x 132 frames, one image panning by 3 px a frame
    under fresh noise; weights/: per content two weight maps (a ramp and part of its complement, so some of every pixel stays unstyled)."""
    from PIL import Image
    root = tmp_path_factory.mktemp("cli_modes")
    rng = np.random.default_rng(17)
    d = {k: root / k for k in ("content", "style", "frames", "weights")}
    for p in d.values():
        p.mkdir()
    for name in ("c1.png", "c2.png"):
        Image.fromarray(blocky(rng, 100, 132)).save(d["content"] / name)
        ramp = np.tile(np.linspace(0, 200, 132).astype(np.uint8), (100, 1))
        if name == "c2.png":
            ramp = ramp[:, ::-1].copy()
        Image.fromarray(ramp).save(d["weights"] / (name.split(".")[0] + "_0.png"))
        Image.fromarray(((255 - ramp.astype(np.int32)) * 3 // 4).astype(np.uint8)).save(d["weights"] / (name.split(".")[0] + "_1.png"))
    for name, (h, w) in (("s1.png", (90, 84)), ("s2.png", (64, 72))):
        Image.fromarray(blocky(rng, h, w)).save(d["style"] / name)
    wide = blocky(rng, 100, 140).astype(np.int32)
    for k in range(3):
        frame = wide[:, 3 * k:3 * k + 132] + rng.integers(-4, 5, size=(100, 132, 3))
        Image.fromarray(np.clip(frame, 0, 255).astype(np.uint8)).save(d["frames"] / ("f%d.png" % k))
    return d


def run_cli(folders, out, content, extra):
    from wct_hip import cli
    assert cli.main(["--mode", "16x", "--contentPath", str(folders[content]), "--stylePath", str(folders["style"]), "--outf", str(out),
                     "--log_mark", "M", "--alpha", str(ALPHA)] + list(extra)) == 0
    written = {f: (out / f).read_bytes() for f in sorted(os.listdir(out)) if f.endswith(".jpg")}
    return written, (out / "log_M_16x.txt").read_text()


def tensor(torch, eng, path):
    from wct_hip import cli
    return eng.to_tensor_u8(torch.from_numpy(cli.load_rgb_u8(str(path))).cuda())


def jpeg_bytes(u8, path):
    from PIL import Image
    Image.fromarray(u8.cpu().numpy()).save(path)
    return path.read_bytes()


def test_weight_maps(torch, ref, folders, tmp_path):
    """--interp_styles with --weightPath: per content one wct_stylize_blend against the styles converted once, with the content's weight
    maps as value / 255; --pipeline 0 leaves no note in the log."""
    from wct_hip import cli
    styles = [folders["style"] / "s1.png", folders["style"] / "s2.png"]
    got, log = run_cli(folders, tmp_path / "out", "content", ["--interp_styles", ",".join(map(str, styles)), "--weightPath", str(folders["weights"]),
                                                             "--pipeline", "0"])
    st = [tensor(torch, ref, p) for p in styles]
    want = {}
    for name in ("c1", "c2"):
        maps = [str(folders["weights"] / ("%s_%d.png" % (name, k))) for k in range(2)]
        wmap = torch.from_numpy(cli.load_weights(maps, (100, 132))).cuda()
        c = tensor(torch, ref, folders["content"] / (name + ".png"))
        want["M_mode=16x_alpha=0.8_%s+blend.jpg" % name] = jpeg_bytes(ref.to_u8(ref.stylize_blend(c, st, wmap, ALPHA, 1), 0), tmp_path / "ref.jpg")
    assert got == want
    assert want["M_mode=16x_alpha=0.8_c1+blend.jpg"] != want["M_mode=16x_alpha=0.8_c2+blend.jpg"]
    assert "Number of contents: 2" in log and "Processed 2 images. Average processing time per image is:" in log
    assert "--pipeline is ignored" not in log and log.count("by weight maps") == 2 and log.count("Elapsed time is:") == 2


def test_auto_regions(torch, ref, folders, tmp_path):
    """--auto_regions 2: per pair wct_feature_regions at level 4 with 10 iterations (the defaults), then wct_stylize_guided against the
    one style, every region of it style 0; --pipeline 3 is noted as ignored."""
    got, log = run_cli(folders, tmp_path / "out", "content", ["--auto_regions", "2", "--pipeline", "3"])
    want = {}
    for cn in ("c1", "c2"):
        for sn in ("s1", "s2"):
            c, s = tensor(torch, ref, folders["content"] / (cn + ".png")), tensor(torch, ref, folders["style"] / (sn + ".png"))
            lab_c, lab_s = ref.feature_regions(c, s, 2, 4, 10)
            res = ref.stylize_guided(c, [s], lab_c, [lab_s], [0, 0], ALPHA, 1)
            want["M_mode=16x_alpha=0.8_auto=2_%s+%s.jpg" % (cn, sn)] = jpeg_bytes(ref.to_u8(res, 0), tmp_path / "ref.jpg")
    assert got == want
    assert "Number of content-style pairs: 4" in log and "Processed 4 images. Average processing time per pair is:" in log
    assert "--pipeline is ignored with --auto_regions: feature-region runs use the serial loop" in log
    assert log.count("(2 feature regions of level 4, 10 iterations)") == 4


@pytest.mark.parametrize("motion", [False, True], ids=["plain", "motion"])
def test_video(torch, ref, folders, tmp_path, motion):
    """--video: per style (sorted) one clip with the default parameters against the style prepared once, then the three frames (sorted)
    through Clip.stylize with the uint8 conversion fused; --motion attaches the default block matching to every clip."""
    got, log = run_cli(folders, tmp_path / "out", "frames", ["--video"] + (["--motion"] if motion else []))
    field = dict(levels=_lib.MOTION_LEVELS, range=_lib.MOTION_RANGE, penalty=_lib.MOTION_PENALTY) if motion else None
    want = {}
    for sn in ("s1", "s2"):
        ref.style_prepare(tensor(torch, ref, folders["style"] / (sn + ".png")))
        clip = ref.clip(100, 132, _lib.CLIP_RATE, _lib.CLIP_CUT, _lib.CLIP_BLEND, _lib.CLIP_SIGMA, _lib.CLIP_RADIUS, motion=field)
        try:
            for k in range(3):
                _, hwc = clip.stylize(tensor(torch, ref, folders["frames"] / ("f%d.png" % k)), ALPHA, u8=True, round_mode=0)
                assert tuple(hwc.shape) == (96, 128, 3)
                want["M_mode=16x_alpha=0.8_f%d+%s.jpg" % (k, sn)] = jpeg_bytes(hwc, tmp_path / "ref.jpg")
        finally:
            clip.close()
    assert got == want
    assert "Number of frames: 3, styles: 2" in log and "Processed 6 images. Average processing time per frame is:" in log
    assert "--pipeline is ignored with --video: a sequence is stylised frame by frame, each against the one before" in log
    assert log.count("motion: levels %d, range %d, penalty %d" % (_lib.MOTION_LEVELS, _lib.MOTION_RANGE, _lib.MOTION_PENALTY)) == (6 if motion else 0)


def test_an_injected_clamp_is_recomputed_in_fp32_by_the_shared_loop(torch, ref, folders, tmp_path, monkeypatch):
    """uint8 images cannot reach the f16 range, so the clamp is injected (as in test_cli.py): the engine cli.main creates is wrapped, and
    the wrapper reports one clamp for the content that is stylised second.  One warning, the engine back in f16x3, that content's file the
    fp32 path's picture and the other content's the f16x3 one."""
    from wct_hip import cli, wct as wct_module
    real = wct_module.WCT
    made = []

    class Injected:
        """The real engine with a clamp reported for the second stylize_interp (and only that one)."""
        def __init__(self, args):
            object.__setattr__(self, "eng", real(args))
            object.__setattr__(self, "state", {"n": 0, "fake": 0, "modes": []})
            made.append(self)
        def __getattr__(self, name):
            return getattr(self.eng, name)
        def __setattr__(self, name, value):
            setattr(self.eng, name, value)
        def stylize_interp(self, *a, **k):
            self.state["n"] += 1
            if self.state["n"] == 2:
                self.state["fake"] = 1
            return self.eng.stylize_interp(*a, **k)
        def saturation_count(self, reset=False):
            n = self.eng.saturation_count(reset) + self.state["fake"]
            if reset:
                self.state["fake"] = 0
            return n
        def set_conv_mode(self, mode):
            self.state["modes"].append(mode)
            return self.eng.set_conv_mode(mode)

    monkeypatch.setattr(wct_module, "WCT", Injected)
    styles = [folders["style"] / "s1.png", folders["style"] / "s2.png"]
    got, log = run_cli(folders, tmp_path / "out", "content", ["--interp_styles", ",".join(map(str, styles)), "--interp_weights", "1,3"])
    assert len(made) == 1 and made[0].state["n"] == 3 and made[0].state["modes"] == ["fp32", "f16x3"]
    assert log.count("WARNING: f16x3 range exceeded for this content -> recomputing it with exact-fp32 convolutions") == 1
    assert log.count("WARNING") == 1 and "Processed 2 images. Average processing time per image is:" in log
    order = [c for c in os.listdir(folders["content"]) if cli.is_image_file(c)]
    want = {}
    for i, cfile in enumerate(order):
        if i == 1:
            ref.set_conv_mode("fp32")
        try:
            st = [tensor(torch, ref, p) for p in styles]
            res = ref.stylize_interp(tensor(torch, ref, folders["content"] / cfile), st, [1.0, 3.0], ALPHA, 1)
            ref.sync()
        finally:
            ref.set_conv_mode("f16x3")
        want["M_mode=16x_alpha=0.8_%s+interp.jpg" % cfile.split(".")[0]] = jpeg_bytes(ref.to_u8(res, 0), tmp_path / "ref.jpg")
    assert got == want
    # the engine cli.main used is in f16x3 again: it gives the f16x3 picture of the first content
    eng = made[0].eng
    res = eng.stylize_interp(tensor(torch, eng, folders["content"] / order[0]), [tensor(torch, eng, p) for p in styles], [1.0, 3.0], ALPHA, 1)
    assert jpeg_bytes(eng.to_u8(res, 0), tmp_path / "again.jpg") == want["M_mode=16x_alpha=0.8_%s+interp.jpg" % order[0].split(".")[0]]
