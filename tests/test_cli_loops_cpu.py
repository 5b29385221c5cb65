"""wct_hip/cli.py without a GPU and without the library: the fp32 recompute helper, the serial loop every one-job-at-a-time mode runs
through, and the table main() picks the mode from -- against a fake engine that records its calls.  The one function that sends a host
array to the device is patched to keep it on the host.

EXPECTED holds, per mode, everything that happens for two jobs of which the first reports a clamp: file reads, timer reads, engine
calls (with the convolution mode they ran under and the tensors they were given and made) and log lines, in order.  The sequences were
recorded from the loops as they stood before they were merged into one (run_regions, run_interp, run_swap, run_scale, run_auto and
run_synthesis, each with its own copy of the loop), driven by this file's fake."""
import os
import re
import time
import types

import numpy as np
import pytest
import torch

from wct_hip import cli


# ---------------------------------------------------------------------------------------------------------------- the fake
class Recorder:
    """The events of one run, and names for the arrays and tensors that take part in it (by address: everything is kept alive)."""

    def __init__(self):
        self.events, self.names, self.keep = [], {}, []

    @staticmethod
    def _addr(x):
        return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()

    def name(self, x, name):
        self.names[self._addr(x)] = name
        self.keep.append(x)
        return x

    def new(self, shape, dtype=torch.float32):
        return self.name(torch.zeros(shape, dtype=dtype), "t%d" % sum(1 for n in self.names.values() if n.startswith("t")))

    def tag(self, x):
        if isinstance(x, (list, tuple)):
            return "[%s]" % ", ".join(self.tag(v) for v in x)
        if isinstance(x, (np.ndarray, torch.Tensor)):
            return self.names[self._addr(x)]
        return repr(x)

    def log(self, line):
        self.events.append("log: " + re.sub(r"\d+\.\d{4} seconds", "N seconds", str(line)).replace("\n", "/"))


class FakeEngine:
    """The engine surface the loops use, with the real one's range behaviour: a stylising call may leave a clamp pending (`clamps`, one
    entry per such call, then none), saturation_count(reset=True) acknowledges it, sync() raises on it."""

    def __init__(self, rec, clamps=()):
        self.rec, self.clamps, self.pending, self.mode = rec, list(clamps), 0, "f16x3"

    def _did(self, what, *args, out=None, stylises=False, **kw):
        if stylises:
            self.pending = self.clamps.pop(0) if self.clamps else 0
        text = ", ".join([self.rec.tag(a) for a in args] + ["%s=%s" % (k, self.rec.tag(v)) for k, v in kw.items()])
        self.rec.events.append("%s[%s](%s)%s" % (what, self.mode, text, " -> " + self.rec.tag(out) if out is not None else ""))
        return out

    def _like(self, c):
        return self.rec.new((1, 3, int(c.shape[-2]), int(c.shape[-1])))

    def to_tensor_u8(self, u8):
        return self._did("to_tensor_u8", u8, out=self.rec.new((1, 3, int(u8.shape[0]), int(u8.shape[1]))))

    def resize_u8(self, u8, size, to_tensor=False, filter="bilinear"):
        h, w = size if isinstance(size, tuple) else cli.resized_shape(int(u8.shape[0]), int(u8.shape[1]), size)
        return self._did("resize_u8", u8, size, to_tensor, filter, out=self.rec.new((1, 3, h, w)))

    def to_u8(self, res, round_mode):
        return self._did("to_u8", res, tuple(res.shape[-2:]), round_mode, out=self.rec.new((int(res.shape[-2]), int(res.shape[-1]), 3), torch.uint8))

    def stylize_regions(self, c, st, lab, alpha, num_run):
        return self._did("stylize_regions", c, st, lab, alpha, num_run, out=self._like(c), stylises=True)

    def stylize_guided(self, c, st, lab, s_lab, region_style, alpha, num_run):
        return self._did("stylize_guided", c, st, lab, s_lab, region_style, alpha, num_run, out=self._like(c), stylises=True)

    def feature_regions(self, c, s, K, level, iters):
        out = (self.rec.new((int(c.shape[-2]), int(c.shape[-1])), torch.uint8), self.rec.new((int(s.shape[-2]), int(s.shape[-1])), torch.uint8))
        return self._did("feature_regions", c, s, K, level, iters, out=out)

    def stylize_interp(self, c, st, lam, alpha, num_run):
        return self._did("stylize_interp", c, st, lam, alpha, num_run, out=self._like(c), stylises=True)

    def stylize_blend(self, c, st, wmap, alpha, num_run):
        return self._did("stylize_blend", c, st, wmap, alpha, num_run, out=self._like(c), stylises=True)

    def stylize_swap(self, c, s, level, match, alpha, num_run):
        return self._did("stylize_swap", c, s, level, match, alpha, num_run, out=self._like(c), stylises=True)

    def style_prepare(self, style, levels):
        self._did("style_prepare", style, list(levels))

    def stylize_scaled(self, c, s, div, gain, alpha, num_run):
        return self._did("stylize_scaled", c, s, tuple(div), gain, alpha, num_run, out=self._like(c), stylises=True)

    def stylize(self, c, s, alpha, num_run):
        return self._did("stylize", c, s, alpha, num_run, out=self._like(c), stylises=True)

    def stylize_color(self, c, s, how, alpha, num_run):
        return self._did("stylize_color", c, s, how, alpha, num_run, out=self._like(c), stylises=True)

    def synthesize(self, t, H, W, seed, stream_id, alpha, num_run):
        return self._did("synthesize", t, H, W, seed=seed, stream_id=stream_id, alpha=alpha, num_run=num_run, out=self.rec.new((1, 3, H, W)),
                         stylises=True)

    def saturation_count(self, reset=False):
        n = self.pending
        if reset:
            self.pending = 0
        self.rec.events.append("saturation_count(reset=%s) -> %d" % (reset, n))
        return n

    def set_conv_mode(self, mode):
        self.mode = mode
        self.rec.events.append("set_conv_mode(%s)" % mode)

    def sync(self):
        self.rec.events.append("sync")
        if self.pending:
            self.pending = 0
            raise OverflowError("an earlier call clamped")


# ---------------------------------------------------------------------------------------------------------------- the helper
def once_of(eng, fail_on_fresh=False):
    def once(fresh):
        if fresh and fail_on_fresh:
            eng.rec.events.append("once(True) raises")
            raise RuntimeError("the recompute failed")
        return eng.stylize("content", "fresh style" if fresh else "style", 1, 1)
    return once


def named_engine(clamps):
    """An engine whose tensors go by the strings they are (the helper hands them through untouched)."""
    rec = Recorder()
    rec.tag = lambda x: x if isinstance(x, str) else Recorder.tag(rec, x)
    eng = FakeEngine(rec, clamps)
    eng._like = lambda c: "result under %s" % eng.mode
    return eng, rec


def test_no_clamp_is_one_pass_with_the_tensors_at_hand():
    eng, rec = named_engine([0])
    assert cli._recompute_fp32(eng, rec.log, "pair", once_of(eng)) == "result under f16x3"
    assert rec.events == ["stylize[f16x3](content, style, 1, 1) -> result under f16x3", "saturation_count(reset=True) -> 0"]


@pytest.mark.parametrize("noun", ["pair", "content", "texture"])
def test_a_clamp_warns_then_recomputes_afresh_in_fp32_syncs_and_restores_f16x3(noun):
    eng, rec = named_engine([3, 0])
    assert cli._recompute_fp32(eng, rec.log, noun, once_of(eng)) == "result under fp32"
    assert rec.events == ["stylize[f16x3](content, style, 1, 1) -> result under f16x3", "saturation_count(reset=True) -> 3",
                          "log: WARNING: f16x3 range exceeded for this %s -> recomputing it with exact-fp32 convolutions" % noun,
                          "set_conv_mode(fp32)", "stylize[fp32](content, fresh style, 1, 1) -> result under fp32", "sync", "set_conv_mode(f16x3)"]


def test_without_sync_a_clamp_in_the_recompute_is_left_to_the_caller():
    eng, rec = named_engine([3, 2])
    assert cli._recompute_fp32(eng, rec.log, "pair", once_of(eng), sync=False) == "result under fp32"
    assert "sync" not in rec.events and rec.events[-2:] == ["stylize[fp32](content, fresh style, 1, 1) -> result under fp32", "set_conv_mode(f16x3)"]
    assert eng.pending == 2 and eng.mode == "f16x3"


def test_a_recompute_that_raises_leaves_the_engine_in_f16x3():
    eng, rec = named_engine([3])
    with pytest.raises(RuntimeError, match="the recompute failed"):
        cli._recompute_fp32(eng, rec.log, "pair", once_of(eng, fail_on_fresh=True))
    assert eng.mode == "f16x3" and rec.events[-3:] == ["set_conv_mode(fp32)", "once(True) raises", "set_conv_mode(f16x3)"]


def test_a_sync_that_raises_leaves_the_engine_in_f16x3():
    eng, rec = named_engine([3, 1])         # the fp32 pass clamps too: WCT.sync() raises OverflowError by design
    with pytest.raises(OverflowError):
        cli._recompute_fp32(eng, rec.log, "pair", once_of(eng))
    assert eng.mode == "f16x3" and rec.events[-3:] == ["stylize[fp32](content, fresh style, 1, 1) -> result under fp32", "sync", "set_conv_mode(f16x3)"]


@pytest.mark.parametrize("color", [None, "match"])
@pytest.mark.parametrize("fails", ["stylise", "sync"])
def test_the_fallback_of_the_cached_loops_leaves_the_engine_in_f16x3_too(fails, color):
    """_fp32_fallback (run_serial, run_pipelined): the same two ways out of the recompute."""
    eng, rec = named_engine([1])
    eng.to_tensor_u8 = lambda u8: "style"
    if fails == "stylise":
        def boom(*a):
            raise RuntimeError("the recompute failed")
        eng.stylize = eng.stylize_color = boom
    args = types.SimpleNamespace(preserve_color=color, style_size=0, alpha=1, num_run=1)
    with pytest.raises(RuntimeError if fails == "stylise" else OverflowError):
        cli._fp32_fallback(eng, args, rec.log, "content", "style u8")
    assert eng.mode == "f16x3" and rec.events[0].startswith("log: WARNING: f16x3 range exceeded for this pair")
    assert rec.events[1] == "set_conv_mode(fp32)" and rec.events[-1] == "set_conv_mode(f16x3)"
    if fails == "sync":
        assert rec.events[2:-1] == ["%s[fp32](content, style, %s1, 1) -> result under fp32" % (("stylize_color", "match, ") if color else ("stylize", "")), "sync"]


def test_the_fallback_returns_the_fp32_result():
    eng, rec = named_engine([0])
    eng.to_tensor_u8 = lambda u8: "style"
    args = types.SimpleNamespace(style_size=0, alpha=1, num_run=1)
    assert cli._fp32_fallback(eng, args, rec.log, "content", "style u8") == "result under fp32"
    assert rec.events[1:] == ["set_conv_mode(fp32)", "stylize[fp32](content, style, 1, 1) -> result under fp32", "sync", "set_conv_mode(f16x3)"]


def test_the_device_image_cache_keeps_the_last_few(monkeypatch):
    loads = []
    monkeypatch.setattr(cli, "_upload_u8", lambda path: loads.append(path) or "u8 of " + path)
    fetch = cli._device_images(2)
    assert [fetch(p) for p in ("a", "b", "a", "c", "b", "a")] == ["u8 of " + p for p in ("a", "b", "a", "c", "b", "a")]
    assert loads == ["a", "b", "c", "a"]        # c pushed a out (the oldest, not the least recently used), the second a pushed b out


# ---------------------------------------------------------------------------------------------------------------- the shared loop
def picture(rng, h, w):
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """content/ c1, c2 (20 x 24); style/ s1, s2 (18 x 16); tex/ t1 (18 x 16), t2 (12 x 40); masks/ c1, c2; smasks/ s1 (s2 is used
    whole); weights/ c1_0 .. c2_1."""
    from PIL import Image
    root = tmp_path_factory.mktemp("cli_loops")
    rng = np.random.default_rng(3)
    d = {k: root / k for k in ("content", "style", "tex", "masks", "smasks", "weights")}
    for p in d.values():
        p.mkdir()
    for name in ("c1", "c2"):
        Image.fromarray(picture(rng, 20, 24)).save(d["content"] / (name + ".png"))
        Image.fromarray(rng.integers(0, 2, size=(20, 24), dtype=np.uint8)).save(d["masks"] / (name + ".png"))
        for k in range(2):
            Image.fromarray(rng.integers(0, 128, size=(20, 24), dtype=np.uint8)).save(d["weights"] / ("%s_%d.png" % (name, k)))
    for name in ("s1", "s2"):
        Image.fromarray(picture(rng, 18, 16)).save(d["style"] / (name + ".png"))
    Image.fromarray(rng.integers(0, 2, size=(18, 16), dtype=np.uint8)).save(d["smasks"] / "s1.png")
    Image.fromarray(picture(rng, 18, 16)).save(d["tex"] / "t1.png")
    Image.fromarray(picture(rng, 12, 40)).save(d["tex"] / "t2.png")
    return d


def mode_argv(d):
    s1, s2 = str(d["style"] / "s1.png"), str(d["style"] / "s2.png")
    return {
        "regions": ["--maskPath", str(d["masks"]), "--region_styles", s1 + "," + s2],
        "regions with style masks": ["--maskPath", str(d["masks"]), "--region_styles", s1 + "," + s2, "--styleMaskPath", str(d["smasks"])],
        "interp": ["--interp_styles", s1 + "," + s2, "--interp_weights", "1,3"],
        "blend": ["--interp_styles", s1 + "," + s2, "--weightPath", str(d["weights"])],
        "swap": ["--swap_level", "3", "--picked_style_mark", "s1"],
        "scale": ["--level_scale", "4,4,2,1,1", "--coarse_style", s2, "--picked_style_mark", "s1"],
        "auto": ["--auto_regions", "2", "--picked_style_mark", "s1"],
        "synthesis": ["--synthesis", "--texturePath", str(d["tex"]), "--seed", "5"],
        "synthesis with a size": ["--synthesis", "--texturePath", str(d["tex"]), "--synthesis_size", "30x20", "--style_size", "16"],
    }


def parse(d, out, extra):
    args = cli.build_parser().parse_args(["--mode", "16x", "--contentPath", str(d["content"]), "--stylePath", str(d["style"]), "--outf", str(out),
                                          "--log_mark", "M", "--alpha", "0.5", "--num_run", "2"] + extra)
    for check in (cli.check_region_args, cli.check_interp_args, cli.check_synthesis_args, cli.check_color_args, cli.check_smooth_args,
                  cli.check_transform_args, cli.check_swap_args, cli.check_scale_args, cli.check_auto_args, cli.check_video_args, cli.check_motion_args):
        check(args)
    return args


def recording(monkeypatch, module, rec):
    """Patch `module` (cli.py) so that its file reads and timer reads land in rec.events and the arrays it reads have names."""
    def reads(fn, what):
        def wrapper(path, *a):
            rec.events.append("%s %s" % (what, ",".join(os.path.basename(p) for p in path) if isinstance(path, list) else os.path.basename(path)))
            return rec.name(fn(path, *a), "%s:%s" % (what, os.path.basename(path[0] if isinstance(path, list) else path).split(".")[0]))
        return wrapper
    for fn, what in (("load_rgb_u8", "image"), ("load_mask", "mask"), ("load_weights", "weights")):
        monkeypatch.setattr(module, fn, reads(getattr(module, fn), what))
    monkeypatch.setattr(module, "time", types.SimpleNamespace(time=lambda: rec.events.append("timer") or time.time(), strftime=time.strftime))


def drive(monkeypatch, d, out, extra):
    """Two jobs of the mode `extra` selects, the first of them clamped, through the mode table's run function."""
    rec = Recorder()
    recording(monkeypatch, cli, rec)
    monkeypatch.setattr(cli, "_on_device", lambda array, pin=False: torch.from_numpy(array))
    args = parse(d, out, extra)
    os.makedirs(args.outf)
    mode = cli.select_mode(args)
    jobs = mode.jobs(args, str(d["content"]), str(d["style"]))
    jobs = tuple(sorted(j) for j in jobs) if mode.name == "video" else sorted(jobs)      # os.listdir's order is the file system's
    total, n = mode.run(args, FakeEngine(rec, clamps=[1]), jobs, str(d["content"]), str(d["style"]), rec.log)
    assert n == 2 and total >= 0
    return rec.events, sorted(os.listdir(out))


MODE_NAMES = ("regions", "regions with style masks", "interp", "blend", "swap", "scale", "auto", "synthesis", "synthesis with a size")
EXPECTED = {'auto': ['log: /****************************** #0: Transferring "c1+s1.jpg" (2 feature regions of level 4, 10 iterations)',
          'image c1.png',
          'image s1.png',
          'timer',
          'to_tensor_u8[f16x3](image:c1) -> t0',
          'to_tensor_u8[f16x3](image:s1) -> t1',
          'feature_regions[f16x3](t0, t1, 2, 4, 10) -> [t2, t3]',
          'stylize_guided[f16x3](t0, [t1], t2, [t3], [0, 0], 0.5, 2) -> t4',
          'saturation_count(reset=True) -> 1',
          'log: WARNING: f16x3 range exceeded for this pair -> recomputing it with exact-fp32 convolutions',
          'set_conv_mode(fp32)',
          'to_tensor_u8[fp32](image:s1) -> t5',
          'feature_regions[fp32](t0, t5, 2, 4, 10) -> [t6, t7]',
          'stylize_guided[fp32](t0, [t5], t6, [t7], [0, 0], 0.5, 2) -> t8',
          'sync',
          'set_conv_mode(f16x3)',
          'to_u8[f16x3](t8, [20, 24], 0) -> t9',
          'timer',
          'log: Elapsed time is: N seconds',
          'log: /****************************** #1: Transferring "c2+s1.jpg" (2 feature regions of level 4, 10 iterations)',
          'image c2.png',
          'image s1.png',
          'timer',
          'to_tensor_u8[f16x3](image:c2) -> t10',
          'to_tensor_u8[f16x3](image:s1) -> t11',
          'feature_regions[f16x3](t10, t11, 2, 4, 10) -> [t12, t13]',
          'stylize_guided[f16x3](t10, [t11], t12, [t13], [0, 0], 0.5, 2) -> t14',
          'saturation_count(reset=True) -> 0',
          'to_u8[f16x3](t14, [20, 24], 0) -> t15',
          'timer',
          'log: Elapsed time is: N seconds'],
 'blend': ['image s1.png',
           'to_tensor_u8[f16x3](image:s1) -> t0',
           'image s2.png',
           'to_tensor_u8[f16x3](image:s2) -> t1',
           'log: /****************************** #0: Transferring "c1.png" by weight maps',
           'image c1.png',
           'weights c1_0.png,c1_1.png',
           'timer',
           'to_tensor_u8[f16x3](image:c1) -> t2',
           'stylize_blend[f16x3](t2, [t0, t1], weights:c1_0, 0.5, 2) -> t3',
           'saturation_count(reset=True) -> 1',
           'log: WARNING: f16x3 range exceeded for this content -> recomputing it with exact-fp32 convolutions',
           'set_conv_mode(fp32)',
           'image s1.png',
           'to_tensor_u8[fp32](image:s1) -> t4',
           'image s2.png',
           'to_tensor_u8[fp32](image:s2) -> t5',
           'stylize_blend[fp32](t2, [t4, t5], weights:c1_0, 0.5, 2) -> t6',
           'sync',
           'set_conv_mode(f16x3)',
           'to_u8[f16x3](t6, [20, 24], 0) -> t7',
           'timer',
           'log: Elapsed time is: N seconds',
           'log: /****************************** #1: Transferring "c2.png" by weight maps',
           'image c2.png',
           'weights c2_0.png,c2_1.png',
           'timer',
           'to_tensor_u8[f16x3](image:c2) -> t8',
           'stylize_blend[f16x3](t8, [t0, t1], weights:c2_0, 0.5, 2) -> t9',
           'saturation_count(reset=True) -> 0',
           'to_u8[f16x3](t9, [20, 24], 0) -> t10',
           'timer',
           'log: Elapsed time is: N seconds'],
 'interp': ['image s1.png',
            'to_tensor_u8[f16x3](image:s1) -> t0',
            'image s2.png',
            'to_tensor_u8[f16x3](image:s2) -> t1',
            'log: /****************************** #0: Transferring "c1.png" by interpolation',
            'image c1.png',
            'timer',
            'to_tensor_u8[f16x3](image:c1) -> t2',
            'stylize_interp[f16x3](t2, [t0, t1], [1.0, 3.0], 0.5, 2) -> t3',
            'saturation_count(reset=True) -> 1',
            'log: WARNING: f16x3 range exceeded for this content -> recomputing it with exact-fp32 convolutions',
            'set_conv_mode(fp32)',
            'image s1.png',
            'to_tensor_u8[fp32](image:s1) -> t4',
            'image s2.png',
            'to_tensor_u8[fp32](image:s2) -> t5',
            'stylize_interp[fp32](t2, [t4, t5], [1.0, 3.0], 0.5, 2) -> t6',
            'sync',
            'set_conv_mode(f16x3)',
            'to_u8[f16x3](t6, [20, 24], 0) -> t7',
            'timer',
            'log: Elapsed time is: N seconds',
            'log: /****************************** #1: Transferring "c2.png" by interpolation',
            'image c2.png',
            'timer',
            'to_tensor_u8[f16x3](image:c2) -> t8',
            'stylize_interp[f16x3](t8, [t0, t1], [1.0, 3.0], 0.5, 2) -> t9',
            'saturation_count(reset=True) -> 0',
            'to_u8[f16x3](t9, [20, 24], 0) -> t10',
            'timer',
            'log: Elapsed time is: N seconds'],
 'regions': ['image s1.png',
             'to_tensor_u8[f16x3](image:s1) -> t0',
             'image s2.png',
             'to_tensor_u8[f16x3](image:s2) -> t1',
             'log: /****************************** #0: Transferring "c1.png" by regions (masks/c1.png)',
             'image c1.png',
             'mask c1.png',
             'timer',
             'to_tensor_u8[f16x3](image:c1) -> t2',
             'stylize_regions[f16x3](t2, [t0, t1], mask:c1, 0.5, 2) -> t3',
             'saturation_count(reset=True) -> 1',
             'log: WARNING: f16x3 range exceeded for this content -> recomputing it with exact-fp32 convolutions',
             'set_conv_mode(fp32)',
             'image s1.png',
             'to_tensor_u8[fp32](image:s1) -> t4',
             'image s2.png',
             'to_tensor_u8[fp32](image:s2) -> t5',
             'stylize_regions[fp32](t2, [t4, t5], mask:c1, 0.5, 2) -> t6',
             'sync',
             'set_conv_mode(f16x3)',
             'to_u8[f16x3](t6, [20, 24], 0) -> t7',
             'timer',
             'log: Elapsed time is: N seconds',
             'log: /****************************** #1: Transferring "c2.png" by regions (masks/c2.png)',
             'image c2.png',
             'mask c2.png',
             'timer',
             'to_tensor_u8[f16x3](image:c2) -> t8',
             'stylize_regions[f16x3](t8, [t0, t1], mask:c2, 0.5, 2) -> t9',
             'saturation_count(reset=True) -> 0',
             'to_u8[f16x3](t9, [20, 24], 0) -> t10',
             'timer',
             'log: Elapsed time is: N seconds'],
 'regions with style masks': ['image s1.png',
                              'to_tensor_u8[f16x3](image:s1) -> t0',
                              'image s2.png',
                              'to_tensor_u8[f16x3](image:s2) -> t1',
                              'mask s1.png',
                              'log: /****************************** #0: Transferring "c1.png" by regions (masks/c1.png)',
                              'image c1.png',
                              'mask c1.png',
                              'timer',
                              'to_tensor_u8[f16x3](image:c1) -> t2',
                              'stylize_guided[f16x3](t2, [t0, t1], mask:c1, [mask:s1, None], None, 0.5, 2) -> t3',
                              'saturation_count(reset=True) -> 1',
                              'log: WARNING: f16x3 range exceeded for this content -> recomputing it with exact-fp32 convolutions',
                              'set_conv_mode(fp32)',
                              'image s1.png',
                              'to_tensor_u8[fp32](image:s1) -> t4',
                              'image s2.png',
                              'to_tensor_u8[fp32](image:s2) -> t5',
                              'stylize_guided[fp32](t2, [t4, t5], mask:c1, [mask:s1, None], None, 0.5, 2) -> t6',
                              'sync',
                              'set_conv_mode(f16x3)',
                              'to_u8[f16x3](t6, [20, 24], 0) -> t7',
                              'timer',
                              'log: Elapsed time is: N seconds',
                              'log: /****************************** #1: Transferring "c2.png" by regions (masks/c2.png)',
                              'image c2.png',
                              'mask c2.png',
                              'timer',
                              'to_tensor_u8[f16x3](image:c2) -> t8',
                              'stylize_guided[f16x3](t8, [t0, t1], mask:c2, [mask:s1, None], None, 0.5, 2) -> t9',
                              'saturation_count(reset=True) -> 0',
                              'to_u8[f16x3](t9, [20, 24], 0) -> t10',
                              'timer',
                              'log: Elapsed time is: N seconds'],
 'scale': ['log: /****************************** #0: Transferring "c1+s1.jpg" (level divisors 4,4,2,1,1, detail 1, coarse style style/s2.png)',
           'image c1.png',
           'image s1.png',
           'image s2.png',
           'timer',
           'to_tensor_u8[f16x3](image:c1) -> t0',
           'to_tensor_u8[f16x3](image:s1) -> t1',
           'to_tensor_u8[f16x3](image:s2) -> t2',
           'style_prepare[f16x3](t2, [5, 4, 3])',
           'style_prepare[f16x3](t1, [2, 1])',
           'stylize_scaled[f16x3](t0, None, [4, 4, 2, 1, 1], 1.0, 0.5, 2) -> t3',
           'saturation_count(reset=True) -> 1',
           'log: WARNING: f16x3 range exceeded for this pair -> recomputing it with exact-fp32 convolutions',
           'set_conv_mode(fp32)',
           'to_tensor_u8[fp32](image:s1) -> t4',
           'to_tensor_u8[fp32](image:s2) -> t5',
           'style_prepare[fp32](t5, [5, 4, 3])',
           'style_prepare[fp32](t4, [2, 1])',
           'stylize_scaled[fp32](t0, None, [4, 4, 2, 1, 1], 1.0, 0.5, 2) -> t6',
           'sync',
           'set_conv_mode(f16x3)',
           'to_u8[f16x3](t6, [20, 24], 0) -> t7',
           'timer',
           'log: Elapsed time is: N seconds',
           'log: /****************************** #1: Transferring "c2+s1.jpg" (level divisors 4,4,2,1,1, detail 1, coarse style style/s2.png)',
           'image c2.png',
           'timer',
           'to_tensor_u8[f16x3](image:c2) -> t8',
           'to_tensor_u8[f16x3](image:s1) -> t9',
           'to_tensor_u8[f16x3](image:s2) -> t10',
           'style_prepare[f16x3](t10, [5, 4, 3])',
           'style_prepare[f16x3](t9, [2, 1])',
           'stylize_scaled[f16x3](t8, None, [4, 4, 2, 1, 1], 1.0, 0.5, 2) -> t11',
           'saturation_count(reset=True) -> 0',
           'to_u8[f16x3](t11, [20, 24], 0) -> t12',
           'timer',
           'log: Elapsed time is: N seconds'],
 'swap': ['log: /****************************** #0: Transferring "c1+s1.jpg" (patch swap at level 3, whitened)',
          'image c1.png',
          'image s1.png',
          'timer',
          'to_tensor_u8[f16x3](image:c1) -> t0',
          'to_tensor_u8[f16x3](image:s1) -> t1',
          "stylize_swap[f16x3](t0, t1, 3, 'whitened', 0.5, 2) -> t2",
          'saturation_count(reset=True) -> 1',
          'log: WARNING: f16x3 range exceeded for this pair -> recomputing it with exact-fp32 convolutions',
          'set_conv_mode(fp32)',
          'to_tensor_u8[fp32](image:s1) -> t3',
          "stylize_swap[fp32](t0, t3, 3, 'whitened', 0.5, 2) -> t4",
          'set_conv_mode(f16x3)',
          'saturation_count(reset=True) -> 0',
          'to_u8[f16x3](t4, [20, 24], 0) -> t5',
          'timer',
          'log: Elapsed time is: N seconds',
          'log: /****************************** #1: Transferring "c2+s1.jpg" (patch swap at level 3, whitened)',
          'image c2.png',
          'timer',
          'to_tensor_u8[f16x3](image:c2) -> t6',
          'to_tensor_u8[f16x3](image:s1) -> t7',
          "stylize_swap[f16x3](t6, t7, 3, 'whitened', 0.5, 2) -> t8",
          'saturation_count(reset=True) -> 0',
          'to_u8[f16x3](t8, [20, 24], 0) -> t9',
          'timer',
          'log: Elapsed time is: N seconds'],
 'synthesis': ['log: /****************************** #0: Transferring "t1.jpg"',
               'image t1.png',
               'timer',
               'to_tensor_u8[f16x3](image:t1) -> t0',
               'synthesize[f16x3](t0, 18, 16, seed=5, stream_id=0, alpha=0.5, num_run=2) -> t1',
               'saturation_count(reset=True) -> 1',
               'log: WARNING: f16x3 range exceeded for this texture -> recomputing it with exact-fp32 convolutions',
               'set_conv_mode(fp32)',
               'synthesize[fp32](t0, 18, 16, seed=5, stream_id=0, alpha=0.5, num_run=2) -> t2',
               'sync',
               'set_conv_mode(f16x3)',
               'to_u8[f16x3](t2, [18, 16], 0) -> t3',
               'timer',
               'log: Elapsed time is: N seconds',
               'log: /****************************** #1: Transferring "t2.jpg"',
               'image t2.png',
               'timer',
               'to_tensor_u8[f16x3](image:t2) -> t4',
               'synthesize[f16x3](t4, 12, 40, seed=5, stream_id=1, alpha=0.5, num_run=2) -> t5',
               'saturation_count(reset=True) -> 0',
               'to_u8[f16x3](t5, [12, 40], 0) -> t6',
               'timer',
               'log: Elapsed time is: N seconds'],
 'synthesis with a size': ['log: /****************************** #0: Transferring "t1.jpg"',
                           'image t1.png',
                           'timer',
                           "resize_u8[f16x3](image:t1, [16, 14], True, 'bicubic') -> t0",
                           'synthesize[f16x3](t0, 32, 32, seed=0, stream_id=0, alpha=0.5, num_run=2) -> t1',
                           'saturation_count(reset=True) -> 1',
                           'log: WARNING: f16x3 range exceeded for this texture -> recomputing it with exact-fp32 convolutions',
                           'set_conv_mode(fp32)',
                           'synthesize[fp32](t0, 32, 32, seed=0, stream_id=0, alpha=0.5, num_run=2) -> t2',
                           'sync',
                           'set_conv_mode(f16x3)',
                           'to_u8[f16x3](t2, [20, 30], 0) -> t3',
                           'timer',
                           'log: Elapsed time is: N seconds',
                           'log: /****************************** #1: Transferring "t2.jpg"',
                           'image t2.png',
                           'timer',
                           "resize_u8[f16x3](image:t2, [4, 16], True, 'bicubic') -> t4",
                           'synthesize[f16x3](t4, 32, 32, seed=0, stream_id=1, alpha=0.5, num_run=2) -> t5',
                           'saturation_count(reset=True) -> 0',
                           'to_u8[f16x3](t5, [20, 30], 0) -> t6',
                           'timer',
                           'log: Elapsed time is: N seconds']}
FILES = {'auto': ['M_mode=16x_alpha=0.5_auto=2_c1+s1.jpg', 'M_mode=16x_alpha=0.5_auto=2_c2+s1.jpg'],
 'blend': ['M_mode=16x_alpha=0.5_c1+blend.jpg', 'M_mode=16x_alpha=0.5_c2+blend.jpg'],
 'interp': ['M_mode=16x_alpha=0.5_c1+interp.jpg', 'M_mode=16x_alpha=0.5_c2+interp.jpg'],
 'regions': ['M_mode=16x_alpha=0.5_c1+regions.jpg', 'M_mode=16x_alpha=0.5_c2+regions.jpg'],
 'regions with style masks': ['M_mode=16x_alpha=0.5_c1+regions.jpg', 'M_mode=16x_alpha=0.5_c2+regions.jpg'],
 'scale': ['M_mode=16x_alpha=0.5_scale=4-4-2-1-1_c1+s1.jpg', 'M_mode=16x_alpha=0.5_scale=4-4-2-1-1_c2+s1.jpg'],
 'swap': ['M_mode=16x_alpha=0.5_swap=3_c1+s1.jpg', 'M_mode=16x_alpha=0.5_swap=3_c2+s1.jpg'],
 'synthesis': ['M_mode=16x_alpha=0.5_t1.jpg', 'M_mode=16x_alpha=0.5_t2.jpg'],
 'synthesis with a size': ['M_mode=16x_alpha=0.5_t1.jpg', 'M_mode=16x_alpha=0.5_t2.jpg']}


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_the_serial_loop_does_what_the_separate_loops_did(monkeypatch, folders, tmp_path, mode):
    events, files = drive(monkeypatch, folders, tmp_path / "out", mode_argv(folders)[mode])
    events = [e.replace(str(folders["content"].parent) + os.sep, "") for e in events]
    assert events == EXPECTED[mode]
    assert files == FILES[mode]
    # the label maps and weight maps are read before the job's timer starts, and the recompute got style tensors of its own
    timers = [i for i, e in enumerate(events) if e == "timer"]
    assert len(timers) == 4
    for i, e in enumerate(events):
        if e.startswith(("mask c", "weights c")):
            assert not any(a < i < b for a, b in (timers[:2], timers[2:]))


# ---------------------------------------------------------------------------------------------------------------- the mode table
TABLE = [
    (["--synthesis"], "synthesis", "--synthesis: texture synthesis uses the serial loop", "pair", False, "Number of content-style pairs: 2"),
    (["--maskPath", "m", "--region_styles", "a.png"], "regions", "--maskPath: region runs use the serial loop", "image", True,
     "Number of contents with label maps: 2"),
    (["--interp_styles", "a.png,b.png", "--interp_weights", "1,1"], "interp",
     "--interp_styles: interpolation and weight-map runs use the serial loop", "image", False, "Number of contents: 2"),
    (["--interp_styles", "a.png,b.png", "--weightPath", "w"], "interp",
     "--interp_styles: interpolation and weight-map runs use the serial loop", "image", False, "Number of contents: 2"),
    (["--video"], "video", "--video: a sequence is stylised frame by frame, each against the one before", "frame", False, None),
    (["--video", "--motion"], "video", "--video: a sequence is stylised frame by frame, each against the one before", "frame", False, None),
    (["--swap_level", "4"], "swap", "--swap_level: patch-swap runs use the serial loop", "pair", True, "Number of content-style pairs: 2"),
    (["--level_scale", "4,4,2,1,1"], "scale", "--level_scale: scale-controlled runs use the serial loop", "pair", True, "Number of content-style pairs: 2"),
    (["--auto_regions", "3"], "auto", "--auto_regions: feature-region runs use the serial loop", "pair", True, "Number of content-style pairs: 2"),
    # what passes the checks together: the mode wins over --pipeline, and a mode's own companions do not change it
    (["--maskPath", "m", "--region_styles", "a.png", "--pipeline", "3"], "regions", "--maskPath: region runs use the serial loop", "image", True, None),
    (["--maskPath", "m", "--region_styles", "a.png", "--preserve_color", "luma", "--smooth_radius", "4"], "regions",
     "--maskPath: region runs use the serial loop", "image", True, None),
    (["--swap_level", "3", "--transform", "ot", "--pipeline", "0"], "swap", "--swap_level: patch-swap runs use the serial loop", "pair", True, None),
    (["--level_scale", "2,2,1,1,1", "--preserve_color", "match", "--numpy"], "scale", "--level_scale: scale-controlled runs use the serial loop",
     "pair", True, None),
    (["--auto_regions", "2", "--preserve_color", "luma"], "auto", "--auto_regions: feature-region runs use the serial loop", "pair", True, None),
    (["--video", "--transform", "adain", "--pipeline", "5"], "video", "--video: a sequence is stylised frame by frame, each against the one before",
     "frame", False, None),
]


@pytest.mark.parametrize("argv,name,reason,noun,early,number", TABLE, ids=[" ".join(t[0]) for t in TABLE])
def test_the_table_selects_the_mode_with_its_note_and_noun(argv, name, reason, noun, early, number):
    args = cli.build_parser().parse_args(["--mode", "16x"] + argv)
    for check in (cli.check_region_args, cli.check_interp_args, cli.check_synthesis_args, cli.check_color_args, cli.check_smooth_args,
                  cli.check_transform_args, cli.check_swap_args, cli.check_scale_args, cli.check_auto_args, cli.check_video_args, cli.check_motion_args):
        check(args)                     # the combination is one main() accepts
    mode = cli.select_mode(args)
    assert (mode.name, mode.reason, mode.noun, mode.early) == (name, reason, noun, early)
    if number:
        assert mode.number(["job", "job"]) == number


def test_the_table_keeps_the_order_of_precedence_and_leaves_plain_runs_alone():
    assert [m.name for m in cli.MODES] == ["synthesis", "regions", "interp", "video", "swap", "scale", "auto"]
    assert cli.MODES[3].number((["f0", "f1", "f2"], ["s"])) == "Number of frames: 3, styles: 1"
    for argv in ([], ["--pipeline", "0"], ["--preserve_color", "match"], ["--transform", "ot", "--smooth_radius", "3"]):
        assert cli.select_mode(cli.build_parser().parse_args(["--mode", "16x"] + argv)) is None


def test_main_lists_the_label_maps_before_it_creates_the_engine(tmp_path, monkeypatch):
    """A content without its label map refuses the run by name, and no engine has been asked for by then."""
    from PIL import Image
    from wct_hip import wct as wct_module
    (tmp_path / "c").mkdir()
    (tmp_path / "m").mkdir()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "c" / "a.png")
    monkeypatch.setattr(wct_module, "WCT", lambda args: pytest.fail("the engine was created first"))
    with pytest.raises(FileNotFoundError, match="label map .*a.png for content a.png not found"):
        cli.main(["--mode", "16x", "--contentPath", str(tmp_path / "c"), "--maskPath", str(tmp_path / "m"), "--region_styles", "s.png",
                  "--outf", str(tmp_path / "o")])


@pytest.mark.parametrize("mode,first,second,last", [
    ("regions", "Number of contents with label maps: 2", "--pipeline is ignored with --maskPath: region runs use the serial loop",
     "Processed 2 images. Average processing time per image is:"),
    ("swap", "Number of content-style pairs: 2", "--pipeline is ignored with --swap_level: patch-swap runs use the serial loop",
     "Processed 2 images. Average processing time per pair is:"),
    ("blend", "--pipeline is ignored with --interp_styles: interpolation and weight-map runs use the serial loop", "Number of contents: 2",
     "Processed 2 images. Average processing time per image is:"),
    ("synthesis", "--pipeline is ignored with --synthesis: texture synthesis uses the serial loop", "Number of content-style pairs: 2",
     "Processed 2 images. Average processing time per pair is:"),
])
def test_main_logs_the_count_the_note_and_the_average_in_the_order_it_always_did(monkeypatch, folders, tmp_path, mode, first, second, last):
    """main() through a fake engine: modes that list their jobs before the engine exists count them ahead of the --pipeline note, the
    others behind it; then the jobs; then the average per the mode's noun."""
    from wct_hip import wct as wct_module
    rec = Recorder()
    recording(monkeypatch, cli, rec)
    monkeypatch.setattr(cli, "_on_device", lambda array, pin=False: torch.from_numpy(array))
    monkeypatch.setattr(wct_module, "WCT", lambda args: FakeEngine(rec))
    out = tmp_path / "out"
    assert cli.main(["--mode", "16x", "--contentPath", str(folders["content"]), "--stylePath", str(folders["style"]), "--outf", str(out),
                     "--log_mark", "M"] + mode_argv(folders)[mode]) == 0
    lines = (out / "log_M_16x.txt").read_text().splitlines()
    assert lines[1] == first and lines[2] == second and lines[-1].startswith(last)
    assert sum(l.startswith("Elapsed time is:") for l in lines) == 2 and sorted(f for f in os.listdir(out) if f.endswith(".jpg")) == [
        f.replace("alpha=0.5", "alpha=1") for f in FILES[mode]]
