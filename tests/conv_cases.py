"""Every loadable conv layer shape through wct_encode / wct_decode: the launch choices restated, and the plan derived from them.
CPU only: no torch, no GPU (tests/test_conv_cases_cpu.py checks it, tests/test_conv_sweep_gpu.py runs it).

`wct_load_module` accepts any layer list whose channel counts are multiples of 4 up to 512 (tests/width_models.loadable), and
wct_api.hip run_conv / encode_impl / decode_impl choose a kernel and a hand-over format per layer from cin, cout, the neighbours and
the debug switches.  `predict` restates those choices for an ARBITRARY layer list (tests/geometry_cases.predict_names does it for the
two shipped graphs, with the size-selected forms this module leaves out); `modules` is the plan: two lines over all 128 widths, a
short line over the first layers 3 -> b, and the switch arms, one per reachable class cell.

    cin class   of a layer behind the first: "f32" (cin % 8 == 4: the exact-fp32 kernel inside f16x3 mode), "half" (cin % 16 == 8:
                register-staged f16x3, half a last chunk), "dma" (cin % 16 == 0: may run the DMA-staged persistent kernel)
    cout class  COUT_CLASSES, by cout_pad (16 / 32 / 64 / 128 / 128 g), the ragged tail and cout % 8 (may the layer write SP16)
    variant     "enc", "enc-pool" (the layer under test pools), "dec", "dec-up" (the layer under test reads an upsampled map)

The layer under test a -> b sits in the middle of its module ([3 -> 16][16 -> a][a -> b][b -> 8] / [16 -> a][a -> b][b -> 3]): its input
arrives in whatever format its producer hands over, its output leaves in whatever format its consumer takes."""
from __future__ import annotations

import collections
import functools
from typing import Dict, List, Sequence, Tuple

from tests import sweep_cases as S
from tests import width_models as wm
from tests.geometry_cases import _family, _sp_ok
from wct_hip.model_zoo import Layer

WIDTHS = S.WIDTHS
VARIANTS = ("enc", "enc-pool", "dec", "dec-up")
CIN_CLASSES = ("f32", "half", "dma")
COUT_CLASSES = ("pad16 cout%8=4", "pad16 cout%8=0", "pad32", "pad64", "pad128 full", "pad128 ragged cout%8=4", "pad128 ragged cout%8=0",
                "multi-group ragged", "multi-group full")

#: Line I: every cin a with these couts -- one per cout class the issue names (the two other classes, 128-ragged with cout % 8 == 0
#: and full multi-group, come from Line II's own widths: 72, 80, .. and 256, 384, 512)
REP_COUT = (12, 8, 24, 40, 128, 68, 264)
#: Line II: every cout b with these cins -- each cin class at one 16-channel chunk (4, 8, 16) and at many (68, 136, 48 / 256)
REP_CIN = (4, 8, 16, 68, 48, 136, 256)
#: first layers 3 -> b
FIRST_COUT = tuple(range(4, 65, 4))

#: API input sizes per variant (image for encoders, feature map for decoders); the map at the layer under test is 5 x 7 / 9 x 35
#: (one ragged tile reflected on all four sides; one row past the 8-row tile and three columns past the 32-column tile),
#: pooled 9 x 35 -> 4 x 17 / 5 x 7 -> 2 x 3 behind it, upsampled 5 x 7 -> 10 x 14 / 5 x 17 -> 10 x 34 in front of it
SIZES = {"enc": ((5, 7), (9, 35)), "enc-pool": ((9, 35), (5, 7)), "dec": ((5, 7), (9, 35)), "dec-up": ((5, 7), (5, 17))}

SWITCHES = ("sp", "upconv", "fuse", "conv_mode")     # conv_mode 0: wct_set_conv_mode(0); the others: wct_debug_set(key, 0)


def cin_class(cin: int) -> str:
    return "f32" if cin % 8 == 4 else "half" if cin % 16 == 8 else "dma"


def cout_class(cout: int) -> str:
    cp = wm.pad_cout(cout)
    if cp == 16:
        return COUT_CLASSES[0] if cout % 8 == 4 else COUT_CLASSES[1]
    if cp <= 64:
        return "pad%d" % cp
    if cp == 128:
        return COUT_CLASSES[4] if cout == 128 else COUT_CLASSES[5] if cout % 8 == 4 else COUT_CLASSES[6]
    return COUT_CLASSES[8] if cout == cp else COUT_CLASSES[7]


# --------------------------------------------------------------------------------------------------------- the restatement
Prediction = collections.namedtuple("Prediction", "names hand kernels")
Prediction.__doc__ = """names: profile family names in launch order (one per launch); hand[i]: the format between layers i and i + 1 ("f32" fp32
NHWC, "sp16", "lds" inside a fused kernel); kernels[i]: the kernel kind that runs layer i (KERNELS)."""

#: kernel kinds: the generic fp32 kernel (conv3x3.hip), the register-staged f16x3 kernel and its 16-cout sibling (conv3x3_f16.hip), the
#: DMA-staged persistent kernel and its upsample form (conv3x3_sp.hip), the fused ends, the level-1 encoder, the wide 3 -> 64 first conv
KERNELS = ("f32", "reg", "c16", "dma", "dma-up", "head", "tail", "l1", "in3wide")
HANDS_IN = ("api", "f32", "sp16", "lds")


def _name32(cout_pad: int, in3: bool, pool: bool, out3: bool) -> str:
    """run_conv's family name of a layer on the fp32 kernel"""
    return "conv3x3_f32<co=%d%s%s%s>" % (min(cout_pad, 128), ",in3" if in3 else "", ",pool" if pool else "", ",out3" if out3 else "")


def predict(kind: str, layers: Sequence[Layer], h: int, w: int, switches: Dict[str, int] = {}) -> Prediction:
    """What one wct_encode (h x w image) / wct_decode (h x w feature) of a loadable layer list launches.  The sizes only matter
    through conv_sp_up_form's even-size rule, which every upsampled map meets."""
    assert set(switches) <= set(SWITCHES), switches
    assert wm.loadable(kind, list(layers)), layers
    mode1 = switches.get("conv_mode", 1) == 1
    sp = mode1 and bool(switches.get("sp", 1))
    fuse = mode1 and bool(switches.get("fuse", 1))
    upconv = bool(switches.get("upconv", 1))
    n = len(layers)
    names: List[str] = []
    hand: List[str] = []
    kernels: List[str] = []

    def runs_f16(i: int) -> bool:        # conv_runs_f16: every layer behind an image input has split-f16 weights
        return mode1 and not (kind == "enc" and i == 0) and layers[i].cin % 8 == 0

    def launch(i: int, cur_sp: bool, out_sp: bool, up_in: bool) -> None:     # run_conv
        l = layers[i]
        cp = wm.pad_cout(l.cout)
        in3, out3 = kind == "enc" and i == 0, kind == "dec" and i + 1 == n
        f16 = runs_f16(i)
        assert f16 or not (cur_sp or (out_sp and not in3)), "SP16 activations need the f16x3 path"
        if not f16:
            names.append(_name32(cp, in3, l.pool_after, out3))
            kernels.append("f32")
            return
        dma = cur_sp and _sp_ok(l.cin, l.cout, cp, out3)
        # wup16 (wct_load_module): per-parity weights where cin % 16 == 0, cout_pad >= 32, no pool, not the last layer
        up = dma and up_in and upconv and cp >= 32 and not l.pool_after
        names.append(_family(cp, l.pool_after, out3, dma, up))
        kernels.append("dma-up" if up else "dma" if dma else "c16" if cp == 16 else "reg")

    cur_sp = False
    if kind == "enc":
        def wants_sp(i: int) -> bool:
            return sp and i + 1 < n and layers[i].cout % 8 == 0 and runs_f16(i + 1)
        i0 = 0
        l0 = layers[0]
        if fuse and n >= 2 and l0.cout == 16 and (layers[1].cin, layers[1].cout, layers[1].pool_after) == (16, 16, True):
            names.append("enc_head_fused<3-16-16,pool>")
            kernels += ["head", "head"]
            cur_sp = wants_sp(1)
            hand.append("lds")
            if n > 2:
                hand.append("sp16" if cur_sp else "f32")
            i0 = 2
        elif fuse and n == 1 and l0.cout <= 32:
            names.append("l1_encode<3-24>")
            kernels.append("l1")
            i0 = 1
        for i in range(i0, n):
            l = layers[i]
            img_in = i == 0 and not l.pool_after and l.cout % 16 == 0
            out_sp = (runs_f16(i) or img_in) and wants_sp(i)
            if i == 0 and fuse and l.cout == 64:
                names.append("conv3x3_fp32<co=64,in3>")
                kernels.append("in3wide")
            else:
                launch(i, cur_sp, out_sp, False)
            if i + 1 < n:
                hand.append("sp16" if out_sp else "f32")
            cur_sp = out_sp
    else:
        for i, l in enumerate(layers):
            last = i + 1 == n
            up_in = i > 0 and layers[i - 1].up_after
            if fuse and i + 2 == n and (l.cin, l.cout) == (16, 16) and layers[i + 1].cin == 16 and not l.up_after:
                names.append("dec_tail_fused<16-16-3>")
                kernels += ["tail", "tail"]
                hand.append("lds")
                break
            out_sp = sp and not last and runs_f16(i) and l.cout % 8 == 0 and runs_f16(i + 1)
            launch(i, cur_sp, out_sp, up_in)
            if not last:
                hand.append("sp16" if out_sp else "f32")
            cur_sp = out_sp
    assert len(hand) == n - 1 and len(kernels) == n, (layers, hand, kernels)
    return Prediction(tuple(names), tuple(hand), tuple(kernels))


def pairs(kind: str, layers: Sequence[Layer], h: int, w: int, switches: Dict[str, int] = {}):
    """(hand-over in, kernel kind) of every layer of one call; "api": the caller's image / fp32 NHWC feature"""
    p = predict(kind, layers, h, w, switches)
    return {(hin, k) for hin, k in zip(("api",) + p.hand, p.kernels)}


#: (hand-over in, kernel) pairs no call can produce, with the rule that excludes each.  Every other pair of HANDS_IN x KERNELS is
#: reachable and occurs in the plan (tests/test_conv_cases_cpu.py)
UNREACHABLE_PAIRS = {
    ("sp16", "f32"): "wants_sp / out_sp: a layer writes SP16 only for a consumer that runs in f16x3, and the fp32 kernel reads fp32 NHWC alone",
    ("api", "dma"): "run_conv: the DMA-staged kernel is chosen only for an SP16 input; the API hands over fp32",
    ("f32", "dma"): "run_conv: the DMA-staged kernel is chosen only for an SP16 input",
    ("lds", "dma"): "a fused kernel's inner hand-over stays in LDS; both fused ends are 16-cout layers, below the DMA kernel's 32",
    ("api", "dma-up"): "the first decoder layer reads no upsampled map and no SP16",
    ("f32", "dma-up"): "conv_sp_up_form is asked only for a layer already on the DMA kernel (SP16 input)",
    ("lds", "dma-up"): "as (lds, dma)",
    ("f32", "head"): "the fused head starts at the image", ("sp16", "head"): "the fused head starts at the image",
    ("f32", "l1"): "l1_encode is a one-layer encoder: its input is the image", ("sp16", "l1"): "as (f32, l1)", ("lds", "l1"): "as (f32, l1)",
    ("f32", "in3wide"): "the wide first conv reads the image", ("sp16", "in3wide"): "as (f32, in3wide)", ("lds", "in3wide"): "as (f32, in3wide)",
    ("lds", "f32"): "a fused kernel's second layer is part of that kernel", ("lds", "reg"): "as (lds, f32)", ("lds", "c16"): "as (lds, f32)",
}

#: (cin class, cout class, variant) cells the loader cannot reach: none -- every multiple of 4 up to 512 is loadable in the middle of a
#: module, with a pool behind it in an encoder and an upsample in front of it in a decoder.  What the LAUNCHERS cannot reach is a
#: property of (hand-over, kernel) pairs and of the DMA kernel's shape rule, listed here by name:
UNREACHABLE_CELLS = {
    "dma kernel x cin class f32 / half": "conv_sp_supported: cin % 16 == 0",
    "dma kernel x cout class pad16": "conv_sp_supported: cout_pad >= 32 (the 16-cout layers run conv3x3_f16_c16_kernel on SP16 input)",
    "dma kernel x cout % 8 == 4": "conv_sp_supported: cout % 8 == 0 (a ragged tail of whole 8-channel halves only)",
    "upsample form x (cin class f32 / half, cout class pad16, enc, enc-pool, dec)": "wct_load_module packs wup16 only where cin % 16 == 0, "
        "cout_pad >= 32, behind an upsample, neither pooling nor last; everything else behind an upsample runs nine taps on the gathered halo",
    "SP16 out x cout % 8 == 4": "wants_sp / out_sp: cout % 8 == 0",
    "SP16 out x cin class f32": "out_sp needs the producer itself on the f16x3 path (or the image-input conv with cout % 16 == 0, no pool)",
}


# --------------------------------------------------------------------------------------------------------- the plan
class Module(collections.namedtuple("Module", "kind level layers lut line variant sizes")):
    """One module to load and the sizes to run it at.  lut: index of the layer under test; line: "I", "II", "II-first", "III-alone",
    "III-pool"."""
    __slots__ = ()

    @property
    def cin(self) -> int:
        return self.layers[self.lut].cin

    @property
    def cout(self) -> int:
        return self.layers[self.lut].cout

    @property
    def key(self) -> str:
        return "%s%d" % ("e" if self.kind == "enc" else "d", self.level)

    @property
    def id(self) -> str:
        return "%s %s %s" % (self.variant, self.line, "-".join([str(self.layers[0].cin)] + [str(l.cout) + ("p" if l.pool_after else "u" if l.up_after else "")
                                                                                      for l in self.layers]))

    @property
    def seed(self) -> int:
        return 9000 + 7 * self.cin + 4099 * self.cout + 1000003 * (VARIANTS.index(self.variant) if self.variant in VARIANTS else 5) + len(self.layers)


def middle(variant: str, a: int, b: int, line: str = "I") -> Module:
    """the layer under test a -> b neither first nor last"""
    if variant in ("enc", "enc-pool"):
        layers = (Layer("p0", 3, 16), Layer("p1", 16, a), Layer("t", a, b, pool_after=variant == "enc-pool"), Layer("c", b, 8))
        return Module("enc", 2 if variant == "enc-pool" else 1, layers, 2, line, variant, SIZES[variant])
    layers = (Layer("p1", 16, a, up_after=variant == "dec-up"), Layer("t", a, b), Layer("c", b, 3))
    return Module("dec", 2 if variant == "dec-up" else 1, layers, 1, line, variant, SIZES[variant])


def first_dec(a: int, b: int) -> Module:
    """a -> b as the first decoder layer: fp32 NHWC straight from the API"""
    return Module("dec", 1, (Layer("t", a, b), Layer("c", b, 3)), 0, "II-first", "dec", SIZES["dec"])


def first_enc(b: int, followed: bool) -> Module:
    """3 -> b alone (the level-1 forms) or followed by [b -> 16 (pool)][16 -> 8] (the in3 kernels, the SP16 hand-over rule, the fused head)"""
    if not followed:
        return Module("enc", 1, (Layer("t", 3, b),), 0, "III-alone", "first", SIZES["enc"])
    return Module("enc", 2, (Layer("t", 3, b), Layer("c1", b, 16, pool_after=True), Layer("c2", 16, 8)), 0, "III-pool", "first", SIZES["enc-pool"])


@functools.lru_cache(maxsize=None)
def modules(band: int, variant: str) -> Tuple[Module, ...]:
    """Lines I and II of one band and variant (duplicates removed); variant "dec" carries Line II's first-layer decoders of the band's
    couts as well."""
    out: Dict[Tuple, Module] = {}
    for a in S.BANDS[band]:
        for b in REP_COUT:
            out.setdefault((a, b, 0), middle(variant, a, b, "I"))
    for b in S.BANDS[band]:
        for a in REP_CIN:
            out.setdefault((a, b, 0), middle(variant, a, b, "II"))
            if variant == "dec":
                out.setdefault((a, b, 1), first_dec(a, b))
    return tuple(out.values())


@functools.lru_cache(maxsize=None)
def first_modules(followed: bool) -> Tuple[Module, ...]:
    return tuple(first_enc(b, followed) for b in FIRST_COUT)


def all_modules() -> List[Module]:
    return [m for v in VARIANTS for b in range(S.N_BANDS) for m in modules(b, v)] + list(first_modules(False)) + list(first_modules(True))


def arms(m: Module) -> Tuple[Tuple[Tuple[str, int], ...], ...]:
    """the switches (one at a time) that change m's path: the prediction under the switch differs from the default one"""
    h, w = m.sizes[0]
    base = predict(m.kind, m.layers, h, w)
    return tuple(((k, 0),) for k in SWITCHES if predict(m.kind, m.layers, h, w, {k: 0}) != base)


@functools.lru_cache(maxsize=None)
def switch_modules(variant: str) -> Tuple[Module, ...]:
    """One module per (cin class, cout class) cell of the variant: the cheapest of the plan's (smallest cin x cout), and every module
    of the variant whose default path has a fused kernel (its "fuse" arm).  Every cell is reachable (UNREACHABLE_CELLS names what is
    not, in other terms)."""
    best: Dict[Tuple[str, str], Module] = {}
    fused: Dict[Tuple, Module] = {}
    for b in range(S.N_BANDS):
        for m in modules(b, variant):
            if any("fused" in n for n in predict(m.kind, m.layers, *m.sizes[0]).names):
                fused[(m.cin, m.cout, m.line == "II-first")] = m
            if m.line == "II-first":
                continue
            cell = (cin_class(m.cin), cout_class(m.cout))
            if cell not in best or (m.cin * m.cout, m.cin) < (best[cell].cin * best[cell].cout, best[cell].cin):
                best[cell] = m
    out = [best[c] for c in sorted(best)]
    return tuple(out + [m for k, m in sorted(fused.items()) if m not in out])
