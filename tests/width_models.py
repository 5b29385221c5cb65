"""Custom-width models for the width tests (tests/test_widths_cpu.py, tests/test_widths_gpu.py).  CPU only: no torch, no GPU.

`wct_load_module` accepts any layer graph whose widths are multiples of 4 and at most 512, and the kernels behind it branch on width
(cout padding and cout groups, cin % 8 / cin % 16, partial 16-channel chunks, the fold and solve variants, the fused level-1 kernels).
The shipped models exercise a handful of those branches.  This module describes other widths as data:

    widths  {1..5: width of VGG block k, "l1": width of the level-1 encoder}

with the layer graph of wct_hip/model_zoo.py (VGG-19 order, pool after conv12/22/34/44, upsample after conv51/41/31/21, level 1 as
one conv), seeded stand-in weights built the way model_zoo.synth_weights builds them, and the fp64 ("truth") and fp32 (the
reference's arithmetic) restatements of a level from oracle/wct_oracle.py's operators.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from oracle import wct_oracle
from wct_hip import model_zoo
from wct_hip.model_zoo import Layer

# --------------------------------------------------------------------------------------------------------- gates
#: encoder / decoder stacks against fp64, relative to max |ref| (the oracle gate of the shipped widths)
ENC_DEC_GATE = 2e-5
#: raw moments of an encoded feature (the level-1 split entry points) against fp64
MOM_GATE = 1e-6

# --------------------------------------------------------------------------------------------------------- width cases
#: the shipped 16x widths (checked against model_zoo by the CPU tests)
W16X = {1: 16, 2: 32, 3: 64, 4: 128, 5: 128, "l1": 24}

#: full models for the conv-family sweep (test_widths_gpu.py section a)
MODELS = {
    # cin % 8 == 4 (fp32 convs inside f16x3 mode), padded cout_pad, fold_affine at ipad 48 / 112, level 1 at 28 channels
    "A": {1: 12, 2: 20, 3: 36, 4: 68, 5: 100, "l1": 28},
    # partial last 16-channel chunks with SP16 fed to a non-DMA consumer, cout_pad 256 in cout groups (small-map form too), C = 136
    "B": {1: 24, 2: 40, 3: 56, 4: 88, 5: 136, "l1": 20},
    # in3 fp32 with cout 48, the DMA kernel and its 2x2 upsample form, cout_pad 384 (3 groups), fold_gemm at d5, solves at 256 / 384
    "C": {1: 48, 2: 80, 3: 160, 4: 256, 5: 384, "l1": 48},
}

#: level-1 encoder widths (section b): 17..24 run the fused level-1 kernels, 25..32 must take the layer-wise path
L1_WIDTHS = (4, 8, 12, 16, 20, 24, 28, 32)

#: feature widths of the moments / solve sweep (section c): ns_pad 192 / 320 / 448 and partial chunks
MOMENT_WIDTHS = (4, 12, 20, 36, 100, 132, 196, 260, 388, 508)

#: module shapes that `wct_load_module` must refuse (no conv kernel runs them): (name, kind, level, [(cin, cout, pool, up), ...])
REFUSED = (
    ("enc_first_cout_68", "enc", 1, [(3, 68, 0, 0)]),
    ("enc_first_cout_128", "enc", 2, [(3, 128, 0, 0), (128, 128, 1, 0), (128, 64, 0, 0)]),
    ("enc_first_pool", "enc", 2, [(3, 16, 1, 0), (16, 32, 0, 0)]),
    ("enc_upsample", "enc", 2, [(3, 16, 0, 1), (16, 32, 0, 0)]),
    ("dec_pool", "dec", 2, [(32, 16, 1, 0), (16, 3, 0, 0)]),
)

#: kernel families (wct_profile_read names) that wct_encode + wct_decode of every level of a model must run in f16x3 mode (conv mode 1),
#: and family substrings that must not appear.  Conv mode 0 runs conv3x3_f32 only.
FAMILIES = {
    # every cin is 4 mod 8: all convs fp32 inside f16x3 mode; level 1 (28 channels) through l1_encode
    "A": (("conv3x3_f32<co=16,in3>", "conv3x3_f32<co=16,pool>", "conv3x3_f32<co=32,pool>", "conv3x3_f32<co=128>",
           "conv3x3_f32<co=16,out3>", "l1_encode<3-24>"), ("f16x3",)),
    # cin 24 / 40 / 56 / 88 / 136: partial last chunks, SP16 into the register-staged kernel, never the DMA kernel
    "B": (("conv3x3_f32<co=32,in3>", "conv3x3_f16x3<co=32,pool>", "conv3x3_f16x3<co=64>", "conv3x3_f16x3<co=64,pool>",
           "conv3x3_f16x3<co=128>", "l1_encode<3-24>"), (",dma",)),
    # cin % 16 == 0 behind the first conv: the DMA kernel, its upsample form, cout groups of 128
    "C": (("conv3x3_f32<co=64,in3>", "conv3x3_f16x3<co=64,pool,dma>", "conv3x3_f16x3<co=128,dma>", "conv3x3_f16x3<co=128,dma,up>",
           "conv3x3_f16x3<co=128,pool,dma>", "conv3x3_f16x3<co=16,out3>"), ("l1_",)),
}


def pad_cout(c: int) -> int:
    """wct_api.hip pad_cout"""
    return 16 if c <= 16 else 32 if c <= 32 else 64 if c <= 64 else (c + 127) // 128 * 128


def loadable(kind: str, layers: List[Layer]) -> bool:
    """The shape rules of wct_load_module (with the refusals of shapes no conv kernel runs)."""
    for i, l in enumerate(layers):
        first, last = i == 0, i == len(layers) - 1
        if not (1 <= l.cin <= 512 and 1 <= l.cout <= 512):
            return False
        if i > 0 and layers[i - 1].cout != l.cin:
            return False
        if kind == "enc" and first and l.cin != 3:
            return False
        if kind == "dec" and last and l.cout != 3:
            return False
        if not (kind == "enc" and first) and l.cin % 4:
            return False
        if not (kind == "dec" and last) and l.cout % 4:
            return False
        if kind == "enc" and last and l.pool_after or kind == "dec" and last and l.up_after:
            return False
        if kind == "enc" and (l.up_after or first and (l.cout > 64 or l.pool_after)):
            return False
        if kind == "dec" and l.pool_after:
            return False
    return True


# --------------------------------------------------------------------------------------------------------- layer graph
def encoder_layers(widths: Dict, level: int) -> List[Layer]:
    """model_zoo.encoder_layers with the widths as data."""
    assert 1 <= level <= 5
    out: List[Layer] = []
    cin = 3
    last = model_zoo._LAST_OF_LEVEL[level]
    for name in model_zoo._VGG_ORDER:
        cout = widths["l1"] if level == 1 else widths[model_zoo._block(name)]
        out.append(Layer(name, cin, cout, pool_after=name in model_zoo._POOL_AFTER and name != last))
        cin = cout
        if name == last:
            break
    return out


def decoder_layers(widths: Dict, level: int) -> List[Layer]:
    """model_zoo.decoder_layers: the mirror of the encoder, upsampling after conv51/41/31/21."""
    enc = encoder_layers(widths, level)
    return [Layer(l.name, l.cout, l.cin, up_after=(l.name in model_zoo._UP_AFTER and i < len(enc) - 1))
            for i, l in enumerate(reversed(enc))]


def feature_channels(widths: Dict, level: int) -> int:
    return widths["l1"] if level == 1 else widths[level]


def level1_widths(C: int) -> Dict:
    """A model whose level-1 encoder has C channels (the other blocks as 16x; only level 1 is loaded from it)."""
    return dict(W16X, l1=C)


# --------------------------------------------------------------------------------------------------------- weights
def synth(widths: Dict, seed: int, levels=(1, 2, 3, 4, 5)) -> Dict[str, np.ndarray]:
    """model_zoo.synth_weights for custom widths: He-uniform filters from Generator.random only, the fixed conv0 of the un-pruned
    encoders, the last decoder conv scaled by 1/128 (features are O(100): the decoded image stays O(1))."""
    rng = np.random.default_rng(seed)
    w: Dict[str, np.ndarray] = {}
    for level in levels:
        for kind, layers in (("enc", encoder_layers(widths, level)), ("dec", decoder_layers(widths, level))):
            key = model_zoo.module_key(kind, level)
            if kind == "enc":
                w[key + ".conv0.weight"] = model_zoo.ORIGINAL_CONV0_W.copy()
                w[key + ".conv0.bias"] = model_zoo.ORIGINAL_CONV0_B.copy()
            for l in layers:
                a = np.sqrt(6.0 / (9 * l.cin))
                wt = (rng.random((l.cout, l.cin, 3, 3)) * 2.0 - 1.0) * a
                if kind == "dec" and l.cout == 3:
                    wt = wt * (1.0 / 128.0)
                w["%s.%s.weight" % (key, l.name)] = wt.astype(np.float32)
                w["%s.%s.bias" % (key, l.name)] = ((rng.random(l.cout) * 0.1) + (0.2 if (kind == "dec" and l.cout == 3) else 0.0)).astype(np.float32)
    return w


def smooth_image(rng: np.random.Generator, H: int, W: int, passes: int = 2) -> np.ndarray:
    """A [0, 1) 3 x H x W test image with some spatial correlation (as smoke()'s)."""
    x = rng.random((3, H, W), dtype=np.float32)
    for _ in range(passes):
        x = (x + np.roll(x, 1, 1) + np.roll(x, 1, 2) + np.roll(x, -1, 1) + np.roll(x, -1, 2)) / 5
    return np.ascontiguousarray(x, np.float32)


# --------------------------------------------------------------------------------------------------------- references
def encode(widths: Dict, w: Dict, level: int, img: np.ndarray, f64: bool = True) -> np.ndarray:
    """Encoder level `level` on a CHW image: fp64 (the yardstick) or fp32 (the reference's arithmetic, oracle.Modules.encode)."""
    key = "e%d" % level
    if f64:
        w0 = np.asarray(w[key + ".conv0.weight"], np.float64).reshape(3, 3)
        y = np.einsum("kc,chw->khw", w0, np.asarray(img, np.float64)) + np.asarray(w[key + ".conv0.bias"], np.float64)[:, None, None]
        conv = wct_oracle.conv3x3_reflect_f64
    else:
        y = wct_oracle.conv1x1(img, w[key + ".conv0.weight"], w[key + ".conv0.bias"])
        conv = wct_oracle.conv3x3_reflect
    for l in encoder_layers(widths, level):
        y = conv(y, w["%s.%s.weight" % (key, l.name)], w["%s.%s.bias" % (key, l.name)], True)
        if l.pool_after:
            y = wct_oracle.maxpool2(y)
    return y


def decode(widths: Dict, w: Dict, level: int, feat: np.ndarray, f64: bool = True) -> np.ndarray:
    """Decoder level `level` on a CHW feature (ReLU after every conv, nearest x2 after conv51/41/31/21)."""
    key = "d%d" % level
    y = np.ascontiguousarray(feat, np.float64 if f64 else np.float32)
    conv = wct_oracle.conv3x3_reflect_f64 if f64 else wct_oracle.conv3x3_reflect
    for l in decoder_layers(widths, level):
        y = conv(y, w["%s.%s.weight" % (key, l.name)], w["%s.%s.bias" % (key, l.name)], True)
        if l.up_after:
            y = wct_oracle.upsample2(y)
    return y


def raw_moments(F: np.ndarray, x0: int = 0, x1: int = None):
    """Raw fp64 (sum[C], sum of x x^T [C, C]) of a CHW feature over columns [x0, x1) -- what wct_moments returns."""
    C, h, w = F.shape
    x1 = w if x1 is None else x1
    X = np.asarray(F, np.float64)[:, :, x0:x1].reshape(C, -1)
    return X.sum(axis=1), X @ X.T


def decode_affine(widths: Dict, w: Dict, level: int, feat: np.ndarray, M: np.ndarray, b: np.ndarray, f64: bool = True) -> np.ndarray:
    """decoder(M f + b): what wct_content_decode computes from a given (M, b)."""
    C = feat.shape[0]
    y = (np.asarray(M, np.float64) @ np.asarray(feat, np.float64).reshape(C, -1) + np.asarray(b, np.float64)[:, None]).reshape(feat.shape)
    return decode(widths, w, level, y if f64 else y.astype(np.float32), f64)


def style_transfer(widths: Dict, w: Dict, level: int, content: np.ndarray, style: np.ndarray, alpha: float, f64: bool = True) -> np.ndarray:
    """One level (WCT.py:98-106) in fp64 or in the reference's fp32 arithmetic (oracle.style_transfer)."""
    cF = encode(widths, w, level, content, f64)
    sF = encode(widths, w, level, style, f64)
    csF = wct_oracle.transform(cF, sF, alpha, out_dtype=np.float64 if f64 else np.float32)[0]
    return decode(widths, w, level, csF, f64)
