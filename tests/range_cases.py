"""The f16x3 range flag as data (tests/test_range_cpu.py, tests/test_range_gpu.py).  CPU only: no torch, no GPU at import.

Conv mode 1 stores every intermediate activation as hi + lo in f16 and clamps it to +-65504; include/wct_hip.h promises that no clamp
is silent.  This module lists

    SITES         every clamp site of every `__global__` kernel that carries a SatTrack::commit or a sat_raise, with the probes that drive it
    MODELS        small purpose-built layer lists (loaded through wct_load_module) that put those kernels on the path
    probes()      (model, target, position, variant) cases: weights + input whose fp64 walk exceeds the range at exactly ONE site ("over"), or
                  peaks just below it at that site ("under": nothing may flag)
    clamped_walk  width_models.encode / decode with np.clip(., lo, 65504) wherever the device stores split halves
    RANGE_EXPECT  every family of tests/state_cases.py (and of the colour / smoothing / transform / swap methods): does a call of it run
                  f16x3 convolutions on its inputs ("flags") or not ("clean")

The carrier.  A probe's weights are He-uniform stand-ins (as width_models.synth) with conv0 = identity, plus K carrier channels
0 .. K-1: the first layer copies image plane 0 into each of them (centre tap 1.0, nothing else in), every layer before the target hands
them on unchanged (centre tap 1.0 channel j -> channel j, no other weight into or out of them), and at the target layer ONE output
channel takes g x (sum of the carriers) through the centre tap on top of its ordinary weights.  Plane 0 is a non-negative pattern
(baseline 1, one spike of amplitude A): ReLU, max-pool and nearest upsampling keep it.  g is 8 x the He bound of the target layer (so the
layer's split-f16 weight scale moves by three bits at most) and A <= 0.45 x 65504 (so the carrier itself is no clamp site); K is the
smallest count with K g A >= 1.15 x 65504.  With g bounded like that ONE carrier does not reach the range behind a 16-channel layer: K
channels that carry the same pattern do.
"""
from __future__ import annotations

import collections
import functools
import math
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import wct_oracle
from tests import geometry_cases as gc
from tests import width_models as wm
from wct_hip.model_zoo import Layer

RANGE = 65504.0
NOTE_HI_FROM = 65488.0        # note_hi() fires from here on (everything that rounds to the largest f16)
OVER_MIN, OTHERS_MAX, UNDER_LO, UNDER_HI = 1.1, 0.5, 0.85, 0.92

# --------------------------------------------------------------------------------------------------------- the sites
#: kind: "input" = external fp32 data split on the way into LDS (range AND NaN, note_hi(.., false));
#:       "lds"   = intermediate of a fused kernel that never leaves LDS;
#:       "sp16"  = SP16 output of an epilogue (the consumer takes the split as it is)
Site = collections.namedtuple("Site", "kernel file name kind what probes")
SITES = (
    Site("conv3x3_kernel", "conv3x3.hip", "out", "sp16", "sp16_store4 of the fp32 image-input conv (3 -> 16 k couts) feeding an f16x3 layer", ("f32in3:0",)),
    Site("conv3x3_f16_kernel", "conv3x3_f16.hip", "in", "input", "commit_act / split8 of an fp32 NHWC feature", ("dec:in", "f128:in")),
    Site("conv3x3_f16_kernel", "conv3x3_f16.hip", "out", "sp16", "sp16_pair_exchange, unpooled epilogue", ("dec:0", "f128:0")),
    Site("conv3x3_f16_kernel", "conv3x3_f16.hip", "out_pool", "sp16", "sp16_pair_exchange, pooled epilogue", ("sp64:3",)),
    Site("conv3x3_f16_c16_kernel", "conv3x3_f16.hip", "in", "input", "commit_act / split8 of an fp32 NHWC feature (<= 16 couts)", ("dec16:in",)),
    Site("conv3x3_f16_c16_kernel", "conv3x3_f16.hip", "out", "sp16", "sp16_store4 of the 16-cout kernel", ("dec:2", "dec16:0")),
    Site("enc_head_kernel", "conv3x3_f16.hip", "in", "input", "head_commit of the image window", ("head:in",)),
    Site("enc_head_kernel", "conv3x3_f16.hip", "conv11", "lds", "store_split4<true> of conv11 (16 channels, LDS)", ("head:0",)),
    Site("enc_head_kernel", "conv3x3_f16.hip", "out_pool", "sp16", "pooled conv12 output as SP16", ("head:1",)),
    Site("enc_head_roles_kernel", "conv3x3_f16.hip", "in", "input", "the two-role head's own staging of the image (producer waves)", ("roles:in",)),
    Site("enc_head_roles_kernel", "conv3x3_f16.hip", "conv11", "lds", "store_split4<true> of conv11 by the producer waves", ("roles:0",)),
    Site("enc_head_roles_kernel", "conv3x3_f16.hip", "out_pool", "sp16", "pooled conv12 output of the consumer waves as SP16", ("roles:1",)),
    Site("dec_tail_kernel", "conv3x3_f16.hip", "in", "input", "tail_commit / split8 of an fp32 16-channel feature", ("tail:in",)),
    Site("dec_tail_kernel", "conv3x3_f16.hip", "conv12", "lds", "store_split4<true> of conv12 (16 channels, LDS), nine-tap form", ("tail:0",)),
    # (no entry point hands this kernel external data: an fp32 feature reaches it only from the layer in front of the upsample with the SP16
    # hand-over switched off -- so its values are non-negative and finite, and the probe's target is that layer's output)
    Site("dec_tail_up_kernel", "conv3x3_f16.hip", "in", "input", "split8 of an fp32 16-channel feature behind an upsample (debug key sp = 0)", ("up16sp0:0",)),
    Site("dec_tail_up_kernel", "conv3x3_f16.hip", "conv12", "lds", "store_split4<true> of conv12 (16 channels, LDS), upsample form", ("dec:3", "up16:1")),
    Site("conv3x3_sp_kernel", "conv3x3_sp.hip", "out", "sp16", "__ballot record of the unpooled epilogue (parked and final flush)", ("sp64:2", "big512:2")),
    Site("conv3x3_sp_kernel", "conv3x3_sp.hip", "out_pool", "sp16", "__ballot record of the pooled epilogue", ("sp64p:2",)),
    Site("conv3x3_sp3_kernel", "conv3x3_sp.hip", "out", "sp16", "__ballot record of the 32-cout kernel, unpooled", ("head:2", "big32:2")),
    Site("conv3x3_sp3_kernel", "conv3x3_sp.hip", "out_pool", "sp16", "__ballot record of the 32-cout kernel, pooled", ("sp32p:2",)),
    Site("conv3x3_sp_up_kernel", "conv3x3_sp.hip", "out", "sp16", "__ballot record of the upsample form", ("dec:1", "bigup:1")),
    Site("l1_encode_kernel", "level1.hip", "in", "input", "head_commit of the image window", ("l1:in@encode",)),
    Site("l1_decode_kernel", "level1.hip", "in", "input", "head_commit of the image window", ("l1:in@split",)),
    Site("l1_decode_kernel", "level1.hip", "conv11", "lds", "store_split4<true> / store_split4_half of the 24-channel relu1_1 map (LDS)", ("l1:0@split",)),
    Site("in3_wide_kernel", "level1.hip", "in", "input", "head_commit of the image window (f16x3 products, in3wide = 1)", ("wide1:in",)),
    Site("in3_wide_kernel", "level1.hip", "out", "sp16", "split4 of the 64-cout first conv, f16x3 products", ("wide1:0",)),
    Site("in3_wide_f32_kernel", "level1.hip", "out", "sp16", "split4 of the 64-cout first conv, exact-fp32 products (the image is not split)", ("wide:0",)),
    Site("l1_moments_kernel", "moments.hip", "in", "input", "head_commit of the image window", ("l1:in@split",)),
    Site("swap_match_kernel", "swap.hip", "in", "input", "stage_tile / split8 of Q and K", ("swap",)),
)

# --------------------------------------------------------------------------------------------------------- probe models
#: name -> (kind, slot (the level the module is loaded as; an encoder's is 1 + its pools, which is how wct_feature_shape sizes the feature), [(cin, cout, pool_after, up_after)], (H, W) of the input (image, or feature of a
#: decoder), op, switches, profile families the call must show in conv mode 1).  H % 8 != 0 and W % 32 != 0 at the input and, where the
#: layer graph allows it, at the target's resolution.
Model = collections.namedtuple("Model", "kind slot spec size op switches families")
MODELS = {
    "head": Model("enc", 2, [(3, 16, 0, 0), (16, 16, 1, 0), (16, 32, 0, 0), (32, 32, 0, 0)], (43, 77), "encode", (),
                  ("enc_head_fused<3-16-16,pool>", "conv3x3_f16x3<co=32,dma>")),
    "sp32p": Model("enc", 3, [(3, 16, 0, 0), (16, 16, 1, 0), (16, 32, 1, 0), (32, 32, 0, 0)], (43, 77), "encode", (),
                   ("conv3x3_f16x3<co=32,pool,dma>",)),
    # 56 of 64 couts: the last real channel is not the last padded one; its consumer (cin 56) is the register-staged kernel reading SP16
    "sp64": Model("enc", 3, [(3, 16, 0, 0), (16, 16, 1, 0), (16, 56, 0, 0), (56, 64, 1, 0), (64, 64, 0, 0)], (43, 77), "encode", (),
                  ("conv3x3_f16x3<co=64,dma>", "conv3x3_f16x3<co=64,pool>")),
    "sp64p": Model("enc", 3, [(3, 16, 0, 0), (16, 16, 1, 0), (16, 64, 1, 0), (64, 64, 0, 0)], (43, 77), "encode", (),
                   ("conv3x3_f16x3<co=64,pool,dma>",)),
    "wide": Model("enc", 1, [(3, 64, 0, 0), (64, 64, 0, 0)], (21, 45), "encode", (), ("conv3x3_fp32<co=64,in3>",)),
    "wide1": Model("enc", 1, [(3, 64, 0, 0), (64, 64, 0, 0)], (21, 45), "encode", (("in3wide", 1),), ("conv3x3_f16x3<co=64,in3>",)),
    "f32in3": Model("enc", 1, [(3, 48, 0, 0), (48, 48, 0, 0)], (21, 45), "encode", (), ("conv3x3_f32<co=64,in3>",)),
    # the level-1 pair: layer 0 is the encoder (3 -> 24), layer 1 the decoder (24 -> 3); wct_content_decode with M = I, b = 0 runs both in
    # l1_decode_kernel, where the 24-channel map lives in LDS
    "l1": Model("enc", 1, [(3, 24, 0, 0), (24, 3, 0, 0)], (21, 45), "l1", (), ("l1_encode<3-24>", "l1_moments_fused<3-24>", "l1_decode_fused<3-24-3>")),
    "dec": Model("dec", 3, [(64, 32, 0, 1), (32, 32, 0, 0), (32, 16, 0, 1), (16, 16, 0, 0), (16, 3, 0, 0)], (11, 19), "decode", (),
                 ("conv3x3_f16x3<co=32>", "conv3x3_f16x3<co=32,dma,up>", "conv3x3_f16x3<co=16>", "dec_tail_fused<16-16-3>")),
    "dec16": Model("dec", 4, [(32, 16, 0, 0), (16, 16, 0, 0), (16, 16, 0, 0), (16, 3, 0, 0)], (21, 45), "decode", (),
                   ("conv3x3_f16x3<co=16>", "dec_tail_fused<16-16-3>")),
    "tail": Model("dec", 2, [(16, 16, 0, 0), (16, 3, 0, 0)], (21, 45), "decode", (), ("dec_tail_fused<16-16-3>",)),
    # the fused tail behind an upsample fed by the 16-cout kernel; 128 couts from an fp32 feature (the small-map form at this size)
    "up16": Model("dec", 2, [(32, 16, 0, 1), (16, 16, 0, 0), (16, 3, 0, 0)], (21, 45), "decode", (), ("conv3x3_f16x3<co=16>", "dec_tail_fused<16-16-3>")),
    "f128": Model("dec", 3, [(64, 128, 0, 0), (128, 16, 0, 0), (16, 3, 0, 0)], (21, 45), "decode", (), ("conv3x3_f16x3<co=128>", "conv3x3_f16x3<co=16>")),
    # the same graph with the SP16 hand-over off: the fused tail splits the fp32 output of the layer in front of the upsample itself
    "up16sp0": Model("dec", 2, [(32, 16, 0, 1), (16, 16, 0, 0), (16, 3, 0, 0)], (21, 45), "decode", (("sp", 0),), ("dec_tail_fused<16-16-3>",)),
    # sized per CU count by model_for() (here: 256 CUs).  The two-role head; the persistent kernels with more (tile, cout group) units than workgroups
    "roles": Model("enc", 2, [(3, 16, 0, 0), (16, 16, 1, 0), (16, 32, 0, 0)], (505, 1001), "encode", (), ("enc_head_fused<3-16-16,pool>",)),
    "big512": Model("enc", 2, [(3, 16, 0, 0), (16, 16, 1, 0), (16, 512, 0, 0), (512, 16, 0, 0)], (83, 683), "encode", (), ("conv3x3_f16x3<co=128,dma>",)),
    "big32": Model("enc", 2, [(3, 16, 0, 0), (16, 16, 1, 0), (16, 32, 0, 0), (32, 32, 0, 0)], (515, 1001), "encode", (), ("conv3x3_f16x3<co=32,dma>",)),
    "bigup": Model("dec", 2, [(32, 16, 0, 1), (16, 128, 0, 0), (128, 16, 0, 0), (16, 3, 0, 0)], (41, 341), "decode", (), ("conv3x3_f16x3<co=128,dma,up>",)),
}
#: models whose target layer runs a persistent kernel over more units than workgroups: name -> target layer
BIG = {"big512": 2, "big32": 2, "bigup": 1}

#: "model:target" -> the profile family that must have run the target (the kernel of the Site that names the probe)
TARGET_FAMILY = {
    "f32in3:0": "conv3x3_f32<co=64,in3>", "dec:in": "conv3x3_f16x3<co=32>", "dec:0": "conv3x3_f16x3<co=32>", "f128:in": "conv3x3_f16x3<co=128>",
    "f128:0": "conv3x3_f16x3<co=128>", "sp64:3": "conv3x3_f16x3<co=64,pool>", "dec16:in": "conv3x3_f16x3<co=16>", "dec16:0": "conv3x3_f16x3<co=16>",
    "dec:2": "conv3x3_f16x3<co=16>", "head:in": "enc_head_fused<3-16-16,pool>", "head:0": "enc_head_fused<3-16-16,pool>",
    "head:1": "enc_head_fused<3-16-16,pool>", "roles:in": "enc_head_fused<3-16-16,pool>", "roles:0": "enc_head_fused<3-16-16,pool>",
    "roles:1": "enc_head_fused<3-16-16,pool>", "tail:in": "dec_tail_fused<16-16-3>", "tail:0": "dec_tail_fused<16-16-3>", "dec:3": "dec_tail_fused<16-16-3>",
    "up16:1": "dec_tail_fused<16-16-3>", "up16sp0:0": "dec_tail_fused<16-16-3>", "sp64:2": "conv3x3_f16x3<co=64,dma>", "big512:2": "conv3x3_f16x3<co=128,dma>",
    "sp64p:2": "conv3x3_f16x3<co=64,pool,dma>", "head:2": "conv3x3_f16x3<co=32,dma>", "big32:2": "conv3x3_f16x3<co=32,dma>",
    "sp32p:2": "conv3x3_f16x3<co=32,pool,dma>", "dec:1": "conv3x3_f16x3<co=32,dma,up>", "bigup:1": "conv3x3_f16x3<co=128,dma,up>",
    "l1:in": "l1_decode_fused<3-24-3>", "l1:0": "l1_decode_fused<3-24-3>", "wide1:in": "conv3x3_f16x3<co=64,in3>", "wide1:0": "conv3x3_f16x3<co=64,in3>",
    "wide:0": "conv3x3_fp32<co=64,in3>",
}


def _sp_units(m: "Model", t: int, cus: int):
    th, tw, f = target_dims(m, t)
    cin, cout = m.spec[t][:2]
    return gc.sp_units(th, tw, cin, wm.pad_cout(cout), f < 0, cus)


def model_for(name: str, cus: int = 256) -> "Model":
    """MODELS[name] at the size that reaches its form on a device with `cus` CUs: the two-role head from 4 tiles per CU on, the persistent
    kernels with more units than workgroups.  Every other model has one size."""
    m = MODELS[name]
    H, W = m.size
    if name == "roles":
        H = 9
        while not gc.head_form(H, W, cus).startswith("#r16"):
            H += 16
    elif name in BIG:
        H = {"big512": 83, "big32": 35, "bigup": 41}[name]
        step = 16 if name == "bigup" else 32
        while True:
            _, nt, units, grid = _sp_units(m._replace(size=(H, W)), BIG[name], cus)
            if units > grid:
                break
            H += step
    return m._replace(size=(H, W))


def sp_spot(m: "Model", t: int, cus: int, which: str) -> Tuple[int, int, int]:
    """(y, x, channel) of the target's output inside one (tile, cout group) unit of a persistent kernel (conv3x3_sp.hip: workgroup b serves XCD
    b & 7, whose units -- its tiles x the groups, group fastest -- it walks from b >> 3 in steps of grid / 8; a unit's epilogue is parked and
    runs inside the workgroup's next job, the last one's in the flush behind the loop).  "parked": the first unit of workgroup 0, which has a
    successor; "final": that workgroup's last unit."""
    th, tw, f = target_dims(m, t)
    up = f < 0
    _, nt, units, grid = _sp_units(m, t, cus)
    ng, ustep = units // nt, grid >> 3
    nun = ((nt >> 3) + (1 if nt & 7 else 0)) * ng                 # units of XCD 0, whose tiles start at tile 0
    assert units > grid and nun > ustep, (m, units, grid)
    u = 0 if which == "parked" else (nun - 1) // ustep * ustep
    tile, grp = u // ng, u % ng
    trow, tcol = divmod(tile, -(-(tw // 2 if up else tw) // 32))
    if up:                                                         # low-resolution tiles; group = 2 x (32-cout group) + output row parity
        return 2 * trow * 16 + (grp & 1), 2 * tcol * 32, (grp >> 1) * 32
    return trow * 16, tcol * 32, grp * (wm.pad_cout(m.spec[t][1]) // ng)

#: the tall instantiations of templates that the probes above cover small: name -> (model, targets, the restated launcher that names the form).
#: tests/test_range_gpu.py finds the smallest ragged size at which the launcher takes the form on the device at hand (flag only, no fp64 walk).
TALL = {
    "dec_tail#t16": ("tail", ("in", 0), "dec_tail_fused<16-16-3>", "#t16"),
    "dec_tail#t24": ("tail", ("in", 0), "dec_tail_fused<16-16-3>", "#t24"),
    "dec_tail_up#u16": ("up16", (1,), "dec_tail_fused<16-16-3>", "#u16"),
    "l1_decode#t16": ("l1", ("in", 0), "l1_decode_fused<3-24-3>", "#t16"),
    "conv3x3_f16#t16": ("f128", ("in", 0), "conv3x3_f16x3<co=128>", "#t16"),
}
SEED = 6550


def layers_of(spec) -> List[Layer]:
    return [Layer("L%d" % i, cin, cout, pool_after=bool(p), up_after=bool(u)) for i, (cin, cout, p, u) in enumerate(spec)]


def he_bound(cin: int) -> float:
    return math.sqrt(6.0 / (9 * cin))


def base_weights(key: str, kind: str, layers: List[Layer], seed: int) -> Dict[str, np.ndarray]:
    """width_models.synth for a layer list: He-uniform filters, small positive biases, conv0 = identity, the image conv of a decoder / 128."""
    rng = np.random.default_rng(seed)
    w: Dict[str, np.ndarray] = {}
    if kind == "enc":
        w[key + ".conv0.weight"] = np.eye(3, dtype=np.float32).reshape(3, 3, 1, 1)
        w[key + ".conv0.bias"] = np.zeros(3, np.float32)
    for l in layers:
        wt = (rng.random((l.cout, l.cin, 3, 3)) * 2.0 - 1.0) * he_bound(l.cin)
        if kind == "dec" and l.cout == 3:
            wt = wt / 128.0
        w["%s.%s.weight" % (key, l.name)] = wt.astype(np.float32)
        w["%s.%s.bias" % (key, l.name)] = (rng.random(l.cout) * 0.1).astype(np.float32)
    return w


# --------------------------------------------------------------------------------------------------------- the walks
def _nan_as_device(x: np.ndarray) -> np.ndarray:
    """v_med3_f32(NaN, -65504, 65504) returns the smaller of the other two: a NaN in external data becomes -65504"""
    return np.where(np.isnan(x), -RANGE, x)


def clamped_walk(kind: str, layers: List[Layer], w: Dict[str, np.ndarray], key: str, x: np.ndarray, f64: bool = True, clamp: bool = True,
                 trace: Optional[list] = None) -> np.ndarray:
    """width_models.encode / decode over a layer list, with the device's clamps: the external input to [-65504, 65504] (NaN -> -65504), every
    activation that is handed on to a further layer (behind its ReLU) to [0, 65504].  The last layer writes fp32 and is not clamped.
    clamp = False: the plain walk.  trace: receives (site, max |value|) of every clamped tensor BEFORE its clamp ("in", 0, 1, ...)."""
    dt = np.float64 if f64 else np.float32
    x = np.ascontiguousarray(x, dt)
    if trace is not None:
        trace.append(("in", float(np.nanmax(np.abs(x))) if np.isfinite(x).any() else float("nan")))
    if clamp:
        x = np.clip(_nan_as_device(x), -RANGE, RANGE).astype(dt)
    if kind == "enc":
        if f64:
            w0 = np.asarray(w[key + ".conv0.weight"], np.float64).reshape(3, 3)
            y = np.einsum("kc,chw->khw", w0, x) + np.asarray(w[key + ".conv0.bias"], np.float64)[:, None, None]
        else:
            y = wct_oracle.conv1x1(x, w[key + ".conv0.weight"], w[key + ".conv0.bias"])
    else:
        y = x
    conv = wct_oracle.conv3x3_reflect_f64 if f64 else wct_oracle.conv3x3_reflect
    for i, l in enumerate(layers):
        y = conv(y, w["%s.%s.weight" % (key, l.name)], w["%s.%s.bias" % (key, l.name)], True)
        if l.pool_after:
            y = wct_oracle.maxpool2(y)
        if i + 1 < len(layers):
            if trace is not None:
                trace.append((i, float(np.abs(y).max())))
            if clamp:
                y = np.clip(y, 0.0, RANGE).astype(dt)
        if l.up_after:
            y = wct_oracle.upsample2(y)
    return y


# --------------------------------------------------------------------------------------------------------- probes
Probe = collections.namedtuple("Probe", "id model target pos chan value variant")


def target_dims(m: Model, target) -> Tuple[int, int, int]:
    """(h, w, f) of the clamped tensor: its size, and f > 0: input pixels per target pixel (pools), f < 0: -f target pixels per input pixel
    (a decoder's upsamples in front of the target layer; the clamp sits in front of the layer's own upsample)"""
    H, W = m.size
    if target == "in":
        return H, W, 1
    h, w, down, up = H, W, 1, 1
    for i, (cin, cout, p, u) in enumerate(m.spec):
        if p:
            h, w, down = h // 2, w // 2, down * 2
        if i == target:
            return h, w, (down if up == 1 else -up)
        if u:
            h, w, up = 2 * h, 2 * w, up * 2
    raise ValueError(target)


def probes() -> List[Probe]:
    """Every probe named by SITES: the positions (0, 0) and the last pixel, the first and the last real channel where the target has
    channels of its own, +over / -over / NaN on external inputs, and the under twin of each."""
    out: List[Probe] = []
    named = sorted({p.split("@")[0] for s in SITES for p in s.probes if ":" in p})
    for name in named:
        model, t = name.split(":")
        target = "in" if t == "in" else int(t)
        m = MODELS[model]
        cout = None if target == "in" else m.spec[target][1]
        if model in BIG:               # the channel follows from the unit (sp_spot)
            out += [Probe("%s-L%d-%s-%s" % (model, target, pos, v), model, target, pos, 0, "pos", v) for pos in ("parked", "final") for v in ("over", "under")]
            continue
        for pos in (("last",) if model == "roles" else ("first", "last")):
            chans = (0,) if target == "in" else (0, cout - 1)
            for chan in chans:
                values = ("pos", "neg", "nan") if target == "in" else ("pos",)
                for value in values:
                    for variant in (("over", "under") if value != "nan" else ("over",)):
                        pid = "%s-%s-%s-c%d-%s-%s" % (model, "in" if target == "in" else "L%d" % target, pos, chan, value, variant)
                        out.append(Probe(pid, model, target, pos, chan, value, variant))
    return out


Built = collections.namedtuple("Built", "layers key weights x plain peak carriers")     # plain: the input without its spike


@functools.lru_cache(maxsize=None)
def build(p: Probe, cus: int = 256) -> Built:
    """Weights and input of a probe (deterministic) on its model at the size for `cus` CUs.  `peak` is the amplitude aimed at (in units of 65504)."""
    return build_on(p, model_for(p.model, cus), cus)


def build_on(p: Probe, m: Model, cus: int = 256) -> Built:
    layers = layers_of(m.spec)
    key = ("e%d" if m.kind == "enc" else "d%d") % m.slot
    w = base_weights(key, m.kind, layers, SEED + sum(m.spec[0]) + len(m.spec))
    H, W = m.size
    rng = np.random.default_rng(SEED + 1)
    cin0 = 3 if m.kind == "enc" else m.spec[0][0]
    # ordinary input: a smooth O(1) image, or a non-negative O(1) feature
    x = rng.random((cin0, H, W))
    for _ in range(2 if H * W <= 65536 else 0):          # (large maps: plain noise)
        x = (x + np.roll(x, 1, 1) + np.roll(x, 1, 2) + np.roll(x, -1, 1) + np.roll(x, -1, 2)) / 5
    aim = 1.15 if p.variant == "over" else 0.885
    th, tw, f = target_dims(m, p.target)
    ty, tx, chan = (0, 0, p.chan) if p.pos == "first" else (th - 1, tw - 1, p.chan)
    if p.pos in ("parked", "final"):
        ty, tx, chan = sp_spot(m, int(p.target), cus, p.pos)
    plain = x.copy()
    if p.target == "in":
        x[1, ty, tx] = float("nan") if p.value == "nan" else (aim if p.value == "pos" else -aim) * RANGE
        if m.kind == "enc":      # 65504 x the He bound of a 3-channel layer (0.47) would itself pass half the range behind the first conv
            w[key + ".L0.weight"][:, 1] *= 0.5
        return Built(layers, key, w, x.astype(np.float32), plain.astype(np.float32), aim, 0)
    # the carrier
    t = int(p.target)
    g = 8.0 * he_bound(m.spec[t][0])
    A = 0.45 * RANGE
    K = 1 if (t == 0 and m.kind == "enc") else int(math.ceil(1.15 * RANGE / (g * A)))
    assert K <= min(c for spec in m.spec[:t + 1] for c in spec[:2] if c > 3), (p, K)
    amp = aim * RANGE / (K * g)
    assert amp <= A * 1.0001
    iy, ix = (ty * f, tx * f) if f > 0 else (ty // -f, tx // -f)
    nc = 1 if m.kind == "enc" else K
    x[:nc], plain[:nc] = 1.0, 1.0
    x[:nc, iy, ix] = amp
    for i in range(t + 1):
        wt = w["%s.L%d.weight" % (key, i)].copy()
        bs = w["%s.L%d.bias" % (key, i)].copy()
        src = 1 if (i == 0 and m.kind == "enc") else K        # carrier channels on the input side of layer i (image plane 0 feeds all K)
        if i < t:
            wt[:K] = 0.0
            wt[:, :src] = 0.0
            for j in range(K):
                wt[j, 0 if src == 1 else j, 1, 1] = 1.0
            bs[:K] = 0.0
        else:
            wt[:, :src] = 0.0
            wt[chan, :src, 1, 1] = g
        w["%s.L%d.weight" % (key, i)] = wt
        w["%s.L%d.bias" % (key, i)] = bs
    # behind upsamples the spike is a block of `side` x `side` target pixels, and the consumer's 3 x 3 window adds up to min(9, side^2) taps
    # of it: its weights on the target channel shrink by that count, so that the consumer's own output stays well inside the range
    side = (-f if f < 0 else 1) * (2 if m.spec[t][3] else 1)
    if side > 1:
        w["%s.L%d.weight" % (key, t + 1)][:, chan] /= min(9, side * side)
    return Built(layers, key, w, x.astype(np.float32), plain.astype(np.float32), aim, K)


# --------------------------------------------------------------------------------------------------------- entry points
#: family of tests/state_cases.CASES, or the Python method of a colour / smoothing / transform / swap symbol -> "flags" (the call runs f16x3
#: convolutions on its inputs) | "clean" (moments, solves, applies, resize, noise, colour, guided filter: nothing is stored as split f16)
RANGE_EXPECT = {
    "stylize": "flags", "prepared": "flags", "export_import": "flags", "stylize_u8": "flags", "level": "flags", "encode_decode": "flags",
    "moments": "clean", "solve": "clean", "apply": "clean", "transform": "clean", "decode_affine": "flags", "split_level": "flags",
    "style_split": "flags", "moments_labeled": "clean", "apply_labeled": "clean", "regions": "flags", "moments_weighted": "clean",
    "apply_mixed": "clean", "interp": "flags", "style_blend": "flags", "blend": "flags", "noise": "clean", "synthesize": "flags",
    "image_edge": "clean", "resize": "clean", "reserve": "flags",
    # wct_hip.lib.SYMBOLS_COLOR / _SMOOTH / _TRANSFORM / _SWAP, by Python method
    "color_moments": "clean", "color_solve": "clean", "color_apply": "clean", "color_match": "clean", "luma_merge": "clean",
    "stylize_color": "flags", "guided_filter": "clean", "stylize_smooth": "flags", "set_transform": "clean", "transform_solve": "clean",
    "patch_match": "flags", "patch_assemble": "clean", "swap_level": "flags", "stylize_swap": "flags",
}
#: symbol -> method of wct_hip.WCT (the symbols of those four lists that have one)
METHOD_OF = {
    "wct_color_moments": "color_moments", "wct_color_solve": "color_solve", "wct_color_apply": "color_apply", "wct_color_match": "color_match",
    "wct_luma_merge": "luma_merge", "wct_stylize_color": "stylize_color", "wct_guided_filter": "guided_filter", "wct_stylize_smooth": "stylize_smooth",
    "wct_set_transform": "set_transform", "wct_get_transform": None, "wct_transform_solve": "transform_solve",
    "wct_patch_match": "patch_match", "wct_patch_assemble": "patch_assemble", "wct_swap_level": "swap_level", "wct_stylize_swap": "stylize_swap",
}
