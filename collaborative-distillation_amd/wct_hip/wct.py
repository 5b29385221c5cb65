"""Host-side mirror of the reference's call surface for the WCT stylisation path.

Same names, argument meaning and error behaviour as `PytorchWCT/util_wct.py` / `WCT.py`:

    wct = WCT(args)                      # util_wct.py:30-59   (args.mode, args.e1..e5, args.d1..d5, args.alpha)
    sF  = wct.e5(styleImg)               # WCT.py:100          NCHW fp32 CUDA tensors in and out
    csF = wct.transform(cF, sF, csF, a)  # util_wct.py:210-223
    img = wct.d5(csF)                    # WCT.py:105
    img = styleTransfer(wct.e5, wct.d5, contentImg, styleImg, csF)   # WCT.py:98-106

All arithmetic happens in libwct_hip.so (hand-written gfx950 kernels) through the C ABI of
include/wct_hip.h; PyTorch only provides device memory, the current HIP stream and (sharded.py)
torch.distributed.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import logging
import os
from ctypes import c_size_t, byref, c_int, c_void_p
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import lib as _lib
from . import model_zoo

_log = logging.getLogger("wct_hip")
_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_16X_WEIGHTS = os.path.join(_PKG, "weights", "16x.npz")


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _load_state(path: str) -> Dict[str, np.ndarray]:
    """A module's tensors from the reference's own checkpoint format (`{"epoch","model"}` or a bare
    state_dict, model_cd.py:712-718) -- torch is used for un-pickling only."""
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)   # plain tensors only: no arbitrary unpickling
    except Exception as e:
        if os.environ.get("WCT_ALLOW_UNSAFE_PICKLE") != "1":
            raise RuntimeError("%s is not a plain tensor checkpoint (%s); set WCT_ALLOW_UNSAFE_PICKLE=1 to unpickle it "
                               "with weights_only=False if you trust the file" % (path, e)) from e
        sd = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(sd, dict) and "model" in sd:
        sd = sd["model"]
    return {k: v.detach().cpu().numpy().astype(np.float32) for k, v in sd.items()}


class _Module:
    """`wct.e5` / `wct.d5`: callable like the reference's nn.Module on NCHW fp32 CUDA tensors."""

    def __init__(self, owner: "WCT", kind: str, level: int):
        self.owner, self.kind, self.level = owner, kind, level

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if self.kind == "enc":
            return self.owner.encode(self.level, x)
        return self.owner.decode(self.level, x)

    forward = __call__

    def __repr__(self):
        return "<wct_hip %s level %d (%s)>" % (self.kind, self.level, self.owner.mode)


class WCT:
    """Drop-in for util_wct.WCT.  `args` needs `.mode` ("16x" | "original" | None) and may carry
    `.e1..e5/.d1..d5` checkpoint paths (reference format, WCT.py:36-58), `.alpha`, `.numpy`.
    `weights` (a dict as produced by model_zoo.load_npz_weights / synth_weights) overrides the paths;
    with neither, mode 16x loads the packaged blob converted from the reference's checkpoints."""

    def __init__(self, args, weights: Optional[Dict[str, np.ndarray]] = None, device: Optional[int] = None):
        mode = getattr(args, "mode", None)
        if mode is None:
            mode = "original"
        if mode not in model_zoo.MODES:
            # the reference prints "Wrong mode. Please check." and exit(1)s (util_wct.py:57-59)
            raise ValueError("Wrong mode. Please check.")
        if not torch.cuda.is_available():
            raise RuntimeError("wct_hip needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
        self.args = args
        self.mode = mode
        self.alpha = float(getattr(args, "alpha", 1.0))
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.stats_device = "cuda:%d" % self.device   # where style_export() tensors live (wct_hip/replicas.py, sharded.py)
        self.strict_range = True                      # see _stream(): f16x3 clamps are reported by the next call
        self.has_comm = False                         # comm_init(): the context owns an RCCL communicator (level_sharded)
        self._lib = _lib.load()
        self._ctx = c_void_p()
        _lib.check(self._lib, None, self._lib.wct_create(self.device, byref(self._ctx)))
        if weights is None:
            weights = self._weights_from_args(args, mode)
        self._load_modules(weights)
        # --numpy (util_wct.py:204-208): whiten_and_color_np = the same steps with + I on the content covariance (:143)
        self.numpy_variant = bool(getattr(args, "numpy", False))
        if self.numpy_variant:
            self._chk(self._lib.wct_set_numpy_variant(self._ctx, 1))
        # --transform (include/wct_hip_transform.h): which closed-form feature transform every level applies
        self.set_transform(getattr(args, "transform", None) or "wct")
        for k in range(1, 6):
            setattr(self, "e%d" % k, _Module(self, "enc", k))
            setattr(self, "d%d" % k, _Module(self, "dec", k))

    # ------------------------------------------------------------------ construction
    @staticmethod
    def _weights_from_args(args, mode) -> Dict[str, np.ndarray]:
        paths = {("e%d" % k): getattr(args, "e%d" % k, None) for k in range(1, 6)}
        paths.update({("d%d" % k): getattr(args, "d%d" % k, None) for k in range(1, 6)})
        have = {k: p for k, p in paths.items() if p and os.path.exists(p)}
        if have and len(have) < 10:
            # the reference fails in torch.load on the first missing file (model_cd.py:712-718); never stylise with a
            # silent mix / substitute of weights
            missing = ["%s=%s" % (k, paths[k]) for k in sorted(paths) if k not in have]
            raise FileNotFoundError("checkpoints missing or not set for: " + ", ".join(missing))
        # per module: ".t7" (torch7, --mode original: model_original.py:24-30) or ".pth" (state_dict), as the reference asserts
        if len(have) == 10:
            bad = [p for p in have.values() if not (p.endswith(".pth") or (p.endswith(".t7") and mode == "original"))]
            if bad:
                raise ValueError("unsupported checkpoint extension (expected .pth%s): %s" % (" or .t7" if mode == "original" else "", ", ".join(bad)))
            _log.info("wct_hip: weights from the checkpoints in args.e1..d5 (%s ...)", paths["e1"])
            w = {}
            for key, p in paths.items():
                if p.endswith(".t7"):
                    state = model_zoo.load_t7_module(p, "enc" if key[0] == "e" else "dec", int(key[1]))
                else:
                    state = _load_state(p)
                for n, v in state.items():
                    if "aux" not in n:  # conv{k}1_aux heads are training-only (model_cd.py:700-704)
                        w["%s.%s" % (key, n)] = v
            return w
        if mode == "16x":
            _log.info("wct_hip: no checkpoint path exists -> packaged 16x weights %s", DEFAULT_16X_WEIGHTS)
            return model_zoo.load_npz_weights(DEFAULT_16X_WEIGHTS)
        if mode == "16x_kd2sd":
            raise FileNotFoundError("mode '16x_kd2sd' needs trained_models/wct_se_16x_new_sd_kd2sd/{1..5}SD.pth (WCT.py:60-70; "
                                    "not in the reference snapshot) -- pass the .pth paths in args.d1..d5 or weights=...")
        raise FileNotFoundError("mode 'original' needs the torch7 checkpoints of README.md:26 in args.e1..e5 / args.d1..d5 "
                                "(trained_models/original_wct_models/*.t7, not in the reference snapshot; read by wct_hip/t7.py) "
                                "-- or pass weights=...")

    def _layers(self, kind: str, level: int):
        """The layer list of one module ("enc" | "dec") of a level: the shipped graphs by mode.  The one place the class reads
        model_zoo's layer tables (a subclass with widths of its own overrides this and _feature_channels)."""
        return model_zoo.encoder_layers(self.mode, level) if kind == "enc" else model_zoo.decoder_layers(self.mode, level)

    def _feature_channels(self, level: int) -> int:
        """Channels of the level's feature map (relu{level}_1)."""
        return model_zoo.feature_channels(self.mode, level)

    def _load_modules(self, w: Dict[str, np.ndarray]):
        self._keep = []  # host arrays must outlive wct_load_module only, but keep them for clarity
        for k in range(1, 6):
            for kind, kid, layers in (("enc", _lib.KIND_ENC, self._layers("enc", k)), ("dec", _lib.KIND_DEC, self._layers("dec", k))):
                key = model_zoo.module_key(kind, k)
                arr = (_lib.WctLayer * len(layers))()
                hold = []
                for i, l in enumerate(layers):
                    wt = np.ascontiguousarray(w["%s.%s.weight" % (key, l.name)], np.float32)
                    bs = np.ascontiguousarray(w["%s.%s.bias" % (key, l.name)], np.float32)
                    if wt.shape != (l.cout, l.cin, 3, 3):
                        raise ValueError("%s.%s: weight shape %s != %s" % (key, l.name, wt.shape, (l.cout, l.cin, 3, 3)))
                    hold += [wt, bs]
                    arr[i] = _lib.WctLayer(l.cin, l.cout, int(l.pool_after), int(l.up_after), _fptr(wt), _fptr(bs))
                c0w = c0b = None
                if kind == "enc":
                    c0w = np.ascontiguousarray(w[key + ".conv0.weight"], np.float32).reshape(9)
                    c0b = np.ascontiguousarray(w[key + ".conv0.bias"], np.float32).reshape(3)
                    hold += [c0w, c0b]
                rc = self._lib.wct_load_module(self._ctx, kid, k, len(layers), arr,
                                               _fptr(c0w) if c0w is not None else None,
                                               _fptr(c0b) if c0b is not None else None)
                _lib.check(self._lib, self._ctx, rc)

    def __del__(self):
        try:
            if getattr(self, "_ctx", None) and self._ctx.value:
                self._lib.wct_destroy(self._ctx)
                self._ctx = c_void_p()
        except Exception:
            pass

    def cuda(self, device=None):  # `WCT(args).cuda()` (WCT.py:97): weights already live on the GPU
        return self

    def eval(self):
        return self

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        """Called at the start of every compute method: bind the caller's stream and -- without synchronising -- raise if an
        EARLIER call that has completed meanwhile clamped an activation to the f16x3 range (include/wct_hip.h wct_range_poll):
        the deviation from the fp32 reference is then reported by the very next call on every path (stylize*, e*/d* modules,
        styleTransfer, the split-level calls of sharded.py / pipeline.py / replicas.py), not only by sync().  `strict_range =
        False` turns the check off; saturation_count(reset=True) or a reported sync() acknowledges and clears it."""
        self._chk(self._lib.wct_set_stream(self._ctx, c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        if self.strict_range:
            n = ctypes.c_ulonglong()
            self._lib.wct_range_poll(self._ctx, byref(n))
            if n.value:
                raise OverflowError("libwct_hip: an earlier call clamped %d activation(s) to the f16x3 range (|x| >= 65504, or NaN input): "
                                    "its results deviate from the fp32 reference.  Use set_conv_mode('fp32') for these weights / inputs; "
                                    "saturation_count(reset=True) acknowledges the flag" % n.value)

    def range_flag(self) -> torch.Tensor:
        """The saturation counter NOW (in stream order) as a 1-element fp64 device tensor -- what a sharded run folds into the
        all-reduce of its moments so that every rank learns of a clamp on any rank (wct_range_flag_f64)."""
        t = torch.empty(1, device=self.stats_device, dtype=torch.float64)
        self._lib.wct_set_stream(self._ctx, c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        self._chk(self._lib.wct_range_flag_f64(self._ctx, t.data_ptr()))
        return t

    def _img(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 4:
            if x.shape[0] != 1:
                raise ValueError("batch size must be 1 (the reference's DataLoader uses batch_size=1, WCT.py:92)")
            x = x[0]
        if x.dim() != 3 or x.shape[0] != 3:
            raise ValueError("expected a [1,3,H,W] or [3,H,W] image, got %s" % (tuple(x.shape),))
        return self._dev_f32(x)

    def _chk(self, rc):
        _lib.check(self._lib, self._ctx, rc)

    def saturation_count(self, reset: bool = False) -> int:
        """Threads of the f16x3 kernels that clamped an activation to +-65504 since the last reset / report (a deviation from the
        fp32 reference; synchronises the context's streams).  sync() raises OverflowError ONCE for a non-zero count and clears
        it; every compute method raises while a completed call's count is non-zero (strict_range)."""
        n = ctypes.c_ulonglong()
        _lib.check(self._lib, self._ctx, self._lib.wct_saturation_count(self._ctx, int(reset), byref(n)))
        return int(n.value)

    def _dev_f32(self, x: torch.Tensor) -> torch.Tensor:
        return x.to(device=self.stats_device, dtype=torch.float32).contiguous()

    def _dev_f64(self, x: torch.Tensor, numel: int, what: str) -> torch.Tensor:
        if x.numel() != numel:
            raise ValueError("%s: expected %d values, got %d" % (what, numel, x.numel()))
        return x.to(device=self.stats_device, dtype=torch.float64).contiguous()

    def _nhwc(self, feat: torch.Tensor, C: Optional[int] = None) -> torch.Tensor:
        f = feat[0] if feat.dim() == 4 else feat
        if f.dim() != 3:
            raise ValueError("expected an NHWC feature [1,h,w,C] or [h,w,C], got %s" % (tuple(feat.shape),))
        if C is not None and int(f.shape[2]) != C:
            raise ValueError("expected %d channels in the last (NHWC) dimension, got %s" % (C, tuple(f.shape)))
        return self._dev_f32(f)

    def _out_image(self, out: Optional[torch.Tensor], H: int, W: int) -> torch.Tensor:
        """Caller-provided result buffer of stylize(): fp32, on this context's device, contiguous, >= 3*H*W values."""
        if out is None:
            return torch.empty((3, H, W), device=self.stats_device, dtype=torch.float32)
        if out.dtype != torch.float32 or not out.is_cuda or out.device.index != self.device or not out.is_contiguous() \
                or out.numel() < 3 * H * W:
            raise ValueError("out must be a contiguous fp32 tensor on cuda:%d with at least %d values" % (self.device, 3 * H * W))
        return out

    def feature_shape(self, level: int, H: int, W: int):
        C, h, w = c_int(), c_int(), c_int()
        self._chk(self._lib.wct_feature_shape(self._ctx, level, H, W, byref(C), byref(h), byref(w)))
        return C.value, h.value, w.value

    # ------------------------------------------------------------------ reference surface
    @torch.no_grad()
    def encode(self, level: int, img: torch.Tensor, layout: str = "nchw") -> torch.Tensor:
        x = self._img(img)
        H, W = int(x.shape[1]), int(x.shape[2])
        C, h, w = self.feature_shape(level, H, W)
        nchw = layout == "nchw"
        out = torch.empty((1, C, h, w) if nchw else (1, h, w, C), device=x.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_encode(self._ctx, level, x.data_ptr(), H, W, out.data_ptr(),
                                       _lib.LAYOUT_NCHW if nchw else _lib.LAYOUT_NHWC))
        return out

    @torch.no_grad()
    def decode(self, level: int, feat: torch.Tensor, layout: str = "nchw") -> torch.Tensor:
        f = feat[0] if feat.dim() == 4 else feat
        if f.dim() != 3:
            raise ValueError("expected a [1,C,h,w] / [C,h,w] (nchw) or [1,h,w,C] / [h,w,C] (nhwc) feature, got %s" % (tuple(feat.shape),))
        f = self._dev_f32(f)
        nchw = layout == "nchw"
        C = self._feature_channels(level)
        if nchw:
            c, h, w = (int(s) for s in f.shape)
        else:
            h, w, c = (int(s) for s in f.shape)
        if c != C:
            raise ValueError("decoder %d expects %d channels, got %d" % (level, C, c))
        out = torch.empty((1, 3, h << (level - 1), w << (level - 1)), device=f.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_decode(self._ctx, level, f.data_ptr(), h, w,
                                       _lib.LAYOUT_NCHW if nchw else _lib.LAYOUT_NHWC, out.data_ptr()))
        return out

    @torch.no_grad()
    def transform(self, cF: torch.Tensor, sF: torch.Tensor, csF: Optional[torch.Tensor] = None,
                  alpha: Optional[float] = None) -> torch.Tensor:
        """util_wct.py:210-223.  cF [C,h,w], sF [C,h',w'] fp32 (CPU like the reference, or CUDA) ->
        csF [1,C,h,w] fp32 on the GPU.  If `csF` is given it is resized in place, filled and returned
        (the reference's `csF.data.resize_().copy_()`, which silently stopped working in torch>=1.1)."""
        alpha = self.alpha if alpha is None else float(alpha)
        dev = self.stats_device
        c = self._dev_f32(cF[0] if cF.dim() == 4 else cF)
        s = self._dev_f32(sF[0] if sF.dim() == 4 else sF)
        if c.dim() != 3 or s.dim() != 3 or c.shape[0] != s.shape[0]:
            raise ValueError("transform expects cF [C,h,w] and sF [C,h',w'] with equal C")
        C, h, w = (int(v) for v in c.shape)
        hs, ws = int(s.shape[1]), int(s.shape[2])
        out = torch.empty((1, C, h, w), device=dev, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_transform(self._ctx, c.data_ptr(), C, h, w, s.data_ptr(), hs, ws, alpha,
                                          _lib.LAYOUT_NCHW, out.data_ptr()))
        if csF is not None and csF.is_cuda:
            csF.resize_(out.shape).copy_(out)
            return csF
        return out

    # ------------------------------------------------------------------ split form (used by the sharded path)
    @torch.no_grad()
    def moments(self, feat_nhwc: torch.Tensor, x0: int = 0, x1: Optional[int] = None):
        """Raw fp64 sums over columns [x0,x1) of an NHWC feature [1,h,w,C]: (n, sum[C], sumsq[C,C])."""
        f = self._nhwc(feat_nhwc)
        h, w, C = (int(v) for v in f.shape)
        x1 = w if x1 is None else x1
        s = torch.empty(C, device=f.device, dtype=torch.float64)
        ss = torch.empty(C, C, device=f.device, dtype=torch.float64)
        self._stream()
        self._chk(self._lib.wct_moments(self._ctx, f.data_ptr(), C, h, w, x0, x1, s.data_ptr(), ss.data_ptr()))
        return float(h * (x1 - x0)), s, ss

    @torch.no_grad()
    def solve(self, n_c, sum_c, sumsq_c, n_s, sum_s, sumsq_s, alpha: Optional[float] = None, want_info=False):
        alpha = self.alpha if alpha is None else float(alpha)
        C = int(sum_c.numel())
        sum_c, sumsq_c = self._dev_f64(sum_c, C, "sum_c"), self._dev_f64(sumsq_c, C * C, "sumsq_c")
        sum_s, sumsq_s = self._dev_f64(sum_s, C, "sum_s"), self._dev_f64(sumsq_s, C * C, "sumsq_s")
        M = torch.empty(C, C, device=sum_c.device, dtype=torch.float64)
        b = torch.empty(C, device=sum_c.device, dtype=torch.float64)
        info = (c_int * 2)()
        self._stream()
        self._chk(self._lib.wct_solve(self._ctx, C, float(n_c), sum_c.data_ptr(), sumsq_c.data_ptr(), float(n_s),
                                      sum_s.data_ptr(), sumsq_s.data_ptr(), alpha, M.data_ptr(), b.data_ptr(),
                                      info if want_info else None))
        return (M, b, (info[0], info[1])) if want_info else (M, b)

    # ------------------------------------------------------------------ the choice of feature transform (include/wct_hip_transform.h)
    def set_transform(self, name: str):
        """"wct" (the reference's whitening / colouring, the default), "ot" (the optimal-transport map between the two Gaussians) or
        "adain" (per-channel mean / std matching): consumed wherever a level's (M, b) is made.  ValueError for another name, and for
        a non-wct transform while the numpy variant is on."""
        if name not in _lib.TRANSFORMS:
            raise ValueError("transform must be one of %s, not %r" % (sorted(_lib.TRANSFORMS), name))
        self._chk(self._lib.wct_set_transform(self._ctx, _lib.TRANSFORMS[name]))

    @property
    def transform_mode(self) -> str:
        mode = c_int()
        self._chk(self._lib.wct_get_transform(self._ctx, byref(mode)))
        return {v: k for k, v in _lib.TRANSFORMS.items()}[mode.value]

    @torch.no_grad()
    def transform_solve(self, mode: str, n_c, sum_c, sumsq_c, style_stats, alpha: Optional[float] = None, want_info=False):
        """(M, b) of the transform `mode` from raw content moments and style statistics in the style_export layout
        (cov_s^(1/2) [C*C] then mu_s [C]); the context's own mode is neither read nor changed."""
        if mode not in _lib.TRANSFORMS:
            raise ValueError("transform must be one of %s, not %r" % (sorted(_lib.TRANSFORMS), mode))
        alpha = self.alpha if alpha is None else float(alpha)
        C = int(sum_c.numel())
        sum_c, sumsq_c = self._dev_f64(sum_c, C, "sum_c"), self._dev_f64(sumsq_c, C * C, "sumsq_c")
        stats = self._dev_f64(style_stats, C * C + C, "style_stats")
        M = torch.empty(C, C, device=sum_c.device, dtype=torch.float64)
        b = torch.empty(C, device=sum_c.device, dtype=torch.float64)
        info = (c_int * 2)()
        self._stream()
        self._chk(self._lib.wct_transform_solve(self._ctx, _lib.TRANSFORMS[mode], C, float(n_c), sum_c.data_ptr(), sumsq_c.data_ptr(),
                                                stats.data_ptr(), alpha, M.data_ptr(), b.data_ptr(), info if want_info else None))
        return (M, b, (info[0], info[1])) if want_info else (M, b)

    @torch.no_grad()
    def decode_affine(self, level: int, feat_nhwc: torch.Tensor, M: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        C = self._feature_channels(level)
        f = self._nhwc(feat_nhwc, C)
        M, b = self._dev_f64(M, C * C, "M"), self._dev_f64(b, C, "b")
        h, w, _ = (int(v) for v in f.shape)
        out = torch.empty((1, 3, h << (level - 1), w << (level - 1)), device=f.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_decode_affine(self._ctx, level, f.data_ptr(), h, w, M.data_ptr(), b.data_ptr(), out.data_ptr()))
        return out

    # ------------------------------------------------------------------ split level (content-sharded runs)
    @torch.no_grad()
    def style_prepare(self, styleImg: torch.Tensor, levels=(5, 4, 3, 2, 1)):
        """Style side of the given levels on the context's side stream (overlaps whatever follows)."""
        s = self._img(styleImg)
        self._style_keep = s   # the side stream reads it asynchronously
        mask = 0
        for L in levels:
            mask |= 1 << int(L)
        self._stream()
        self._chk(self._lib.wct_style_prepare_levels(self._ctx, s.data_ptr(), int(s.shape[1]), int(s.shape[2]), mask))

    def style_stats_count(self, level: int) -> int:
        n = c_size_t()
        self._chk(self._lib.wct_style_stats_count(self._ctx, level, byref(n)))
        return int(n.value)

    def style_export(self, level: int) -> torch.Tensor:
        """Style statistics of a prepared level as one fp64 vector: cov_s^(1/2) [C*C] then mu_s [C]."""
        n = c_size_t()
        self._chk(self._lib.wct_style_stats_count(self._ctx, level, byref(n)))
        buf = torch.empty(n.value, device=self.stats_device, dtype=torch.float64)
        self._stream()
        self._chk(self._lib.wct_style_export(self._ctx, level, buf.data_ptr()))
        return buf

    def style_import(self, level: int, stats: torch.Tensor):
        n = c_size_t()
        self._chk(self._lib.wct_style_stats_count(self._ctx, level, byref(n)))
        if stats.dtype != torch.float64 or not stats.is_cuda or stats.numel() != n.value:
            raise ValueError("style_import: expected %d fp64 values on the GPU" % n.value)
        stats = stats.to(self.stats_device).contiguous()
        self._stream()
        self._chk(self._lib.wct_style_import(self._ctx, level, stats.data_ptr()))

    @torch.no_grad()
    def stylize_prepared(self, contentImg: torch.Tensor, alpha: Optional[float] = None, num_run: int = 1,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The cascade against the style statistics already in the context (style_prepare / style_import): content x style
        batches pay the style side once per style (data_loader.py:32-36 builds the Cartesian product)."""
        alpha = self.alpha if alpha is None else float(alpha)
        c = self._img(contentImg)
        H, W = int(c.shape[1]), int(c.shape[2])
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_prepared(self._ctx, c.data_ptr(), H, W, alpha, int(num_run), out.data_ptr(), byref(ho), byref(wo)))
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ seeded style variations (include/wct_hip_diverse.h)
    @staticmethod
    def _diverse_args(what: str, strength, seed, stream_id, levels=None):
        strength, seed, stream_id = float(strength), int(seed), int(stream_id)
        if not (0.0 <= strength <= _lib.DIVERSE_MAX_STRENGTH):
            raise ValueError("%s: strength must lie in [0, %d], got %r" % (what, _lib.DIVERSE_MAX_STRENGTH, strength))
        if not (0 <= seed < 1 << 64) or not (0 <= stream_id < 1 << 32):
            raise ValueError("%s: seed must fit 64 bits and stream_id 32 bits (unsigned), got %d, %d" % (what, seed, stream_id))
        mask = 0
        for L in () if levels is None else levels:
            if int(L) not in (1, 2, 3, 4, 5):
                raise ValueError("%s: levels must be among 1..5, got %r" % (what, tuple(levels)))
            mask |= 1 << int(L)
        if levels is not None and not mask:
            raise ValueError("%s: no level given" % what)
        return strength, seed, stream_id, mask

    @torch.no_grad()
    def rotation(self, C: int, strength: float, seed: int = 0, stream_id: int = 0, tag: int = 0, want_skew: bool = False):
        """The orthogonal Z(C, seed, stream_id, tag, strength) [C, C] fp64 of include/wct_hip_diverse.h (the Cayley transform of a seeded
        skew-symmetric A; the identity at strength 0), a function of its arguments alone, bit for bit.  want_skew: -> (Z, A)."""
        strength, seed, stream_id, _ = self._diverse_args("rotation", strength, seed, stream_id)
        C, tag = int(C), int(tag)
        if C < 2 or C % 2 or C > 512 or not (0 <= tag <= 255):
            raise ValueError("rotation: C even in 2..512 and tag in 0..255 expected, got C=%d, tag=%d" % (C, tag))
        Z = torch.empty(C, C, device=self.stats_device, dtype=torch.float64)
        A = torch.empty(C, C, device=self.stats_device, dtype=torch.float64) if want_skew else None
        self._stream()
        self._chk(self._lib.wct_rotation_make(self._ctx, C, seed, stream_id, tag, strength, Z.data_ptr(), A.data_ptr() if want_skew else None))
        return (Z, A) if want_skew else Z

    def style_diversify(self, strength: float, seed: int = 0, stream_id: int = 0, levels=(5,)):
        """Post-multiply the prepared style slots of `levels` by the seeded rotation (tag = level), in place: the same target covariance
        through a different colouring map, so everything that reads prepared statistics afterwards (stylize_prepared, clips, style_export,
        ...) gives a variation.  wct transform only; two calls compose; whatever rewrites a slot (style_prepare, style_import, ...) resets it;
        strength 0 changes nothing."""
        strength, seed, stream_id, mask = self._diverse_args("style_diversify", strength, seed, stream_id, levels)
        self._stream()
        self._chk(self._lib.wct_style_diversify(self._ctx, mask, strength, seed, stream_id))

    @torch.no_grad()
    def stylize_diverse(self, contentImg: torch.Tensor, styleImg: torch.Tensor, strength: float, seed: int = 0, stream_id: int = 0, levels=(5,),
                        alpha: Optional[float] = None, num_run: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """style_prepare + style_diversify + stylize_prepared in one library call (wct_stylize_diverse), bit-identical to the three."""
        alpha = self.alpha if alpha is None else float(alpha)
        strength, seed, stream_id, mask = self._diverse_args("stylize_diverse", strength, seed, stream_id, levels)
        c, s = self._img(contentImg), self._img(styleImg)
        self._style_keep = s      # the side stream reads it asynchronously
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_diverse(self._ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, mask, strength, seed, stream_id, alpha, int(num_run),
                                                out.data_ptr(), byref(ho), byref(wo)))
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ image edge (ToTensor / save_image on the device)
    def _u8(self, img: torch.Tensor) -> torch.Tensor:
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("expected a uint8 H x W x 3 image, got %s %s" % (img.dtype, tuple(img.shape)))
        return img.to(self.stats_device).contiguous()

    @torch.no_grad()
    def to_tensor_u8(self, img_u8: torch.Tensor) -> torch.Tensor:
        """transforms.ToTensor() of data_loader.py:57-58 on the GPU: uint8 HWC -> fp32 1x3xHxW in [0,1]."""
        x = self._u8(img_u8)
        H, W = int(x.shape[0]), int(x.shape[1])
        out = torch.empty((1, 3, H, W), device=x.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_u8_to_planar(self._ctx, x.data_ptr(), H, W, out.data_ptr()))
        return out

    def resize_shape(self, H: int, W: int, size: int):
        """Output (H, W) of transforms.Resize(size) (torchvision 0.2.1: the smaller edge becomes `size`; 0 = no resize)."""
        oh, ow = c_int(), c_int()
        if self._lib.wct_resize_shape(int(H), int(W), int(size), byref(oh), byref(ow)) != 0:
            raise ValueError("resize_shape: bad arguments %s x %s -> %s" % (H, W, size))
        return oh.value, ow.value

    @torch.no_grad()
    def resize_u8(self, img_u8: torch.Tensor, size, to_tensor: bool = False, filter: str = "bilinear") -> torch.Tensor:
        """transforms.Resize(size) of data_loader.py:52-56 on the GPU, bit-exact with Pillow's bilinear Image.resize: `size` is an
        int (smaller edge, torchvision's rule) or an (oH, oW) pair.  to_tensor=True returns ToTensor()'s fp32 1x3xoHxoW instead of
        uint8 HWC (one pass less).  filter="bicubic" is Pillow's Image.BICUBIC -- what the reference's texture resize
        (data_loader.py:72: Image.resize without a filter argument, at its Pillow pin) uses; it takes an explicit (oH, oW)."""
        if filter not in _lib.RESIZE_FILTERS:
            raise ValueError("filter must be 'bilinear' or 'bicubic', got %r" % (filter,))
        if filter != "bilinear" and isinstance(size, int):
            raise ValueError("resize_u8: filter=%r takes an explicit (oH, oW); torchvision's smaller-edge rule belongs to the bilinear Resize" % filter)
        x = self._u8(img_u8)
        H, W = int(x.shape[0]), int(x.shape[1])
        oH, oW = self.resize_shape(H, W, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
        self._stream()
        if filter != "bilinear":
            out = torch.empty((1, 3, oH, oW), device=x.device, dtype=torch.float32) if to_tensor else \
                torch.empty((oH, oW, 3), device=x.device, dtype=torch.uint8)
            self._chk(self._lib.wct_resize_u8_filter(self._ctx, x.data_ptr(), H, W, None if to_tensor else out.data_ptr(),
                                                     out.data_ptr() if to_tensor else None, oH, oW, _lib.RESIZE_FILTERS[filter]))
        elif to_tensor:
            out = torch.empty((1, 3, oH, oW), device=x.device, dtype=torch.float32)
            self._chk(self._lib.wct_resize_u8_to_planar(self._ctx, x.data_ptr(), H, W, out.data_ptr(), oH, oW))
        else:
            out = torch.empty((oH, oW, 3), device=x.device, dtype=torch.uint8)
            self._chk(self._lib.wct_resize_u8(self._ctx, x.data_ptr(), H, W, out.data_ptr(), oH, oW))
        return out

    @torch.no_grad()
    def to_u8(self, img: torch.Tensor, round_mode: int = 0) -> torch.Tensor:
        """save_image's conversion (WCT.py:128; torchvision 0.2.1: mul(255).clamp(0,255).byte()) on the GPU: fp32 CHW -> uint8 HWC."""
        x = self._img(img)
        H, W = int(x.shape[1]), int(x.shape[2])
        out = torch.empty((H, W, 3), device=x.device, dtype=torch.uint8)
        self._stream()
        self._chk(self._lib.wct_planar_to_u8(self._ctx, x.data_ptr(), H, W, out.data_ptr(), int(round_mode)))
        return out

    @torch.no_grad()
    def stylize_u8(self, content_u8: torch.Tensor, style_u8: torch.Tensor, alpha: Optional[float] = None, num_run: int = 1,
                   round_mode: int = 0) -> torch.Tensor:
        """uint8 HWC content + style -> uint8 HWC result (ToTensor -> cascade -> save_image conversion), one call."""
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._u8(content_u8), self._u8(style_u8)
        H, W, Hs, Ws = int(c.shape[0]), int(c.shape[1]), int(s.shape[0]), int(s.shape[1])
        out = torch.empty((H, W, 3), device=c.device, dtype=torch.uint8)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_u8(self._ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, alpha, int(num_run), out.data_ptr(),
                                           byref(ho), byref(wo), int(round_mode)))
        return out.view(-1)[: 3 * ho.value * wo.value].view(ho.value, wo.value, 3)

    @torch.no_grad()
    def content_encode(self, level: int, img: torch.Tensor, x0: int = 0, x1: int = -1):
        """cF = encoder(img), kept inside the context; returns (h, w, sum[C], sumsq[C,C]) over feature columns [x0,x1)."""
        x = self._img(img)
        self._content_keep = x
        H, W = int(x.shape[1]), int(x.shape[2])
        C = self._feature_channels(level)
        s = torch.empty(C, device=x.device, dtype=torch.float64)
        ss = torch.empty(C, C, device=x.device, dtype=torch.float64)
        h, w = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_content_encode(self._ctx, level, x.data_ptr(), H, W, x0, x1, s.data_ptr(), ss.data_ptr(), byref(h), byref(w)))
        return h.value, w.value, s, ss

    @torch.no_grad()
    def content_solve(self, level: int, n_c: float, sum_c: torch.Tensor, sumsq_c: torch.Tensor, alpha: Optional[float] = None):
        alpha = self.alpha if alpha is None else float(alpha)
        C = self._feature_channels(level)
        sum_c, sumsq_c = self._dev_f64(sum_c, C, "sum_c"), self._dev_f64(sumsq_c, C * C, "sumsq_c")
        M = torch.empty(C, C, device=sum_c.device, dtype=torch.float64)
        b = torch.empty(C, device=sum_c.device, dtype=torch.float64)
        self._stream()
        self._chk(self._lib.wct_content_solve(self._ctx, level, float(n_c), sum_c.data_ptr(), sumsq_c.data_ptr(), alpha, M.data_ptr(), b.data_ptr()))
        return M, b

    @torch.no_grad()
    def content_decode(self, level: int, M: torch.Tensor, b: torch.Tensor, H: int, W: int) -> torch.Tensor:
        """H, W: size of the image wct.content_encode() was given (the output is floor-shrunk like the reference's)."""
        C, h, w = self.feature_shape(level, H, W)
        M, b = self._dev_f64(M, C * C, "M"), self._dev_f64(b, C, "b")
        out = torch.empty((1, 3, h << (level - 1), w << (level - 1)), device=M.device, dtype=torch.float32)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_content_decode(self._ctx, level, M.data_ptr(), b.data_ptr(), out.data_ptr(), byref(ho), byref(wo)))
        assert (ho.value, wo.value) == tuple(out.shape[2:])
        return out

    # ------------------------------------------------------------------ RCCL behind the boundary (include/wct_hip.h wct_comm_*, wct_level_sharded)
    def comm_init(self, dist, group=None) -> None:
        """Give this engine's context its own RCCL communicator over the ranks of `dist` (torch.distributed, any backend: it only carries
        the 128-byte unique id from rank 0): every rank calls this once.  The library then runs the per-level all-reduce of a sharded
        job itself (level_sharded); RCCL is the librccl.so torch has loaded -- one RCCL per process."""
        import os as _os
        path = _os.path.join(_os.path.dirname(torch.__file__), "lib", "librccl.so")
        if self._lib.wct_comm_load(path.encode() if _os.path.exists(path) else None) != 0:
            raise RuntimeError("libwct_hip: librccl.so could not be loaded (%s)" % (path if _os.path.exists(path) else "the loader's search path, /opt/rocm/lib"))
        rank, world = dist.get_rank(), dist.get_world_size()
        buf = ctypes.create_string_buffer(128)
        if rank == 0:
            if self._lib.wct_comm_unique_id(buf) != 0:
                raise RuntimeError("libwct_hip: ncclGetUniqueId failed")
        if world > 1:
            box = [bytes(buf.raw)]
            dist.broadcast_object_list(box, src=0, group=group)
            buf = ctypes.create_string_buffer(box[0], 128)
        with torch.cuda.device(self.device):
            self._chk(self._lib.wct_comm_init(self._ctx, world, rank, buf))
        self.has_comm = True

    def comm_destroy(self) -> None:
        self._chk(self._lib.wct_comm_destroy(self._ctx))
        self.has_comm = False
        self._coll_keep = None

    def comm_info(self):
        """(nranks, rank) of the communicator / transport the context holds; (0, 0) without one."""
        n, r = c_int(), c_int()
        self._chk(self._lib.wct_comm_info(self._ctx, byref(n), byref(r)))
        return n.value, r.value

    def comm_attach_collectives(self, all_reduce, broadcast, sendrecv, nranks: int, rank: int) -> None:
        """Install a caller-supplied transport for stylize_sharded / level_sharded (include/wct_hip.h wct_collectives): three Python
        callables `all_reduce(buf_ptr, count, stream) -> int`, `broadcast(buf_ptr, nbytes, root, stream) -> int`,
        `sendrecv(ops, stream) -> int` with ops = [(peer, is_send, buf_ptr, nbytes)]; device pointers and the HIP stream arrive as
        integers, 0 = success.  (Test infrastructure drives the C cascade through rank threads this way; a production transport would be C.)"""
        def _sr(user, ops, n, stream):
            return int(sendrecv([(ops[i].peer, ops[i].is_send, ops[i].buf, ops[i].bytes) for i in range(n)], stream))
        table = _lib.WctCollectives(None, _lib.ALL_REDUCE_FN(lambda user, buf, count, stream: int(all_reduce(buf, count, stream))),
                                    _lib.BROADCAST_FN(lambda user, buf, nbytes, root, stream: int(broadcast(buf, nbytes, root, stream))),
                                    _lib.SENDRECV_FN(_sr))
        self._chk(self._lib.wct_comm_attach_collectives(self._ctx, byref(table), int(nranks), int(rank)))
        self._coll_keep = table          # the C side copied the table; the callback thunks must outlive it
        self.has_comm = True

    def comm_selftest(self) -> None:
        """Exercise the context's transport between the job's ranks with known data (all-reduce, broadcast, ring and neighbour
        send / recv) and raise if anything comes back wrong (wct_comm_selftest; collective: every rank calls it)."""
        self._stream()
        self._chk(self._lib.wct_comm_selftest(self._ctx))

    def shard_geometry(self, W_total: int, nranks: int, rank: int, halo_mode: str = "auto"):
        """-> (own0, own1, in0, in1, resolved halo mode) of `rank` in an `nranks`-strip job over a W_total-wide content (wct_shard_geometry)."""
        v = [c_int() for _ in range(5)]
        rc = self._lib.wct_shard_geometry(int(W_total), int(nranks), int(rank), _lib.HALO_MODES[halo_mode], *[byref(x) for x in v])
        if rc != 0:
            raise ValueError("shard_geometry: width %d cannot be cut into %d strips under halo mode %r" % (W_total, nranks, halo_mode))
        return v[0].value, v[1].value, v[2].value, v[3].value, {0: "auto", 1: "recompute", 2: "exchange"}[v[4].value]

    @torch.no_grad()
    def stylize_sharded(self, content_ext: torch.Tensor, style: torch.Tensor, W_total: int, in0: int, in1: int, alpha: Optional[float] = None,
                        halo_mode: str = "auto", style_mode: str = "auto", broadcast_map: bool = False,
                        range_total: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, fast_fold: bool = False) -> torch.Tensor:
        """The WHOLE column-sharded cascade in ONE library call (wct_stylize_sharded): this rank's strip + level-5 margin in
        (columns [in0, in1) of the W_total-wide content, see shard_geometry), its owned columns of the stylised image out
        ([1, 3, H', own_w']).  Geometry, crops, the style side (strips / owner / replicate), the per-level all-reduce, the optional
        broadcasts and the neighbour exchange all run inside the library on the context's communicator (comm_init) or transport."""
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(content_ext), self._img(style)
        H, Win = int(c.shape[1]), int(c.shape[2])
        if Win != in1 - in0:
            raise ValueError("stylize_sharded: content_ext has %d columns, [in0, in1) = [%d, %d)" % (Win, in0, in1))
        nr, rk = self.comm_info()
        own0, own1 = self.shard_geometry(W_total, max(nr, 1), rk, halo_mode)[:2]
        if out is None:
            out = torch.empty(3 * H * (own1 - own0), device=c.device, dtype=torch.float32)
        elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() < 3 * H * (own1 - own0):
            raise ValueError("out must be a contiguous fp32 CUDA tensor with at least %d values" % (3 * H * (own1 - own0)))
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_sharded(self._ctx, c.data_ptr(), H, int(W_total), int(in0), int(in1), s.data_ptr(), int(s.shape[1]), int(s.shape[2]),
                                                alpha, _lib.HALO_MODES[halo_mode], _lib.STYLE_MODES[style_mode], (_lib.SHARD_BROADCAST_MAP if broadcast_map else 0) | (_lib.SHARD_FAST_FOLD if fast_fold else 0),
                                                out.data_ptr(), byref(ho), byref(wo), range_total.data_ptr() if range_total is not None else None))
        self._style_keep = s
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    @torch.no_grad()
    def style_moments(self, level: int, style_strip: torch.Tensor, x0: int = 0, x1: int = -1):
        """Encoder of a STRIP of the style image + raw fp64 moments over its feature columns [x0, x1) -> (sum[C], sumsq[C, C]) on the
        context's side stream, visible to the caller's stream (wct_style_moments; the style side of sharded.py's "strips" mode)."""
        x = self._img(style_strip)
        self._style_keep = x
        C = self._feature_channels(level)
        s = torch.empty(C, device=x.device, dtype=torch.float64)
        ss = torch.empty(C, C, device=x.device, dtype=torch.float64)
        self._stream()
        self._chk(self._lib.wct_style_moments(self._ctx, level, x.data_ptr(), int(x.shape[1]), int(x.shape[2]), int(x0), int(x1), s.data_ptr(), ss.data_ptr()))
        return s, ss

    @torch.no_grad()
    def style_solve(self, level: int, n_s: float, sum_s: torch.Tensor, sumsq_s: torch.Tensor) -> None:
        """Global style moments of a level -> cov_s^(1/2), mu_s inside the context (what style_prepare leaves), on the side stream."""
        C = self._feature_channels(level)
        sum_s, sumsq_s = self._dev_f64(sum_s, C, "sum_s"), self._dev_f64(sumsq_s, C * C, "sumsq_s")
        self._solve_keep = getattr(self, "_solve_keep", {})
        self._solve_keep[level] = (sum_s, sumsq_s)       # read asynchronously by the side stream
        self._stream()
        self._chk(self._lib.wct_style_solve(self._ctx, level, float(n_s), sum_s.data_ptr(), sumsq_s.data_ptr()))

    @torch.no_grad()
    def level_sharded(self, level: int, img: torch.Tensor, x0: int, x1: int, n_total: float, alpha: Optional[float] = None,
                      range_total: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One level of a column-sharded cascade in ONE library call (encoder + owned-column moments -> ncclAllReduce -> solve -> fold ->
        decoder; wct_level_sharded).  img: this rank's strip + halo [3, H, W]; [x0, x1): owned FEATURE columns; n_total: feature
        pixels of the whole image.  range_total: optional 1-element fp64 device tensor receiving the node-wide f16x3 clamp count."""
        alpha = self.alpha if alpha is None else float(alpha)
        x = self._img(img)
        H, W = int(x.shape[1]), int(x.shape[2])
        C, h, w = self.feature_shape(level, H, W)
        out = torch.empty((1, 3, h << (level - 1), w << (level - 1)), device=x.device, dtype=torch.float32)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_level_sharded(self._ctx, level, x.data_ptr(), H, W, int(x0), int(x1), float(n_total), alpha, out.data_ptr(),
                                              byref(ho), byref(wo), range_total.data_ptr() if range_total is not None else None))
        assert (ho.value, wo.value) == tuple(out.shape[2:])
        return out

    # ------------------------------------------------------------------ fused level / cascade
    @torch.no_grad()
    def style_transfer_level(self, level: int, contentImg: torch.Tensor, styleImg: torch.Tensor,
                             alpha: Optional[float] = None) -> torch.Tensor:
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        _, h, w = self.feature_shape(level, H, W)
        out = torch.empty((1, 3, h << (level - 1), w << (level - 1)), device=c.device, dtype=torch.float32)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_style_transfer_level(self._ctx, level, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, alpha,
                                                     out.data_ptr(), byref(ho), byref(wo)))
        assert (ho.value, wo.value) == tuple(out.shape[2:])
        return out

    @torch.no_grad()
    def stylize(self, contentImg: torch.Tensor, styleImg: torch.Tensor, alpha: Optional[float] = None,
                num_run: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The 5 -> 1 cascade of WCT.py:120-125 in one call (no host round trips, no allocation after the
        first call of a size)."""
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize(self._ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, alpha, int(num_run),
                                        out.data_ptr(), byref(ho), byref(wo)))
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ texture synthesis
    @torch.no_grad()
    def noise(self, H: int, W: int, seed: int = 0, stream_id: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Uniform noise in [0, 1) as a [1, 3, H, W] fp32 image made on the GPU (wct_noise_uniform): Philox4x32-10 keyed by the 64-bit
        `seed`, values defined by (seed, stream_id, position) alone -- include/wct_hip.h states the mapping; torch's generator is not
        involved.  `out`: an fp32 tensor on this device with 3*H*W values, contiguous, any 4-byte alignment (a view is fine)."""
        H, W, seed, stream_id = int(H), int(W), int(seed), int(stream_id)
        if not (0 <= seed < 1 << 64) or not (0 <= stream_id < 1 << 32):
            raise ValueError("noise: seed must fit 64 bits and stream_id 32 bits (unsigned), got %d, %d" % (seed, stream_id))
        if H < 1 or W < 1:
            raise ValueError("noise: H, W >= 1 expected, got %d x %d" % (H, W))
        if out is None:
            out = torch.empty((1, 3, H, W), device=self.stats_device, dtype=torch.float32)
        elif out.dtype != torch.float32 or not out.is_cuda or out.device.index != self.device or not out.is_contiguous() \
                or out.numel() != 3 * H * W:
            raise ValueError("out must be a contiguous fp32 tensor on cuda:%d with %d values" % (self.device, 3 * H * W))
        self._stream()
        self._chk(self._lib.wct_noise_uniform(self._ctx, seed, stream_id, H, W, out.data_ptr()))
        return out.view(1, 3, H, W)

    @torch.no_grad()
    def synthesize(self, texture: Optional[torch.Tensor], H: Optional[int] = None, W: Optional[int] = None, seed: int = 0,
                   stream_id: int = 0, alpha: Optional[float] = None, num_run: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Texture synthesis (`--synthesis`, data_loader.py:61-76): the cascade with noise(H, W, seed, stream_id) as the content and
        `texture` as the style, in one library call (wct_synthesize) -- bit-identical to stylize(noise(...), texture, ...), with the
        noise kept inside the context.  The default size is the texture's.  texture=None runs against the style statistics already in
        the context (style_prepare / style_import / style_blend), H and W are then required.  Texture interpolation needs no entry of
        its own: stylize_interp(wct.noise(H, W, seed), textures, weights) composes."""
        alpha = self.alpha if alpha is None else float(alpha)
        seed, stream_id = int(seed), int(stream_id)
        if not (0 <= seed < 1 << 64) or not (0 <= stream_id < 1 << 32):
            raise ValueError("synthesize: seed must fit 64 bits and stream_id 32 bits (unsigned), got %d, %d" % (seed, stream_id))
        t = None
        Ht = Wt = 0
        if texture is not None:
            t = self._img(texture)
            Ht, Wt = int(t.shape[1]), int(t.shape[2])
        elif H is None or W is None:
            raise ValueError("synthesize: texture=None (prepared statistics) needs H and W")
        H = Ht if H is None else int(H)
        W = Wt if W is None else int(W)
        out = self._out_image(out, max(H, 0), max(W, 0))
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_synthesize(self._ctx, t.data_ptr() if t is not None else None, Ht, Wt, H, W, seed, stream_id, alpha,
                                           int(num_run), out.data_ptr(), byref(ho), byref(wo)))
        self._style_keep = t      # the side stream reads it asynchronously
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ colour preservation (include/wct_hip_color.h)
    def _out_like(self, out: Optional[torch.Tensor], what: str, numel: int, dtype=torch.float32) -> Optional[torch.Tensor]:
        """A caller-provided result buffer with exactly `numel` values (contiguous, this device; a view is fine), or None."""
        if out is not None and (out.dtype != dtype or not out.is_cuda or out.device.index != self.device or not out.is_contiguous()
                                or out.numel() != numel):
            raise ValueError("%s: out must be a contiguous %s tensor on cuda:%d with %d values" % (what, dtype, self.device, numel))
        return out

    @torch.no_grad()
    def color_moments(self, img: torch.Tensor):
        """Raw fp64 colour sums of a [1,3,H,W] / [3,H,W] image over all its pixels: (n, sum[3], sumsq[3,3]) (wct_color_moments).
        The summation tree depends on (H, W) alone: bitwise reproducible across calls, alignments and contexts."""
        x = self._img(img)
        H, W = int(x.shape[1]), int(x.shape[2])
        s = torch.empty(3, device=x.device, dtype=torch.float64)
        ss = torch.empty(3, 3, device=x.device, dtype=torch.float64)
        self._stream()
        self._chk(self._lib.wct_color_moments(self._ctx, x.data_ptr(), H, W, s.data_ptr(), ss.data_ptr()))
        return float(H * W), s, ss

    @torch.no_grad()
    def color_solve(self, n_c, sum_c, sumsq_c, n_s, sum_s, sumsq_s, eps: float = _lib.COLOR_EPS):
        """(n, sum, sumsq) of content and style -> (A [3,3], t [3]) fp64 on the device: A = cov_c^(1/2) cov_s^(-1/2) with unbiased
        covariances + eps I, t = mu_c - A mu_s (wct_color_solve; no host synchronisation)."""
        sum_c, sumsq_c = self._dev_f64(sum_c, 3, "sum_c"), self._dev_f64(sumsq_c, 9, "sumsq_c")
        sum_s, sumsq_s = self._dev_f64(sum_s, 3, "sum_s"), self._dev_f64(sumsq_s, 9, "sumsq_s")
        A = torch.empty(3, 3, device=sum_c.device, dtype=torch.float64)
        t = torch.empty(3, device=sum_c.device, dtype=torch.float64)
        self._stream()
        self._chk(self._lib.wct_color_solve(self._ctx, float(n_c), sum_c.data_ptr(), sumsq_c.data_ptr(), float(n_s), sum_s.data_ptr(),
                                            sumsq_s.data_ptr(), float(eps), A.data_ptr(), t.data_ptr()))
        return A, t

    @torch.no_grad()
    def color_apply(self, img: torch.Tensor, A: torch.Tensor, t: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out_p = float(A x_p + t) per pixel, evaluated in fp64, not clamped (wct_color_apply).  `out` may be `img` itself."""
        x = self._img(img)
        H, W = int(x.shape[1]), int(x.shape[2])
        A, t = self._dev_f64(A, 9, "A"), self._dev_f64(t, 3, "t")
        out = self._out_like(out, "color_apply", 3 * H * W)
        if out is None:
            out = torch.empty((1, 3, H, W), device=x.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_color_apply(self._ctx, x.data_ptr(), H, W, A.data_ptr(), t.data_ptr(), out.data_ptr()))
        return out.view(1, 3, H, W)

    @torch.no_grad()
    def color_match(self, style: torch.Tensor, content: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The style image with its colours mapped onto the content's colour distribution (Gatys et al. 2017, section 5; the
        reference's whiten_and_color on pixels): color_moments of both + color_solve + color_apply in one call (wct_color_match),
        bit-identical to that chain.  `out` may be `style` itself."""
        s, c = self._img(style), self._img(content)
        Hs, Ws, H, W = int(s.shape[1]), int(s.shape[2]), int(c.shape[1]), int(c.shape[2])
        out = self._out_like(out, "color_match", 3 * Hs * Ws)
        if out is None:
            out = torch.empty((1, 3, Hs, Ws), device=s.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_color_match(self._ctx, s.data_ptr(), Hs, Ws, c.data_ptr(), H, W, out.data_ptr()))
        return out.view(1, 3, Hs, Ws)

    @torch.no_grad()
    def luma_merge(self, stylised: torch.Tensor, content: torch.Tensor, out: Optional[torch.Tensor] = None, u8: bool = False,
                   round_mode: int = 0) -> torch.Tensor:
        """The content's chroma with the stylised luminance: out_c = content_c + (Y(stylised) - Y(content)) over the top-left window
        of the content that the result covers (wct_luma_merge).  u8=False: fp32 [1,3,Ho,Wo]; u8=True: uint8 [Ho,Wo,3] with the
        conversion of to_u8(., round_mode) fused in, byte-identical to to_u8 of the fp32 result."""
        s, c = self._img(stylised), self._img(content)
        Ho, Wo, Hc, Wc = int(s.shape[1]), int(s.shape[2]), int(c.shape[1]), int(c.shape[2])
        if Ho > Hc or Wo > Wc:
            raise ValueError("luma_merge: the result (%d x %d) is larger than the content (%d x %d)" % (Ho, Wo, Hc, Wc))
        out = self._out_like(out, "luma_merge", 3 * Ho * Wo, torch.uint8 if u8 else torch.float32)
        if out is None:
            out = torch.empty((Ho, Wo, 3), device=s.device, dtype=torch.uint8) if u8 else \
                torch.empty((1, 3, Ho, Wo), device=s.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_luma_merge(self._ctx, s.data_ptr(), Ho, Wo, c.data_ptr(), Hc, Wc, None if u8 else out.data_ptr(),
                                           out.data_ptr() if u8 else None, int(round_mode)))
        return out.view(Ho, Wo, 3) if u8 else out.view(1, 3, Ho, Wo)

    @torch.no_grad()
    def stylize_color(self, contentImg: torch.Tensor, styleImg: torch.Tensor, mode: str, alpha: Optional[float] = None, num_run: int = 1,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """stylize() with colour preservation, one library call (wct_stylize_color).  mode "match": the style is colour-matched to
        the content once, before the cascade; "luma": the result keeps the content's chroma (luma_merge after the last run);
        "match+luma": both.  Bit-identical to the composition of color_match / stylize / luma_merge; afterwards the prepared style
        statistics are the MATCHED style's."""
        if mode not in _lib.COLOR_MODES:
            raise ValueError("stylize_color: mode must be one of %s, got %r" % (", ".join(repr(m) for m in _lib.COLOR_MODES), mode))
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_color(self._ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, alpha, int(num_run), _lib.COLOR_MODES[mode],
                                              out.data_ptr(), byref(ho), byref(wo)))
        self._style_keep = s      # the matching reads it asynchronously
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ guided-filter smoothing (include/wct_hip_smooth.h)
    @staticmethod
    def _smooth_args(what: str, radius, eps) -> None:
        if int(radius) != radius or not 1 <= int(radius) <= _lib.SMOOTH_MAX_RADIUS:
            raise ValueError("%s: radius must be an integer in 1 .. %d, got %r" % (what, _lib.SMOOTH_MAX_RADIUS, radius))
        if not (float(eps) > 0.0 and float(eps) < float("inf")):
            raise ValueError("%s: eps must be finite and positive, got %r" % (what, eps))

    @torch.no_grad()
    def guided_filter(self, src: torch.Tensor, guide: torch.Tensor, radius: int, eps: float = _lib.SMOOTH_EPS, out: Optional[torch.Tensor] = None,
                      u8: bool = False, round_mode: int = 0) -> torch.Tensor:
        """He et al.'s guided image filter of `src` with the colour image `guide` (its top-left window that `src` covers): windows
        of radius `radius` clipped to the image, regulariser `eps` relative to [0, 1] images, fp64 inside, not clamped
        (wct_guided_filter).  u8=False: fp32 [1,3,Ho,Wo], `out` may be `src` itself; u8=True: uint8 [Ho,Wo,3] with the conversion
        of to_u8(., round_mode) fused in, byte-identical to to_u8 of the fp32 result."""
        s, g = self._img(src), self._img(guide)
        Ho, Wo, Hg, Wg = int(s.shape[1]), int(s.shape[2]), int(g.shape[1]), int(g.shape[2])
        if Ho > Hg or Wo > Wg:
            raise ValueError("guided_filter: the source (%d x %d) is larger than the guide (%d x %d)" % (Ho, Wo, Hg, Wg))
        self._smooth_args("guided_filter", radius, eps)
        out = self._out_like(out, "guided_filter", 3 * Ho * Wo, torch.uint8 if u8 else torch.float32)
        if out is None:
            out = torch.empty((Ho, Wo, 3), device=s.device, dtype=torch.uint8) if u8 else \
                torch.empty((1, 3, Ho, Wo), device=s.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_guided_filter(self._ctx, s.data_ptr(), Ho, Wo, g.data_ptr(), Hg, Wg, int(radius), float(eps),
                                              None if u8 else out.data_ptr(), out.data_ptr() if u8 else None, int(round_mode)))
        return out.view(Ho, Wo, 3) if u8 else out.view(1, 3, Ho, Wo)

    @torch.no_grad()
    def stylize_smooth(self, contentImg: torch.Tensor, styleImg: torch.Tensor, radius: int, eps: float = _lib.SMOOTH_EPS,
                       color: Optional[str] = None, alpha: Optional[float] = None, num_run: int = 1,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """stylize() followed by guided_filter() with the ORIGINAL content as guide, one library call (wct_stylize_smooth).  `color`
        is None or a mode of stylize_color: "match" before the cascade, "luma" after the filter.  Bit-identical to the composition
        of color_match / stylize / guided_filter / luma_merge; the prepared style statistics afterwards are those of the cascade it
        wraps (the MATCHED style's with "match")."""
        if color is not None and color not in _lib.COLOR_MODES:
            raise ValueError("stylize_smooth: color must be None or one of %s, got %r" % (", ".join(repr(m) for m in _lib.COLOR_MODES), color))
        self._smooth_args("stylize_smooth", radius, eps)
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_smooth(self._ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, alpha, int(num_run),
                                               _lib.COLOR_MODES[color] if color else 0, int(radius), float(eps), out.data_ptr(), byref(ho), byref(wo)))
        self._style_keep = s      # the side stream (and the matching) read it asynchronously
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ patch swap (include/wct_hip_swap.h)
    @staticmethod
    def _swap_match(what: str, match: str) -> int:
        if match not in _lib.SWAP_MATCHES:
            raise ValueError("%s: match must be one of %s, got %r" % (what, ", ".join(repr(m) for m in _lib.SWAP_MATCHES), match))
        return _lib.SWAP_MATCHES[match]

    @torch.no_grad()
    def patch_match(self, q: torch.Tensor, k: torch.Tensor, want_best: bool = False):
        """For every 3x3 patch of the NHWC query map `q` [1,h,w,C] the index of the best-matching 3x3 patch of the key map `k`
        [1,hs,ws,C] under the key-normalised cross-correlation (wct_patch_match): an int32 tensor [(h-2)*(w-2)], and the winning
        scores (fp32) with want_best.  The lowest index wins among equal scores."""
        qf, kf = self._nhwc(q), self._nhwc(k)
        h, w, C = (int(v) for v in qf.shape)
        hs, ws, Ck = (int(v) for v in kf.shape)
        if Ck != C:
            raise ValueError("patch_match: the maps have %d and %d channels" % (C, Ck))
        if min(h, w, hs, ws) < 3:
            raise ValueError("patch_match: maps %dx%d and %dx%d must be at least 3x3" % (h, w, hs, ws))
        idx = torch.empty((h - 2) * (w - 2), device=qf.device, dtype=torch.int32)
        best = torch.empty((h - 2) * (w - 2), device=qf.device, dtype=torch.float32) if want_best else None
        self._stream()
        self._chk(self._lib.wct_patch_match(self._ctx, qf.data_ptr(), h, w, kf.data_ptr(), hs, ws, C, idx.data_ptr(),
                                            best.data_ptr() if want_best else None))
        return (idx, best) if want_best else idx

    @torch.no_grad()
    def patch_assemble(self, idx: torch.Tensor, h: int, w: int, v: torch.Tensor, base: Optional[torch.Tensor] = None,
                       alpha: float = 1.0) -> torch.Tensor:
        """alpha * (the average of the value patches of `v` [1,hs,ws,C] that the queries covering each pixel chose) + (1 - alpha) *
        `base` [1,h,w,C] (wct_patch_assemble); `base` may be None only with alpha == 1.  Returns [1,h,w,C] fp32."""
        vf = self._nhwc(v)
        hs, ws, C = (int(t) for t in vf.shape)
        h, w = int(h), int(w)
        if idx.dtype != torch.int32 or idx.numel() != max(h - 2, 0) * max(w - 2, 0):
            raise ValueError("patch_assemble: idx must be int32 with (h-2)*(w-2) = %d entries" % (max(h - 2, 0) * max(w - 2, 0)))
        ix = idx.to(self.stats_device).contiguous()
        bf = None
        if base is not None:
            bf = self._nhwc(base)
            if tuple(bf.shape) != (h, w, C):
                raise ValueError("patch_assemble: base must be [1,%d,%d,%d], got %s" % (h, w, C, tuple(base.shape)))
        elif float(alpha) != 1.0:
            raise ValueError("patch_assemble: base may be None only with alpha == 1")
        out = torch.empty((1, h, w, C), device=vf.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_patch_assemble(self._ctx, ix.data_ptr(), h, w, vf.data_ptr(), hs, ws, C,
                                               bf.data_ptr() if bf is not None else None, float(alpha), out.data_ptr()))
        return out

    @torch.no_grad()
    def swap_level(self, level: int, contentImg: torch.Tensor, styleImg: torch.Tensor, match: str = "whitened",
                   alpha: Optional[float] = None) -> torch.Tensor:
        """One level with the style decorator instead of an affine transform (wct_swap_level): encode both images, replace every 3x3
        content patch by its best-matching style patch (`match`: "whitened" = in both whitened domains, "raw" = on the features),
        blend with the content feature by alpha, decode."""
        mode = self._swap_match("swap_level", match)
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        lv = int(level) if int(level) in (1, 2, 3, 4, 5) else 1
        out = torch.empty((1, 3, (H >> (lv - 1)) << (lv - 1), (W >> (lv - 1)) << (lv - 1)), device=c.device, dtype=torch.float32)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_swap_level(self._ctx, int(level), c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, mode, alpha,
                                           out.data_ptr(), byref(ho), byref(wo)))
        assert (ho.value, wo.value) == tuple(out.shape[2:])
        return out

    @torch.no_grad()
    def stylize_swap(self, contentImg: torch.Tensor, styleImg: torch.Tensor, swap_level: int, match: str = "whitened",
                     alpha: Optional[float] = None, num_run: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The 5 -> 1 cascade with level `swap_level` (2..5) run through swap_level() and every other level through
        style_transfer_level() under the context's transform, one library call (wct_stylize_swap); bit-identical to that
        composition."""
        mode = self._swap_match("stylize_swap", match)
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_swap(self._ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, int(swap_level), mode, alpha,
                                             int(num_run), out.data_ptr(), byref(ho), byref(wo)))
        self._style_keep = s      # the side stream reads it asynchronously
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ attention statistics (include/wct_hip_attn.h)
    @staticmethod
    def _attn_domain(what: str, match: str) -> int:
        if match not in _lib.ATTN_MATCHES:
            raise ValueError("%s: match must be one of %s, got %r" % (what, ", ".join(repr(m) for m in _lib.ATTN_MATCHES), match))
        return _lib.ATTN_MATCHES[match]

    @torch.no_grad()
    def attn_project(self, feat: torch.Tensor, match: str = "attention", want_std: bool = True):
        """The unit rows of the NHWC map `feat` [1,h,w,C] projected into the match domain ("attention": the standardised map,
        "attention_whitened": the whitened map of the patch swap), and with want_std the standardised map (wct_attn_project):
        (unit, std) or unit, each [1,h,w,C] fp32."""
        domain = self._attn_domain("attn_project", match)
        f = self._nhwc(feat)
        h, w, C = (int(v) for v in f.shape)
        unit = torch.empty((1, h, w, C), device=f.device, dtype=torch.float32)
        std = torch.empty((1, h, w, C), device=f.device, dtype=torch.float32) if want_std else None
        self._stream()
        self._chk(self._lib.wct_attn_project(self._ctx, f.data_ptr(), h, w, C, domain, unit.data_ptr(), std.data_ptr() if want_std else None))
        return (unit, std) if want_std else unit

    @torch.no_grad()
    def attn_stats(self, qhat: torch.Tensor, khat: torch.Tensor, v: torch.Tensor, tau: float):
        """Per query row of `qhat` [Nq,C] the softmax(tau <q^, k^>)-weighted mean and variance of the value rows `v` [Nk,C] over the
        key rows `khat` [Nk,C] (wct_attn_stats): (mean, var), each [Nq,C] fp32.  No Nq x Nk matrix exists anywhere."""
        q, k, vv = (self._dev_f32(t.reshape(-1, t.shape[-1])) for t in (qhat, khat, v))
        Nq, C = (int(t) for t in q.shape)
        Nk = int(k.shape[0])
        if tuple(k.shape) != (Nk, C) or tuple(vv.shape) != (Nk, C):
            raise ValueError("attn_stats: qhat %s, khat %s and v %s do not agree" % (tuple(q.shape), tuple(k.shape), tuple(vv.shape)))
        mean = torch.empty((Nq, C), device=q.device, dtype=torch.float32)
        var = torch.empty((Nq, C), device=q.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_attn_stats(self._ctx, q.data_ptr(), Nq, k.data_ptr(), vv.data_ptr(), Nk, C, float(tau), mean.data_ptr(), var.data_ptr()))
        return mean, var

    @torch.no_grad()
    def attn_apply(self, mean: torch.Tensor, var: torch.Tensor, c_std: torch.Tensor, cF: torch.Tensor, mu_s: torch.Tensor,
                   sigma_s: torch.Tensor, alpha: Optional[float] = None) -> torch.Tensor:
        """alpha (sigma_s (sqrt(var) c_std + mean) + mu_s) + (1 - alpha) cF per position (wct_attn_apply); the four maps [n,C] (or
        NHWC) fp32, mu_s and sigma_s [C] fp64.  Returns a tensor shaped like cF."""
        alpha = self.alpha if alpha is None else float(alpha)
        C = int(cF.shape[-1])
        m, vr, z, x = (self._dev_f32(t.reshape(-1, C)) for t in (mean, var, c_std, cF))
        n = int(x.shape[0])
        if not all(tuple(t.shape) == (n, C) for t in (m, vr, z)):
            raise ValueError("attn_apply: the four maps must have one shape")
        mu = self._dev_f64(mu_s, C, "attn_apply: mu_s")
        sg = self._dev_f64(sigma_s, C, "attn_apply: sigma_s")
        out = torch.empty((n, C), device=x.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_attn_apply(self._ctx, m.data_ptr(), vr.data_ptr(), z.data_ptr(), x.data_ptr(), n, C, mu.data_ptr(), sg.data_ptr(),
                                           alpha, out.data_ptr()))
        return out.view(cF.shape)

    @torch.no_grad()
    def attn_level(self, level: int, contentImg: torch.Tensor, styleImg: torch.Tensor, match: str = "attention", tau: float = _lib.ATTN_TEMP,
                   alpha: Optional[float] = None) -> torch.Tensor:
        """One level with attention-weighted style statistics instead of one affine transform (wct_attn_level): encode both images,
        give every content position the softmax-weighted style mean and deviation, blend with the content feature by alpha, decode."""
        domain = self._attn_domain("attn_level", match)
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        lv = int(level) if int(level) in (1, 2, 3, 4, 5) else 1
        out = torch.empty((1, 3, (H >> (lv - 1)) << (lv - 1), (W >> (lv - 1)) << (lv - 1)), device=c.device, dtype=torch.float32)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_attn_level(self._ctx, int(level), c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, domain, float(tau), alpha,
                                           out.data_ptr(), byref(ho), byref(wo)))
        assert (ho.value, wo.value) == tuple(out.shape[2:])
        return out

    @torch.no_grad()
    def stylize_attn(self, contentImg: torch.Tensor, styleImg: torch.Tensor, attn_level: int, match: str = "attention",
                     tau: float = _lib.ATTN_TEMP, alpha: Optional[float] = None, num_run: int = 1,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The 5 -> 1 cascade with level `attn_level` (2..5) run through attn_level() and every other level through
        style_transfer_level() under the context's transform, one library call (wct_stylize_attn); bit-identical to that
        composition."""
        domain = self._attn_domain("stylize_attn", match)
        alpha = self.alpha if alpha is None else float(alpha)
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_attn(self._ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, int(attn_level), domain, float(tau), alpha,
                                             int(num_run), out.data_ptr(), byref(ho), byref(wo)))
        self._style_keep = s      # the side stream reads it asynchronously
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ scale control (include/wct_hip_scale.h)
    @staticmethod
    def scale_shape(H: int, W: int, divisor: int):
        """(h_d, w_d) = (16 floor(H / (16 d)), 16 floor(W / (16 d))): the working size of a content of H x W at `divisor`
        (wct_scale_shape, host only).  ValueError for a divisor outside 1 .. 16 or a working size under 32."""
        h, w = c_int(), c_int()
        if _lib.load().wct_scale_shape(int(H), int(W), int(divisor), byref(h), byref(w)) != _lib.WCT_OK:
            raise ValueError("scale_shape: %d x %d at divisor %r: a divisor in 1 .. %d and a working size of 32 x 32 at least expected"
                             % (H, W, divisor, _lib.SCALE_MAX_DIVISOR))
        return h.value, w.value

    @staticmethod
    def _scale_filter(what: str, filter: str) -> int:
        if filter not in _lib.RESIZE_FILTERS:
            raise ValueError("%s: filter must be one of %s, got %r" % (what, ", ".join(repr(f) for f in _lib.RESIZE_FILTERS), filter))
        return _lib.RESIZE_FILTERS[filter]

    @staticmethod
    def _scale_sizes(what: str, H: int, W: int, oH: int, oW: int) -> None:
        if min(H, W, oH, oW) < 1:
            raise ValueError("%s: empty shape (%d x %d -> %d x %d)" % (what, H, W, oH, oW))
        if H > _lib.SCALE_MAX_SHRINK * oH or W > _lib.SCALE_MAX_SHRINK * oW:
            raise ValueError("%s: %d x %d -> %d x %d shrinks an axis by more than %d" % (what, H, W, oH, oW, _lib.SCALE_MAX_SHRINK))

    @torch.no_grad()
    def resample(self, img: torch.Tensor, size, filter: str = "bicubic", out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The planar fp32 image `img` resampled to size = (oH, oW) with Pillow's bilinear or bicubic weights in floating point
        (wct_resample_planar): separable, horizontal pass first, fp32 sums in tap order, not clamped, bitwise reproducible; equal
        sizes are a copy.  `out`: an fp32 tensor on this device with 3*oH*oW values, contiguous, any 4-byte alignment."""
        f = self._scale_filter("resample", filter)
        x = self._img(img)
        H, W, oH, oW = int(x.shape[1]), int(x.shape[2]), int(size[0]), int(size[1])
        self._scale_sizes("resample", H, W, oH, oW)
        out = self._out_like(out, "resample", 3 * oH * oW)
        if out is None:
            out = torch.empty((1, 3, oH, oW), device=x.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_resample_planar(self._ctx, x.data_ptr(), H, W, out.data_ptr(), oH, oW, f))
        return out.view(1, 3, oH, oW)

    @torch.no_grad()
    def pyramid_merge(self, a: torch.Tensor, b: Optional[torch.Tensor], c: Optional[torch.Tensor], gain: float = _lib.SCALE_DETAIL,
                      size=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """resample(a - gain * b, c's size, "bicubic") + gain * c in one kernel (wct_pyramid_merge): `a` and `b` at the coarse
        size, `c` at the fine one.  gain == 0 is resample(a) bit for bit; b and c may then be None and `size` names the result's."""
        gain = float(gain)
        if not (0.0 <= gain < float("inf")):
            raise ValueError("pyramid_merge: gain must be finite and >= 0, got %r" % (gain,))
        af = self._img(a)
        hc, wc = int(af.shape[1]), int(af.shape[2])
        if (b is None or c is None) and gain != 0.0:
            raise ValueError("pyramid_merge: b and c may be None only with gain == 0")
        bf = cf = None
        if b is not None and c is not None:
            bf, cf = self._img(b), self._img(c)
            if tuple(bf.shape) != tuple(af.shape):
                raise ValueError("pyramid_merge: a and b must have one shape, got %s and %s" % (tuple(af.shape), tuple(bf.shape)))
            if size is not None and (int(size[0]), int(size[1])) != (int(cf.shape[1]), int(cf.shape[2])):
                raise ValueError("pyramid_merge: size %r is not c's %s" % (size, tuple(cf.shape[1:])))
            size = (int(cf.shape[1]), int(cf.shape[2]))
        elif size is None:
            raise ValueError("pyramid_merge: without b and c the result's size is required")
        hf, wf = int(size[0]), int(size[1])
        self._scale_sizes("pyramid_merge", hc, wc, hf, wf)
        out = self._out_like(out, "pyramid_merge", 3 * hf * wf)
        if out is None:
            out = torch.empty((1, 3, hf, wf), device=af.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_pyramid_merge(self._ctx, af.data_ptr(), bf.data_ptr() if bf is not None else None, hc, wc,
                                              cf.data_ptr() if cf is not None else None, hf, wf, gain, out.data_ptr()))
        return out.view(1, 3, hf, wf)

    @staticmethod
    def _level_div(what: str, level_scale) -> List[int]:
        div = [int(d) for d in level_scale]
        if len(div) != 5 or any(int(d) != d for d in level_scale):
            raise ValueError("%s: five integer divisors expected (levels 5, 4, 3, 2, 1), got %r" % (what, level_scale))
        if any(not 1 <= d <= _lib.SCALE_MAX_DIVISOR for d in div):
            raise ValueError("%s: every divisor must lie in 1 .. %d, got %r" % (what, _lib.SCALE_MAX_DIVISOR, div))
        if any(div[i] > div[i - 1] for i in range(1, 5)) or div[4] != 1:
            raise ValueError("%s: the divisors must not increase from level 5 to level 1 and must end in 1, got %r" % (what, div))
        return div

    @torch.no_grad()
    def stylize_scaled(self, contentImg: torch.Tensor, styleImg: Optional[torch.Tensor], level_scale, detail_gain: float = _lib.SCALE_DETAIL,
                       alpha: Optional[float] = None, num_run: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The 5 -> 1 cascade with level L run on the content reduced by level_scale[5 - L] (divisors of levels 5, 4, 3, 2, 1, e.g.
        (4, 4, 2, 1, 1)), one library call (wct_stylize_scaled): where the divisor changes, the running image is brought to the next
        working size by pyramid_merge(cur, content at the old size, content at the new size, detail_gain).  Bit-identical to the
        composition of resample / pyramid_merge / style_transfer_level; all divisors 1 is stylize().  styleImg=None runs against
        the statistics already in the context (style_prepare per level set = scale mixing), which then survive the call."""
        div = self._level_div("stylize_scaled", level_scale)
        detail_gain = float(detail_gain)
        if not (0.0 <= detail_gain < float("inf")):
            raise ValueError("stylize_scaled: detail_gain must be finite and >= 0, got %r" % (detail_gain,))
        alpha = self.alpha if alpha is None else float(alpha)
        c = self._img(contentImg)
        H, W = int(c.shape[1]), int(c.shape[2])
        for d in sorted(set(div)):
            self.scale_shape(H, W, d)
        s, Hs, Ws = None, 0, 0
        if styleImg is not None:
            s = self._img(styleImg)
            Hs, Ws = int(s.shape[1]), int(s.shape[2])
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_scaled(self._ctx, c.data_ptr(), H, W, s.data_ptr() if s is not None else None, Hs, Ws, alpha,
                                               int(num_run), (c_int * 5)(*div), detail_gain, out.data_ptr(), byref(ho), byref(wo)))
        if s is not None:
            self._style_keep = s      # the side stream reads it asynchronously
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ proxy mode (include/wct_hip_bgrid.h)
    @staticmethod
    def bgrid_shape(h: int, w: int, cell: int = _lib.BGRID_CELL):
        """(gh, gw) = (ceil(h / cell) + 1, ceil(w / cell) + 1): the spatial vertices of a bilateral grid over an h x w image
        (wct_bgrid_shape, host only).  ValueError for an empty shape, cell < 1 or a result above 256."""
        gh, gw = c_int(), c_int()
        if _lib.load().wct_bgrid_shape(int(h), int(w), int(cell), byref(gh), byref(gw)) != _lib.WCT_OK:
            raise ValueError("bgrid_shape: %d x %d with cell %r: a non-empty shape, cell >= 1 and at most %d vertices per axis expected"
                             % (h, w, cell, _lib.BGRID_MAX_XY))
        return gh.value, gw.value

    @staticmethod
    def _bgrid_args(what: str, gz=None, gh=None, gw=None, eps=None, smooth=None) -> None:
        for name, g, top in (("gz", gz, _lib.BGRID_MAX_Z), ("gh", gh, _lib.BGRID_MAX_XY), ("gw", gw, _lib.BGRID_MAX_XY)):
            if g is not None and (int(g) != g or not 1 <= int(g) <= top):
                raise ValueError("%s: %s must be an integer in 1 .. %d, got %r" % (what, name, top, g))
        if eps is not None and not (float(eps) > 0.0 and float(eps) < float("inf")):
            raise ValueError("%s: eps must be finite and positive, got %r" % (what, eps))
        if smooth is not None and (int(smooth) != smooth or not 0 <= int(smooth) <= _lib.BGRID_MAX_SMOOTH):
            raise ValueError("%s: smooth must be an integer in 0 .. %d, got %r" % (what, _lib.BGRID_MAX_SMOOTH, smooth))

    @torch.no_grad()
    def bgrid_fit(self, reduced: torch.Tensor, stylised: torch.Tensor, gz: int, gh: int, gw: int, eps: float = _lib.BGRID_EPS,
                  smooth: int = _lib.BGRID_SMOOTH, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The bilateral grid of local 3 x 4 affine colour maps that takes `reduced` to `stylised` (two images of one size): an fp32
        tensor [gz, gh, gw, 3, 4] (wct_bgrid_fit; Chen et al. 2016).  Weighted least squares per vertex, regularised towards the
        global fit by `eps`, the sums blurred `smooth` times; fp64 inside, rounded once; bitwise reproducible."""
        a, b = self._img(reduced), self._img(stylised)
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError("bgrid_fit: the two images must have one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
        self._bgrid_args("bgrid_fit", gz, gh, gw, eps, smooth)
        h, w = int(a.shape[1]), int(a.shape[2])
        out = self._out_like(out, "bgrid_fit", int(gz) * int(gh) * int(gw) * 12)
        if out is None:
            out = torch.empty((int(gz), int(gh), int(gw), 3, 4), device=a.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_bgrid_fit(self._ctx, a.data_ptr(), b.data_ptr(), h, w, int(gz), int(gh), int(gw), float(eps), int(smooth),
                                          out.data_ptr()))
        return out.view(int(gz), int(gh), int(gw), 3, 4)

    @torch.no_grad()
    def bgrid_slice(self, grid: torch.Tensor, content: torch.Tensor, out: Optional[torch.Tensor] = None, u8: bool = False,
                    round_mode: int = 0) -> torch.Tensor:
        """The grid [gz, gh, gw, 3, 4] applied to a full-resolution image: per pixel the affine map interpolated from its 8 vertices
        (x, y, and the pixel's own luminance), evaluated in fp64, not clamped (wct_bgrid_slice).  u8=False: fp32 [1,3,H,W], `out`
        may be `content` itself; u8=True: uint8 [H,W,3] with the conversion of to_u8(., round_mode) fused in, byte-identical to
        to_u8 of the fp32 result."""
        if grid.dim() != 5 or tuple(grid.shape[3:]) != (3, 4):
            raise ValueError("bgrid_slice: expected a [gz, gh, gw, 3, 4] grid, got %s" % (tuple(grid.shape),))
        gz, gh, gw = int(grid.shape[0]), int(grid.shape[1]), int(grid.shape[2])
        self._bgrid_args("bgrid_slice", gz, gh, gw)
        g, c = self._dev_f32(grid), self._img(content)
        H, W = int(c.shape[1]), int(c.shape[2])
        out = self._out_like(out, "bgrid_slice", 3 * H * W, torch.uint8 if u8 else torch.float32)
        if out is None:
            out = torch.empty((H, W, 3), device=c.device, dtype=torch.uint8) if u8 else \
                torch.empty((1, 3, H, W), device=c.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_bgrid_slice(self._ctx, g.data_ptr(), gz, gh, gw, c.data_ptr(), H, W, None if u8 else out.data_ptr(),
                                            out.data_ptr() if u8 else None, int(round_mode)))
        return out.view(H, W, 3) if u8 else out.view(1, 3, H, W)

    @torch.no_grad()
    def stylize_proxy(self, contentImg: torch.Tensor, styleImg: Optional[torch.Tensor], divisor: int, cell: int = _lib.BGRID_CELL,
                      bins: int = _lib.BGRID_BINS, eps: float = _lib.BGRID_EPS, smooth: int = _lib.BGRID_SMOOTH, alpha: Optional[float] = None,
                      num_run: int = 1, out: Optional[torch.Tensor] = None, u8: bool = False, round_mode: int = 0) -> torch.Tensor:
        """Proxy mode, one library call (wct_stylize_proxy): the content reduced to scale_shape(H, W, divisor), stylised there, a
        bilateral grid (bgrid_shape(., cell) x `bins` luminance vertices) fitted to the reduced pair and applied to the FULL content.
        The result has the content's exact H x W and its edges -- colour and tone, no strokes.  Bit-identical to the composition of
        resample / stylize / bgrid_fit / bgrid_slice.  styleImg=None runs against the statistics already in the context."""
        if int(divisor) != divisor or not 1 <= int(divisor) <= _lib.SCALE_MAX_DIVISOR:
            raise ValueError("stylize_proxy: divisor must be an integer in 1 .. %d, got %r" % (_lib.SCALE_MAX_DIVISOR, divisor))
        self._bgrid_args("stylize_proxy", gz=bins, eps=eps, smooth=smooth)
        alpha = self.alpha if alpha is None else float(alpha)
        c = self._img(contentImg)
        H, W = int(c.shape[1]), int(c.shape[2])
        h, w = self.scale_shape(H, W, int(divisor))
        self.bgrid_shape(h, w, cell)
        s, Hs, Ws = None, 0, 0
        if styleImg is not None:
            s = self._img(styleImg)
            Hs, Ws = int(s.shape[1]), int(s.shape[2])
        out = self._out_like(out, "stylize_proxy", 3 * H * W, torch.uint8 if u8 else torch.float32)
        if out is None:
            out = torch.empty((H, W, 3), device=c.device, dtype=torch.uint8) if u8 else \
                torch.empty((1, 3, H, W), device=c.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_stylize_proxy(self._ctx, c.data_ptr(), H, W, s.data_ptr() if s is not None else None, Hs, Ws, alpha, int(num_run),
                                              int(divisor), int(cell), int(bins), float(eps), int(smooth), None if u8 else out.data_ptr(),
                                              out.data_ptr() if u8 else None, int(round_mode)))
        if s is not None:
            self._style_keep = s      # the side stream reads it asynchronously
        return out.view(H, W, 3) if u8 else out.view(1, 3, H, W)

    # ------------------------------------------------------------------ device JPEG encoder (include/wct_hip_jpeg.h)
    @staticmethod
    def _jpeg_args(what: str, H: int, W: int, quality=None) -> None:
        if not (1 <= int(H) <= _lib.JPEG_MAX_DIM and 1 <= int(W) <= _lib.JPEG_MAX_DIM):
            raise ValueError("%s: %d x %d is outside 1 .. %d per axis" % (what, H, W, _lib.JPEG_MAX_DIM))
        if quality is not None and (isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100):
            raise ValueError("%s: quality must be an integer in 1 .. 100, got %r" % (what, quality))

    @staticmethod
    def jpeg_header(H: int, W: int, quality: int = _lib.JPEG_QUALITY):
        """(the 623 header bytes SOI .. SOS, the scaled Y table, the scaled chroma table; tables as 8 x 8 uint16 in natural order) of an
        H x W file at `quality` (wct_jpeg_header, host only)."""
        WCT._jpeg_args("jpeg_header", H, W, quality)
        hdr = (ctypes.c_uint8 * _lib.JPEG_HEADER_BYTES)()
        qy, qc = (ctypes.c_uint16 * 64)(), (ctypes.c_uint16 * 64)()
        if _lib.load().wct_jpeg_header(int(H), int(W), int(quality), hdr, qy, qc) != _lib.WCT_OK:
            raise ValueError("jpeg_header: refused %d x %d at quality %r" % (H, W, quality))
        return bytes(hdr), np.array(qy, dtype=np.uint16).reshape(8, 8), np.array(qc, dtype=np.uint16).reshape(8, 8)

    @staticmethod
    def jpeg_bound(H: int, W: int) -> int:
        """A capacity that no H x W image can overflow, header included (wct_jpeg_bound, host only)."""
        WCT._jpeg_args("jpeg_bound", H, W)
        n = ctypes.c_uint64()
        if _lib.load().wct_jpeg_bound(int(H), int(W), byref(n)) != _lib.WCT_OK:
            raise ValueError("jpeg_bound: refused %d x %d" % (H, W))
        return int(n.value)

    @staticmethod
    def jpeg_num_blocks(H: int, W: int) -> int:
        return 6 * ((int(H) + 15) // 16) * ((int(W) + 15) // 16)

    @torch.no_grad()
    def jpeg_blocks(self, img_u8: torch.Tensor, quality: int = _lib.JPEG_QUALITY) -> torch.Tensor:
        """The quantised coefficients of a uint8 H x W x 3 device image: int16 [blocks, 64], zig-zag order inside a block, blocks in
        scan order -- per 16 x 16 MCU Y00 Y01 Y10 Y11 Cb Cr, MCUs row-major (wct_jpeg_blocks)."""
        x = self._u8(img_u8)
        H, W = int(x.shape[0]), int(x.shape[1])
        self._jpeg_args("jpeg_blocks", H, W, quality)
        coef = torch.empty((self.jpeg_num_blocks(H, W), 64), device=x.device, dtype=torch.int16)
        self._stream()
        self._chk(self._lib.wct_jpeg_blocks(self._ctx, x.data_ptr(), H, W, int(quality), coef.data_ptr()))
        return coef

    def _jpeg_out(self, what: str, device, capacity, out, length):
        if out is None:
            out = torch.empty(int(capacity), device=device, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
            raise ValueError("%s: `out` must be a contiguous uint8 tensor on the context's device" % what)
        if length is None:
            length = torch.empty(1, device=device, dtype=torch.int64)
        elif length.dtype != torch.int64 or length.numel() != 1 or length.device != device:
            raise ValueError("%s: `length` must be a one-element int64 tensor on the context's device" % what)
        return out, length

    @torch.no_grad()
    def jpeg_pack(self, coef: torch.Tensor, H: int, W: int, capacity: Optional[int] = None, out: Optional[torch.Tensor] = None,
                  length: Optional[torch.Tensor] = None):
        """The entropy-coded segment of jpeg_blocks' coefficients -- stuffed, padded, FF D9 behind it -- without synchronising
        (wct_jpeg_pack): (uint8 device buffer, one-element int64 device tensor with the length; -1 = the capacity did not suffice)."""
        self._jpeg_args("jpeg_pack", H, W)
        if coef.dtype != torch.int16 or coef.numel() != 64 * self.jpeg_num_blocks(H, W):
            raise ValueError("jpeg_pack: expected int16 [%d, 64] coefficients, got %s %s" % (self.jpeg_num_blocks(H, W), coef.dtype, tuple(coef.shape)))
        c = coef.to(self.stats_device).contiguous()
        out, length = self._jpeg_out("jpeg_pack", c.device, self.jpeg_bound(H, W) if capacity is None else capacity, out, length)
        cap = out.numel() if capacity is None else min(int(capacity), out.numel())
        self._stream()
        self._chk(self._lib.wct_jpeg_pack(self._ctx, c.data_ptr(), int(H), int(W), out.data_ptr(), cap, length.data_ptr()))
        return out, length

    @torch.no_grad()
    def jpeg_encode_async(self, img_u8: torch.Tensor, quality: int = _lib.JPEG_QUALITY, capacity: Optional[int] = None,
                          out: Optional[torch.Tensor] = None, length: Optional[torch.Tensor] = None):
        """The complete JPEG file of a uint8 H x W x 3 device image, byte-identical to Pillow's Image.fromarray(img).save(path,
        quality=quality), enqueued on the current stream without synchronising (wct_jpeg_encode): (uint8 device buffer, one-element
        int64 device tensor with the file's length; -1 = the capacity did not suffice and nothing was written beyond it).  The
        default capacity is jpeg_bound(H, W); `out` / `length` reuse a caller's buffers."""
        x = self._u8(img_u8)
        H, W = int(x.shape[0]), int(x.shape[1])
        self._jpeg_args("jpeg_encode", H, W, quality)
        out, length = self._jpeg_out("jpeg_encode", x.device, self.jpeg_bound(H, W) if capacity is None else capacity, out, length)
        cap = out.numel() if capacity is None else min(int(capacity), out.numel())
        self._stream()
        self._chk(self._lib.wct_jpeg_encode(self._ctx, x.data_ptr(), H, W, int(quality), out.data_ptr(), cap, length.data_ptr()))
        return out, length

    def jpeg_encode(self, img_u8: torch.Tensor, quality: int = _lib.JPEG_QUALITY) -> bytes:
        """jpeg_encode_async, then the file's bytes on the host (synchronises: for convenience and for tests).  The first attempt
        uses a capacity of the raw image's size; one that overflows is repeated at jpeg_bound."""
        H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
        for cap in (min(3 * H * W + 4096, self.jpeg_bound(H, W)), self.jpeg_bound(H, W)):
            buf, length = self.jpeg_encode_async(img_u8, quality, capacity=cap)
            n = int(length.item())
            if n >= 0:
                return buf[:n].cpu().numpy().tobytes()
        raise _lib.WctError(_lib.WCT_ERR_STATE, "jpeg_encode: %d x %d overflowed its own bound" % (H, W))

    # ------------------------------------------------------------------ device JPEG decoder (include/wct_hip_jdec.h)
    @staticmethod
    def jdec_parse(data: bytes):
        """The wct_jdec_info of a JPEG file's bytes (wct_jdec_parse, host only), or None when the file is not one the device decoder
        takes (WCT_JDEC_UNSUPPORTED): progressive, CMYK, several scans, truncated, ..."""
        buf = bytes(data)
        info = _lib.WctJdecInfo()
        rc = _lib.load().wct_jdec_parse(buf, len(buf), byref(info))
        if rc == _lib.JDEC_UNSUPPORTED:
            return None
        if rc != _lib.WCT_OK:
            raise ValueError("jdec_parse: refused (code %d)" % rc)
        return info

    @staticmethod
    def jdec_num_blocks(info) -> int:
        n = ctypes.c_uint64()
        if _lib.load().wct_jdec_num_blocks(byref(info), byref(n)) != _lib.WCT_OK:
            raise ValueError("jdec_num_blocks: not an info that jdec_parse fills")
        return int(n.value)

    def _jdec_scan(self, what: str, scan: torch.Tensor, info) -> torch.Tensor:
        if scan.dtype != torch.uint8 or scan.dim() != 1 or not scan.is_contiguous() or scan.numel() < int(info.scan_length):
            raise ValueError("%s: the segment must be a contiguous 1-D uint8 tensor of at least info.scan_length = %d bytes" % (what, info.scan_length))
        return scan.to(self.stats_device)

    @staticmethod
    def _jdec_rounds(what: str, rounds) -> int:
        if isinstance(rounds, bool) or not isinstance(rounds, int) or not 0 <= rounds <= _lib.JDEC_MAX_ROUNDS:
            raise ValueError("%s: rounds 0 .. %d expected, got %r" % (what, _lib.JDEC_MAX_ROUNDS, rounds))
        return rounds

    @torch.no_grad()
    def jdec_coefficients(self, scan: torch.Tensor, info, rounds: int = 0):
        """The coefficients of a file's entropy-coded segment on the device (file[info.scan_offset:][:info.scan_length] as a uint8
        tensor), without synchronising (wct_jdec_coefficients): (int16 [blocks, 64] in zig-zag order, blocks in scan order, DC absolute
        -- the layout of jpeg_blocks; one-element int32 device tensor with the status JDEC_STATUS_*)."""
        s = self._jdec_scan("jdec_coefficients", scan, info)
        coef = torch.empty((self.jdec_num_blocks(info), 64), device=s.device, dtype=torch.int16)
        status = torch.empty(1, device=s.device, dtype=torch.int32)
        self._stream()
        self._chk(self._lib.wct_jdec_coefficients(self._ctx, s.data_ptr(), byref(info), self._jdec_rounds("jdec_coefficients", rounds),
                                                  coef.data_ptr(), status.data_ptr()))
        return coef, status

    @torch.no_grad()
    def jdec_pixels(self, coef: torch.Tensor, info) -> torch.Tensor:
        """uint8 H x W x 3 of jdec_coefficients' coefficients (wct_jdec_pixels): what Pillow's Image.open(path).convert("RGB") holds."""
        if coef.dtype != torch.int16 or coef.numel() != 64 * self.jdec_num_blocks(info):
            raise ValueError("jdec_pixels: expected int16 [%d, 64] coefficients, got %s %s" % (self.jdec_num_blocks(info), coef.dtype, tuple(coef.shape)))
        c = coef.to(self.stats_device).contiguous()
        out = torch.empty((int(info.H), int(info.W), 3), device=c.device, dtype=torch.uint8)
        self._stream()
        self._chk(self._lib.wct_jdec_pixels(self._ctx, c.data_ptr(), byref(info), out.data_ptr()))
        return out

    @torch.no_grad()
    def jdec_decode_async(self, scan: torch.Tensor, info, rounds: int = 0, out: Optional[torch.Tensor] = None,
                          status: Optional[torch.Tensor] = None):
        """The pixels of a file's entropy-coded segment, enqueued on the current stream without synchronising (wct_jdec_decode):
        (uint8 H x W x 3 device tensor, one-element int32 device tensor with the status).  Unless the status is JDEC_STATUS_OK the
        pixels are not to be used.  `out` / `status` reuse a caller's buffers."""
        s = self._jdec_scan("jdec_decode", scan, info)
        H, W = int(info.H), int(info.W)
        if out is None:
            out = torch.empty((H, W, 3), device=s.device, dtype=torch.uint8)
        elif out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous() or out.device != s.device:
            raise ValueError("jdec_decode: `out` must be a contiguous uint8 [%d, %d, 3] tensor on the context's device" % (H, W))
        if status is None:
            status = torch.empty(1, device=s.device, dtype=torch.int32)
        elif status.dtype != torch.int32 or status.numel() != 1 or status.device != s.device:
            raise ValueError("jdec_decode: `status` must be a one-element int32 tensor on the context's device")
        self._stream()
        self._chk(self._lib.wct_jdec_decode(self._ctx, s.data_ptr(), byref(info), self._jdec_rounds("jdec_decode", rounds), out.data_ptr(),
                                            status.data_ptr()))
        return out, status

    def jdec_decode(self, data: bytes, rounds: int = 0):
        """A JPEG file's bytes to (uint8 H x W x 3 device tensor, status), or None when jdec_parse does not take the file
        (synchronises: for convenience and for tests)."""
        info = self.jdec_parse(data)
        if info is None:
            return None
        seg = np.frombuffer(data, np.uint8, int(info.scan_length), int(info.scan_offset))
        scan = torch.from_numpy(seg.copy()).to(self.stats_device) if len(seg) else torch.zeros(0, dtype=torch.uint8, device=self.stats_device)
        out, status = self.jdec_decode_async(scan, info, rounds)
        return out, int(status.item())

    # ------------------------------------------------------------------ video mode (include/wct_hip_video.h)
    def clip(self, H: int, W: int, rate: float = _lib.CLIP_RATE, cut: float = _lib.CLIP_CUT, blend: float = _lib.CLIP_BLEND,
             sigma: float = _lib.CLIP_SIGMA, radius: int = _lib.CLIP_RADIUS, motion=None) -> "Clip":
        """The state of one sequence of H x W frames (wct_clip_create): content statistics tracked over time at `rate` with a
        scene-cut reset above the distance `cut`, and a recursive blend of the output with weight `blend` where the content did not
        move (`sigma`, `radius`).  Allocates everything once; frames then go through Clip.stylize().  motion: None -- the blend
        compares the frames pixel by pixel; True or a dict of levels / range / penalty -- against the previous frame displaced by a
        block-matched field (Clip.attach_motion; include/wct_hip_motion.h)."""
        c = Clip(self, int(H), int(W), float(rate), float(cut), float(blend), float(sigma), int(radius))
        if motion is not None and motion is not False:
            try:
                c.attach_motion(**({} if motion is True else dict(motion)))
            except Exception:
                c.close()
                raise
        return c

    # ------------------------------------------------------------------ motion compensation (include/wct_hip_motion.h)
    @staticmethod
    def motion_shape(Ho: int, Wo: int) -> Tuple[int, int]:
        """The 8 x 8 block grid (nby, nbx) of an Ho x Wo image (wct_motion_shape)."""
        nby, nbx = c_int(), c_int()
        if _lib.load().wct_motion_shape(int(Ho), int(Wo), byref(nby), byref(nbx)) != _lib.WCT_OK:
            raise ValueError("libwct_hip: wct_motion_shape: a non-empty image expected, got %dx%d" % (Ho, Wo))
        return nby.value, nbx.value

    def _window(self, c: torch.Tensor, Ho: Optional[int], Wo: Optional[int]) -> Tuple[int, int]:
        return (int(c.shape[1]) if Ho is None else int(Ho)), (int(c.shape[2]) if Wo is None else int(Wo))

    @torch.no_grad()
    def motion_luma(self, img: torch.Tensor, levels: int = _lib.MOTION_LEVELS, Ho: Optional[int] = None, Wo: Optional[int] = None):
        """The uint8 luma pyramid of the top-left Ho x Wo (default: all) of a [1,3,H,W] / [3,H,W] image (wct_motion_luma): a list of
        `levels` uint8 [H_k, W_k] device tensors, level 0 first."""
        c = self._img(img)
        Ho, Wo = self._window(c, Ho, Wo)
        levels = int(levels)
        shapes = [(Ho >> k, Wo >> k) for k in range(max(levels, 0))]
        out = torch.empty(max(sum(h * w for h, w in shapes), 1), device=c.device, dtype=torch.uint8)
        self._stream()
        self._chk(self._lib.wct_motion_luma(self._ctx, c.data_ptr(), int(c.shape[1]), int(c.shape[2]), Ho, Wo, levels, out.data_ptr()))
        res, at = [], 0
        for h, w in shapes:
            res.append(out[at:at + h * w].view(h, w))
            at += h * w
        return res

    @torch.no_grad()
    def motion_estimate(self, content: torch.Tensor, prev_content: torch.Tensor, levels: int = _lib.MOTION_LEVELS, range: int = _lib.MOTION_RANGE,
                        penalty: int = _lib.MOTION_PENALTY, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The block-matched field between the top-left Ho x Wo of `content` and `prev_content` ([1,3,Ho,Wo]) (wct_motion_estimate):
        int16 [nby, nbx, 2] = (vy, vx) per 8 x 8 block, content(y, x) ~ prev_content(y + vy, x + vx)."""
        c, q = self._img(content), self._img(prev_content)
        Ho, Wo = int(q.shape[1]), int(q.shape[2])
        nby, nbx = (Ho + 7) // 8, (Wo + 7) // 8
        out = self._out_like(out, "motion_estimate", nby * nbx * 2, torch.int16)
        if out is None:
            out = torch.empty((nby, nbx, 2), device=c.device, dtype=torch.int16)
        p = _lib.WctMotionParams(int(levels), int(range), int(penalty))
        self._stream()
        self._chk(self._lib.wct_motion_estimate(self._ctx, c.data_ptr(), int(c.shape[1]), int(c.shape[2]), q.data_ptr(), Ho, Wo, byref(p), out.data_ptr()))
        return out.view(nby, nbx, 2)

    @torch.no_grad()
    def motion_blend(self, content: torch.Tensor, prev_content: torch.Tensor, stylised: torch.Tensor, prev_out: torch.Tensor,
                     mv: Optional[torch.Tensor], blend: float = _lib.CLIP_BLEND, sigma: float = _lib.CLIP_SIGMA, radius: int = _lib.CLIP_RADIUS,
                     cut_flag: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, u8: bool = False, round_mode: int = 0):
        """temporal_blend against prev_content and prev_out displaced by the field `mv` (int16 [nby, nbx, 2]; None: the zero
        field) (wct_motion_blend).  Returns what temporal_blend returns."""
        c, q, s, p = self._img(content), self._img(prev_content), self._img(stylised), self._img(prev_out)
        Hc, Wc, Ho, Wo = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        if tuple(q.shape) != (3, Ho, Wo) or tuple(p.shape) != (3, Ho, Wo):
            raise ValueError("motion_blend: prev_content %s and prev_out %s must have the stylised image's shape %s"
                             % (tuple(q.shape), tuple(p.shape), tuple(s.shape)))
        if cut_flag is not None and (cut_flag.dtype != torch.int32 or not cut_flag.is_cuda or cut_flag.numel() != 1):
            raise ValueError("motion_blend: cut_flag must be an int32 device tensor with one value")
        if mv is not None:
            mv = self._out_like(mv, "motion_blend: mv", ((Ho + 7) // 8) * ((Wo + 7) // 8) * 2, torch.int16)
        out = self._out_like(out, "motion_blend", 3 * Ho * Wo)
        if out is None:
            out = torch.empty((1, 3, Ho, Wo), device=s.device, dtype=torch.float32)
        hwc = torch.empty((Ho, Wo, 3), device=s.device, dtype=torch.uint8) if u8 else None
        self._stream()
        self._chk(self._lib.wct_motion_blend(self._ctx, c.data_ptr(), Hc, Wc, q.data_ptr(), s.data_ptr(), p.data_ptr(), Ho, Wo, float(blend),
                                             float(sigma), int(radius), cut_flag.data_ptr() if cut_flag is not None else None, out.data_ptr(),
                                             hwc.data_ptr() if u8 else None, int(round_mode), mv.data_ptr() if mv is not None else None))
        out = out.view(1, 3, Ho, Wo)
        return (out, hwc) if u8 else out

    @torch.no_grad()
    def moments_track(self, clip: "Clip", level: int, sum_c: torch.Tensor, sumsq_c: torch.Tensor, decide: bool = False):
        """The tracking step of one level IN PLACE on fp64 device sums (wct_moments_track), committed at once: r' = c on a cut (decided
        here when `decide`, else the clip's stored flag), else r + rate (c - r); returns (sum_c, sumsq_c), now holding r'."""
        C = clip.channels(level)
        for t, numel, what in ((sum_c, C, "sum_c"), (sumsq_c, C * C, "sumsq_c")):
            if t.dtype != torch.float64 or not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or t.numel() != numel:
                raise ValueError("moments_track: %s must be a contiguous fp64 tensor on cuda:%d with %d values" % (what, self.device, numel))
        self._stream()
        self._chk(self._lib.wct_moments_track(self._ctx, clip._handle(), int(level), int(bool(decide)), sum_c.data_ptr(), sumsq_c.data_ptr()))
        return sum_c, sumsq_c

    @torch.no_grad()
    def temporal_blend(self, content: torch.Tensor, prev_content: torch.Tensor, stylised: torch.Tensor, prev_out: torch.Tensor,
                       blend: float = _lib.CLIP_BLEND, sigma: float = _lib.CLIP_SIGMA, radius: int = _lib.CLIP_RADIUS,
                       cut_flag: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, u8: bool = False, round_mode: int = 0):
        """out = s + w (p - s), w = blend exp(-d / (2 sigma^2)), d = the mean squared difference of the content (its top-left
        Ho x Wo) and prev_content over a (2 radius + 1)^2 window (wct_temporal_blend); a non-zero `cut_flag` (an int32 device
        scalar) gives s.  Returns fp32 [1,3,Ho,Wo]; with u8=True (that, uint8 [Ho,Wo,3]), the bytes equal to to_u8(out, round_mode)."""
        c, q, s, p = self._img(content), self._img(prev_content), self._img(stylised), self._img(prev_out)
        Hc, Wc, Ho, Wo = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        if tuple(q.shape) != (3, Ho, Wo) or tuple(p.shape) != (3, Ho, Wo):
            raise ValueError("temporal_blend: prev_content %s and prev_out %s must have the stylised image's shape %s"
                             % (tuple(q.shape), tuple(p.shape), tuple(s.shape)))
        if cut_flag is not None and (cut_flag.dtype != torch.int32 or not cut_flag.is_cuda or cut_flag.numel() != 1):
            raise ValueError("temporal_blend: cut_flag must be an int32 device tensor with one value")
        out = self._out_like(out, "temporal_blend", 3 * Ho * Wo)
        if out is None:
            out = torch.empty((1, 3, Ho, Wo), device=s.device, dtype=torch.float32)
        hwc = torch.empty((Ho, Wo, 3), device=s.device, dtype=torch.uint8) if u8 else None
        self._stream()
        self._chk(self._lib.wct_temporal_blend(self._ctx, c.data_ptr(), Hc, Wc, q.data_ptr(), s.data_ptr(), p.data_ptr(), Ho, Wo, float(blend),
                                               float(sigma), int(radius), cut_flag.data_ptr() if cut_flag is not None else None, out.data_ptr(),
                                               hwc.data_ptr() if u8 else None, int(round_mode)))
        out = out.view(1, 3, Ho, Wo)
        return (out, hwc) if u8 else out

    # ------------------------------------------------------------------ spatial control (regions)
    def _labels(self, labels: torch.Tensor, h: int, w: int) -> torch.Tensor:
        if labels.dtype != torch.uint8 or tuple(labels.shape) != (h, w):
            raise ValueError("labels must be a uint8 tensor of shape (%d, %d), got %s %s" % (h, w, labels.dtype, tuple(labels.shape)))
        return labels.to(self.stats_device).contiguous()

    @torch.no_grad()
    def moments_labeled(self, feat_nhwc: torch.Tensor, labels: torch.Tensor, K: int):
        """Raw fp64 sums per label k < K of an NHWC feature [1,h,w,C] with an (h, w) uint8 label map: (n[K], sum[K,C], sumsq[K,C,C])."""
        f = self._nhwc(feat_nhwc)
        h, w, C = (int(v) for v in f.shape)
        lab = self._labels(labels, h, w)
        n = torch.empty(K, device=f.device, dtype=torch.float64)
        s = torch.empty(K, C, device=f.device, dtype=torch.float64)
        ss = torch.empty(K, C, C, device=f.device, dtype=torch.float64)
        self._stream()
        self._chk(self._lib.wct_moments_labeled(self._ctx, f.data_ptr(), C, h, w, lab.data_ptr(), int(K), n.data_ptr(), s.data_ptr(), ss.data_ptr()))
        return n, s, ss

    @torch.no_grad()
    def apply_labeled(self, feat: torch.Tensor, labels: torch.Tensor, M: torch.Tensor, b: torch.Tensor, layout: str = "nhwc") -> torch.Tensor:
        """out_p = M[lab(p)] feat_p + b[lab(p)] with M [K,C,C], b [K,C]; labels >= K (255) copied through.  feat is [1,h,w,C] (nhwc) or
        [1,C,h,w] (nchw); the result has the same shape."""
        f = feat[0] if feat.dim() == 4 else feat
        if f.dim() != 3:
            raise ValueError("expected a feature map [1,h,w,C] / [1,C,h,w], got %s" % (tuple(feat.shape),))
        f = self._dev_f32(f)
        nchw = layout == "nchw"
        if nchw:
            C, h, w = (int(v) for v in f.shape)
        else:
            h, w, C = (int(v) for v in f.shape)
        K = int(b.shape[0]) if b.dim() == 2 else int(b.numel()) // C
        lab = self._labels(labels, h, w)
        M, b = self._dev_f64(M, K * C * C, "M"), self._dev_f64(b, K * C, "b")
        out = torch.empty((1,) + tuple(f.shape), device=f.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_apply_labeled(self._ctx, f.data_ptr(), C, h, w, _lib.LAYOUT_NCHW if nchw else _lib.LAYOUT_NHWC,
                                              lab.data_ptr(), K, M.data_ptr(), b.data_ptr(), out.data_ptr()))
        return out

    @torch.no_grad()
    def stylize_regions(self, contentImg: torch.Tensor, styles, labels: torch.Tensor, alpha=None, num_run: int = 1,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The cascade with spatial control: `labels` (uint8 H x W, CUDA) gives each content pixel a style index k < len(styles) or 255
        (unstyled); `alpha` is one float or one per style.  Region k is whitened / coloured with its own statistics against style k."""
        c = self._img(contentImg)
        H, W = int(c.shape[1]), int(c.shape[2])
        ss = [self._img(s) for s in styles]
        K = len(ss)
        if alpha is None:
            alpha = self.alpha
        al = [float(alpha)] * K if isinstance(alpha, (int, float)) else [float(a) for a in alpha]
        if len(al) != K:
            raise ValueError("alpha: expected 1 or %d values, got %d" % (K, len(al)))
        if not labels.is_cuda:
            raise ValueError("labels must be a CUDA uint8 tensor")
        lab = self._labels(labels, H, W)
        out = self._out_image(out, H, W)
        ptrs = (c_void_p * max(K, 1))(*[s.data_ptr() for s in ss])
        hs = (c_int * max(K, 1))(*[int(s.shape[1]) for s in ss])
        ws = (c_int * max(K, 1))(*[int(s.shape[2]) for s in ss])
        av = (ctypes.c_float * max(K, 1))(*al)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_regions(self._ctx, c.data_ptr(), H, W, lab.data_ptr(), K, ptrs, hs, ws, av, int(num_run),
                                                out.data_ptr(), byref(ho), byref(wo)))
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    # ------------------------------------------------------------------ region-to-region transfer (include/wct_hip_guided.h)
    @torch.no_grad()
    def stylize_guided(self, contentImg: torch.Tensor, styles, labels: torch.Tensor, style_labels=None, region_style=None, alpha=None,
                       num_run: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The cascade with content regions AND style regions: `labels` (uint8 H x W, CUDA) as in stylize_regions; `style_labels` one
        uint8 map (or None = the whole image) per style, at the style's size: only the style pixels with label k enter region k's style
        statistics; `region_style[k]` names the style of region k (default: one region per style, region k against style k);
        `alpha` is one float or one per region."""
        c = self._img(contentImg)
        H, W = int(c.shape[1]), int(c.shape[2])
        ss = [self._img(s) for s in styles]
        S = len(ss)
        maps = [None] * S if style_labels is None else list(style_labels)
        if len(maps) != S:
            raise ValueError("style_labels: expected %d entries (one per style, None = unmapped), got %d" % (S, len(maps)))
        if not labels.is_cuda:
            raise ValueError("labels must be a CUDA uint8 tensor")
        lab = self._labels(labels, H, W)
        for i, m in enumerate(maps):
            if m is not None:
                if not m.is_cuda:
                    raise ValueError("style_labels[%d] must be a CUDA uint8 tensor" % i)
                maps[i] = self._labels(m, int(ss[i].shape[1]), int(ss[i].shape[2]))
        if region_style is None:
            K, rs = S, list(range(S))
        else:
            rs = [int(v) for v in region_style]
            K = len(rs)
        if alpha is None:
            alpha = self.alpha
        al = [float(alpha)] * K if isinstance(alpha, (int, float)) else [float(a) for a in alpha]
        if len(al) != K:
            raise ValueError("alpha: expected 1 or %d values, got %d" % (K, len(al)))
        out = self._out_image(out, H, W)
        ptrs = (c_void_p * max(S, 1))(*[s.data_ptr() for s in ss])
        mptrs = (c_void_p * max(S, 1))(*[(m.data_ptr() if m is not None else None) for m in maps])
        hs = (c_int * max(S, 1))(*[int(s.shape[1]) for s in ss])
        ws = (c_int * max(S, 1))(*[int(s.shape[2]) for s in ss])
        rv = (c_int * max(K, 1))(*rs)
        av = (ctypes.c_float * max(K, 1))(*al)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_guided(self._ctx, c.data_ptr(), H, W, lab.data_ptr(), K, S, ptrs, hs, ws, mptrs, rv, av, int(num_run),
                                               out.data_ptr(), byref(ho), byref(wo)))
        self._guided_keep = (ss, maps)      # the side stream reads them asynchronously
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    def _kmeans_args(self, feat_nhwc, shift, scale):
        f = self._nhwc(feat_nhwc)
        h, w, C = (int(v) for v in f.shape)
        return f, h, w, C, self._dev_f64(shift, C, "shift"), self._dev_f64(scale, C, "scale")

    @torch.no_grad()
    def kmeans_assign(self, feat_nhwc: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, centroids: torch.Tensor, want_labels: bool = True,
                      want_next: bool = True):
        """One Lloyd step on an NHWC feature [1,h,w,C] in the standardised space z = (x - shift) * scale against `centroids` [K,C] (fp64):
        (labels uint8 [h,w] or None, n [K], sum [K,C], cost [1], next [K,C] or None), all on the device, nothing read back."""
        f, h, w, C, sh, sc = self._kmeans_args(feat_nhwc, shift, scale)
        K = int(centroids.numel()) // C
        cen = self._dev_f64(centroids, K * C, "centroids")
        dev = f.device
        lab = torch.empty((h, w), device=dev, dtype=torch.uint8) if want_labels else None
        n = torch.empty(K, device=dev, dtype=torch.float64)
        s = torch.empty((K, C), device=dev, dtype=torch.float64)
        cost = torch.empty(1, device=dev, dtype=torch.float64)
        nxt = torch.empty((K, C), device=dev, dtype=torch.float64) if want_next else None
        self._stream()
        self._chk(self._lib.wct_kmeans_assign(self._ctx, f.data_ptr(), C, h, w, sh.data_ptr(), sc.data_ptr(), cen.data_ptr(), K,
                                              lab.data_ptr() if want_labels else None, n.data_ptr(), s.data_ptr(), cost.data_ptr(),
                                              nxt.data_ptr() if want_next else None))
        return lab, n, s, cost, nxt

    @torch.no_grad()
    def kmeans_seed(self, feat_nhwc: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, K: int):
        """The deterministic farthest-first start: (centroids [K,C] fp64, idx [K] int32 pixel indices)."""
        f, h, w, C, sh, sc = self._kmeans_args(feat_nhwc, shift, scale)
        cen = torch.empty((int(K), C), device=f.device, dtype=torch.float64)
        idx = torch.empty(int(K), device=f.device, dtype=torch.int32)
        self._stream()
        self._chk(self._lib.wct_kmeans_seed(self._ctx, f.data_ptr(), C, h, w, sh.data_ptr(), sc.data_ptr(), int(K), cen.data_ptr(), idx.data_ptr()))
        return cen, idx

    @torch.no_grad()
    def feature_regions(self, contentImg: torch.Tensor, styleImg: torch.Tensor, K: int, level: int = 4, iters: int = 10, want_centroids: bool = False):
        """Label maps from k-means on the level's features: K clusters of the STYLE's standardised features, every content feature pixel
        given the nearest one: (labels_c uint8 [H,W], labels_s uint8 [Hs,Ws][, centroids [K,C]]) for
        stylize_guided(content, [style], labels_c, [labels_s], region_style=[0] * K)."""
        c, s = self._img(contentImg), self._img(styleImg)
        H, W, Hs, Ws = int(c.shape[1]), int(c.shape[2]), int(s.shape[1]), int(s.shape[2])
        lc = torch.empty((H, W), device=c.device, dtype=torch.uint8)
        ls = torch.empty((Hs, Ws), device=c.device, dtype=torch.uint8)
        cen = torch.empty((int(K), self._feature_channels(int(level)) if 1 <= int(level) <= 5 else 1), device=c.device, dtype=torch.float64) if want_centroids else None
        self._stream()
        self._chk(self._lib.wct_feature_regions(self._ctx, int(level), c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, int(K), int(iters), lc.data_ptr(),
                                                ls.data_ptr(), cen.data_ptr() if want_centroids else None))
        return (lc, ls, cen) if want_centroids else (lc, ls)

    # ------------------------------------------------------------------ style interpolation and per-pixel style weights
    def _styles(self, styles):
        ss = [self._img(s) for s in styles]
        K = len(ss)
        ptrs = (c_void_p * max(K, 1))(*[s.data_ptr() for s in ss])
        hs = (c_int * max(K, 1))(*[int(s.shape[1]) for s in ss])
        ws = (c_int * max(K, 1))(*[int(s.shape[2]) for s in ss])
        return ss, ptrs, hs, ws

    @staticmethod
    def _lambda(weights, K: int):
        lam = [float(v) for v in weights]
        if len(lam) != K:
            raise ValueError("weights: expected %d values (one per style), got %d" % (K, len(lam)))
        return (ctypes.c_float * max(K, 1))(*lam)

    def _weight_maps(self, weights: torch.Tensor, K: int, h: int, w: int) -> torch.Tensor:
        if weights.dtype != torch.float32 or tuple(weights.shape) != (K, h, w):
            raise ValueError("weights must be a float32 tensor of shape (%d, %d, %d), got %s %s" % (K, h, w, weights.dtype, tuple(weights.shape)))
        if not weights.is_cuda:
            raise ValueError("weights must be a CUDA float32 tensor")
        return weights.to(self.stats_device).contiguous()

    @torch.no_grad()
    def moments_weighted(self, feat_nhwc: torch.Tensor, weights: torch.Tensor):
        """Raw fp64 weighted sums of an NHWC feature [1,h,w,C] with K weight maps [K,h,w] (fp32): (sum[K,C], sumsq[K,C,C]),
        sum[k] = sum_p w_k(p) x_p, sumsq[k] = sum_p w_k(p) x_p x_p^T."""
        f = self._nhwc(feat_nhwc)
        h, w, C = (int(v) for v in f.shape)
        K = int(weights.shape[0]) if weights.dim() == 3 else 0
        wt = self._weight_maps(weights, K, h, w)
        s = torch.empty(K, C, device=f.device, dtype=torch.float64)
        ss = torch.empty(K, C, C, device=f.device, dtype=torch.float64)
        self._stream()
        self._chk(self._lib.wct_moments_weighted(self._ctx, f.data_ptr(), C, h, w, wt.data_ptr(), K, s.data_ptr(), ss.data_ptr()))
        return s, ss

    @torch.no_grad()
    def apply_mixed(self, feat: torch.Tensor, weights: torch.Tensor, M: torch.Tensor, b: torch.Tensor, layout: str = "nhwc") -> torch.Tensor:
        """out_p = x_p + sum_k w_k(p) ((M[k] x_p + b[k]) - x_p) with weights [K,h,w] (fp32), M [K,C,C], b [K,C].  feat is [1,h,w,C] (nhwc)
        or [1,C,h,w] (nchw); the result has the same shape."""
        f = feat[0] if feat.dim() == 4 else feat
        if f.dim() != 3:
            raise ValueError("expected a feature map [1,h,w,C] / [1,C,h,w], got %s" % (tuple(feat.shape),))
        f = self._dev_f32(f)
        nchw = layout == "nchw"
        if nchw:
            C, h, w = (int(v) for v in f.shape)
        else:
            h, w, C = (int(v) for v in f.shape)
        K = int(b.shape[0]) if b.dim() == 2 else int(b.numel()) // C
        wt = self._weight_maps(weights, K, h, w)
        M, b = self._dev_f64(M, K * C * C, "M"), self._dev_f64(b, K * C, "b")
        out = torch.empty((1,) + tuple(f.shape), device=f.device, dtype=torch.float32)
        self._stream()
        self._chk(self._lib.wct_apply_mixed(self._ctx, f.data_ptr(), C, h, w, _lib.LAYOUT_NCHW if nchw else _lib.LAYOUT_NHWC,
                                            wt.data_ptr(), K, M.data_ptr(), b.data_ptr(), out.data_ptr()))
        return out

    @torch.no_grad()
    def stylize_interp(self, contentImg: torch.Tensor, styles, weights, alpha: Optional[float] = None, num_run: int = 1,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Style interpolation (-styleInterpWeights): csF = alpha sum_k l_k WCT(cF, style_k) + (1 - alpha) cF at every level, with
        l = weights / sum(weights) (one finite weight >= 0 per style, sum > 0).  Under set_transform("ot" | "adain") the target is the
        style whose square-root covariance is the blended slot sum_k l_k S_k (mean sum_k l_k mu_k), no longer the linear mix of the K results."""
        alpha = self.alpha if alpha is None else float(alpha)
        c = self._img(contentImg)
        H, W = int(c.shape[1]), int(c.shape[2])
        ss, ptrs, hs, ws = self._styles(styles)
        K = len(ss)
        lam = self._lambda(weights, K)
        out = self._out_image(out, H, W)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_interp(self._ctx, c.data_ptr(), H, W, K, ptrs, hs, ws, lam, alpha, int(num_run),
                                               out.data_ptr(), byref(ho), byref(wo)))
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    def style_blend(self, stats_per_style, weights, levels=(5, 4, 3, 2, 1)):
        """Blend cached style statistics into the context (as style_import): stats_per_style[k][L] is style k's style_export(L);
        the context then holds sum_k l_k stats_k for each level L in `levels` (l = weights / sum(weights)).  stylize_prepared follows."""
        K = len(stats_per_style)
        lam = self._lambda(weights, K)
        self._stream()
        for L in levels:
            n = c_size_t()
            self._chk(self._lib.wct_style_stats_count(self._ctx, int(L), byref(n)))
            parts = [st[L] for st in stats_per_style]
            for p in parts:
                if p.dtype != torch.float64 or not p.is_cuda or p.numel() != n.value:
                    raise ValueError("style_blend: level %d expects %d fp64 values on the GPU per style" % (L, n.value))
            buf = torch.stack([p.to(self.stats_device).reshape(-1) for p in parts]).contiguous()
            self._blend_keep = buf     # read by the blend launch on the context's stream
            self._chk(self._lib.wct_style_blend(self._ctx, int(L), K, buf.data_ptr(), lam))

    @torch.no_grad()
    def stylize_blend(self, contentImg: torch.Tensor, styles, weights_map: torch.Tensor, alpha=None, num_run: int = 1,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The cascade with per-pixel style weights: `weights_map` (float32 [K, H, W], CUDA) gives each content pixel a weight in [0, 1]
        per style, summing to <= 1 (the rest stays unstyled); `alpha` is one float or one per style."""
        c = self._img(contentImg)
        H, W = int(c.shape[1]), int(c.shape[2])
        ss, ptrs, hs, ws = self._styles(styles)
        K = len(ss)
        if alpha is None:
            alpha = self.alpha
        al = [float(alpha)] * K if isinstance(alpha, (int, float)) else [float(a) for a in alpha]
        if len(al) != K:
            raise ValueError("alpha: expected 1 or %d values, got %d" % (K, len(al)))
        wt = self._weight_maps(weights_map, K, H, W)
        out = self._out_image(out, H, W)
        av = (ctypes.c_float * max(K, 1))(*al)
        ho, wo = c_int(), c_int()
        self._stream()
        self._chk(self._lib.wct_stylize_blend(self._ctx, c.data_ptr(), H, W, wt.data_ptr(), K, ptrs, hs, ws, av, int(num_run),
                                              out.data_ptr(), byref(ho), byref(wo)))
        return out.view(-1)[: 3 * ho.value * wo.value].view(1, 3, ho.value, wo.value)

    def set_conv_mode(self, mode: str):
        """'f16x3' (default: split-f16 MFMA, fp32-class accuracy) or 'fp32' (exact fp32 MFMA)."""
        self._chk(self._lib.wct_set_conv_mode(self._ctx, {"fp32": 0, "f16x3": 1}[mode]))

    def debug_set(self, key: str, value) -> None:
        """Experiment switches of the context ("fuse", "sp", "l1fuse", "u8fuse", "upconv"): kernel formulations of the same operators."""
        self._chk(self._lib.wct_debug_set(self._ctx, key.encode(), float(value)))

    def debug_get(self, key: str) -> float:
        """Health counters of the context: "nscoop_solves", "nscoop_aborts", "nscoop_off" (include/wct_hip.h wct_debug_get)."""
        v = ctypes.c_double()
        self._chk(self._lib.wct_debug_get(self._ctx, key.encode(), byref(v)))
        return float(v.value)

    def set_overlap(self, on: bool):
        self._chk(self._lib.wct_set_overlap(self._ctx, int(on)))

    def reserve(self, H, W, Hs, Ws):
        self._chk(self._lib.wct_reserve(self._ctx, H, W, Hs, Ws))

    def sync(self):
        self._chk(self._lib.wct_sync(self._ctx))

    # ------------------------------------------------------------------ profiling (bench.py roofline leg)
    def profile(self, on: bool):
        self._chk(self._lib.wct_profile_enable(self._ctx, int(on)))

    def profile_reset(self):
        self._chk(self._lib.wct_profile_reset(self._ctx))

    def profile_read(self):
        n = c_int()
        buf = (_lib.WctProfEntry * 64)()
        self._chk(self._lib.wct_profile_read(self._ctx, buf, 64, byref(n)))
        return [{"name": buf[i].name.decode(), "ms": buf[i].ms, "flops": buf[i].flops, "bytes": buf[i].bytes,
                 "launches": buf[i].launches} for i in range(min(n.value, 64))]


class Clip:
    """One frame sequence of a WCT engine (include/wct_hip_video.h wct_clip; made by WCT.clip).  The state -- tracked content sums,
    the previous frame's content and output -- lives in the clip, not in the engine: other calls of the engine between frames
    change nothing here, and the clip changes nothing of theirs.  close() (or garbage collection) frees it; close it before the
    engine goes."""

    def __init__(self, owner: WCT, H: int, W: int, rate: float, cut: float, blend: float, sigma: float, radius: int):
        self.owner, self.H, self.W = owner, H, W
        self.params = _lib.WctClipParams(rate, cut, blend, sigma, radius)
        self._clip = c_void_p()
        owner._chk(owner._lib.wct_clip_create(owner._ctx, H, W, byref(self.params), byref(self._clip)))
        self.Ho, self.Wo = H // 16 * 16, W // 16 * 16
        self.motion = None                # attach_motion: the parameters of the attached motion compensation

    def _handle(self) -> c_void_p:
        if not self._clip.value:
            raise RuntimeError("the clip is closed")
        return self._clip

    def channels(self, level: int) -> int:
        return self.owner._feature_channels(level)

    @torch.no_grad()
    def stylize(self, content: torch.Tensor, alpha: Optional[float] = None, out: Optional[torch.Tensor] = None, u8: bool = False,
                round_mode: int = 0):
        """The next frame (wct_stylize_clip) against the engine's prepared style (style_prepare / style_import): fp32 [1,3,Ho,Wo]; with
        u8=True (that, uint8 [Ho,Wo,3]).  Asynchronous, allocation-free after the first frame, and capturable into one HIP graph
        when `content` and `out` are the caller's fixed buffers."""
        o = self.owner
        alpha = o.alpha if alpha is None else float(alpha)
        c = o._img(content)
        H, W = int(c.shape[1]), int(c.shape[2])
        out = o._out_like(out, "Clip.stylize", 3 * self.Ho * self.Wo)
        if out is None:
            out = torch.empty((1, 3, self.Ho, self.Wo), device=c.device, dtype=torch.float32)
        hwc = torch.empty((self.Ho, self.Wo, 3), device=c.device, dtype=torch.uint8) if u8 else None
        ho, wo = c_int(), c_int()
        o._stream()
        o._chk(o._lib.wct_stylize_clip(o._ctx, self._handle(), c.data_ptr(), H, W, alpha, out.data_ptr(), hwc.data_ptr() if u8 else None,
                                       int(round_mode), byref(ho), byref(wo)))
        out = out.view(1, 3, self.Ho, self.Wo)
        return (out, hwc) if u8 else out

    def attach_motion(self, levels: int = _lib.MOTION_LEVELS, range: int = _lib.MOTION_RANGE, penalty: int = _lib.MOTION_PENALTY) -> None:
        """Motion compensation for the frames from now on (wct_motion_attach): allocates the clip's motion block once; the next frame
        is a first frame."""
        o = self.owner
        p = _lib.WctMotionParams(int(levels), int(range), int(penalty))
        o._stream()
        o._chk(o._lib.wct_motion_attach(o._ctx, self._handle(), byref(p)))
        self.motion = {"levels": int(levels), "range": int(range), "penalty": int(penalty)}

    def detach_motion(self) -> None:
        """Video mode without motion compensation again (wct_motion_attach with NULL); the next frame is a first frame."""
        o = self.owner
        o._stream()
        o._chk(o._lib.wct_motion_attach(o._ctx, self._handle(), None))
        self.motion = None

    @torch.no_grad()
    def motion_field(self) -> torch.Tensor:
        """The last frame's field, int16 [nby, nbx, 2] = (vy, vx) per 8 x 8 block, as a device tensor in stream order
        (wct_motion_export); all zero after a cut."""
        o = self.owner
        nby, nbx = (self.Ho + 7) // 8, (self.Wo + 7) // 8
        mv = torch.empty((nby, nbx, 2), device=o.stats_device, dtype=torch.int16)
        o._stream()
        o._chk(o._lib.wct_motion_export(o._ctx, self._handle(), mv.data_ptr()))
        return mv

    def reset(self) -> None:
        """The next frame is a first frame: tracked statistics and the previous output are not used (asynchronous)."""
        o = self.owner
        o._stream()
        o._chk(o._lib.wct_clip_reset(o._ctx, self._handle()))

    @torch.no_grad()
    def export(self, level: int):
        """(sum [C], sumsq [C,C], flags [2] = (frames, cut)) of `level` as device tensors, in stream order (wct_clip_export)."""
        o = self.owner
        C = self.channels(level)
        s = torch.empty(C, device=o.stats_device, dtype=torch.float64)
        ss = torch.empty(C, C, device=o.stats_device, dtype=torch.float64)
        flags = torch.empty(2, device=o.stats_device, dtype=torch.int32)
        o._stream()
        o._chk(o._lib.wct_clip_export(o._ctx, self._handle(), int(level), s.data_ptr(), ss.data_ptr(), flags.data_ptr()))
        return s, ss, flags

    def close(self) -> None:
        if getattr(self, "_clip", None) is not None and self._clip.value:
            o = self.owner
            alive = getattr(o, "_ctx", None) is not None and o._ctx.value
            o._lib.wct_clip_destroy(o._ctx if alive else None, self._clip)   # the allocation is the clip's own: freed either way
            self._clip = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@torch.no_grad()
def styleTransfer(encoder, decoder, contentImg, styleImg, csF=None, alpha=None):
    """WCT.py:98-106.  With an encoder/decoder pair of one wct_hip.WCT level this runs the fused HIP
    level (features never leave HBM, M/b folded into the decoder); otherwise it falls back to the
    reference's literal op sequence on the given callables (still GPU: they are wct_hip modules)."""
    if isinstance(encoder, _Module) and isinstance(decoder, _Module) and encoder.owner is decoder.owner \
            and encoder.level == decoder.level and encoder.kind == "enc" and decoder.kind == "dec":
        return encoder.owner.style_transfer_level(encoder.level, contentImg, styleImg, alpha)
    owner = getattr(encoder, "owner", None) or getattr(decoder, "owner", None)
    if owner is None:
        raise TypeError("styleTransfer needs wct_hip modules")
    sF = encoder(styleImg)
    cF = encoder(contentImg)
    csF = owner.transform(cF.squeeze(0), sF.squeeze(0), csF, alpha)
    return decoder(csF)
