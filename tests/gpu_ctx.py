"""One wct_ctx driven through the C ABI with numpy in and numpy out: the harness of the GPU tests that load modules of their own
(tests/test_widths_gpu.py, tests/test_range_gpu.py, tests/test_sweep_gpu.py, tests/test_conv_sweep_gpu.py).  The WCT class hard-codes model_zoo's widths; `wct_load_module` takes any layer list."""
import ctypes
from ctypes import byref, c_int, c_void_p

import numpy as np

from tests import width_models as wm
from wct_hip import lib as _lib


class Ctx:
    """One wct_ctx with custom-width modules; numpy in, numpy out."""

    def __init__(self, torch):
        self.t = torch
        self.L = _lib.load()
        self.ctx = c_void_p()
        _lib.check(self.L, None, self.L.wct_create(0, byref(self.ctx)))
        self.widths = None

    def close(self):
        if self.ctx.value:
            self.L.wct_destroy(self.ctx)
            self.ctx = c_void_p()

    def chk(self, rc):
        _lib.check(self.L, self.ctx, rc)

    def rc_msg(self, rc):
        return rc, self.L.wct_last_error(self.ctx).decode() if rc else ""

    def dev(self, a, dtype=None):
        return self.t.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()

    def sync(self):
        self.t.cuda.synchronize()
        self.chk(self.L.wct_sync(self.ctx))

    def sync_rc(self):
        """sync() that returns wct_sync's code (WCT_OK or WCT_ERR_RANGE: the range report, made once) instead of raising; any other
        error still raises."""
        self.t.cuda.synchronize()
        rc = self.L.wct_sync(self.ctx)
        if rc not in (_lib.WCT_OK, _lib.WCT_ERR_RANGE):
            self.chk(rc)
        return rc

    def poll(self):
        n = ctypes.c_ulonglong()
        self.chk(self.L.wct_range_poll(self.ctx, byref(n)))
        return n.value

    def load_layers(self, kind, level, layers, w, key):
        arr = (_lib.WctLayer * len(layers))()
        hold = []
        for i, l in enumerate(layers):
            wt = np.ascontiguousarray(w["%s.%s.weight" % (key, l.name)], np.float32)
            bs = np.ascontiguousarray(w["%s.%s.bias" % (key, l.name)], np.float32)
            hold += [wt, bs]
            arr[i] = _lib.WctLayer(l.cin, l.cout, int(l.pool_after), int(l.up_after), wt.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                   bs.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        c0 = [np.ascontiguousarray(w[key + ".conv0.weight"], np.float32).reshape(9), np.ascontiguousarray(w[key + ".conv0.bias"], np.float32)] \
            if kind == "enc" else [None, None]
        fp = [a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) if a is not None else None for a in c0]
        return self.L.wct_load_module(self.ctx, _lib.KIND_ENC if kind == "enc" else _lib.KIND_DEC, level, len(layers), arr, fp[0], fp[1])

    def load(self, widths, w, levels=(1, 2, 3, 4, 5)):
        for level in levels:
            self.chk(self.load_layers("enc", level, wm.encoder_layers(widths, level), w, "e%d" % level))
            self.chk(self.load_layers("dec", level, wm.decoder_layers(widths, level), w, "d%d" % level))
        self.widths = widths

    def set(self, key, value):
        self.chk(self.L.wct_debug_set(self.ctx, key.encode(), float(value)))

    def conv_mode(self, m):
        self.chk(self.L.wct_set_conv_mode(self.ctx, m))

    def saturation(self, reset=False):
        n = ctypes.c_ulonglong()
        self.chk(self.L.wct_saturation_count(self.ctx, int(reset), byref(n)))
        return n.value

    def profile_start(self):
        self.chk(self.L.wct_profile_enable(self.ctx, 1))
        self.chk(self.L.wct_profile_reset(self.ctx))

    def profile_counts(self):
        """{profile name: launches} since profile_start(); turns profiling off"""
        n = c_int()
        self.chk(self.L.wct_profile_read(self.ctx, None, 0, byref(n)))
        e = (_lib.WctProfEntry * max(n.value, 1))()
        self.chk(self.L.wct_profile_read(self.ctx, e, n.value, byref(n)))
        self.chk(self.L.wct_profile_enable(self.ctx, 0))
        return {e[i].name.decode(): int(e[i].launches) for i in range(n.value)}

    def profile_names(self):
        return set(self.profile_counts())

    # ---- entry points
    def encode(self, level, img):
        H, W = img.shape[1:]
        C, h, w = c_int(), c_int(), c_int()
        self.chk(self.L.wct_feature_shape(self.ctx, level, H, W, byref(C), byref(h), byref(w)))
        x = self.dev(img)
        out = self.t.empty((h.value, w.value, C.value), device="cuda", dtype=self.t.float32)
        self.sync()
        self.chk(self.L.wct_encode(self.ctx, level, x.data_ptr(), H, W, out.data_ptr(), _lib.LAYOUT_NHWC))
        self.sync()
        return out.cpu().numpy().transpose(2, 0, 1)

    def decode(self, level, feat):
        C, h, w = feat.shape
        f = self.dev(feat.transpose(1, 2, 0), np.float32)
        out = self.t.empty((3, h << (level - 1), w << (level - 1)), device="cuda", dtype=self.t.float32)
        self.sync()
        self.chk(self.L.wct_decode(self.ctx, level, f.data_ptr(), h, w, _lib.LAYOUT_NHWC, out.data_ptr()))
        self.sync()
        return out.cpu().numpy()

    def content_encode(self, level, img, x0=0, x1=-1):
        H, W = img.shape[1:]
        C = wm.feature_channels(self.widths, level)
        self._keep = x = self.dev(img)
        s = self.t.empty(C, device="cuda", dtype=self.t.float64)
        ss = self.t.empty(C, C, device="cuda", dtype=self.t.float64)
        h, w = c_int(), c_int()
        self.sync()
        self.chk(self.L.wct_content_encode(self.ctx, level, x.data_ptr(), H, W, x0, x1, s.data_ptr(), ss.data_ptr(), byref(h), byref(w)))
        self.sync()
        return s.cpu().numpy(), ss.cpu().numpy()

    def content_decode(self, level, M, b, Ho, Wo):
        Md, bd = self.dev(M, np.float64), self.dev(b, np.float64)
        out = self.t.empty((3, Ho, Wo), device="cuda", dtype=self.t.float32)
        ho, wo = c_int(), c_int()
        self.sync()
        self.chk(self.L.wct_content_decode(self.ctx, level, Md.data_ptr(), bd.data_ptr(), out.data_ptr(), byref(ho), byref(wo)))
        self.sync()
        assert (ho.value, wo.value) == (Ho, Wo)
        return out.cpu().numpy()

    def moments(self, feat_hwc, x0, x1):
        h, w, C = feat_hwc.shape
        f = self.dev(feat_hwc, np.float32)
        s = self.t.empty(C, device="cuda", dtype=self.t.float64)
        ss = self.t.empty(C, C, device="cuda", dtype=self.t.float64)
        self.sync()
        self.chk(self.L.wct_moments(self.ctx, f.data_ptr(), C, h, w, x0, x1, s.data_ptr(), ss.data_ptr()))
        self.sync()
        return s.cpu().numpy(), ss.cpu().numpy()

    def solve(self, C, n_c, s_c, ss_c, n_s, s_s, ss_s, alpha):
        a = [self.dev(v, np.float64) for v in (s_c, ss_c, s_s, ss_s)]
        M = self.t.empty(C, C, device="cuda", dtype=self.t.float64)
        b = self.t.empty(C, device="cuda", dtype=self.t.float64)
        self.sync()
        self.chk(self.L.wct_solve(self.ctx, C, float(n_c), a[0].data_ptr(), a[1].data_ptr(), float(n_s), a[2].data_ptr(), a[3].data_ptr(),
                                  float(alpha), M.data_ptr(), b.data_ptr(), None))
        self.sync()
        return M.cpu().numpy(), b.cpu().numpy()

    def style_transfer_level(self, level, content, style, alpha):
        H, W = content.shape[1:]
        Hs, Ws = style.shape[1:]
        c, s = self.dev(content, np.float32), self.dev(style, np.float32)
        _, h, w = self._shape(level, H, W)
        out = self.t.empty((3, h << (level - 1), w << (level - 1)), device="cuda", dtype=self.t.float32)
        ho, wo = c_int(), c_int()
        self.sync()
        self.chk(self.L.wct_style_transfer_level(self.ctx, level, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, float(alpha), out.data_ptr(),
                                                 byref(ho), byref(wo)))
        self.sync()
        return out.cpu().numpy()

    def stylize(self, content, style, alpha, prepared=False):
        H, W = content.shape[1:]
        Hs, Ws = style.shape[1:]
        c, s = self.dev(content, np.float32), self.dev(style, np.float32)
        out = self.t.empty((3, H, W), device="cuda", dtype=self.t.float32)
        ho, wo = c_int(), c_int()
        self.sync()
        if prepared:
            self.chk(self.L.wct_style_prepare(self.ctx, s.data_ptr(), Hs, Ws))
            self.chk(self.L.wct_stylize_prepared(self.ctx, c.data_ptr(), H, W, float(alpha), 1, out.data_ptr(), byref(ho), byref(wo)))
        else:
            self.chk(self.L.wct_stylize(self.ctx, c.data_ptr(), H, W, s.data_ptr(), Hs, Ws, float(alpha), 1, out.data_ptr(), byref(ho), byref(wo)))
        self.sync()
        return out.view(-1)[: 3 * ho.value * wo.value].view(3, ho.value, wo.value).cpu().numpy()

    def _shape(self, level, H, W):
        C, h, w = c_int(), c_int(), c_int()
        self.chk(self.L.wct_feature_shape(self.ctx, level, H, W, byref(C), byref(h), byref(w)))
        return C.value, h.value, w.value

    # ---- the un-fused feature-space entries (tests/test_sweep_gpu.py); features are h x w x C (NHWC) unless nchw is set
    def _layout(self, feat, nchw):
        """-> (device tensor, C, h, w, layout id); nchw: feat is C x h x w"""
        if nchw:
            C, h, w = feat.shape
        else:
            h, w, C = feat.shape
        return self.dev(feat, np.float32), C, h, w, _lib.LAYOUT_NCHW if nchw else _lib.LAYOUT_NHWC

    def apply(self, feat, M, b, nchw=False):
        f, C, h, w, layout = self._layout(feat, nchw)
        Md, bd = self.dev(M, np.float64), self.dev(b, np.float64)
        out = self.t.empty_like(f)
        self.sync()
        self.chk(self.L.wct_apply(self.ctx, f.data_ptr(), C, h, w, layout, Md.data_ptr(), bd.data_ptr(), out.data_ptr()))
        self.sync()
        return out.cpu().numpy()

    def moments_labeled(self, feat_hwc, lab, K):
        """-> n [K], sum [K, C], sumsq [K, C, C]"""
        h, w, C = feat_hwc.shape
        f, l = self.dev(feat_hwc, np.float32), self.dev(lab, np.uint8)
        n = self.t.empty(K, device="cuda", dtype=self.t.float64)
        s = self.t.empty((K, C), device="cuda", dtype=self.t.float64)
        ss = self.t.empty((K, C, C), device="cuda", dtype=self.t.float64)
        self.sync()
        self.chk(self.L.wct_moments_labeled(self.ctx, f.data_ptr(), C, h, w, l.data_ptr(), K, n.data_ptr(), s.data_ptr(), ss.data_ptr()))
        self.sync()
        return n.cpu().numpy(), s.cpu().numpy(), ss.cpu().numpy()

    def moments_weighted(self, feat_hwc, wts):
        """wts [K, h, w] fp32 -> sum [K, C], sumsq [K, C, C]"""
        h, w, C = feat_hwc.shape
        K = wts.shape[0]
        f, wd = self.dev(feat_hwc, np.float32), self.dev(wts, np.float32)
        s = self.t.empty((K, C), device="cuda", dtype=self.t.float64)
        ss = self.t.empty((K, C, C), device="cuda", dtype=self.t.float64)
        self.sync()
        self.chk(self.L.wct_moments_weighted(self.ctx, f.data_ptr(), C, h, w, wd.data_ptr(), K, s.data_ptr(), ss.data_ptr()))
        self.sync()
        return s.cpu().numpy(), ss.cpu().numpy()

    def apply_labeled(self, feat, lab, M, b, nchw=False):
        """M [K, C, C], b [K, C]"""
        f, C, h, w, layout = self._layout(feat, nchw)
        l, Md, bd = self.dev(lab, np.uint8), self.dev(M, np.float64), self.dev(b, np.float64)
        out = self.t.empty_like(f)
        self.sync()
        self.chk(self.L.wct_apply_labeled(self.ctx, f.data_ptr(), C, h, w, layout, l.data_ptr(), M.shape[0], Md.data_ptr(), bd.data_ptr(), out.data_ptr()))
        self.sync()
        return out.cpu().numpy()

    def apply_mixed(self, feat, wts, M, b, nchw=False):
        f, C, h, w, layout = self._layout(feat, nchw)
        wd, Md, bd = self.dev(wts, np.float32), self.dev(M, np.float64), self.dev(b, np.float64)
        out = self.t.empty_like(f)
        self.sync()
        self.chk(self.L.wct_apply_mixed(self.ctx, f.data_ptr(), C, h, w, layout, wd.data_ptr(), M.shape[0], Md.data_ptr(), bd.data_ptr(), out.data_ptr()))
        self.sync()
        return out.cpu().numpy()

    def solve_info(self, C, n_c, s_c, ss_c, n_s, s_s, ss_s, alpha):
        """solve() that also returns wct_solve's info: how (content, style) were solved"""
        a = [self.dev(v, np.float64) for v in (s_c, ss_c, s_s, ss_s)]
        M = self.t.empty(C, C, device="cuda", dtype=self.t.float64)
        b = self.t.empty(C, device="cuda", dtype=self.t.float64)
        info = (c_int * 2)(-1, -1)
        self.sync()
        self.chk(self.L.wct_solve(self.ctx, C, float(n_c), a[0].data_ptr(), a[1].data_ptr(), float(n_s), a[2].data_ptr(), a[3].data_ptr(),
                                  float(alpha), M.data_ptr(), b.data_ptr(), info))
        self.sync()
        return M.cpu().numpy(), b.cpu().numpy(), (info[0], info[1])

    def transform_solve(self, mode, C, n_c, s_c, ss_c, style_stats, alpha):
        """mode: "wct" | "ot" | "adain"; style_stats in the wct_style_export layout -> M, b, info"""
        a = [self.dev(v, np.float64) for v in (s_c, ss_c, style_stats)]
        M = self.t.empty(C, C, device="cuda", dtype=self.t.float64)
        b = self.t.empty(C, device="cuda", dtype=self.t.float64)
        info = (c_int * 2)(-1, -1)
        self.sync()
        self.chk(self.L.wct_transform_solve(self.ctx, _lib.TRANSFORMS[mode], C, float(n_c), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), float(alpha),
                                            M.data_ptr(), b.data_ptr(), info))
        self.sync()
        return M.cpu().numpy(), b.cpu().numpy(), (info[0], info[1])

    def decode_affine(self, level, feat_chw, M, b):
        C, h, w = feat_chw.shape
        f = self.dev(feat_chw.transpose(1, 2, 0), np.float32)
        Md, bd = self.dev(M, np.float64), self.dev(b, np.float64)
        out = self.t.empty((3, h << (level - 1), w << (level - 1)), device="cuda", dtype=self.t.float32)
        self.sync()
        self.chk(self.L.wct_decode_affine(self.ctx, level, f.data_ptr(), h, w, Md.data_ptr(), bd.data_ptr(), out.data_ptr()))
        self.sync()
        return out.cpu().numpy()
