"""Command line of the stylisation path: the flags, pairing, naming and log lines of PytorchWCT/WCT.py, on libwct_hip.

    python -m wct_hip.cli --mode 16x --contentPath content --stylePath style --outf stylized_results [--alpha 0.6] ...

What the reference script does around the hot path and where it lives here:
  WCT.py:15-35      argparse flags                     -> build_parser()   (same names, defaults and choices)
  WCT.py:37-75      checkpoint paths per --mode        -> checkpoint_args()
  data_loader.py:22-36   content x style pairs filtered by --picked_*_mark, listdir order   -> list_pairs()
  data_loader.py:50-59   PIL decode (.convert('RGB')), optional Resize, ToTensor            -> load_rgb_u8() + wct_resize_u8_to_planar / wct_u8_to_planar (GPU)
  data_loader.py:61-76   --synthesis: textures of --texturePath, resized to --style_size, noise as content  -> texture_jobs() + synthesis_shape() +
                         wct_resize_u8_filter (bicubic, GPU) + wct_synthesize (noise made on the GPU)
  WCT.py:120-125    the 5-level cascade, --num_run times -> wct_stylize (one C call)
  WCT.py:127-128    output name and save_image          -> out_name() + wct_planar_to_u8 (GPU) + PIL save
A frame crosses PCIe as uint8 (3 B/px each way).  The reference's loop is strictly serial -- decode, .cuda(), cascade, save_image
(WCT.py:112-131: its timer covers cascade + save) -- which leaves the GPU idle for ~90 % of a folder run once the cascade takes 10 ms:
`--pipeline N` (default 3; 0 = the serial loop) keeps N pairs in flight: a decode-ahead pool (PIL decode + copy into pinned memory, GIL
released), asynchronous H2D / D2H around the GPU work of the SAME single engine in the SAME order, and a writer pool for Image.save.
Output files are byte-identical to the serial loop's (tests/test_cli.py).  --numpy selects the reference's whiten_and_color_np semantics (+ I on the
content covariance).  --synthesis does what the reference's branch intends (it cannot run there: data_loader.py:74 calls
torch.rand_like on a PIL image): every image of --texturePath, resized so that its long side is --style_size (Pillow's default
filter at the reference's pin, bicubic), is the style of a cascade whose content is uniform noise -- seeded (--seed, the texture's
index in the listing as the stream id: Philox4x32-10, include/wct_hip.h) and made on the GPU at the texture's size or
--synthesis_size WxH; the result is saved as <log_mark>_mode=<m>_alpha=<a>_<texture stem>.jpg.  At the texture's size the result
is the cascade's, as in the reference: every edge a multiple of 16 (floor pooling, four times).  --synthesis_size is the size of the
FILE: the noise is made at the next multiples of 16 and the result cropped (top left) to WxH.  Only the decoded texture goes to the
GPU and only the uint8 result comes back.
--preserve_color match | luma (not in the reference; Gatys et al. 2017, section 5) keeps the content's colours: `match` maps the style's
colours onto the content's colour distribution before the cascade (per pair: wct_stylize_color, no style-statistics cache), `luma`
keeps the content's chroma and takes the stylised luminance (wct_luma_merge fused with the uint8 conversion; also behind --maskPath
and --interp_styles / --weightPath).  The files carry _color=<mode> in their names.
--smooth_radius R (not in the reference; the smoothing step of Li et al. 2018 as He et al.'s guided image filter) re-imposes the content's
edge structure on the result: wct_guided_filter with the content tensor the cascade was given as colour guide, windows of radius R,
regulariser --smooth_eps; it runs behind the cascade in every content-driven mode (before the luminance merge of --preserve_color luma),
with the uint8 conversion fused into whichever kernel comes last.  The files carry _smooth=<R> in their names, after _color=<mode>.
--swap_level L (not in the reference; Chen & Schmidt 2016, Avatar-Net's style decorator) runs level L (2..5) of the cascade as a patch swap:
every 3x3 patch of the content feature is replaced by its best-matching style feature patch, matched in the whitened domains of both
features (--swap_match whitened, the default) or on the features themselves (raw); the other levels keep --transform.  One pair at a time
(wct_stylize_swap, the serial loop: the swapped level needs the style's feature map, not its statistics); --preserve_color luma and
--smooth_radius follow as usual.  The files carry _swap=<L> in their names, after the transform mark.  --swap_match attention |
attention_whitened replaces the hard match by attention-weighted style statistics (include/wct_hip_attn.h: every content position takes
the style mean and deviation under a softmax of feature similarity, temperature --swap_temp T in 0..32, default 8; wct_stylize_attn, the
same loop); those files carry _swap=<L>_<match>=<T>.
--level_scale d5,d4,d3,d2,d1 (not in the reference; Gatys et al. 2017, section 6: scale control) runs level L on the content reduced by the
divisor dL and, where the working size grows, brings the running image up and puts the content's fine detail back (--scale_detail, a look);
--coarse_style gives the reduced levels a style of their own (scale mixing).  One pair at a time (wct_stylize_scaled, the serial loop);
--transform, --preserve_color and --smooth_radius go with it through the public calls around it.  The files carry _scale=<d5-d4-d3-d2-d1>.
--styleMaskPath DIR (with --maskPath; not in the reference; Gatys et al. 2017, section 4) gives the styles label maps of their own: only the
style pixels with label k enter region k's style statistics (wct_stylize_guided).  --auto_regions K makes both label maps itself, by k-means
on the style's features of --auto_level (wct_feature_regions), for ordinary content x style pairs; the files carry _auto=<K>.
--video (not in the reference) treats the picked content files, sorted by name, as the frames of one sequence: per style one clip
(wct_stylize_clip) tracks the content statistics over the frames (--temporal_rate, reset at a scene cut: --scene_cut) and blends every
output with the previous one where the content did not move (--temporal_blend, --temporal_sigma, --temporal_radius); the defaults are
looks, not measurements.  The style is prepared once, the frames run one at a time; --transform and --alpha go with it, the other modes
and --mode original do not.  One image per frame under the usual name.  --motion (with --video) estimates a block-matched motion field
between consecutive frames (--motion_levels, --motion_range, --motion_penalty) and blends against the previous frame displaced by it
(wct_motion_attach): panning and moving regions keep their strokes as the still ones do.
--diversity D (not in the reference; Wang et al., "Diversified Arbitrary Style Transfer via Deep Feature Perturbation", CVPR 2020) gives
several takes on one pair: the style's square-root covariance of --diversity_levels (default 5) is post-multiplied by a seeded rotation of
strength D in (0, 8] before the colouring step (wct_style_diversify: the same target statistics through a different map); --variations N
writes N images per pair, variation k from stream id k of --seed.  The style is prepared once per pair, one image at a time (the serial
loop); --alpha, --num_run, --preserve_color luma, --smooth_radius and --video (one rotation for the whole clip) go with it, --transform
ot | adain and the other modes do not.  The files carry _div=<D> after the transform mark and, with N > 1, _v<k> before the pair name.
--proxy_scale D (not in the reference; Chen et al., "Bilateral Guided Upsampling", SIGGRAPH Asia 2016) stylises the content reduced by the
divisor D in 1..16 and applies the result at full size: from the reduced pair a bilateral grid of local affine colour maps is fitted (one
vertex per --proxy_cell reduced pixels, --proxy_bins luminance vertices, regulariser --proxy_eps, --proxy_smooth blur passes; the defaults
are looks) and sliced by the full content (wct_stylize_proxy; include/wct_hip_bgrid.h).  The saved image has the content's exact size and
its edges; colour and tone are transferred, strokes are not.  One pair at a time (the serial loop); --alpha, --num_run, --transform,
--content_size, --style_size and --round go with it, the other modes, --diversity, --preserve_color and --smooth_radius do not.  The files
carry _proxy=<D> after the transform mark.
--device_jpeg (not in the reference; off by default) encodes every .jpg / .jpeg output on the GPU (wct_jpeg_encode;
include/wct_hip_jpeg.h) and writes the bytes: the file Pillow would write, byte for byte, without the host encode, and in the pipelined
loop with the compressed file instead of the image copied to the host.  Other extensions are saved by Pillow as before.
--jpeg_quality Q (1 .. 100, default 75 = Pillow's default) applies to .jpg / .jpeg outputs on either encoder.
--device_decode (not in the reference; off by default) decodes every .jpg / .jpeg input on the GPU (wct_jdec_decode;
include/wct_hip_jdec.h): the pixels Pillow would give, value for value, with the file's entropy-coded segment instead of the image
copied to the device.  A file the device decoder does not take (progressive, CMYK, ...) or does not finish (status UNSYNC / CORRUPT) is
decoded by Pillow as before, logged once per file; nothing is ever computed from bad pixels.  Masks, weight maps and PNGs are untouched.
Decoding/encoding files needs Pillow on the host (the reference's own dependency); the GPU library is mandatory: there
is no CPU fallback.
"""
from __future__ import annotations

import argparse
import collections
import math
import os
import sys
import threading
import time
from typing import List, Optional, Tuple

IMG_EXT = (".png", ".jpg", ".jpeg")   # data_loader.py:15


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="WCT on MI355X (libwct_hip)")
    p.add_argument("--UHD_contentPath", type=str, default="content/UHD_content")
    p.add_argument("--UHD_stylePath", type=str, default="style/UHD_style")
    p.add_argument("--contentPath", type=str, default="content")
    p.add_argument("--stylePath", type=str, default="style")
    p.add_argument("--texturePath", type=str, default="style/texture")
    p.add_argument("--outf", type=str, default="stylized_results", help="folder to output images")
    p.add_argument("--picked_content_mark", type=str, default=".")
    p.add_argument("--picked_style_mark", type=str, default=".")
    p.add_argument("--mode", type=str, default=None, choices=["original", "16x", "16x_kd2sd"], help="to choose different trained models")
    p.add_argument("--UHD", action="store_true", help="if use the UHD images")
    p.add_argument("--synthesis", action="store_true", help="for style synthesis")
    p.add_argument("--content_size", type=int, default=0, help="resize content, leave it to 0 if not resize")
    p.add_argument("--style_size", type=int, default=0, help="resize style, leave it to 0 if not resize")
    p.add_argument("--alpha", type=float, default=1, help="hyperparameter to blend wct feature and content feature")
    p.add_argument("--log_mark", type=str, default=time.strftime("%Y%m%d-%H%M"))
    p.add_argument("--num_run", type=int, default=1, help="you can run WCT for multiple times")
    p.add_argument("--debug", action="store_true")
    p.add_argument("--numpy", action="store_true", help="if use numpy for stylization rather than torch")
    # not in the reference: where its trained_models/ directory is (default: the paths of WCT.py:37-75 relative to the cwd)
    p.add_argument("--models_root", type=str, default="..", help="directory that holds trained_models/ (reference layout)")
    p.add_argument("--round", dest="round_mode", type=int, default=0, choices=[0, 1],
                   help="uint8 conversion of the result: 0 = truncation (torchvision 0.2.1, the reference's pin), 1 = +0.5")
    p.add_argument("--pipeline", type=int, default=3, help="pairs in flight (decode-ahead, async copies, writer pool); 0 = the reference's serial loop")
    p.add_argument("--io_threads", type=int, default=8, help="threads of the decode pool and of the writer pool (--pipeline > 0)")
    # not in the reference: spatial control (wct_stylize_regions)
    p.add_argument("--maskPath", type=str, default=None,
                   help="folder of label maps: content X.* uses DIR/X.png (mode L or P, pixel value = index into --region_styles, 255 = unstyled)")
    p.add_argument("--region_styles", type=str, default=None, help="comma-separated style images of the regions (with --maskPath)")
    # not in the reference: style interpolation (wct_stylize_interp) and per-pixel style weights (wct_stylize_blend)
    p.add_argument("--interp_styles", type=str, default=None,
                   help="comma-separated style images (1 to 8): every content is stylised with their blend (--interp_weights) or, with "
                        "--weightPath, with per-pixel weights")
    p.add_argument("--interp_weights", type=str, default=None,
                   help="comma-separated weights, one per --interp_styles image (>= 0, normalised to sum 1)")
    p.add_argument("--weightPath", type=str, default=None,
                   help="folder of weight maps: content X.* uses DIR/X_0.png .. DIR/X_{K-1}.png (mode L, weight = value / 255, "
                        "summing to <= 1 at every pixel; the rest stays unstyled)")
    # not in the reference: the noise of --synthesis (wct_noise_uniform) and the size of its output
    p.add_argument("--seed", type=int, default=0, help="seed of the noise image of --synthesis (0 .. 2^64 - 1); the texture's index is the stream id")
    p.add_argument("--synthesis_size", type=str, default=None,
                   help="WxH of the images --synthesis writes, exactly (default: noise of the texture's size after --style_size, as in the "
                        "reference, whose cascade floors every edge to a multiple of 16)")
    # not in the reference: colour preservation (include/wct_hip_color.h)
    p.add_argument("--preserve_color", type=str, default=None, choices=["match", "luma"],
                   help="keep the content's colours: match = map the style's colours onto the content's colour distribution before "
                        "stylisation, luma = keep the content's chroma and take only the stylised luminance")
    # not in the reference: guided-filter smoothing by the content image (include/wct_hip_smooth.h)
    p.add_argument("--smooth_radius", type=int, default=0,
                   help="radius in pixels of the guided filter that re-imposes the content's edges on the result (0 = off)")
    p.add_argument("--smooth_eps", type=float, default=None,
                   help="regulariser of --smooth_radius, relative to images in [0, 1] (default 1e-3); smaller follows the content's edges "
                        "more tightly, larger smooths more")
    # not in the reference: the choice of feature transform (include/wct_hip_transform.h)
    p.add_argument("--transform", type=str, default="wct", choices=["wct", "ot", "adain"],
                   help="feature transform of every level: wct = the reference's whitening and colouring, ot = the optimal-transport map "
                        "between the two feature Gaussians (same target statistics, moves the content least), adain = per-channel "
                        "mean / std matching")
    # not in the reference: patch-based style swap at one cascade level (include/wct_hip_swap.h)
    p.add_argument("--styleMaskPath", type=str, default=None,
                   help="with --maskPath / --region_styles: folder of STYLE label maps, style image X.* uses DIR/X.png (same rules as "
                        "--maskPath, at the style's size after --style_size); only the style pixels with label k enter region k's style "
                        "statistics; a style without a file is used whole")
    p.add_argument("--auto_regions", type=int, default=None,
                   help="K = 2..8: cluster the style's features into K regions (k-means at --auto_level), give every content feature pixel "
                        "the nearest cluster, and transfer region to region (wct_feature_regions + wct_stylize_guided)")
    p.add_argument("--auto_level", type=int, default=None, choices=[2, 3, 4, 5], help="with --auto_regions: the level whose features are clustered (default 4)")
    p.add_argument("--auto_iters", type=int, default=None, help="with --auto_regions: Lloyd iterations, 1..64 (default 10)")
    p.add_argument("--swap_level", type=int, default=None, choices=[2, 3, 4, 5],
                   help="run this level of the cascade as a patch swap (style decorator): every 3x3 content feature patch is replaced by "
                        "its best-matching style patch; the other levels keep --transform (default: off)")
    p.add_argument("--swap_match", type=str, default=None, choices=["whitened", "raw", "attention", "attention_whitened"],
                   help="where --swap_level matches patches: whitened = in the whitened domains of both features (Avatar-Net's style "
                        "decorator, the default), raw = on the features themselves (Chen & Schmidt); attention / attention_whitened = no "
                        "hard match at all: every content position takes the style mean and deviation weighted by a softmax of feature "
                        "similarity (on the standardised / the whitened features; include/wct_hip_attn.h)")
    p.add_argument("--swap_temp", type=float, default=None,
                   help="with --swap_match attention | attention_whitened: the softmax temperature, 0 .. 32 (0 = AdaIN with the population "
                        "variance, large = a 1x1 nearest-feature swap; default 8)")
    # not in the reference: scale control, a coarse-to-fine cascade on a device image pyramid (include/wct_hip_scale.h)
    p.add_argument("--level_scale", type=str, default=None,
                   help="d5,d4,d3,d2,d1: run level L of the cascade on the content reduced by the integer divisor dL (1 .. 16, not "
                        "increasing towards level 1, d1 = 1), e.g. 4,4,2,1,1: the reduced levels lay down strokes dL times as large "
                        "(default: off)")
    p.add_argument("--scale_detail", type=float, default=None,
                   help="with --level_scale: how much of the content's fine detail is put back where the working size grows (default "
                        "1.0 = the Laplacian-pyramid step, 0 = plain upsampling); a look, not a measurement")
    p.add_argument("--coarse_style", type=str, default=None,
                   help="with --level_scale: a second style image for the levels whose divisor is > 1 (scale mixing); the other levels "
                        "take the pair's style")
    # not in the reference: video mode, temporally stable stylisation of a frame sequence (include/wct_hip_video.h)
    p.add_argument("--video", action="store_true",
                   help="the picked content files, sorted by name, are the frames of ONE sequence: content statistics are tracked over "
                        "the frames and the output is blended with the previous one where the content did not move; one clip per style")
    p.add_argument("--temporal_rate", type=float, default=None,
                   help="with --video: weight of the new frame in the tracked content statistics, in (0, 1] (default 0.25; 1 = per-frame "
                        "statistics); a look, not a measurement")
    p.add_argument("--scene_cut", type=float, default=None,
                   help="with --video: a frame whose mean level-5 feature moved by more than this many running variances starts afresh "
                        "(default 0.5; inf = never, 0 = every frame)")
    p.add_argument("--temporal_blend", type=float, default=None,
                   help="with --video: weight of the previous output where the content stands still, in [0, 1) (default 0.6; 0 = off)")
    p.add_argument("--temporal_sigma", type=float, default=None,
                   help="with --video: the content difference (images in [0, 1]) at which the blend has faded to exp(-1/2) (default 0.05)")
    p.add_argument("--temporal_radius", type=int, default=None,
                   help="with --video: radius in pixels of the window the content difference is averaged over, 0 .. 8 (default 2)")
    # not in the reference: motion compensation for video mode (include/wct_hip_motion.h)
    p.add_argument("--motion", action="store_true",
                   help="with --video: the blend compares every frame with the previous one displaced by a block-matched motion field, so "
                        "that panning and moving regions keep their strokes too")
    p.add_argument("--motion_levels", type=int, default=None,
                   help="with --motion: levels of the luma pyramid the search runs over, 1 .. 4 (default 4); a look, not a measurement")
    p.add_argument("--motion_range", type=int, default=None,
                   help="with --motion: search range at the coarsest level in its pixels, 0 .. 7 (default 4)")
    p.add_argument("--motion_penalty", type=int, default=None,
                   help="with --motion: cost per pixel of vector length, in grey levels, 0 .. 255 (default 4)")
    # not in the reference: seeded style variations, a rotation inside the colouring step (include/wct_hip_diverse.h)
    p.add_argument("--diversity", type=float, default=None,
                   help="D in (0, 8]: post-multiply the style's square-root covariance by a seeded rotation of this strength before the "
                        "colouring step (Wang et al., CVPR 2020): same feature statistics, a different stylisation per --seed and variation "
                        "(default: off)")
    p.add_argument("--variations", type=int, default=None,
                   help="with --diversity: images per pair, 1 .. 64 (default 1); variation k uses stream id k of --seed and is saved as _v<k>")
    p.add_argument("--diversity_levels", type=str, default=None,
                   help="with --diversity: comma-separated cascade levels whose style is rotated (default 5, the paper's choice; a look, "
                        "not a measurement)")
    # not in the reference: proxy mode, stylise reduced and apply at full size by bilateral grid (include/wct_hip_bgrid.h)
    p.add_argument("--proxy_scale", type=int, default=None,
                   help="D in 1 .. 16: stylise the content reduced by D, fit a bilateral grid of local affine colour maps to the reduced pair "
                        "and apply it to the full content (Chen et al., SIGGRAPH Asia 2016): the content's exact size and edges, colour and "
                        "tone but no strokes (default: off)")
    p.add_argument("--proxy_cell", type=int, default=None, help="with --proxy_scale: reduced pixels per grid cell (default 16; a look, not a measurement)")
    p.add_argument("--proxy_bins", type=int, default=None, help="with --proxy_scale: luminance vertices of the grid, 1 .. 32 (default 8)")
    p.add_argument("--proxy_eps", type=float, default=None,
                   help="with --proxy_scale: regulariser of the local fits towards the global one, relative to images in [0, 1] (default 1e-2)")
    p.add_argument("--proxy_smooth", type=int, default=None, help="with --proxy_scale: [1 2 1] blur passes over the grid's sums, 0 .. 4 (default 1)")
    # not in the reference: the .jpg / .jpeg outputs encoded on the device (include/wct_hip_jpeg.h), byte-identical to Pillow's file
    p.add_argument("--device_jpeg", action="store_true",
                   help="encode every .jpg / .jpeg output on the GPU and write the bytes: the same file as Pillow's, without the host encode "
                        "and with the compressed file instead of the image copied to the host (default: off, Pillow encodes)")
    # not in the reference: the .jpg / .jpeg inputs decoded on the device (include/wct_hip_jdec.h), pixel-identical to Pillow's decode
    p.add_argument("--device_decode", action="store_true",
                   help="decode every baseline .jpg / .jpeg input on the GPU: the same pixels as Pillow's, with the compressed segment instead "
                        "of the image copied to the device; other files fall back to Pillow (default: off, Pillow decodes)")
    p.add_argument("--jpeg_quality", type=int, default=75, help="quality of the .jpg / .jpeg outputs, 1 .. 100, with and without --device_jpeg "
                                                                "(default 75, Pillow's default)")
    return p


def checkpoint_args(args) -> None:
    """e1..e5 / d1..d5 exactly as WCT.py:37-75 assigns them (relative to --models_root)."""
    root = os.path.join(args.models_root, "trained_models")
    if args.mode == "original" or args.mode is None:
        enc = [os.path.join(root, "original_wct_models", "vgg_normalised_conv%d_1.t7" % k) for k in range(1, 6)]
        dec = [os.path.join(root, "original_wct_models", "feature_invertor_conv%d_1.t7" % k) for k in range(1, 6)]
    else:
        sd = "wct_se_16x_new_sd" if args.mode == "16x" else "wct_se_16x_new_sd_kd2sd"
        enc = [os.path.join(root, "wct_se_16x_new", "%dSE.pth" % k) for k in range(1, 6)]
        dec = [os.path.join(root, sd, "%dSD.pth" % k) for k in range(1, 6)]
    for k in range(1, 6):
        setattr(args, "e%d" % k, enc[k - 1])
        setattr(args, "d%d" % k, dec[k - 1])


def is_image_file(name: str) -> bool:
    return any(name.endswith(e) for e in IMG_EXT)


def list_pairs(content_dir: str, style_dir: str, content_mark: str = ".", style_mark: str = ".") -> List[Tuple[str, str]]:
    """The Cartesian product of data_loader.py:32-36: contents outer, styles inner, os.listdir order, substring filters."""
    cs = [x for x in os.listdir(content_dir) if is_image_file(x) and content_mark in x]
    ss = [x for x in os.listdir(style_dir) if is_image_file(x) and style_mark in x]
    return [(c, s) for c in cs for s in ss]


def pair_name(content_file: str, style_file: str) -> str:
    """data_loader.py:60: '<content stem>+<style stem>.jpg' (stem = text before the FIRST dot)."""
    return content_file.split(".")[0] + "+" + style_file.split(".")[0] + ".jpg"


def out_name(args, imname: str, variation: Optional[int] = None) -> str:
    """WCT.py:127 (str(1) for the integer default of --alpha, like '%s' % args.alpha there).  variation: the k of --variations N > 1."""
    color = getattr(args, "preserve_color", None)
    radius = getattr(args, "smooth_radius", 0)
    transform = getattr(args, "transform", None) or "wct"
    tmark = "_transform=%s" % transform if transform != "wct" else ""                          # directly after alpha; wct names are unchanged
    if getattr(args, "diversity", None):
        tmark += "_div=%g" % args.diversity                                                     # after the transform mark (wct only, so: in its place)
    if getattr(args, "proxy_scale", None):
        tmark += "_proxy=%d" % args.proxy_scale                                                 # after the transform mark (mixes with no other mode)
    swap = getattr(args, "swap_level", None)
    if swap:
        tmark += "_swap=%d" % swap                                                              # after the transform mark
        if getattr(args, "swap_match", None) in ATTN_MATCH_NAMES:                               # the patch swap's names are unchanged
            tmark += "_%s=%g" % (args.swap_match, getattr(args, "swap_temp", None) or 0.0)
    scale = getattr(args, "level_scale", None)
    if scale:
        tmark += "_scale=%s" % "-".join(t.strip() for t in scale.split(","))                    # in the same place (the two do not mix)
    auto = getattr(args, "auto_regions", None)
    if auto:
        tmark += "_auto=%d" % auto                                                              # in the same place (mixes with neither)
    marks = ("_color=%s" % color if color else "") + ("_smooth=%d" % radius if radius else "")   # runs with and without the flags never collide
    if variation is not None:
        marks += "_v%d" % variation                                                              # directly before the pair name
    return os.path.join(args.outf, "%s_mode=%s_alpha=%s%s%s_%s" % (args.log_mark, args.mode, args.alpha, tmark, marks, imname))


def load_rgb_u8(path: str, size: int = 0):
    """default_loader of data_loader.py:18-19: RGB uint8 HWC.  With `size`, also transforms.Resize(size) of :52-56 by Pillow on the
    host -- the CLI itself passes 0 and resizes on the GPU (WCT.resize_u8, bit-identical); this form is the host-side reference of
    tests/test_cli.py."""
    import numpy as np
    from PIL import Image
    img = Image.open(path).convert("RGB")
    if size:
        w, h = img.size
        if not ((w <= h and w == size) or (h <= w and h == size)):
            if w < h:
                ow, oh = size, int(size * h / w)
            else:
                oh, ow = size, int(size * w / h)
            img = img.resize((ow, oh), Image.BILINEAR)
    return np.array(img, dtype=np.uint8)   # a writable, contiguous copy


def resized_shape(H: int, W: int, size: int) -> Tuple[int, int]:
    """(H, W) after transforms.Resize(size) (data_loader.py:52-56; the rule of load_rgb_u8 and wct_resize_shape)."""
    if not size or (W <= H and W == size) or (H <= W and H == size):
        return H, W
    if W < H:
        return int(size * H / W), size
    return size, int(size * W / H)


def region_jobs(content_dir: str, mask_dir: str, content_mark: str = ".") -> List[Tuple[str, str]]:
    """--maskPath: every content X.* (listdir order, --picked_content_mark) with its label map DIR/X.png (X = text before the first
    dot, as pair_name); a content without a map is an error that names the missing file."""
    jobs = []
    for c in os.listdir(content_dir):
        if not (is_image_file(c) and content_mark in c):
            continue
        m = os.path.join(mask_dir, c.split(".")[0] + ".png")
        if not os.path.isfile(m):
            raise FileNotFoundError("label map %s for content %s not found" % (m, c))
        jobs.append((c, m))
    return jobs


def load_mask(path: str, shape: Tuple[int, int]):
    """A label map as uint8 H x W: a mode L or P PNG whose pixel values are region indices.  It must have the content's size after
    --content_size (`shape`); masks are never resampled."""
    import numpy as np
    from PIL import Image
    img = Image.open(path)
    if img.mode not in ("L", "P"):
        raise ValueError("label map %s has mode %s; expected L or P (pixel value = region index)" % (path, img.mode))
    lab = np.array(img, dtype=np.uint8)
    if tuple(lab.shape) != tuple(shape):
        raise ValueError("label map %s is %dx%d (HxW) but the content is %dx%d after --content_size; masks are not resampled"
                         % (path, lab.shape[0], lab.shape[1], shape[0], shape[1]))
    return lab


def style_mask_path(mask_dir: Optional[str], style_path: str) -> Optional[str]:
    """--styleMaskPath: style image X.* uses DIR/X.png (X = text before the first dot of the file name); None when there is no such
    file -- that style is used whole."""
    if not mask_dir:
        return None
    m = os.path.join(mask_dir, os.path.basename(style_path).split(".")[0] + ".png")
    return m if os.path.isfile(m) else None


def region_out_name(args, content_file: str) -> str:
    """<log_mark>_mode=<m>_alpha=<a>_<X>+regions.jpg (out_name with the style stem replaced by 'regions')."""
    return out_name(args, content_file.split(".")[0] + "+regions.jpg")


def run_regions(args, wct, jobs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--maskPath: one stylisation per content of region_jobs(), region k against --region_styles[k] (wct_stylize_regions); the serial
    loop.  Returns (total seconds, contents)."""
    styles = [p for p in args.region_styles.split(",") if p]

    def convert():
        return [_to_tensor(wct, _upload_u8(p), args.style_size) for p in styles]

    s_dev = convert()       # once per run, outside every job's timer
    # --styleMaskPath: the styles' own label maps, at each style's size after --style_size (wct_stylize_guided); none -> wct_stylize_regions
    smask = [style_mask_path(getattr(args, "styleMaskPath", None), p) for p in styles]
    s_lab = [_on_device(load_mask(m, (int(t.shape[-2]), int(t.shape[-1])))) if m else None for m, t in zip(smask, s_dev)]
    guided = any(m is not None for m in s_lab)

    def label_map(mpath):
        return lambda c_u8: _on_device(load_mask(mpath, resized_shape(int(c_u8.shape[0]), int(c_u8.shape[1]), args.content_size)))

    def stylise(c_f32, lab):
        def once(fresh):
            st = convert() if fresh else s_dev      # the recompute reads and converts the styles again
            if guided:
                return wct.stylize_guided(c_f32, st, lab, s_lab, None, args.alpha, args.num_run)
            return wct.stylize_regions(c_f32, st, lab, args.alpha, args.num_run)
        return _recompute_fp32(wct, logprinter, "content", once)

    return _run_jobs(args, wct, logprinter, [
        Job(' #%s: Transferring "%s" by regions (%s)' % (i, cfile, mpath), os.path.join(content_dir, cfile), label_map(mpath), stylise,
            region_out_name(args, cfile)) for i, (cfile, mpath) in enumerate(jobs)]), len(jobs)


def check_region_args(args) -> None:
    if (args.maskPath is None) != (args.region_styles is None):
        raise ValueError("--maskPath and --region_styles go together")
    if args.region_styles is not None:
        n = len([p for p in args.region_styles.split(",") if p])
        if not 1 <= n <= 8:
            raise ValueError("--region_styles: 1 to 8 style images, got %d" % n)
    if getattr(args, "styleMaskPath", None) is not None:
        if args.maskPath is None:
            raise ValueError("--styleMaskPath does nothing without --maskPath / --region_styles")
        if not os.path.isdir(args.styleMaskPath):
            raise ValueError("--styleMaskPath %s is not a folder" % args.styleMaskPath)


def check_auto_args(args) -> None:
    """--auto_regions K / --auto_level / --auto_iters: ordinary content x style pairs through the plain wct cascade, region to region."""
    K, level, iters = getattr(args, "auto_regions", None), getattr(args, "auto_level", None), getattr(args, "auto_iters", None)
    if K is None:
        for v, name in ((level, "--auto_level"), (iters, "--auto_iters")):
            if v is not None:
                raise ValueError("%s does nothing without --auto_regions" % name)
        return
    if not 2 <= K <= 8:
        raise ValueError("--auto_regions: K = 2..8 expected, got %r" % (K,))
    if iters is not None and not 1 <= iters <= 64:
        raise ValueError("--auto_iters: 1..64 expected, got %r" % (iters,))
    transform = getattr(args, "transform", None) or "wct"
    clash = [name for flag, name in ((args.maskPath is not None, "--maskPath"), (args.interp_styles is not None, "--interp_styles"),
                                     (args.weightPath is not None, "--weightPath"), (args.synthesis, "--synthesis"),
                                     (getattr(args, "swap_level", None), "--swap_level"), (getattr(args, "level_scale", None), "--level_scale"),
                                     (transform != "wct", "--transform %s" % transform)) if flag]
    if clash:
        raise ValueError("--auto_regions does not mix with %s" % ", ".join(clash))
    if getattr(args, "preserve_color", None) in ("match", "match+luma"):
        raise ValueError("--auto_regions does not mix with --preserve_color match (it is for one whole style per content); luma goes with it")
    args.auto_level = 4 if level is None else level
    args.auto_iters = 10 if iters is None else iters


def run_auto(args, wct, pairs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--auto_regions: per pair, k-means label maps from the features of --auto_level (wct_feature_regions), then the region-to-region
    cascade against the one style (wct_stylize_guided); one pair at a time.  Returns (total seconds, pairs)."""
    K = args.auto_regions

    def stylise(c_f32, s_u8):
        def once(fresh):        # every pass converts the style and clusters again
            s_f32 = _to_tensor(wct, s_u8, args.style_size)
            lab_c, lab_s = wct.feature_regions(c_f32, s_f32, K, args.auto_level, args.auto_iters)
            return wct.stylize_guided(c_f32, [s_f32], lab_c, [lab_s], [0] * K, args.alpha, args.num_run)
        return _recompute_fp32(wct, logprinter, "pair", once)

    def job(i, cfile, sfile):
        imname = pair_name(cfile, sfile)
        return Job(' #%s: Transferring "%s" (%d feature regions of level %d, %d iterations)' % (i, imname, K, args.auto_level, args.auto_iters),
                   os.path.join(content_dir, cfile), lambda c_u8: _upload_u8(os.path.join(style_dir, sfile)), stylise, out_name(args, imname))

    return _run_jobs(args, wct, logprinter, [job(i, c, s) for i, (c, s) in enumerate(pairs)]), len(pairs)


def check_color_args(args) -> None:
    """--preserve_color: luma is a post-merge and goes with every content-driven mode; match needs ONE style per content."""
    color = getattr(args, "preserve_color", None)
    if color is None:
        return
    if color not in ("match", "luma"):
        raise ValueError("--preserve_color: match or luma expected, got %r" % (color,))
    if args.synthesis:
        raise ValueError("--preserve_color does not mix with --synthesis: there is no content whose colours could be kept")
    if color == "match":
        for flag, name in ((args.maskPath, "--maskPath"), (args.interp_styles, "--interp_styles"), (args.weightPath, "--weightPath")):
            if flag is not None:
                raise ValueError("--preserve_color match does not mix with %s (several styles per content); use --preserve_color luma" % name)


def check_smooth_args(args) -> None:
    """--smooth_radius / --smooth_eps: the filter needs a content to guide by; --smooth_eps alone means nothing.  Fills in the default
    regulariser."""
    from .lib import SMOOTH_EPS, SMOOTH_MAX_RADIUS      # WCT_SMOOTH_EPS, WCT_SMOOTH_MAX_RADIUS (include/wct_hip_smooth.h)
    radius, eps = getattr(args, "smooth_radius", 0), getattr(args, "smooth_eps", None)
    if radius < 0:
        raise ValueError("--smooth_radius: a radius >= 0 expected (0 = off), got %d" % radius)
    if radius > SMOOTH_MAX_RADIUS:
        raise ValueError("--smooth_radius: at most %d, got %d" % (SMOOTH_MAX_RADIUS, radius))
    if radius == 0:
        if eps is not None:
            raise ValueError("--smooth_eps does nothing without --smooth_radius")
        return
    if args.synthesis:
        raise ValueError("--smooth_radius does not mix with --synthesis: there is no content to guide the filter by")
    if eps is None:
        args.smooth_eps = SMOOTH_EPS
    elif not (0.0 < eps < float("inf")):
        raise ValueError("--smooth_eps: a finite positive value expected, got %r" % (eps,))


def check_transform_args(args) -> None:
    """--transform ot | adain: everything goes with them (--pipeline, the style cache, the fp32 fallback, --synthesis, --interp_weights,
    --preserve_color, --smooth_radius) but the wct-only variants: --numpy (+ I on the content covariance) and the per-pixel K-slot
    paths of --maskPath and --weightPath (weighted-moment normalisations)."""
    from .lib import TRANSFORMS
    transform = getattr(args, "transform", None) or "wct"
    if transform not in TRANSFORMS:
        raise ValueError("--transform: one of %s expected, got %r" % (", ".join(sorted(TRANSFORMS)), transform))
    if transform == "wct":
        return
    for flag, name in ((args.numpy, "--numpy"), (args.maskPath is not None, "--maskPath"), (args.weightPath is not None, "--weightPath")):
        if flag:
            raise ValueError("--transform %s does not mix with %s (defined for the wct transform only)" % (transform, name))


ATTN_MATCH_NAMES = ("attention", "attention_whitened")       # lib.ATTN_MATCHES: the --swap_match values that route to wct_stylize_attn


def check_swap_args(args) -> None:
    """--swap_level L / --swap_match: one style per content, a content to take patches for, and the plain cascade around the swapped
    level; --preserve_color luma and --smooth_radius are post-steps and go with it.  Fills in the default match."""
    from .lib import ATTN_MAX_TEMP, ATTN_TEMP, SWAP_LEVELS, SWAP_MATCHES
    level, match = getattr(args, "swap_level", None), getattr(args, "swap_match", None)
    temp = getattr(args, "swap_temp", None)
    if temp is not None and match not in ATTN_MATCH_NAMES:
        raise ValueError("--swap_temp needs --swap_level with --swap_match attention or attention_whitened")
    if not level:
        if match is not None:
            raise ValueError("--swap_match does nothing without --swap_level")
        return
    if level not in SWAP_LEVELS:
        raise ValueError("--swap_level: one of %s expected, got %r" % (", ".join(str(v) for v in SWAP_LEVELS), level))
    if match is None:
        args.swap_match = "whitened"
    elif match in ATTN_MATCH_NAMES:
        if temp is None:
            args.swap_temp = ATTN_TEMP
        elif not 0.0 <= temp <= ATTN_MAX_TEMP:           # a NaN fails both comparisons
            raise ValueError("--swap_temp: a temperature in 0 .. %d expected, got %r" % (ATTN_MAX_TEMP, temp))
    elif match not in SWAP_MATCHES:
        raise ValueError("--swap_match: whitened or raw expected, got %r" % (match,))
    clash = [name for flag, name in ((args.synthesis, "--synthesis"), (args.maskPath is not None, "--maskPath"),
                                     (args.interp_styles is not None, "--interp_styles"), (args.weightPath is not None, "--weightPath"),
                                     (args.numpy, "--numpy"), (getattr(args, "preserve_color", None) == "match", "--preserve_color match")) if flag]
    if clash:
        raise ValueError("--swap_level does not mix with %s" % ", ".join(clash))


def _swap_pair(wct, args, logprinter, c_f32, style_f32):
    """One pair of --swap_level: wct_stylize_swap, and after a clamp of the f16x3 range the same call under the exact-fp32 convolutions
    (`style_f32()` makes the style tensor afresh for it).  The patch match stays f16x3 in that recompute -- whitened features are O(1) --
    so a clamp inside it is not cured: it still counts, is reported in the log, and the pair's result is returned all the same."""
    passes = []

    def once(fresh):
        passes.append(fresh)
        if args.swap_match in ATTN_MATCH_NAMES:
            return wct.stylize_attn(c_f32, style_f32(), args.swap_level, args.swap_match, args.swap_temp, args.alpha, args.num_run)
        return wct.stylize_swap(c_f32, style_f32(), args.swap_level, args.swap_match, args.alpha, args.num_run)

    # no wct.sync() in the recompute: it raises on a clamp; saturation_count synchronises, counts and acknowledges it instead
    res = _recompute_fp32(wct, logprinter, "pair", once, sync=False)
    if passes[-1] and wct.saturation_count(reset=True):
        logprinter("WARNING: a feature of this pair left the f16 range inside the patch match and was clamped there; the chosen "
                   "patches may deviate")
    return res


def run_swap(args, wct, pairs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--swap_level: the reference's loop with the cascade of wct_stylize_swap, one pair at a time (the swapped level needs the style's
    feature map itself, so there are no style statistics to cache).  Returns (total seconds, pairs)."""
    on_device = _device_images(8)

    def stylise(c_f32, s_u8):
        return _swap_pair(wct, args, logprinter, c_f32, lambda: _to_tensor(wct, s_u8, args.style_size))

    def job(i, cfile, sfile):
        imname = pair_name(cfile, sfile)
        what = "attention statistics at level %d, %s, temperature %g" % (args.swap_level, args.swap_match, args.swap_temp) \
            if args.swap_match in ATTN_MATCH_NAMES else "patch swap at level %d, %s" % (args.swap_level, args.swap_match)
        return Job(' #%s: Transferring "%s" (%s)' % (i, imname, what),
                   os.path.join(content_dir, cfile), lambda c_u8: on_device(os.path.join(style_dir, sfile)), stylise, out_name(args, imname))

    return _run_jobs(args, wct, logprinter, [job(i, c, s) for i, (c, s) in enumerate(pairs)]), len(pairs)


def level_scale_list(text: str) -> Tuple[int, ...]:
    """'4,4,2,1,1' -> (4, 4, 2, 1, 1): the divisors of levels 5, 4, 3, 2, 1."""
    try:
        div = tuple(int(t) for t in text.split(","))
    except ValueError:
        raise ValueError("--level_scale: five comma-separated integers expected (d5,d4,d3,d2,d1), got %r" % (text,))
    if len(div) != 5:
        raise ValueError("--level_scale: five divisors expected (d5,d4,d3,d2,d1), got %d in %r" % (len(div), text))
    return div


def check_scale_args(args) -> None:
    """--level_scale / --scale_detail / --coarse_style: one style per content (two with --coarse_style), a content to reduce, and the
    affine cascade at every level; --transform, --numpy, --preserve_color and --smooth_radius go with it.  Fills in the default gain."""
    from .lib import SCALE_DETAIL, SCALE_MAX_DIVISOR
    text, gain, coarse = getattr(args, "level_scale", None), getattr(args, "scale_detail", None), getattr(args, "coarse_style", None)
    if not text:
        for flag, name in ((gain is not None, "--scale_detail"), (coarse is not None, "--coarse_style")):
            if flag:
                raise ValueError("%s does nothing without --level_scale" % name)
        return
    div = level_scale_list(text)
    if any(not 1 <= d <= SCALE_MAX_DIVISOR for d in div):
        raise ValueError("--level_scale: every divisor must lie in 1 .. %d, got %r" % (SCALE_MAX_DIVISOR, text))
    if any(div[i] > div[i - 1] for i in range(1, 5)):
        raise ValueError("--level_scale: the divisors must not increase from level 5 to level 1, got %r" % (text,))
    if div[4] != 1:
        raise ValueError("--level_scale: the divisor of level 1 must be 1 (the result is made at full size), got %r" % (text,))
    clash = [name for flag, name in ((args.synthesis, "--synthesis"), (args.maskPath is not None, "--maskPath"),
                                     (args.interp_styles is not None, "--interp_styles"), (args.weightPath is not None, "--weightPath"),
                                     (getattr(args, "swap_level", None), "--swap_level")) if flag]
    if clash:
        raise ValueError("--level_scale does not mix with %s" % ", ".join(clash))
    if gain is None:
        args.scale_detail = SCALE_DETAIL
    elif not (0.0 <= gain < float("inf")):
        raise ValueError("--scale_detail: a finite value >= 0 expected, got %r" % (gain,))
    if coarse is not None and div[0] == 1:
        raise ValueError("--coarse_style does nothing with --level_scale %s: no level has a divisor > 1" % text)


def _scale_once(wct, args, c_f32, style, coarse):
    """One wct_stylize_scaled of a pair.  --preserve_color match maps each style's colours onto the content first (wct_color_match);
    with --coarse_style the levels whose divisor is > 1 are prepared from it and the rest from the pair's style, and the cascade runs
    against those prepared statistics."""
    div = level_scale_list(args.level_scale)
    if getattr(args, "preserve_color", None) == "match":
        style = wct.color_match(style, c_f32)
        coarse = wct.color_match(coarse, c_f32) if coarse is not None else None
    if coarse is None:
        return wct.stylize_scaled(c_f32, style, div, args.scale_detail, args.alpha, args.num_run)
    reduced = [5 - i for i in range(5) if div[i] > 1]
    wct.style_prepare(coarse, levels=reduced)
    wct.style_prepare(style, levels=[L for L in (5, 4, 3, 2, 1) if L not in reduced])
    res = wct.stylize_scaled(c_f32, None, div, args.scale_detail, args.alpha, args.num_run)
    wct._scale_keep = (style, coarse)     # the side stream reads both asynchronously
    return res


def _scale_pair(wct, args, logprinter, c_f32, style_f32, coarse_f32):
    """One pair of --level_scale, and after a clamp of the f16x3 range the same under the exact-fp32 convolutions (`style_f32()` and
    `coarse_f32()` make the style tensors afresh for it; the resampler and the merge are fp32 and clamp nothing)."""
    return _recompute_fp32(wct, logprinter, "pair", lambda fresh: _scale_once(wct, args, c_f32, style_f32(), coarse_f32()))


def run_scale(args, wct, pairs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--level_scale: the reference's loop with the cascade of wct_stylize_scaled, one pair at a time.  Returns (total seconds, pairs)."""
    on_device = _device_images(8)

    def stylise(c_f32, u8):
        s_u8, k_u8 = u8
        return _scale_pair(wct, args, logprinter, c_f32, lambda: _to_tensor(wct, s_u8, args.style_size),
                           lambda: _to_tensor(wct, k_u8, args.style_size) if k_u8 is not None else None)

    def job(i, cfile, sfile):
        imname = pair_name(cfile, sfile)
        return Job(' #%s: Transferring "%s" (level divisors %s, detail %g%s)' % (
                       i, imname, args.level_scale, args.scale_detail, ", coarse style %s" % args.coarse_style if args.coarse_style else ""),
                   os.path.join(content_dir, cfile),
                   lambda c_u8: (on_device(os.path.join(style_dir, sfile)), on_device(args.coarse_style) if args.coarse_style else None),
                   stylise, out_name(args, imname))

    return _run_jobs(args, wct, logprinter, [job(i, c, s) for i, (c, s) in enumerate(pairs)]), len(pairs)


def diversity_level_list(text: str) -> Tuple[int, ...]:
    """'5,4' -> (5, 4): the levels of --diversity_levels."""
    try:
        levels = tuple(int(t) for t in text.split(","))
    except ValueError:
        raise ValueError("--diversity_levels: comma-separated levels among 1..5 expected, got %r" % (text,)) from None
    if not levels or any(not 1 <= L <= 5 for L in levels) or len(set(levels)) != len(levels):
        raise ValueError("--diversity_levels: distinct levels among 1..5 expected, got %r" % (text,))
    return levels


def check_diverse_args(args) -> None:
    """--diversity D / --variations N / --diversity_levels: ordinary content x style pairs (or the frames of --video, one variation)
    through the wct cascade against prepared statistics; --alpha, --num_run, --preserve_color luma and --smooth_radius go with it.
    Fills in the defaults; --diversity_levels becomes a tuple of levels."""
    from .lib import DIVERSE_LEVELS, DIVERSE_MAX_STRENGTH
    D, N, levels = getattr(args, "diversity", None), getattr(args, "variations", None), getattr(args, "diversity_levels", None)
    if D is None:
        for v, name in ((N, "--variations"), (levels, "--diversity_levels")):
            if v is not None:
                raise ValueError("%s does nothing without --diversity" % name)
        return
    if not 0.0 < D <= DIVERSE_MAX_STRENGTH:              # a NaN fails both comparisons
        raise ValueError("--diversity: a strength in (0, %d] expected, got %r" % (DIVERSE_MAX_STRENGTH, D))
    if N is not None and not 1 <= N <= 64:
        raise ValueError("--variations: 1 .. 64 expected, got %r" % (N,))
    parsed = DIVERSE_LEVELS if levels is None else levels if isinstance(levels, tuple) else diversity_level_list(levels)
    if not 0 <= args.seed < 1 << 64:
        raise ValueError("--seed: 0 .. 2^64 - 1 expected, got %d" % args.seed)
    transform = getattr(args, "transform", None) or "wct"
    clash = [name for flag, name in ((transform != "wct", "--transform %s" % transform), (args.numpy, "--numpy"), (args.synthesis, "--synthesis"),
                                     (args.maskPath is not None, "--maskPath"), (args.interp_styles is not None, "--interp_styles"),
                                     (args.weightPath is not None, "--weightPath"), (getattr(args, "swap_level", None), "--swap_level"),
                                     (getattr(args, "level_scale", None), "--level_scale"), (getattr(args, "auto_regions", None), "--auto_regions"),
                                     (getattr(args, "preserve_color", None) == "match", "--preserve_color match")) if flag]
    if clash:
        raise ValueError("--diversity does not mix with %s" % ", ".join(clash))
    if getattr(args, "video", False) and N not in (None, 1):
        raise ValueError("--video takes one variation of --diversity (the same rotation for every frame), got --variations %d" % N)
    args.variations = 1 if N is None else N
    args.diversity_levels = parsed


def run_diverse(args, wct, pairs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--diversity: per pair the style is prepared once and the slots of --diversity_levels exported; every variation v imports them
    again, rotates them (wct_style_diversify: --seed, stream id v) and runs the cascade against the prepared statistics.  One job of
    the serial loop per image.  Returns (total seconds, images)."""
    on_device = _device_images(8)
    levels, N = args.diversity_levels, args.variations
    held = {}                   # the pair whose style the engine holds: {"pair": i, "slots": {level: its statistics before any rotation}}

    def job(i, cfile, sfile, v):
        imname = pair_name(cfile, sfile)

        def stylise(c_f32, s_u8):
            def once(fresh):        # the recompute prepares the style again, and what it prepared is not kept for the next variation
                if fresh or held.get("pair") != i:
                    held.clear()
                    wct.style_prepare(_to_tensor(wct, s_u8, args.style_size))
                    if not fresh:
                        held.update(pair=i, slots={L: wct.style_export(L) for L in levels})
                else:
                    for L, stats in held["slots"].items():
                        wct.style_import(L, stats)
                wct.style_diversify(args.diversity, args.seed, v, levels)
                return wct.stylize_prepared(c_f32, args.alpha, args.num_run)
            return _recompute_fp32(wct, logprinter, "pair", once)

        return Job(' #%s: Transferring "%s" (diversity %g at level%s %s, variation %d of %d)' % (
                       i * N + v, imname, args.diversity, "s" if len(levels) > 1 else "", ",".join(str(L) for L in levels), v, N),
                   os.path.join(content_dir, cfile), lambda c_u8: on_device(os.path.join(style_dir, sfile)), stylise,
                   out_name(args, imname, v if N > 1 else None))

    jobs = [job(i, c, s, v) for i, (c, s) in enumerate(pairs) for v in range(N)]
    return _run_jobs(args, wct, logprinter, jobs), len(jobs)


PROXY_FLAGS = (("proxy_cell", "--proxy_cell"), ("proxy_bins", "--proxy_bins"), ("proxy_eps", "--proxy_eps"), ("proxy_smooth", "--proxy_smooth"))


def check_proxy_args(args) -> None:
    """--proxy_scale D and its four parameters: ordinary content x style pairs, one at a time; --alpha, --num_run, --transform,
    --content_size, --style_size and --round go with it.  The result already carries the content's edges and colours are what it
    transfers, so the post-steps and every other mode are refused by name.  Fills in the defaults."""
    from .lib import BGRID_BINS, BGRID_CELL, BGRID_EPS, BGRID_MAX_SMOOTH, BGRID_MAX_Z, BGRID_SMOOTH, SCALE_MAX_DIVISOR
    D = getattr(args, "proxy_scale", None)
    if D is None:
        for attr, name in PROXY_FLAGS:
            if getattr(args, attr, None) is not None:
                raise ValueError("%s does nothing without --proxy_scale" % name)
        return
    if not 1 <= D <= SCALE_MAX_DIVISOR:
        raise ValueError("--proxy_scale: a divisor in 1 .. %d expected, got %r" % (SCALE_MAX_DIVISOR, D))
    clash = [name for flag, name in ((args.synthesis, "--synthesis"), (args.maskPath is not None, "--maskPath"),
                                     (args.interp_styles is not None, "--interp_styles"), (args.weightPath is not None, "--weightPath"),
                                     (getattr(args, "video", False), "--video"), (getattr(args, "swap_level", None), "--swap_level"),
                                     (getattr(args, "level_scale", None), "--level_scale"), (getattr(args, "auto_regions", None), "--auto_regions"),
                                     (getattr(args, "diversity", None), "--diversity"),
                                     (getattr(args, "preserve_color", None), "--preserve_color"),
                                     (getattr(args, "smooth_radius", 0), "--smooth_radius")) if flag]
    if clash:
        raise ValueError("--proxy_scale does not mix with %s" % ", ".join(clash))
    for attr, default in (("proxy_cell", BGRID_CELL), ("proxy_bins", BGRID_BINS), ("proxy_eps", BGRID_EPS), ("proxy_smooth", BGRID_SMOOTH)):
        if getattr(args, attr, None) is None:
            setattr(args, attr, default)
    if args.proxy_cell < 1:
        raise ValueError("--proxy_cell: a cell of 1 reduced pixel at least expected, got %r" % (args.proxy_cell,))
    if not 1 <= args.proxy_bins <= BGRID_MAX_Z:
        raise ValueError("--proxy_bins: 1 .. %d expected, got %r" % (BGRID_MAX_Z, args.proxy_bins))
    if not 0.0 < args.proxy_eps < float("inf"):              # a NaN fails both comparisons
        raise ValueError("--proxy_eps: a finite value > 0 expected, got %r" % (args.proxy_eps,))
    if not 0 <= args.proxy_smooth <= BGRID_MAX_SMOOTH:
        raise ValueError("--proxy_smooth: 0 .. %d expected, got %r" % (BGRID_MAX_SMOOTH, args.proxy_smooth))


def check_jpeg_args(args) -> None:
    """--jpeg_quality applies to every .jpg / .jpeg output, on either encoder; --device_jpeg only chooses the encoder."""
    q = getattr(args, "jpeg_quality", 75)
    if not 1 <= q <= 100:
        raise ValueError("--jpeg_quality: 1 .. 100 expected, got %r" % (q,))


def is_jpeg_file(path: str) -> bool:
    return path.lower().endswith((".jpg", ".jpeg"))


def save_host_u8(args, array, path: str) -> None:
    """Pillow's save of a uint8 H x W x 3 host array; a JPEG at --jpeg_quality (75, the default, is what save(path) alone writes)."""
    from PIL import Image
    if is_jpeg_file(path):
        Image.fromarray(array).save(path, quality=getattr(args, "jpeg_quality", 75))
    else:
        Image.fromarray(array).save(path)


def device_jpeg_wanted(args, path: str) -> bool:
    return bool(getattr(args, "device_jpeg", False)) and is_jpeg_file(path)


def save_u8(wct, args, out_dev, path: str) -> None:
    """The one place a loop saves its uint8 H x W x 3 DEVICE result (synchronises): with --device_jpeg a .jpg / .jpeg output is encoded
    on the device and its bytes are written; everything else is copied to the host and saved by Pillow as before."""
    if device_jpeg_wanted(args, path):
        data = wct.jpeg_encode(out_dev, args.jpeg_quality)
        with open(path, "wb") as f:
            f.write(data)
    else:
        save_host_u8(args, out_dev.cpu().numpy(), path)   # .cpu() syncs


def run_proxy(args, wct, pairs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--proxy_scale: the reference's loop with wct_stylize_proxy in the cascade's place, one pair at a time; the uint8 conversion is
    fused into the slice.  Returns (total seconds, pairs)."""
    on_device = _device_images(8)

    def stylise(c_f32, s_u8):
        return _recompute_fp32(wct, logprinter, "pair", lambda fresh: wct.stylize_proxy(
            c_f32, _to_tensor(wct, s_u8, args.style_size), args.proxy_scale, args.proxy_cell, args.proxy_bins, args.proxy_eps, args.proxy_smooth,
            args.alpha, args.num_run, u8=True, round_mode=args.round_mode))

    def job(i, cfile, sfile):
        imname = pair_name(cfile, sfile)
        return Job(' #%s: Transferring "%s" (proxy: divisor %d, cell %d, %d bins, eps %g, smooth %d)' % (
                       i, imname, args.proxy_scale, args.proxy_cell, args.proxy_bins, args.proxy_eps, args.proxy_smooth),
                   os.path.join(content_dir, cfile), lambda c_u8: on_device(os.path.join(style_dir, sfile)), stylise, out_name(args, imname))

    return _run_jobs(args, wct, logprinter, [job(i, c, s) for i, (c, s) in enumerate(pairs)]), len(pairs)


VIDEO_FLAGS = (("temporal_rate", "--temporal_rate"), ("scene_cut", "--scene_cut"), ("temporal_blend", "--temporal_blend"),
               ("temporal_sigma", "--temporal_sigma"), ("temporal_radius", "--temporal_radius"))


def video_frames(content_dir: str, content_mark: str = ".") -> List[str]:
    """The frames of --video: the picked content files sorted by NAME (os.listdir's order is the file system's)."""
    return sorted(x for x in os.listdir(content_dir) if is_image_file(x) and content_mark in x)


def check_video_args(args, frame_shapes=None) -> None:
    """--video and its five parameters: a plain content x style run of the affine cascade with a model the clip supports; --transform,
    --alpha, --numpy and --round go with it.  Fills in the defaults.  frame_shapes: [(file, (H, W)), ...] of the frames after
    --content_size, when known -- one clip has one size, so a frame that differs from the first is refused by name."""
    from .lib import CLIP_BLEND, CLIP_CUT, CLIP_MAX_RADIUS, CLIP_RADIUS, CLIP_RATE, CLIP_SIGMA
    if not getattr(args, "video", False):
        for attr, name in VIDEO_FLAGS:
            if getattr(args, attr, None) is not None:
                raise ValueError("%s does nothing without --video" % name)
        return
    clash = [name for flag, name in ((args.synthesis, "--synthesis"), (args.maskPath is not None, "--maskPath"),
                                     (args.interp_styles is not None, "--interp_styles"), (args.weightPath is not None, "--weightPath"),
                                     (getattr(args, "swap_level", None), "--swap_level"), (getattr(args, "level_scale", None), "--level_scale"),
                                     (getattr(args, "auto_regions", None), "--auto_regions"),
                                     (getattr(args, "preserve_color", None), "--preserve_color"),
                                     (getattr(args, "smooth_radius", 0), "--smooth_radius")) if flag]
    if clash:
        raise ValueError("--video does not mix with %s" % ", ".join(clash))
    if args.mode == "original" or args.mode is None:
        raise ValueError("--video needs --mode 16x or 16x_kd2sd: the un-pruned models (--mode original) may solve a frame twice, which "
                         "would track it twice (wct_stylize_clip refuses them)")
    if args.num_run != 1:
        raise ValueError("--video runs the cascade once per frame (--num_run 1), got %r" % (args.num_run,))
    for attr, default in (("temporal_rate", CLIP_RATE), ("scene_cut", CLIP_CUT), ("temporal_blend", CLIP_BLEND), ("temporal_sigma", CLIP_SIGMA),
                          ("temporal_radius", CLIP_RADIUS)):
        if getattr(args, attr, None) is None:
            setattr(args, attr, default)
    if not (0.0 < args.temporal_rate <= 1.0):
        raise ValueError("--temporal_rate: a value in (0, 1] expected, got %r" % (args.temporal_rate,))
    if not (args.scene_cut >= 0.0):
        raise ValueError("--scene_cut: a value >= 0 (or inf) expected, got %r" % (args.scene_cut,))
    if not (0.0 <= args.temporal_blend < 1.0):
        raise ValueError("--temporal_blend: a value in [0, 1) expected, got %r" % (args.temporal_blend,))
    if not (0.0 < args.temporal_sigma < float("inf")):
        raise ValueError("--temporal_sigma: a finite value > 0 expected, got %r" % (args.temporal_sigma,))
    if not (0 <= args.temporal_radius <= CLIP_MAX_RADIUS):
        raise ValueError("--temporal_radius: 0 .. %d expected, got %r" % (CLIP_MAX_RADIUS, args.temporal_radius))
    if frame_shapes:
        first_file, first = frame_shapes[0]
        for name, shape in frame_shapes[1:]:
            if tuple(shape) != tuple(first):
                raise ValueError("--video: frame %s is %dx%d, the first frame %s is %dx%d -- one sequence has one size"
                                 % (name, shape[1], shape[0], first_file, first[1], first[0]))


MOTION_FLAGS = (("motion", "--motion"), ("motion_levels", "--motion_levels"), ("motion_range", "--motion_range"),
                ("motion_penalty", "--motion_penalty"))


def check_motion_args(args) -> None:
    """--motion and its three parameters: they go with --video only, and the parameters with --motion only.  Fills in the defaults."""
    from .lib import MOTION_LEVELS, MOTION_MAX_LEVELS, MOTION_MAX_RANGE, MOTION_PENALTY, MOTION_RANGE
    given = [name for attr, name in MOTION_FLAGS if getattr(args, attr, None) is not None and getattr(args, attr) is not False]
    if not getattr(args, "video", False):
        if given:
            raise ValueError("%s does nothing without --video" % given[0])
        return
    if not getattr(args, "motion", False):
        if given:
            raise ValueError("%s does nothing without --motion" % given[0])
        return
    for attr, default in (("motion_levels", MOTION_LEVELS), ("motion_range", MOTION_RANGE), ("motion_penalty", MOTION_PENALTY)):
        if getattr(args, attr, None) is None:
            setattr(args, attr, default)
    if not (1 <= args.motion_levels <= MOTION_MAX_LEVELS):
        raise ValueError("--motion_levels: 1 .. %d expected, got %r" % (MOTION_MAX_LEVELS, args.motion_levels))
    if not (0 <= args.motion_range <= MOTION_MAX_RANGE):
        raise ValueError("--motion_range: 0 .. %d expected, got %r" % (MOTION_MAX_RANGE, args.motion_range))
    if not (0 <= args.motion_penalty <= 255):
        raise ValueError("--motion_penalty: 0 .. 255 expected, got %r" % (args.motion_penalty,))


def video_jobs(args, content_dir, style_dir) -> Tuple[List[str], List[str]]:
    """(frames, styles) of --video, both sorted by name."""
    return (video_frames(content_dir, args.picked_content_mark),
            sorted(x for x in os.listdir(style_dir) if is_image_file(x) and args.picked_style_mark in x))


def run_video(args, wct, jobs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--video: per style one clip -- the style prepared once, then the frames in name order through wct_stylize_clip, one at a time;
    one image per (frame, style) of video_jobs() under the usual name.  Returns (summed per-frame time, frames written)."""
    from PIL import Image
    frames, styles = jobs
    if not frames or not styles:
        return 0.0, 0
    shapes = []
    for f in frames:
        with Image.open(os.path.join(content_dir, f)) as im:
            shapes.append((f, resized_shape(im.size[1], im.size[0], args.content_size)))
    check_video_args(args, shapes)
    check_motion_args(args)
    motion = dict(levels=args.motion_levels, range=args.motion_range, penalty=args.motion_penalty) if getattr(args, "motion", False) else None
    motion_note = ", motion: levels %d, range %d, penalty %d" % (args.motion_levels, args.motion_range, args.motion_penalty) if motion else ""
    H, W = shapes[0][1]
    avg, n = 0.0, 0
    for sfile in styles:
        wct.style_prepare(_to_tensor(wct, _upload_u8(os.path.join(style_dir, sfile)), args.style_size))
        if getattr(args, "diversity", None):          # once per clip: every frame is coloured through the same rotation
            wct.style_diversify(args.diversity, args.seed, 0, args.diversity_levels)
        clip =wct.clip(H, W, args.temporal_rate, args.scene_cut, args.temporal_blend, args.temporal_sigma, args.temporal_radius, motion=motion)
        try:
            for i, cfile in enumerate(frames):
                imname = pair_name(cfile, sfile)
                logprinter("\n" + "*" * 30 + ' #%s: Transferring "%s" (video: rate %g, cut %g, blend %g%s)' % (
                    i, imname, args.temporal_rate, args.scene_cut, args.temporal_blend, motion_note))
                c_u8 = _upload_u8(os.path.join(content_dir, cfile))
                t0 = time.time()
                c_f32 = _to_tensor(wct, c_u8, args.content_size)
                _, hwc = clip.stylize(c_f32, args.alpha, u8=True, round_mode=args.round_mode)
                if wct.saturation_count(reset=True):   # syncs
                    logprinter("WARNING: f16x3 range exceeded in this frame: its result deviates from the fp32 reference")
                save_u8(wct, args, hwc, out_name(args, imname))
                dt = time.time() - t0
                avg += dt
                n += 1
                logprinter("Elapsed time is: %.4f seconds" % dt)
        finally:
            clip.close()
    return avg, n


def _finish_u8(wct, args, res, c_f32):
    """The result as uint8 HWC on the device: save_image's conversion, fused into whichever kernel comes last -- the guided filter of
    --smooth_radius, then the luminance merge of --preserve_color luma, both against the content tensor the cascade was given."""
    luma = getattr(args, "preserve_color", None) == "luma"
    radius = getattr(args, "smooth_radius", 0)
    if getattr(args, "proxy_scale", None):
        return res          # the slice of --proxy_scale has converted it already (it goes with neither post-step)
    if radius:
        if not luma:
            return wct.guided_filter(res, c_f32, radius, args.smooth_eps, u8=True, round_mode=args.round_mode)
        res = wct.guided_filter(res, c_f32, radius, args.smooth_eps)
    if luma:
        return wct.luma_merge(res, c_f32, u8=True, round_mode=args.round_mode)
    return wct.to_u8(res, args.round_mode)


def interp_style_list(args) -> List[str]:
    return [p for p in args.interp_styles.split(",") if p]


def interp_weight_list(args) -> List[float]:
    """--interp_weights as floats."""
    return [float(v) for v in args.interp_weights.split(",") if v.strip()]


def check_interp_args(args) -> None:
    if args.interp_styles is None:
        if args.interp_weights is not None:
            raise ValueError("--interp_weights needs --interp_styles")
        if args.weightPath is not None:
            raise ValueError("--weightPath needs --interp_styles")
        return
    if args.maskPath is not None:
        raise ValueError("--interp_styles does not mix with --maskPath")
    n = len(interp_style_list(args))
    if not 1 <= n <= 8:
        raise ValueError("--interp_styles: 1 to 8 style images, got %d" % n)
    if args.weightPath is not None:
        if args.interp_weights is not None:
            raise ValueError("--interp_weights does not mix with --weightPath (the weight maps are the weights)")
        return
    if args.interp_weights is None:
        raise ValueError("--interp_styles goes with --interp_weights (one weight per style) or --weightPath (weight maps)")
    try:
        lam = interp_weight_list(args)
    except ValueError:
        raise ValueError("--interp_weights: comma-separated numbers expected, got %r" % args.interp_weights) from None
    if len(lam) != n:
        raise ValueError("--interp_weights: one weight per style image: %d styles, %d weights" % (n, len(lam)))
    if any(not math.isfinite(v) or v < 0 for v in lam) or not sum(lam) > 0:
        raise ValueError("--interp_weights: weights must be finite and >= 0 with a positive sum, got %s" % args.interp_weights)


def weight_jobs(content_dir: str, weight_dir: str, K: int, content_mark: str = ".") -> List[Tuple[str, List[str]]]:
    """--weightPath: every content X.* (listdir order, --picked_content_mark) with its K weight maps DIR/X_k.png (X = text before the
    first dot, as pair_name); a missing map is an error that names the file."""
    jobs = []
    for c in os.listdir(content_dir):
        if not (is_image_file(c) and content_mark in c):
            continue
        stem = c.split(".")[0]
        maps = [os.path.join(weight_dir, "%s_%d.png" % (stem, k)) for k in range(K)]
        for m in maps:
            if not os.path.isfile(m):
                raise FileNotFoundError("weight map %s for content %s not found" % (m, c))
        jobs.append((c, maps))
    return jobs


def load_weights(paths: List[str], shape: Tuple[int, int]):
    """K weight maps as float32 K x H x W: mode L PNGs, weight = value / 255, at the content's size after --content_size (`shape`);
    never resampled."""
    import numpy as np
    from PIL import Image
    out = np.empty((len(paths),) + tuple(shape), np.float32)
    for k, path in enumerate(paths):
        img = Image.open(path)
        if img.mode != "L":
            raise ValueError("weight map %s has mode %s; expected L (weight = value / 255)" % (path, img.mode))
        a = np.array(img, dtype=np.uint8)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("weight map %s is %dx%d (HxW) but the content is %dx%d after --content_size; weight maps are not resampled"
                             % (path, a.shape[0], a.shape[1], shape[0], shape[1]))
        out[k] = a.astype(np.float32) / np.float32(255)
    return out


def interp_out_name(args, content_file: str, blend: bool = False) -> str:
    """<log_mark>_mode=<m>_alpha=<a>_<X>+interp.jpg (+blend.jpg with --weightPath)."""
    return out_name(args, content_file.split(".")[0] + ("+blend.jpg" if blend else "+interp.jpg"))


def interp_jobs(args, content_dir, style_dir)-> List[Tuple[str, Optional[List[str]]]]:
    """--interp_styles: every picked content (listdir order), with its weight maps under --weightPath (weight_jobs) or None."""
    if args.weightPath is not None:
        return weight_jobs(content_dir, args.weightPath, len(interp_style_list(args)), args.picked_content_mark)
    return [(c, None) for c in os.listdir(content_dir) if is_image_file(c) and args.picked_content_mark in c]


def run_interp(args, wct, jobs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--interp_styles: one stylisation per content of interp_jobs() against the blend of the styles (wct_stylize_interp) or, with
    --weightPath, with per-pixel weights (wct_stylize_blend); the serial loop.  Returns (total seconds, contents)."""
    styles = interp_style_list(args)

    def convert():
        return [_to_tensor(wct, _upload_u8(p), args.style_size) for p in styles]

    s_dev = convert()       # once per run, outside every job's timer
    blend = args.weightPath is not None
    lam = None if blend else interp_weight_list(args)

    def weight_maps(wpaths):
        return lambda c_u8: _on_device(load_weights(wpaths, resized_shape(int(c_u8.shape[0]), int(c_u8.shape[1]), args.content_size)))

    def stylise(c_f32, wmap):
        def once(fresh):
            st = convert() if fresh else s_dev      # the recompute reads and converts the styles again
            if blend:
                return wct.stylize_blend(c_f32, st, wmap, args.alpha, args.num_run)
            return wct.stylize_interp(c_f32, st, lam, args.alpha, args.num_run)
        return _recompute_fp32(wct, logprinter, "content", once)

    return _run_jobs(args, wct, logprinter, [
        Job(' #%s: Transferring "%s" by %s' % (i, cfile, "weight maps" if blend else "interpolation"), os.path.join(content_dir, cfile),
            weight_maps(wpaths) if blend else None, stylise, interp_out_name(args, cfile, blend)) for i, (cfile, wpaths) in enumerate(jobs)]), len(jobs)


def synthesis_shape(H: int, W: int, size: int) -> Tuple[int, int]:
    """(H, W) of a texture after the resize of data_loader.py:64-72: the LONGER edge becomes `size` (the second branch when they are
    equal), the other int(short * size / long) -- Python's float division, then truncation; applied even when the long edge already
    equals `size`; size 0 = no resize.  An edge that comes out as 0 is an error."""
    if not size:
        return H, W
    if W > H:
        neww = size
        newh = int(H * neww / W)
    else:
        newh = size
        neww = int(W * newh / H)
    if newh < 1 or neww < 1:
        raise ValueError("--style_size %d turns a %dx%d (WxH) texture into %dx%d" % (size, W, H, neww, newh))
    return newh, neww


def texture_jobs(texture_dir: str) -> List[str]:
    """data_loader.py:28: the images of --texturePath in os.listdir order (no --picked_* filter)."""
    return [x for x in os.listdir(texture_dir) if is_image_file(x)]


def synthesis_out_name(args, texture_file: str) -> str:
    """data_loader.py:76 + WCT.py:127: <log_mark>_mode=<m>_alpha=<a>_<texture stem>.jpg (stem = text before the FIRST dot)."""
    return out_name(args, texture_file.split(".")[0] + ".jpg")


def synthesis_size(text: str) -> Tuple[int, int]:
    """--synthesis_size 'WxH' -> (H, W)."""
    parts = text.lower().split("x")
    try:
        w, h = (int(v) for v in parts)
    except ValueError:
        raise ValueError("--synthesis_size: WxH expected (e.g. 3840x2160), got %r" % text) from None
    if w < 1 or h < 1:
        raise ValueError("--synthesis_size: positive WxH expected, got %r" % text)
    return h, w


def synthesis_noise_shape(H: int, W: int) -> Tuple[int, int]:
    """The noise size behind a --synthesis_size H x W file: the cascade returns 16 floor(edge / 16) (floor pooling at every level), so
    the noise takes the next multiples of 16 and the result is cropped to H x W."""
    return (H + 15) // 16 * 16, (W + 15) // 16 * 16


def check_synthesis_args(args) -> None:
    if not args.synthesis:
        if args.seed != 0 and getattr(args, "diversity", None) is None:
            raise ValueError("--seed needs --synthesis or --diversity")
        if args.synthesis_size is not None:
            raise ValueError("--synthesis_size needs --synthesis")
        return
    for flag, name in ((args.maskPath, "--maskPath"), (args.interp_styles, "--interp_styles"), (args.weightPath, "--weightPath")):
        if flag is not None:
            raise ValueError("--synthesis does not mix with %s" % name)
    if not 0 <= args.seed < 1 << 64:
        raise ValueError("--seed: 0 .. 2^64 - 1 expected, got %d" % args.seed)
    if args.synthesis_size is not None:
        synthesis_size(args.synthesis_size)


def run_synthesis(args, wct, jobs, content_dir, style_dir, logprinter) -> Tuple[float, int]:
    """--synthesis: one image per texture of texture_jobs() (wct_synthesize: noise of --seed and stream id = the texture's index as
    the content, the texture as the style); the serial loop.  There is no content: the job's pre-timer step uploads the texture, and
    _finish_u8 is the plain uint8 conversion (--preserve_color and --smooth_radius are refused).  Returns (total seconds, textures)."""
    size = synthesis_size(args.synthesis_size) if args.synthesis_size is not None else None

    def job(i, tfile):
        def stylise(_, t_u8):
            if args.style_size:
                t_f32 = wct.resize_u8(t_u8, synthesis_shape(int(t_u8.shape[0]), int(t_u8.shape[1]), args.style_size), to_tensor=True, filter="bicubic")
            else:
                t_f32 = wct.to_tensor_u8(t_u8)
            H, W = synthesis_noise_shape(*size) if size is not None else (int(t_f32.shape[2]), int(t_f32.shape[3]))

            def once(fresh):        # nothing to remake: the recompute reuses the texture tensor
                res = wct.synthesize(t_f32, H, W, seed=args.seed, stream_id=i, alpha=args.alpha, num_run=args.num_run)
                return res[:, :, :size[0], :size[1]] if size is not None else res
            return _recompute_fp32(wct, logprinter, "texture", once)

        return Job(' #%s: Transferring "%s"' % (i, tfile.split(".")[0] + ".jpg"), None,
                   lambda _: _upload_u8(os.path.join(args.texturePath, tfile)), stylise, synthesis_out_name(args, tfile))

    return _run_jobs(args, wct, logprinter, [job(i, t) for i, t in enumerate(jobs)]), len(jobs)


class LogPrinter:     # WCT.py:78-82
    def __init__(self, debug: bool, path: str):
        self.log = sys.stdout if debug else open(path, "a+")

    def __call__(self, sth):
        print(str(sth), file=self.log, flush=True)


def _to_tensor(wct, u8, size):
    """Resize (data_loader.py:52-56) + ToTensor (:57-58) on the GPU from the decoded uint8 frame."""
    return wct.resize_u8(u8, size, to_tensor=True) if size else wct.to_tensor_u8(u8)


def _fp32_fallback(wct, args, logprinter, c_f32, style_u8_dev):
    """An activation left the f16x3 range (+-65504) and was clamped: a deviation from the fp32 reference -- never silent.
    Recompute this pair with the exact-fp32 convolutions (style statistics included), under the same colour control (--preserve_color
    match here; luma is applied by the caller's _finish_u8)."""
    logprinter("WARNING: f16x3 range exceeded for this pair -> recomputing it with exact-fp32 convolutions")
    wct.set_conv_mode("fp32")
    try:
        if getattr(args, "preserve_color", None) == "match":
            res = wct.stylize_color(c_f32, _to_tensor(wct, style_u8_dev, args.style_size), "match", args.alpha, args.num_run)
        else:
            res = wct.stylize(c_f32, _to_tensor(wct, style_u8_dev, args.style_size), args.alpha, args.num_run)
        wct.sync()
    finally:
        wct.set_conv_mode("f16x3")
    return res


def _recompute_fp32(wct, logprinter, noun, once, sync=True):
    """The result of once(False) -- or, when that pass clamped an activation at the f16x3 range (+-65504), of once(True) under the
    exact-fp32 convolutions: never a silent deviation from the fp32 reference.  `once(fresh)` stylises one `noun` (pair, content,
    texture); fresh = make the style tensors anew.  sync: wct.sync() behind the second pass -- it raises OverflowError if that one
    clamped too.  The engine is back in f16x3 however the recompute ends."""
    res = once(False)
    if wct.saturation_count(reset=True):
        logprinter("WARNING: f16x3 range exceeded for this %s -> recomputing it with exact-fp32 convolutions" % noun)
        wct.set_conv_mode("fp32")
        try:
            res = once(True)
            if sync:
                wct.sync()
        finally:
            wct.set_conv_mode("f16x3")
    return res


def _on_device(array, pin=False):
    """A host array on the device; pin = through pinned memory, asynchronously."""
    import torch
    t = torch.from_numpy(array)
    return t.pin_memory().cuda(non_blocking=True) if pin else t.cuda()


# --device_decode: the decoder of the running main(), set once its engine exists and cleared in main()'s finally (None: Pillow decodes
# everything); _upload_u8, which its many callers give a path and nothing else, and run_pipelined's decode ask it
_DEVICE_DECODER = None


class DeviceDecoder:
    """The host side of --device_decode.  read(path), in any thread: (info, pinned segment) of a .jpg / .jpeg file the device decoder
    takes; Pillow's uint8 H x W x 3 array, decoded from the bytes already read, of one it does not take (logged once per file); None
    for any other file and for one the device has refused before.  enqueue(item), in the main thread: the uint8 H x W x 3 device
    image and a pinned status word that is valid once the stream has passed this point."""
    STATUS = {1: "the synchronisation did not converge (status UNSYNC)", 2: "the scan is not what its header promises (status CORRUPT)"}

    def __init__(self, wct, logprinter):
        self.wct, self.log = wct, logprinter
        self.host_only = set()
        self.lock = threading.Lock()

    def refuse(self, path, why):
        with self.lock:
            if path not in self.host_only:
                self.host_only.add(path)
                self.log("--device_decode: %s: %s; Pillow decodes it" % (path, why))

    def read(self, path):
        import io
        import numpy as np
        import torch
        from PIL import Image
        if not is_jpeg_file(path) or path in self.host_only:
            return None
        with open(path, "rb") as f:
            data = f.read()
        info = self.wct.jdec_parse(data)
        if info is None or not info.scan_length:
            self.refuse(path, "not a baseline file the device decoder takes")
            return np.array(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)     # load_rgb_u8 of the same bytes
        seg = np.frombuffer(data, np.uint8, int(info.scan_length), int(info.scan_offset)).copy()
        return info, torch.from_numpy(seg).pin_memory()

    def enqueue(self, item):
        import torch
        info, seg = item
        out, status = self.wct.jdec_decode_async(seg.cuda(non_blocking=True), info)
        host = torch.zeros(1, dtype=torch.int32).pin_memory()
        host.copy_(status, non_blocking=True)
        return out, host


def _upload_u8(path):
    """Decode `path` to uint8 HWC and send it off to the device: a decoded frame crosses PCIe as it is (3 B/px, pinned); Resize and
    ToTensor run on the GPU.  With --device_decode a baseline .jpg / .jpeg file crosses as its compressed segment and is decoded
    there (synchronises for the status: a file the device does not finish is decoded by Pillow)."""
    d = _DEVICE_DECODER
    item = d.read(path) if d is not None else None
    if item is not None and not isinstance(item, tuple):
        return _on_device(item, pin=True)
    if item is not None:
        import torch
        out, host = d.enqueue(item)
        torch.cuda.current_stream().synchronize()
        if int(host[0]) == 0:
            return out
        d.refuse(path, d.STATUS.get(int(host[0]), "status %d" % int(host[0])))
    return _on_device(load_rgb_u8(path), pin=True)


def _device_images(limit):
    """fetch(path): _upload_u8(path), keeping the last `limit` images on the device (the oldest is dropped first)."""
    held = {}

    def fetch(path):
        u8 = held.get(path)
        if u8 is None:
            u8 = held[path] = _upload_u8(path)
            while len(held) > limit:
                held.pop(next(iter(held)))
        return u8
    return fetch


# One job of the serial loop: header = its log line behind the asterisks; content = the content's path (None: there is none);
# before(c_u8) = an optional step after the upload and outside the timer, whose result goes to stylise (label map, weight maps, the
# pair's decoded style); stylise(c_f32, that result) = the cascade with its fp32 recompute (_recompute_fp32); out = the file to write.
Job = collections.namedtuple("Job", "header content before stylise out")


def _run_jobs(args, wct, logprinter, jobs) -> float:
    """The reference's loop (WCT.py:112-131) for every mode that takes one job at a time; its timer covers the conversion of the content,
    the cascade and the save.  Returns the summed per-job time."""
    from PIL import Image
    total = 0.0
    for job in jobs:
        logprinter("\n" + "*" * 30 + job.header)
        c_u8 = _upload_u8(job.content) if job.content else None
        extra = job.before(c_u8) if job.before else None
        t0 = time.time()
        c_f32 = _to_tensor(wct, c_u8, args.content_size) if job.content else None
        res = job.stylise(c_f32, extra)
        save_u8(wct, args, _finish_u8(wct, args, res, c_f32), job.out)   # syncs
        dt = time.time() - t0
        total += dt
        logprinter("Elapsed time is: %.4f seconds" % dt)
    return total


def run_serial(args, wct, pairs, content_dir, style_dir, logprinter) -> float:
    """The reference's loop (WCT.py:112-131), one pair at a time; returns the summed per-pair time (cascade + save, like its timer)."""
    from PIL import Image
    avg = 0.0
    # style statistics are computed once per style image and reused for every content it is paired with
    # (data_loader.py:32-36 builds the content x style product; the reference re-encodes the style for every pair)
    style_cache = {}
    # --preserve_color match: the matched style depends on the content, so there are no statistics to cache -- every pair matches and
    # prepares its own style (wct_stylize_color); the decoded style stays on the device (uint8, the last few) instead
    match = getattr(args, "preserve_color", None) == "match"
    on_device = _device_images(8)
    for i, (cfile, sfile) in enumerate(pairs):
        imname = pair_name(cfile, sfile)
        logprinter("\n" + "*" * 30 + ' #%s: Transferring "%s"' % (i, imname))
        c_u8 = _upload_u8(os.path.join(content_dir, cfile))
        if match:
            s_u8 = on_device(os.path.join(style_dir, sfile))
        else:
            s_u8 = _upload_u8(os.path.join(style_dir, sfile)) if sfile not in style_cache else None
        t0 = time.time()
        if match:
            c_f32 = _to_tensor(wct, c_u8, args.content_size)
            res = wct.stylize_color(c_f32, _to_tensor(wct, s_u8, args.style_size), "match", args.alpha, args.num_run)
        elif s_u8 is not None:
            wct.style_prepare(_to_tensor(wct, s_u8, args.style_size))
            style_cache[sfile] = {L: wct.style_export(L) for L in (5, 4, 3, 2, 1)}
        else:
            for L, stats in style_cache[sfile].items():
                wct.style_import(L, stats)
        if not match:
            c_f32 = _to_tensor(wct, c_u8, args.content_size)
            res = wct.stylize_prepared(c_f32, args.alpha, args.num_run)
        if wct.saturation_count(reset=True):
            if s_u8 is None:
                s_u8 = _upload_u8(os.path.join(style_dir, sfile))
            res = _fp32_fallback(wct, args, logprinter, c_f32, s_u8)
            style_cache.pop(sfile, None)          # its cached statistics may carry the clamp too
        save_u8(wct, args, _finish_u8(wct, args, res, c_f32), out_name(args, imname))   # syncs
        dt = time.time() - t0
        avg += dt
        logprinter("Elapsed time is: %.4f seconds" % dt)
    return avg


def run_pipelined(args, wct, pairs, content_dir, style_dir, logprinter) -> float:
    """The same pairs, the same engine, the same GPU work in the same order -- with the host work taken off the GPU's critical path:
      decode pool   PIL decode + copy into pinned memory of the next pairs' files (both release the GIL), `--io_threads` wide
      main thread   H2D (async), style statistics (once per style) / import, cascade, uint8 conversion, D2H (async) + an event
      writer pool   waits for a pair's event, Image.save (JPEG encode releases the GIL)
    At most `--pipeline` pairs are between "enqueued on the GPU" and "handed to a writer".  The f16x3 range flag of pair i is read
    (counter in stream order, copied with the image) when the pair leaves that window; a clamped pair is recomputed in exact fp32
    and everything enqueued after it is discarded and redone (its style statistics may carry the clamp) -- the serial loop's
    results.  Returns the wall time of the whole run."""
    import concurrent.futures as cf
    import torch
    from PIL import Image
    n = len(pairs)
    depth = max(1, int(args.pipeline))
    io = max(1, int(args.io_threads))
    ahead = depth + io                                # pairs whose files are decoded (or being decoded) ahead of the GPU
    dec = cf.ThreadPoolExecutor(io, thread_name_prefix="wct-decode")
    wr = cf.ThreadPoolExecutor(io, thread_name_prefix="wct-write")

    jdec = _DEVICE_DECODER

    def decode(path):
        """Pool thread: the pinned image, or -- --device_decode, a file the device takes -- its parsed header and pinned segment."""
        item = jdec.read(path) if jdec is not None else None
        if isinstance(item, tuple):
            return item
        return torch.from_numpy(item if item is not None else load_rgb_u8(path)).pin_memory()

    def upload(item, path, pending):
        """Main thread: the uint8 device image of what decode() returned; a device decode leaves (path, pinned status) in `pending`."""
        if isinstance(item, tuple):
            out, host = jdec.enqueue(item)
            pending.append((path, host))
            return out
        return item.cuda(non_blocking=True)

    copy_streams = threading.local()

    def stage(rec, out_dev):
        """What of a pair's result goes to the host behind its event: the image for Pillow, or -- a .jpg / .jpeg output with
        --device_jpeg -- only the length of the file that the device encodes; the writer then copies exactly that many bytes."""
        if device_jpeg_wanted(args, rec["path"]):
            rec["jpeg_dev"], length = wct.jpeg_encode_async(out_dev, args.jpeg_quality)
            rec["len_host"] = torch.zeros(1, dtype=torch.int64).pin_memory()
            rec["len_host"].copy_(length, non_blocking=True)
            rec["jpeg_keep"] = length
        else:
            rec["host"] = torch.empty(out_dev.shape, dtype=torch.uint8, pin_memory=True)
            rec["host"].copy_(out_dev, non_blocking=True)

    def save(rec):
        rec["ev"].synchronize()
        if "jpeg_dev" in rec:
            n = int(rec["len_host"][0])
            if n < 0:
                raise RuntimeError("--device_jpeg: %s overflowed the encoder's own bound" % rec["path"])
            if not hasattr(copy_streams, "s"):
                copy_streams.s = torch.cuda.Stream()      # this writer's own: the copy must not queue behind the next pairs' cascades
            host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.stream(copy_streams.s):
                host.copy_(rec["jpeg_dev"][:n], non_blocking=True)
            copy_streams.s.synchronize()
            with open(rec["path"], "wb") as f:
                f.write(host.numpy().tobytes())
            rec.pop("jpeg_dev")
        else:
            save_host_u8(args, rec["host"].numpy(), rec["path"])
        return time.time()

    match = getattr(args, "preserve_color", None) == "match"     # per-pair matched styles (wct_stylize_color): no statistics cache, style_dev is the cache
    strict = wct.strict_range
    wct.strict_range = False                          # the flag is read per pair below, never raised in the middle of the window
    t_start = time.time()
    fut = {}                                          # ("c" | "s", file) -> decode future
    style_cache = {}                                  # sfile -> {level: statistics}
    style_dev = {}                                    # sfile -> uint8 device image while pairs using it may still need the fp32 fallback
    style_by = {}                                     # sfile -> index of the pair whose style_prepare produced the cached statistics
    inflight = collections.deque()
    writes = []
    last_flag = 0.0
    nxt = 0
    done_log = t_start

    def want(i):
        for j in range(i, min(n, i + ahead)):
            cfile, sfile = pairs[j]
            if ("c", cfile) not in fut:
                fut[("c", cfile)] = dec.submit(decode, os.path.join(content_dir, cfile))
            if sfile not in (style_dev if match else style_cache) and ("s", sfile) not in fut:
                fut[("s", sfile)] = dec.submit(decode, os.path.join(style_dir, sfile))
        live = {("c", pairs[j][0]) for j in range(i, min(n, i + ahead))} | {("s", pairs[j][1]) for j in range(i, min(n, i + ahead))}
        for k in [k for k in fut if k not in live]:
            del fut[k]

    def retire(rec):
        """Pair leaves the window: its flag has been copied with its image."""
        nonlocal last_flag, nxt, done_log
        rec["ev"].synchronize()
        bad = [(p, int(h[0])) for p, h in rec["jdec"] if int(h[0]) != 0]
        if bad:
            # the device did not finish one of this pair's files: nothing computed from it may be written.  Like a clamped pair, drop
            # what was enqueued behind it and the statistics prepared since; the pair itself is redone from Pillow's decode
            torch.cuda.synchronize()
            inflight.clear()
            for p, st in bad:
                jdec.refuse(p, jdec.STATUS.get(st, "status %d" % st))
            for f in [f for f, by in style_by.items() if by >= rec["i"]] + [rec["sfile"]]:
                style_cache.pop(f, None)
                style_dev.pop(f, None)
                style_by.pop(f, None)
            fut.clear()
            last_flag = float(wct.range_flag().reshape(-1)[0].item())   # a clamp of a dropped pair is dropped with it
            nxt = rec["i"]
            return
        flag = float(rec["flag_host"][0])
        if flag > last_flag:
            # clamped: redo this pair in fp32, drop what was enqueued behind it (same statistics objects) and resume after it
            torch.cuda.synchronize()
            inflight.clear()
            wct.saturation_count(reset=True)          # acknowledged: the counter restarts at zero
            sfile = rec["sfile"]
            s_u8 = style_dev.get(sfile)
            if s_u8 is None:
                s_u8 = _upload_u8(os.path.join(style_dir, sfile))
            res = _fp32_fallback(wct, args, logprinter, rec["c_f32"], s_u8)
            stage(rec, _finish_u8(wct, args, res, rec["c_f32"]))
            rec["ev"] = torch.cuda.Event()
            rec["ev"].record()
            # the reset above acknowledged EVERY clamp so far, also one inside a style_prepare of a discarded pair (index > i): statistics
            # prepared by this pair or any later one are dropped with the pairs, so the redone pairs prepare them again under a live flag
            # (only the clamped pair's own style used to be dropped)
            for f in [f for f, by in style_by.items() if by >= rec["i"]] + [sfile]:
                style_cache.pop(f, None)
                style_dev.pop(f, None)
                style_by.pop(f, None)
            last_flag = 0.0
            nxt = rec["i"] + 1
        else:
            last_flag = flag
        rec.pop("c_f32", None)
        rec.pop("keep", None)                         # the event has passed: the GPU is done with the pair's device buffers
        writes.append(wr.submit(save, rec))
        # bound the writer queue too: a slow disk must not let pinned result buffers pile up behind Image.save
        for w in [w for w in writes if w.done()]:
            w.result()                                # (re-raises a writer's exception here, not at the end of the folder)
            writes.remove(w)
        while len(writes) > 2 * io:
            writes.pop(0).result()
        now = time.time()
        logprinter('#%s "%s" left the pipeline, %.4f seconds after the previous pair' % (rec["i"], rec["imname"], now - done_log))
        done_log = now

    try:
        while nxt < n or inflight:
            while inflight and (len(inflight) >= depth or nxt >= n):
                retire(inflight.popleft())
            if nxt >= n:
                continue
            i = nxt
            nxt += 1
            want(i)
            cfile, sfile = pairs[i]
            imname = pair_name(cfile, sfile)
            logprinter("\n" + "*" * 30 + ' #%s: Transferring "%s"' % (i, imname))
            pending = []
            c_u8 = upload(fut[("c", cfile)].result(), os.path.join(content_dir, cfile), pending)
            if match:
                s_u8 = style_dev.pop(sfile, None)
                if s_u8 is None:
                    s_u8 = upload(fut[("s", sfile)].result(), os.path.join(style_dir, sfile), pending)
                style_dev[sfile] = s_u8                     # (re-inserted: most recently used last)
                while len(style_dev) > depth + 2:
                    style_dev.pop(next(iter(style_dev)))
            elif sfile not in style_cache:
                s_u8 = upload(fut[("s", sfile)].result(), os.path.join(style_dir, sfile), pending)
                style_dev[sfile] = s_u8
                while len(style_dev) > depth + 2:           # the fallback reloads a style it no longer finds here: keep the few that can be in flight
                    style_dev.pop(next(iter(style_dev)))
                wct.style_prepare(_to_tensor(wct, s_u8, args.style_size))
                style_cache[sfile] = {L: wct.style_export(L) for L in (5, 4, 3, 2, 1)}
                style_by[sfile] = i
            else:
                for L, stats in style_cache[sfile].items():
                    wct.style_import(L, stats)
            c_f32 = _to_tensor(wct, c_u8, args.content_size)
            if match:
                s_f32 = _to_tensor(wct, s_u8, args.style_size)
                res = wct.stylize_color(c_f32, s_f32, "match", args.alpha, args.num_run)
            else:
                s_f32 = None
                res = wct.stylize_prepared(c_f32, args.alpha, args.num_run)
            out_dev = _finish_u8(wct, args, res, c_f32)
            rec = {"i": i, "imname": imname, "path": out_name(args, imname), "sfile": sfile, "c_f32": c_f32, "keep": (out_dev, res, c_u8, s_f32),
                   "jdec": pending}
            stage(rec, out_dev)
            flag_host = torch.zeros(1, dtype=torch.float64).pin_memory()
            flag_host.copy_(wct.range_flag(), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            rec.update(flag_host=flag_host, ev=ev)
            inflight.append(rec)
        for w in writes:
            w.result()
    finally:
        wct.strict_range = strict
        dec.shutdown(wait=True)
        wr.shutdown(wait=True)
    return time.time() - t_start


def pair_jobs(args, content_dir, style_dir) -> List[Tuple[str, str]]:
    return list_pairs(content_dir, style_dir, args.picked_content_mark, args.picked_style_mark)


def _number_of(what):
    return lambda jobs: "Number of %s: %s" % (what, len(jobs))


# The modes that take one job at a time, in their order of precedence; whatever none of them takes is a plain run (run_pipelined or
# run_serial).  chosen(args): this mode runs; reason: the rest of its "--pipeline is ignored with" line; jobs(args, content_dir,
# style_dir) and early: its job list and when main() makes it; number(jobs): its "Number of" line; noun: what the closing average is
# per; run(args, wct, jobs, content_dir, style_dir, logprinter) -> (total seconds, images written).
Mode = collections.namedtuple("Mode", "name chosen reason jobs early number noun run")
MODES = (
    Mode("synthesis", lambda a: a.synthesis, "--synthesis: texture synthesis uses the serial loop",
         lambda a, c, s: texture_jobs(a.texturePath), False, _number_of("content-style pairs"), "pair", run_synthesis),
    Mode("regions", lambda a: a.maskPath is not None, "--maskPath: region runs use the serial loop",
         lambda a, c, s: region_jobs(c, a.maskPath, a.picked_content_mark), True, _number_of("contents with label maps"), "image", run_regions),
    Mode("interp", lambda a: a.interp_styles is not None, "--interp_styles: interpolation and weight-map runs use the serial loop",
         interp_jobs, False, _number_of("contents"), "image", run_interp),
    Mode("video", lambda a: a.video, "--video: a sequence is stylised frame by frame, each against the one before",
         video_jobs, False, lambda jobs: "Number of frames: %s, styles: %s" % (len(jobs[0]), len(jobs[1])), "frame", run_video),
    Mode("swap", lambda a: a.swap_level, "--swap_level: patch-swap runs use the serial loop",
         pair_jobs, True, _number_of("content-style pairs"), "pair", run_swap),
    Mode("scale", lambda a: a.level_scale, "--level_scale: scale-controlled runs use the serial loop",
         pair_jobs, True, _number_of("content-style pairs"), "pair", run_scale),
    Mode("auto", lambda a: a.auto_regions, "--auto_regions: feature-region runs use the serial loop",
         pair_jobs, True, _number_of("content-style pairs"), "pair", run_auto),
)


# --diversity is a variation of the plain run, not of any mode above (of those only --video goes with it, and keeps its own loop): it is
# looked at last, behind the table
DIVERSE_MODE = Mode("diverse", lambda a: getattr(a, "diversity", None), "--diversity: variations of a pair use the serial loop",
                    pair_jobs, True, _number_of("content-style pairs"), "image", run_diverse)


# --proxy_scale mixes with none of the above (check_proxy_args): like --diversity it is looked at behind the table
PROXY_MODE = Mode("proxy", lambda a: getattr(a, "proxy_scale", None), "--proxy_scale: proxy runs use the serial loop",
                  pair_jobs, True, _number_of("content-style pairs"), "pair", run_proxy)


def select_mode(args) -> Optional[Mode]:
    """The first mode of MODES that `args` choose, then --diversity, then --proxy_scale; None for a plain content x style run."""
    return next((m for m in MODES + (DIVERSE_MODE, PROXY_MODE) if m.chosen(args)), None)


def main(argv: Optional[List[str]] = None) -> int:
    args = build_parser().parse_args(argv)
    checkpoint_args(args)
    check_region_args(args)
    check_interp_args(args)
    check_synthesis_args(args)
    check_color_args(args)
    check_smooth_args(args)
    check_transform_args(args)
    check_swap_args(args)
    check_scale_args(args)
    check_auto_args(args)
    check_video_args(args)
    check_motion_args(args)
    check_diverse_args(args)
    check_proxy_args(args)
    check_jpeg_args(args)
    global _DEVICE_DECODER
    try:
        return _run(args)
    finally:
        _DEVICE_DECODER = None      # however the run ends: the decoder holds the engine


def _run(args) -> int:
    """main() behind its argument checks: the log, the engine, the mode's or the plain run's loop."""
    global _DEVICE_DECODER
    os.makedirs(args.outf, exist_ok=True)
    logprinter = LogPrinter(args.debug, os.path.join(args.outf, "log_%s_%s.txt" % (args.log_mark, args.mode)))
    logprinter(sorted(vars(args).items()))
    content_dir = args.UHD_contentPath if args.UHD else args.contentPath
    style_dir = args.UHD_stylePath if args.UHD else args.stylePath
    mode = select_mode(args)
    if mode is not None:
        # early: the jobs are listed before the engine exists (a missing label map refuses the run there) and counted in the log ahead
        # of the --pipeline note; the other modes list and count theirs behind it
        jobs = mode.jobs(args, content_dir, style_dir) if mode.early else None
        from .wct import WCT
        wct = WCT(args)
        _DEVICE_DECODER = DeviceDecoder(wct, logprinter) if getattr(args, "device_decode", False) else None
        if mode.early:
            logprinter(mode.number(jobs))
        if args.pipeline > 0:
            logprinter("--pipeline is ignored with " + mode.reason)
        if not mode.early:
            jobs = mode.jobs(args, content_dir, style_dir)
            logprinter(mode.number(jobs))
        total, n = mode.run(args, wct, jobs, content_dir, style_dir, logprinter)
        if n:
            logprinter("Processed %d images. Average processing time per %s is: %.4f seconds" % (n, mode.noun, total / n))
        return 0
    pairs = pair_jobs(args, content_dir, style_dir)

    from .wct import WCT      # raises ImportError if libwct_hip.so is missing: no CPU fallback
    wct = WCT(args)
    _DEVICE_DECODER = DeviceDecoder(wct, logprinter) if getattr(args, "device_decode", False) else None
    logprinter("Number of content-style pairs: %s" % len(pairs))
    if args.pipeline > 0:
        wall = run_pipelined(args, wct, pairs, content_dir, style_dir, logprinter)
        if pairs:
            logprinter("Processed %d images. Average processing time per pair is: %.4f seconds (pipelined: wall time / pairs, decode and "
                       "save included)" % (len(pairs), wall / len(pairs)))
    else:
        avg = run_serial(args, wct, pairs, content_dir, style_dir, logprinter)
        if pairs:
            logprinter("Processed %d images. Average processing time per pair is: %.4f seconds" % (len(pairs), avg / len(pairs)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
