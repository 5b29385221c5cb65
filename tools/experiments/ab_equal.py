"""Bitwise A/B of two builds of libwct_hip: python tools/experiments/ab_equal.py <other.so>

Runs itself once per build in a fresh child process (the in-tree library, then <other.so> through WCT_LIB_PATH), each under its own
time limit, and compares what the two wrote: per call of every stylize entry point "bitwise equal" or the largest difference, and
whether the profiled launch lists (name with the launcher's form, launches, flops, bytes -- no times) are identical.  Exit 1 on any
difference; a leg that fails or runs out of time ends the run before the next one starts.  The shapes are small; one 1080x1920 stylize
on the 16x model keeps the multi-tile launch forms in the comparison.  The column-sharded path is not here: tests/test_sharded_gpu.py
holds it against the split-level path bit for bit."""
import json, os, subprocess, sys, tempfile, types
REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEG_SECONDS = 300


def calls(wct, H, W, Hs, Ws, big=None):
    """(tag, thunk) per entry point; inputs from one seeded host generator, made once"""
    import torch
    g = torch.Generator().manual_seed(3)
    rnd = lambda *shape: torch.rand(shape, generator=g).cuda()
    c, s, s2 = rnd(3, H, W), rnd(3, Hs, Ws), rnd(3, Hs, Ws)
    c8, s8 = (rnd(H, W, 3) * 255).to(torch.uint8), (rnd(Hs, Ws, 3) * 255).to(torch.uint8)
    halves = lambda h, w: (torch.arange(w, device="cuda") >= w // 2).to(torch.uint8).repeat(h, 1).contiguous()
    lab, slab = halves(H, W), halves(Hs, Ws)
    ramp = torch.linspace(0.0, 0.8, W, device="cuda").repeat(H, 1)
    wmap = torch.stack([ramp, 0.8 - ramp]).contiguous()

    cb, sb = (rnd(3, *big[:2]), rnd(3, *big[2:])) if big else (None, None)

    def prepared():
        wct.style_prepare(s)
        return wct.stylize_prepared(c, alpha=0.8)

    return [
        ("stylize", lambda: wct.stylize(c, s, alpha=0.7)),
        ("style_prepare+stylize_prepared", prepared),
        ("stylize_u8", lambda: wct.stylize_u8(c8, s8)),
        ("synthesize", lambda: wct.synthesize(s, H, W, seed=5, stream_id=1)),
        ("stylize_color match", lambda: wct.stylize_color(c, s, "match")),
        ("stylize_color luma", lambda: wct.stylize_color(c, s, "luma")),
        ("stylize_smooth", lambda: wct.stylize_smooth(c, s, 2)),
        ("stylize_swap", lambda: wct.stylize_swap(c, s, 3)),
        ("stylize_scaled", lambda: wct.stylize_scaled(c, s, (2, 2, 1, 1, 1))),
        ("stylize_regions", lambda: wct.stylize_regions(c, [s, s2], lab)),
        ("stylize_guided", lambda: wct.stylize_guided(c, [s], lab, [slab], region_style=[0, 0])),
        ("feature_regions", lambda: torch.cat([t.flatten() for t in wct.feature_regions(c, s, 2, level=4, iters=3)])),
        ("stylize_interp", lambda: wct.stylize_interp(c, [s, s2], (0.3, 0.7))),
        ("stylize_blend", lambda: wct.stylize_blend(c, [s, s2], wmap)),
        ("style_transfer_level 5", lambda: wct.style_transfer_level(5, c, s)),
        ("style_transfer_level 1", lambda: wct.style_transfer_level(1, c, s)),
    ] + ([("stylize %dx%d" % big[:2], lambda: wct.stylize(cb, sb, alpha=0.7))] if big else [])


def run(path):
    sys.path[:0] = [REPO, os.path.join(REPO, "collaborative-distillation_amd")]
    import numpy as np, torch
    from wct_hip import WCT, model_zoo
    models = (("16x", model_zoo.load_npz_weights(os.path.join(REPO, "collaborative-distillation_amd", "weights", "16x.npz")), (96, 128, 80, 96, (1080, 1920, 1024, 1024))),
              ("original", model_zoo.synth_weights("original", 7), (64, 80, 48, 64)))
    outs, launches = {}, {}
    for mode, weights, shape in models:
        wct = WCT(types.SimpleNamespace(mode=mode, alpha=1.0), weights=weights)
        todo = calls(wct, *shape)
        for tag, fn in todo:
            outs["%s %s" % (mode, tag)] = fn().cpu().numpy()
        wct.profile(True)
        wct.debug_set("prof_forms", 1)
        for tag, fn in todo:
            wct.profile_reset()
            fn()
            torch.cuda.synchronize()
            launches["%s %s" % (mode, tag)] = [(r["name"], r["launches"], r["flops"], r["bytes"]) for r in wct.profile_read()]
        wct.profile(False)
    np.savez(path, __launches__=np.array(json.dumps(launches)), **outs)


def compare(other):
    with tempfile.TemporaryDirectory(prefix="ab_equal_") as tmp:
        return compare_in(other, tmp)


def compare_in(other, tmp):
    import numpy as np
    for tag, lib in (("a", ""), ("b", other)):   # check_call: a leg that fails starts nothing further
        subprocess.check_call(["timeout", "-k", "10", str(LEG_SECONDS), sys.executable, os.path.abspath(__file__), "--run", os.path.join(tmp, tag + ".npz")],
                              env=dict(os.environ, WCT_LIB_PATH=lib))
    a, b = np.load(os.path.join(tmp, "a.npz")), np.load(os.path.join(tmp, "b.npz"))
    la, lb = json.loads(str(a["__launches__"])), json.loads(str(b["__launches__"]))
    keys = [k for k in a.files if k != "__launches__"]
    bad = sorted(set(keys) ^ set(k for k in b.files if k != "__launches__"))
    print("%-46s %-16s %-22s %s" % ("call", "shape", "output", "launch list"))
    for k in keys:
        if k not in b.files:
            continue
        same = a[k].shape == b[k].shape and np.array_equal(a[k], b[k])
        diff = "bitwise equal" if same else ("DIFFER shape" if a[k].shape != b[k].shape else
                                             "DIFFER max %.3e" % np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
        same_l = k in la and la[k] == lb.get(k)
        print("%-46s %-16s %-22s %s" % (k, "x".join(map(str, a[k].shape)), diff, "identical (%d rows)" % len(la[k]) if same_l else "DIFFER"))
        if not (same and same_l):
            bad.append(k)
    print("all equal" if not bad else "DIFFERENT: " + ", ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--run":
        run(sys.argv[2])
    elif len(sys.argv) == 2:
        sys.exit(compare(sys.argv[1]))
    else:
        sys.exit(__doc__)
