"""The WCT class with the widths of tests/width_models.py (the engine of tests/test_shard_widths_gpu.py), and rank threads for calls that
tools/sharded_standins.run_in_process does not make (one sharded level at a time).  Needs torch; imports without a GPU."""
import threading
import types
from ctypes import byref, c_int

from tests import width_models as wm
from wct_hip import WCT
from wct_hip import lib as _lib


class WidthWCT(WCT):
    """wct_hip.WCT over a custom-width layer graph: the two reads of model_zoo's tables answered from `widths`.  Everything else -- the
    split-level calls, the sharded entries, ShardedStylizer on top -- is the product's code.  (`mode` stays "16x": nothing reads it.)"""

    def __init__(self, widths, weights, transform="wct", alpha=1.0):
        self.widths = widths
        super().__init__(types.SimpleNamespace(mode="16x", alpha=alpha, transform=transform), weights=weights)

    def _layers(self, kind, level):
        return wm.encoder_layers(self.widths, level) if kind == "enc" else wm.decoder_layers(self.widths, level)

    def _feature_channels(self, level):
        return wm.feature_channels(self.widths, level)


def profile_counts(eng):
    """{profile name: launches} of an engine since its last profile_reset(), all entries (WCT.profile_read stops at 64)."""
    n = c_int()
    eng._chk(eng._lib.wct_profile_read(eng._ctx, None, 0, byref(n)))
    e = (_lib.WctProfEntry * max(n.value, 1))()
    eng._chk(eng._lib.wct_profile_read(eng._ctx, e, n.value, byref(n)))
    return {e[i].name.decode(): int(e[i].launches) for i in range(n.value)}


def run_rank_threads(world, fn, sync_every=False):
    """fn(rank, group) on `world` threads of this process, each under a stream of its own, with the device-buffer collectives of
    tools/sharded_standins.InProcessWorld between them (the frame of run_in_process around another body).  Returns the ranks' results."""
    import torch
    from tools.sharded_standins import InProcessWorld
    wd = InProcessWorld(world, sync_every)
    groups = [wd.group(r) for r in range(world)]
    streams = [torch.cuda.Stream() for _ in range(world)]
    outs, errs = [None] * world, [None] * world
    dev = torch.cuda.current_device()
    ready = torch.cuda.Event()
    ready.record()

    def work(r):
        try:
            torch.cuda.set_device(dev)
            with torch.cuda.stream(streams[r]):
                streams[r].wait_event(ready)
                outs[r] = fn(r, groups[r])
        except BaseException as e:      # noqa: BLE001  a dead rank must not leave its peers in a barrier
            errs[r] = e
            wd._bar.abort()

    threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    errs = [getattr(g, "error", None) for g in groups] + errs
    first = next((e for e in errs if e is not None and not isinstance(e, threading.BrokenBarrierError)), None) or next((e for e in errs if e is not None), None)
    if first is not None:
        raise first
    torch.cuda.synchronize()
    return outs, groups
