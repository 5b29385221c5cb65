"""CPU-only checks of the drop-in boundary: the built library loads and exports every symbol that
include/wct_hip.h declares (no compute calls without a GPU), and the host mirror's error behaviour."""
import os
import re
import types

import pytest

import numpy as np

from tests.conftest import PKG, REPO


def _build():
    import __graft_entry__ as g
    g.build()


def test_library_exports_every_declared_symbol():
    _build()
    from wct_hip import lib
    hdr = open(os.path.join(REPO, "include", "wct_hip.h")).read()
    declared = sorted(set(re.findall(r"\b(wct_[a-z_0-9]+)\s*\(", hdr)) - {"wct_ctx"})
    assert declared and sorted(lib.SYMBOLS) == declared
    L = lib.load()
    for s in declared:
        assert hasattr(L, s), s
    assert L.wct_version() >= 1


def test_header_cites_reference_interfaces():
    hdr = open(os.path.join(REPO, "include", "wct_hip.h")).read()
    for cite in ("WCT.py:98-106", "util_wct.py:210-223", "WCT.py:120-125", "util_wct.py:68-70", "model_cd.py:724-743"):
        assert cite in hdr


def test_create_without_gpu_reports_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    _build()
    import ctypes
    from wct_hip import lib
    L = lib.load()
    ctx = ctypes.c_void_p()
    assert L.wct_create(0, ctypes.byref(ctx)) == lib.WCT_ERR_HIP and not ctx.value
    assert L.wct_sync(None) == lib.WCT_ERR_INVALID  # NULL context is rejected, never dereferenced


def test_host_mirror_error_behaviour():
    import torch
    from wct_hip import WCT
    with pytest.raises(ValueError, match="Wrong mode"):          # util_wct.py:57-59 prints this and exits
        WCT(types.SimpleNamespace(mode="32x"))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):   # the product never falls back to the CPU
            WCT(types.SimpleNamespace(mode="16x"))


def test_product_does_not_import_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may touch oracle/."""
    pkg = os.path.join(REPO, "collaborative-distillation_amd")
    bad = re.compile(r"(from|import)\s+oracle|wct_oracle|liboracle|oracle/")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".sh", ".cpp")):
                src = open(os.path.join(root, f)).read()
                assert not bad.search(src), os.path.join(root, f)


def test_checkpoint_paths_never_fall_back_silently(tmp_path, weights16x):
    """with SOME of args.e1..d5 present the reference would fail in torch.load (model_cd.py:712-718); the mirror
    must not substitute the packaged weights for a partial / mistyped set.  No path at all (the reference snapshot's layout
    is absent) -> the packaged 16x blob; a complete set -> exactly those tensors, aux heads dropped."""
    import torch
    from wct_hip.wct import WCT
    args = types.SimpleNamespace(mode="16x")
    for k in range(1, 6):
        for key in ("e%d" % k, "d%d" % k):
            sd = {n[len(key) + 1:]: torch.from_numpy(v.copy()) for n, v in weights16x.items() if n.startswith(key + ".")}
            if key[0] == "e":
                sd["conv%d1_aux.weight" % k] = torch.zeros(2, 2, 1, 1)
            path = str(tmp_path / (key + ".pth"))
            torch.save({"epoch": 20, "model": sd} if k % 2 else sd, path)
            setattr(args, key, path)
    w = WCT._weights_from_args(args, "16x")
    assert sorted(w) == sorted(weights16x) and all((w[k] == weights16x[k]).all() for k in w)
    os.remove(args.d4)
    with pytest.raises(FileNotFoundError, match="d4"):
        WCT._weights_from_args(args, "16x")
    none = types.SimpleNamespace(mode="16x", e1="../trained_models/wct_se_16x_new/1SE.pth")     # WCT.py:49: path that does not exist here
    assert sorted(WCT._weights_from_args(none, "16x")) == sorted(weights16x)
    args.d4 = str(tmp_path / "d4.t7")
    open(args.d4, "wb").close()
    with pytest.raises(ValueError, match="extension"):
        WCT._weights_from_args(args, "16x")


def test_debug_environment_is_gated():
    """WCT_* experiment variables must not change results unless WCT_DEBUG is set."""
    src = ""
    for f in os.listdir(os.path.join(REPO, "collaborative-distillation_amd", "csrc")):
        src += open(os.path.join(REPO, "collaborative-distillation_amd", "csrc", f)).read()
    raw = [m for m in re.findall(r'[^_a-z]getenv\("(WCT_[A-Z_0-9]+)"\)', src) if m not in ("WCT_DEBUG", "WCT_PROF_SHAPES")]
    assert raw == [], raw


def test_weights_only_loader_reads_the_reference_checkpoints(tmp_path):
    """wct_hip.wct._load_state un-pickles with weights_only=True (no arbitrary code from a checkpoint).  Files in the reference's
    own on-disk layout -- torch's legacy (pre-zip) serialization of {"epoch", "model": OrderedDict} for all ten modules, the
    encoders with their unused conv{j}1_aux heads (j <= k; model_cd.py:712-718) -- written here from the packaged blob, must load
    that way, without WCT_ALLOW_UNSAFE_PICKLE, into exactly the blob's tensors (aux heads aside)."""
    import collections
    import zipfile
    import torch
    from wct_hip import model_zoo
    from wct_hip.wct import _load_state
    blob = model_zoo.load_npz_weights(os.path.join(PKG, "weights", "16x.npz"))
    assert os.environ.get("WCT_ALLOW_UNSAFE_PICKLE") != "1"
    rng = np.random.default_rng(3)
    aux = {1: (64, 16), 2: (128, 32), 3: (256, 64), 4: (512, 128), 5: (512, 128)}
    for k in range(1, 6):
        for key in ("e%d" % k, "d%d" % k):
            sd = collections.OrderedDict((n[len(key) + 1:], torch.from_numpy(v.copy())) for n, v in blob.items() if n.startswith(key + "."))
            for j in range(1, k + 1) if key[0] == "e" else ():
                co, ci = aux[j] if (k, j) != (1, 1) else (64, 24)
                sd["conv%d1_aux.weight" % j] = torch.from_numpy(rng.standard_normal((co, ci, 1, 1), dtype=np.float32))
                sd["conv%d1_aux.bias" % j] = torch.from_numpy(rng.standard_normal(co, dtype=np.float32))
            path = str(tmp_path / ("%d%s.pth" % (k, "SE" if key[0] == "e" else "SD")))
            torch.save({"epoch": 20, "model": sd}, path, _use_new_zipfile_serialization=False)
            assert not zipfile.is_zipfile(path)
            sd = _load_state(path)
            mine = {n[len(key) + 1:]: v for n, v in blob.items() if n.startswith(key + ".")}
            assert set(mine) <= set(sd) and all("aux" in n for n in set(sd) - set(mine)), key
            for n, v in mine.items():
                assert v.shape == sd[n].shape and np.array_equal(v, sd[n]), (key, n)


def test_experiment_scripts_reference_live_switches():
    """tools/experiments/ is the recipe book behind DESIGN's numbers: every script must byte-compile and use only WCT_* variables and
    wct_debug_set keys that still exist in the library (tools/experiments/audit.py; VERDICT r3 task 8)."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "experiments", "audit.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout



def test_c_host_of_the_sharded_cascade_compiles_and_links(tmp_path):
    """a NON-Python host drives one rank of the multi-GPU job through the C ABI alone.  That host, as plain C99, compiles
    against include/wct_hip.h (prototypes checked by the compiler) and links against libwct_hip.so; without a GPU it runs as far as wct_create's
    error and the pure geometry function, whose answers for BASELINE configs[3] (10240 columns, 8 ranks) are checked."""
    import subprocess
    src = tmp_path / "host.c"
    src.write_text(r'''
#include <stdio.h>
#include "wct_hip.h"
static int dummy_ar(void* u, double* b, size_t n, void* s) { (void)u; (void)b; (void)n; (void)s; return 0; }
static int dummy_bc(void* u, void* b, size_t n, int r, void* s) { (void)u; (void)b; (void)n; (void)r; (void)s; return 0; }
static int dummy_sr(void* u, const wct_p2p* o, int n, void* s) { (void)u; (void)o; (void)n; (void)s; return 0; }
int run_rank(wct_ctx* ctx, int nranks, int rank, const unsigned char* id, const float* content_ext, const float* style, float* out_owned) {
  int own0, own1, in0, in1, mode, Ho, Wo;
  if (wct_comm_load(NULL) != WCT_OK || wct_comm_init(ctx, nranks, rank, id) != WCT_OK || wct_comm_selftest(ctx) != WCT_OK) return -1;
  if (wct_shard_geometry(10240, nranks, rank, WCT_HALO_AUTO, &own0, &own1, &in0, &in1, &mode) != WCT_OK) return -2;
  return wct_stylize_sharded(ctx, content_ext, 4096, 10240, in0, in1, style, 2048, 2048, 1.0f, WCT_HALO_AUTO, WCT_STYLE_AUTO, 0, out_owned, &Ho, &Wo, NULL);
}
int main(void) {
  wct_collectives t = {NULL, dummy_ar, dummy_bc, dummy_sr};
  int own0, own1, in0, in1, mode, n, r;
  (void)t;
  if (wct_shard_geometry(10240, 8, 3, WCT_HALO_AUTO, &own0, &own1, &in0, &in1, &mode) != WCT_OK) return 1;
  printf("%d %d %d %d %d\n", own0, own1, in0, in1, mode);
  if (wct_shard_geometry(400, 4, 0, WCT_HALO_EXCHANGE, &own0, &own1, &in0, &in1, &mode) == WCT_OK) return 2;   /* strips too narrow to exchange */
  if (wct_comm_info(NULL, &n, &r) == WCT_OK) return 3;
  printf("version %d library '%s'\n", wct_version(), wct_comm_library());
  return 0;
}
''')
    exe = tmp_path / "host"
    _build()
    from wct_hip import lib
    libdir = os.path.dirname(lib.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lwct_hip", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, LD_LIBRARY_PATH=os.pathsep.join([libdir, "/opt/rocm/lib", os.environ.get("LD_LIBRARY_PATH", "")]))
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    assert r.stdout.splitlines()[0] == "3840 5120 3680 5280 2"          # rank 3 of 8: owns [3840, 5120), is given +-160 columns, exchange mode
    assert "version 1 library ''" in r.stdout
