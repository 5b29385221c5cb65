"""The catalogue of tests/state_cases.py cannot silently fall behind the ABI: every symbol of wct_hip.lib.SYMBOLS is either covered
by a case or excluded here, by name, with a reason.  Runs without a GPU."""
from tests import state_cases as sc
from wct_hip import lib

LIFECYCLE = "lifecycle / query / switch: exercised by tests/test_state_gpu.py as an action BETWEEN cases"
PEERS = "communicator family: needs peers, belongs to tests/test_sharded_gpu.py"
EXCLUDED = {
    "wct_create": LIFECYCLE, "wct_destroy": LIFECYCLE, "wct_version": LIFECYCLE, "wct_last_error": LIFECYCLE, "wct_sync": LIFECYCLE,
    "wct_set_stream": LIFECYCLE, "wct_feature_shape": LIFECYCLE, "wct_resize_shape": LIFECYCLE, "wct_style_stats_count": LIFECYCLE,
    "wct_profile_enable": LIFECYCLE, "wct_profile_reset": LIFECYCLE, "wct_profile_read": LIFECYCLE,
    "wct_saturation_count": LIFECYCLE, "wct_range_poll": LIFECYCLE, "wct_range_flag_f64": LIFECYCLE,
    "wct_debug_set": LIFECYCLE, "wct_debug_get": LIFECYCLE, "wct_load_module": LIFECYCLE,
    "wct_set_conv_mode": LIFECYCLE, "wct_set_numpy_variant": LIFECYCLE, "wct_set_overlap": LIFECYCLE,
    "wct_comm_load": PEERS, "wct_comm_library": PEERS, "wct_comm_unique_id": PEERS, "wct_comm_init": PEERS, "wct_comm_attach": PEERS,
    "wct_comm_destroy": PEERS, "wct_comm_attach_collectives": PEERS, "wct_comm_info": PEERS, "wct_comm_selftest": PEERS,
    "wct_level_sharded": PEERS, "wct_stylize_sharded": PEERS, "wct_shard_geometry": PEERS,
}


def test_catalogue_covers_every_compute_entry_point():
    symbols = set(lib.SYMBOLS)
    assert len(symbols) == len(lib.SYMBOLS), "duplicate names in wct_hip.lib.SYMBOLS"
    stale = sorted(set(EXCLUDED) - symbols)
    assert not stale, "excluded names that wct_hip.lib.SYMBOLS does not list: %s" % stale
    covered = sc.covered()
    unknown = sorted(covered - symbols)
    assert not unknown, "cases claim entry points that do not exist: %s" % unknown
    both = sorted(covered & set(EXCLUDED))
    assert not both, "both covered and excluded: %s" % both
    missing = sorted(symbols - covered - set(EXCLUDED))
    assert not missing, "compute entry points without a case in tests/state_cases.py: %s" % missing


def test_catalogue_shape():
    """Every family at both sizes; the sizes differ in every tile count; the wide engine sees small cases only."""
    fams = {}
    for name, c in sc.CASES.items():
        assert name == "%s/%s" % (c.family, c.size) and c.covers
        fams.setdefault(c.family, set()).add(c.size)
        assert not c.wide or c.size == "small", name
    assert all(v == {"small", "large"} for v in fams.values()), fams
    (h, w, hs, ws), (H, W, Hs, Ws) = sc.SIZES["small"], sc.SIZES["large"]
    assert h % 16 and w % 16 and (H % 32 or W % 32) and H * W <= 600000
    for a, b in ((h, H), (w, W), (hs, Hs), (ws, Ws)):
        assert all(-(-a // t) != -(-b // t) for t in (16, 32, 64, 128))
    assert sc.names("wide") and set(sc.names("wide")) < set(sc.names("16x"))
