"""The conv sweep's plan, proved on the CPU (tests/conv_cases.py; tests/test_conv_sweep_gpu.py runs it on the MI355X)."""
import collections
import itertools

from tests import conv_cases as K
from tests import geometry_cases as G
from tests import sweep_cases as S
from tests import width_models as wm
from wct_hip import model_zoo
from wct_hip.model_zoo import Layer

BANDS = range(S.N_BANDS)


def _line_modules(variant):
    return [m for b in BANDS for m in K.modules(b, variant)]


def test_every_planned_module_is_loadable():
    mods = K.all_modules() + [m for v in K.VARIANTS for m in K.switch_modules(v)]
    assert len(mods) > 7000
    for m in mods:
        assert wm.loadable(m.kind, list(m.layers)), m.id
        assert m.level == 1 + sum(l.pool_after or l.up_after for l in m.layers), m.id      # wct_feature_shape / the decoded size follow the level
        assert all(min(h, w) >= 2 << (m.level - 1) for h, w in m.sizes) or m.kind == "dec", m.id
    assert not wm.loadable("enc", [Layer("a", 3, 16), Layer("b", 16, 6)]) and not wm.loadable("dec", [Layer("a", 16, 516), Layer("b", 516, 3)])


def test_every_width_is_cin_and_cout_in_every_variant():
    for v in K.VARIANTS:
        mid = [m for m in _line_modules(v) if m.line in ("I", "II")]
        assert {m.cin for m in mid} == set(K.WIDTHS) and {m.cout for m in mid} == set(K.WIDTHS), v
        for m in mid:                                                    # the layer under test is neither first nor last
            assert 0 < m.lut < len(m.layers) - 1, m.id
            assert m.layers[m.lut].pool_after == (v == "enc-pool") and m.layers[m.lut - 1].up_after == (v == "dec-up"), m.id
        # Line I: every cin against every representative cout; Line II: every cout against every representative cin
        have = {(m.cin, m.cout) for m in mid}
        assert {(a, b) for a in K.WIDTHS for b in K.REP_COUT} | {(a, b) for a in K.REP_CIN for b in K.WIDTHS} == have, v
    first = {(m.cin, m.cout) for m in _line_modules("dec") if m.line == "II-first"}
    assert first == {(a, b) for a in K.REP_CIN for b in K.WIDTHS}
    assert {m.cout for m in K.first_modules(False)} == {m.cout for m in K.first_modules(True)} == set(range(4, 65, 4))


def test_representatives_cover_their_classes():
    assert [K.cout_class(b) for b in K.REP_COUT] == [K.COUT_CLASSES[i] for i in (0, 1, 2, 3, 4, 5, 7)]
    assert {K.cout_class(b) for b in K.WIDTHS} == set(K.COUT_CLASSES)
    chunks = collections.defaultdict(set)
    for a in K.REP_CIN:
        chunks[K.cin_class(a)].add("one" if a <= 16 else "many")
    assert chunks == {c: {"one", "many"} for c in K.CIN_CLASSES}


def test_every_class_cell_occurs_and_has_its_switch_arms():
    for v in K.VARIANTS:
        cells = {(K.cin_class(m.cin), K.cout_class(m.cout)) for m in _line_modules(v) if m.line != "II-first"}
        assert cells == set(itertools.product(K.CIN_CLASSES, K.COUT_CLASSES)), v          # all 27: no cell is unreachable for the loader
        sw = K.switch_modules(v)
        assert {(K.cin_class(m.cin), K.cout_class(m.cout)) for m in sw} == cells, v
        arms = collections.Counter(k for m in sw for ((k, _),) in K.arms(m))
        assert all(("conv_mode", 0) in [a[0] for a in K.arms(m)] for m in sw), v
        assert arms["sp"] > 0 and (arms["upconv"] > 0) == (v == "dec-up") and (arms["fuse"] > 0) == (v in ("dec", "dec-up")), (v, arms)
        assert all(m in _line_modules(v) for m in sw), v                                   # the arms re-run planned cases, nothing new
    # the fused head and the level-1 / wide first convs get their fuse arm on the first-layer line
    fuse = {m.cout for f in (False, True) for m in K.first_modules(f) if (("fuse", 0),) in K.arms(m)}
    assert fuse == {4, 8, 12, 16, 20, 24, 28, 32, 64}


def _produced(mods, with_arms):
    out = set()
    for m in mods:
        for sw in [()] + (list(K.arms(m)) if with_arms else []):
            out |= K.pairs(m.kind, m.layers, *m.sizes[0], dict(sw))
    return out


def test_every_producible_hand_over_and_kernel_pair_occurs():
    # what predict can produce: the plan's placements over a width set with every class at one and at many chunks, every producer cin
    # class in front (the plan's own producers are 16 -> a), every switch
    widths = [c for c in K.WIDTHS if c <= 144] + [256, 264, 384, 512]
    space = set()
    for a, b in itertools.product(widths, widths):
        for p in (4, 8, 16):
            for up in (False, True):
                layers = (Layer("p", p, a, up_after=up), Layer("t", a, b), Layer("c", b, 3))
                for sw in ({}, {"sp": 0}, {"upconv": 0}, {"fuse": 0}, {"conv_mode": 0}):
                    space |= K.pairs("dec", layers, 5, 7, sw)
        if a <= 64:
            for pool in (False, True):
                layers = (Layer("p", 3, a), Layer("t", a, b, pool_after=pool), Layer("c", b, 8))
                for sw in ({}, {"sp": 0}, {"fuse": 0}, {"conv_mode": 0}):
                    space |= K.pairs("enc", layers, 9, 35, sw)
    for b in K.FIRST_COUT:
        space |= K.pairs("enc", (Layer("t", 3, b),), 5, 7) | K.pairs("enc", (Layer("t", 3, b),), 5, 7, {"fuse": 0})
    plan = _produced(K.all_modules(), False) | _produced([m for v in K.VARIANTS for m in K.switch_modules(v)], True) | \
        _produced(list(K.first_modules(False)) + list(K.first_modules(True)), True)
    assert space <= plan, sorted(space - plan)
    # ... and what it cannot produce is listed by name, with the rule
    every = set(itertools.product(K.HANDS_IN, K.KERNELS))
    assert every - plan == set(K.UNREACHABLE_PAIRS), (sorted(every - plan - set(K.UNREACHABLE_PAIRS)), sorted(set(K.UNREACHABLE_PAIRS) - (every - plan)))
    assert all(rule.strip() for rule in list(K.UNREACHABLE_PAIRS.values()) + list(K.UNREACHABLE_CELLS.values()))
    # the launcher-level exclusions, checked against predict over the whole plan
    for m in K.all_modules():
        p = K.predict(m.kind, m.layers, *m.sizes[0])
        for i, (l, k) in enumerate(zip(m.layers, p.kernels)):
            if k in ("dma", "dma-up"):
                assert l.cin % 16 == 0 and l.cout % 8 == 0 and wm.pad_cout(l.cout) >= 32, m.id
            if k == "dma-up":
                assert m.variant == "dec-up" and i == m.lut, m.id
            if i < len(p.hand) and p.hand[i] == "sp16":
                assert l.cout % 8 == 0 and (l.cin % 8 == 0 or l.cin == 3), m.id


def test_predict_reproduces_the_width_models_families():
    for model, (want, banned) in wm.FAMILIES.items():
        widths = wm.MODELS[model]
        names = set()
        for level in (1, 2, 3, 4, 5):
            names |= set(K.predict("enc", wm.encoder_layers(widths, level), 64, 64).names)
            names |= set(K.predict("dec", wm.decoder_layers(widths, level), 4, 4).names)
        assert set(want) <= names, (model, sorted(set(want) - names))
        assert not [n for n in names for b in banned if b in n], (model, sorted(names))
        mode0 = set(K.predict("enc", wm.encoder_layers(widths, 5), 64, 64, {"conv_mode": 0}).names)
        assert all(n.startswith("conv3x3_f32<") for n in mode0) and "conv3x3_f32<co=%d,in3>" % min(wm.pad_cout(widths[1]), 128) in mode0


def test_predict_reproduces_the_shipped_graphs():
    """geometry_cases.predict_names with its form suffixes dropped: the families of both shipped graphs, every level, both upconv arms"""
    for mode in ("16x", "original"):
        for level in (1, 2, 3, 4, 5):
            for kind, layers in (("enc", model_zoo.encoder_layers(mode, level)), ("dec", model_zoo.decoder_layers(mode, level))):
                for sw in ({}, {"upconv": 0}):
                    got = K.predict(kind, layers, 96, 128, sw).names
                    ref = tuple(dict.fromkeys(n.split("#")[0] for n in G.predict_names(kind, mode, level, 96, 128, 256, sw)))
                    assert tuple(dict.fromkeys(got)) == ref, (mode, kind, level, sw, got, ref)


def test_bands_are_balanced():
    for v in K.VARIANTS:
        n = [sum(len(m.sizes) for m in K.modules(b, v)) for b in BANDS]
        print("conv cases %s per band: %s (mean %.1f)" % (v, n, sum(n) / len(n)))
        assert max(n) <= 2 * sum(n) / len(n), (v, n)
    n_sw = {v: sum(len(m.sizes) * len(K.arms(m)) for m in K.switch_modules(v)) for v in K.VARIANTS}
    n_first = [sum(len(m.sizes) * (1 + len(K.arms(m))) for m in K.first_modules(f)) for f in (False, True)]
    print("conv cases switch arms: %s; first layers alone / followed: %s" % (n_sw, n_first))
