"""The tables of tests/packed_corpus.py on the host (-m "not gpu"): what the corpus must contain is asserted on the corpus alone, every
built table is a legal layout, HostTable.from_slots / raw round-trip, bfc_ch_restore equals a restatement of its place-and-grow rule, and
the host twins -- the reference side of test_gpu_packed.py -- give the recorded answers and the string oracles' graphs on full regions
and wrapped chains.  test_gpu_packed.py takes its tables and expected values from this file."""
import functools
import struct

import numpy as np
import pytest

import bubble_oracle
import clip_oracle
import packed_corpus as pc
import test_clip_host
import test_dense_graph_host as H
import test_pop_host
import unitig_oracle
from graph_oracle import revcomp

U = np.uint64
CASES = [(k, l_pre, cshift) for k in pc.KS for l_pre, cshift in pc.GEOMS]
FIXTURES = ["bubble21", "fork21", "d11", "d15"]
RELAID = {"bubble21": 3, "fork21": 4, "d11": 6, "d15": 13}      # the cshift of relaid(): 2^(cshift - 1) lanes a region below 7, a wave from 7 on
FORMS = ["relaid", "filled"]
FULL = ["bubble21", "d15"]                                         # the fixtures of the full result regions: c = 2 and a region of thousands
POP_SETS = (dict(max_diff=2), dict())


def clip_sets(name):
    """test_gpu_clip.py's parameter sets: the forked fixture's, and those of every other table"""
    return (dict(min_cnt=2, max_tip=12), dict(min_cnt=1, max_tip=12, islands=True)) if name == "fork21" else (dict(min_cnt=2), dict(min_cnt=1, islands=True, max_rounds=3))


def key_of(kw):
    return tuple(sorted(kw.items()))


def legal(slots, cshift):
    """no empty slot between a key's home and its slot: what linear probing from the home slot needs to find every key"""
    slots = np.asarray(slots, dtype=U)
    cm = (1 << cshift) - 1
    at = np.flatnonzero(slots)
    home = ((slots[at] >> U(14)) & U(cm)).astype(np.int64)
    disp = ((at & cm) - home) & cm
    for i, h, d in zip(at[disp > 0], home[disp > 0], disp[disp > 0]):
        base = int(i) & ~cm
        if not slots[base + ((int(h) + np.arange(int(d))) & cm)].all():
            return False
    return True


@functools.lru_cache(maxsize=None)
def base(gpu_lib, name):
    """a graph fixture as the restored host table the other host tests use"""
    return {"bubble21": lambda: test_pop_host._tab(gpu_lib, 21), "fork21": lambda: test_clip_host._fork_tab(gpu_lib, 21)}.get(name, lambda: H.tab(gpu_lib, name))()


@functools.lru_cache(maxsize=None)
def table(gpu_lib, name, form):
    """(HostTable, its dict for the string oracles, the sub-tables made full) of a fixture relaid or filled -- made once, never changed"""
    if form == "relaid":
        t, full = pc.relaid(gpu_lib, base(gpu_lib, name), RELAID[name]), []
    else:
        t, cshift, full = pc.filled(gpu_lib, base(gpu_lib, name))
    return t, unitig_oracle.dict_of_table(t), full


@functools.lru_cache(maxsize=None)
def want_clip(d, kw):
    """the string oracle's (survivors, stats, survivors' unitigs) of a clip -- computed once"""
    surv, stats = clip_oracle.clip(d, **dict(kw))
    return surv, stats, clip_oracle.unitigs_of(d.k, surv)


@functools.lru_cache(maxsize=None)
def want_pop(d, kw):
    surv, stats = bubble_oracle.pop(d, **dict(kw))
    return surv, stats, bubble_oracle.unitigs_of(d.k, surv)


@functools.lru_cache(maxsize=None)
def want_unitigs(d, min_cnt):
    return unitig_oracle.unitigs(d, min_cnt)


FULL_KW = {"clip": dict(min_cnt=1, islands=False), "pop": dict(max_diff=2)}


@functools.lru_cache(maxsize=None)
def full_input(gpu_lib, name, how):
    """pc.full_result of a fixture: clip / pop -> (input HostTable, its dict, c, sub-table); union -> (A, B, c, sub-table)"""
    t = base(gpu_lib, name)
    if how == "union":
        return pc.full_result(gpu_lib, t, how, None)
    d = unitig_oracle.dict_of_table(t)
    surv = (want_clip if how == "clip" else want_pop)(d, key_of(FULL_KW[how]))[0]
    inp, c, sub = pc.full_result(gpu_lib, t, how, set(surv))
    return inp, unitig_oracle.dict_of_table(inp), c, sub


def stats_of(s):
    return [tuple(int(v) for v in r) for r in s]


# ---- the corpus alone ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,l_pre,cshift", CASES)
def test_corpus_holds_every_class(gpu_lib, k, l_pre, cshift):
    """over a case's variants every region class stands in the first, the last and a middle sub-table; class b has every displacement;
    a key at home stands in all three places; every kind of absent query is there, one per home of every full region; a full region
    with a wrapped chain in every variant; counts 1, 2, 255 and high counts 0, 63; slot 0 and the last slot occupied unless the empty
    region stands there"""
    tabs = pc.chain_case(k, l_pre, cshift)
    n_sub, R = 1 << l_pre, 1 << cshift
    first, last, middle, home_at = set(), set(), set(), set()
    for t in tabs:
        inv = pc.inventory(t)
        for c in pc.CLASSES:
            subs = inv["regions"][c]
            first |= {c} & ({c} if 0 in subs else set())
            last |= {c} & ({c} if n_sub - 1 in subs else set())
            if subs - {0, n_sub - 1}:
                middle.add((t.variant, c))
        for sub, disp in inv["b_disp"].items():
            assert disp == set(range(R))
        n_full = len(inv["regions"]["b"] | inv["regions"]["c"])
        assert inv["absent"]["full-home"] == n_full * R and inv["wrapped_full"] >= inv["regions"]["b"] and len(inv["wrapped_full"]) >= 2
        for kind in ("wrap-empty", "empty-region", "miss-high", "miss-sub", "miss-key"):
            assert inv["absent"][kind] >= 1, kind
        home_at |= {"first"} & ({"first"} if 0 in inv["at_home"] else set()) | ({"last"} if n_sub - 1 in inv["at_home"] else set())
        home_at |= {"middle"} if inv["at_home"] - {0, n_sub - 1} else set()
        assert {p.value & 0xff for p in t.placed} == set(pc.COUNTS) and {p.value >> 8 for p in t.placed} == set(pc.HIGHS)
        assert (t.slots[0] != 0) == (t.roles[0] != "f") and (t.slots[-1] != 0) == (t.roles[n_sub - 1] != "f")
        assert len(t.queries) == 2 * len(t.placed) + 2 * sum(inv["absent"].values())
        assert legal(t.slots, cshift) and len({(p.sub, p.key) for p in t.placed}) == len(t.placed) == int((t.slots != 0).sum())
    assert first == last == set(pc.CLASSES) and middle == {(v, c) for v in range(pc.VARIANTS) for c in pc.CLASSES}
    assert home_at == {"first", "last", "middle"}
    assert sum(1 for t in tabs if t.slots[0] and t.slots[-1]) >= pc.VARIANTS - 2


def test_accepted_share_of_candidates(gpu_lib):
    """the decode inverts the hash of the strand the forward hash chose: about half of the candidates that chain_case decoded hash back
    (each table's own count, so the figure printed does not depend on what else ran)"""
    stats = [t.stats for case in CASES for t in pc.chain_case(*case)]
    tried, kept = sum(s["tried"] for s in stats), sum(s["kept"] for s in stats)
    print("packed_corpus: %d of %d decoded candidates hash back to their (sub-table, key): %.3f" % (kept, tried, kept / tried))
    assert tried > 10000 and 0.4 < kept / tried < 0.6


@pytest.mark.parametrize("l_pre,cshift", [(l, c) for l in (1, 4, 8) for c in range(1, 9)])
def test_sweep_holds_a_full_and_an_empty_region(l_pre, cshift):
    regs = (pc.sweep_case(l_pre, cshift) != 0).reshape(1 << l_pre, -1)
    assert regs.all(axis=1).any() and (~regs).all(axis=1).any() and regs.size == 1 << (l_pre + cshift)


# ---- from_slots / raw / restore ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,l_pre,cshift", CASES)
def test_from_slots_round_trips(gpu_lib, k, l_pre, cshift):
    for t in pc.chain_case(k, l_pre, cshift):
        h = t.host(gpu_lib)
        c, slots = h.raw()
        assert c == cshift and np.array_equal(slots, t.slots) and (h.k, h.l_pre, h.count()) == (k, l_pre, len(t.placed))
        slots[0] ^= U(1 << 20)   # a copy: the table does not change
        assert np.array_equal(h.raw()[1], t.slots)
        h.close()


def test_from_slots_refusals(gpu_lib):
    """a wrong length and a table of one slot per sub-table are refused"""
    for args in ((21, 4, 2, np.zeros(63, dtype=U)), (21, 4, 2, np.zeros(128, dtype=U)), (21, 4, 0, np.zeros(16, dtype=U)), (21, 4, -1, np.zeros(8, dtype=U)), (64, 4, 2, np.zeros(64, dtype=U))):
        with pytest.raises(gpu_lib.BfcGpuError, match="from_slots"):
            gpu_lib.HostTable.from_slots(*args)
    t = gpu_lib.HostTable.from_slots(21, 0, 1, np.array([0, 5 << 14 | 3], dtype=U))
    assert t.count() == 1 and t.raw()[0] == 1
    t.close()


def _restore_py(l_pre, subs):
    """bfc_ch_restore's rule restated: from 4 slots per sub-table, every stored value goes to the first free slot from its home; a value
    that finds its region full doubles every region (the slots re-placed in slot order) and tries again"""
    cshift, slots = 2, np.zeros(4 << l_pre, dtype=U)
    for s, vals in enumerate(subs):
        for v in vals:
            while True:
                cm = (1 << cshift) - 1
                free = [p & cm for p in range(int(v) >> 14 & cm, (int(v) >> 14 & cm) + cm + 1) if not slots[(s << cshift) + (p & cm)]]
                if free:
                    slots[(s << cshift) + free[0]] = v
                    break
                at = np.flatnonzero(slots)
                slots, cshift = pc.place(l_pre, cshift + 1, at >> cshift, slots[at]), cshift + 1
    return cshift, slots


def _dump(fn, k, l_pre, subs):
    with open(fn, "wb") as f:
        f.write(struct.pack("<II", k, l_pre))
        for vals in subs:
            f.write(struct.pack("<II", 4 if len(vals) else 0, len(vals)) + np.asarray(vals, dtype=U).tobytes())


def _random_subs(rng, l_pre, n, bits):
    keys = np.unique(rng.integers(0, 1 << bits, n, dtype=np.uint64))
    rng.shuffle(keys)
    sub = rng.integers(0, 1 << l_pre, len(keys))
    return [[int(k) << 14 | int(rng.integers(1, 256)) for k in keys[sub == s]] for s in range(1 << l_pre)]


@pytest.mark.parametrize("which", ["l_pre4", "l_pre8", "one_home"])
def test_restore_equals_its_restatement(gpu_lib, tmp_path, which):
    """random dumps written here restore to the restatement's table slot for slot: 3000 keys in 16 sub-tables (more than 4/7 full), 300
    keys in 256 (regions exactly full), and a dump whose sub-table 5 holds 8 keys of one home (cshift 3, that region full and wrapped)"""
    rng = np.random.default_rng(11)   # (a draw whose fullest sub-table of the 256 holds exactly 4 keys: no growth beyond cshift 2)
    if which == "one_home":
        l_pre, subs = 4, [[] for _ in range(16)]
        subs[5] = [int(k) << 14 | 2 for k in np.unique(rng.integers(0, 1 << 30, 8, dtype=np.uint64)) << U(3) | U(6)]
        subs[0] = [77 << 14 | 1]
    else:
        l_pre, n = (4, 3000) if which == "l_pre4" else (8, 300)
        subs = _random_subs(rng, l_pre, n, 42 - l_pre)
    fn = str(tmp_path / "t.dump")
    _dump(fn, 21, l_pre, subs)
    t = gpu_lib.HostTable.restore(fn)
    cshift, slots = _restore_py(l_pre, subs)
    got = t.raw()
    regs = (got[1] != 0).reshape(1 << l_pre, -1)
    load, n_full = regs.mean(), int(regs.all(axis=1).sum())
    print("restore %s: cshift %d, load %.2f, fullest region %d of %d, %d regions full" % (which, got[0], load, regs.sum(axis=1).max(), regs.shape[1], n_full))
    assert got[0] == cshift and np.array_equal(got[1], slots) and legal(got[1], cshift) and t.count() == sum(len(v) for v in subs)
    if which == "l_pre4":
        assert load > 4 / 7
    elif which == "l_pre8":
        assert n_full >= 1
    else:
        assert cshift == 3 and regs[5].all() and (got[1][5 << 3:6 << 3] >> U(14) & U(7) == 6).all()
    t.close()


# ---- the probe on the host: the reference side of the GPU tests ----------------------------------------------------------------------------

@pytest.mark.parametrize("k,l_pre,cshift", CASES)
def test_host_lookup_and_export(gpu_lib, k, l_pre, cshift):
    """occ_planes of every query, on both strands, is the recorded answer; export_sorted is the chosen keys"""
    for t in pc.chain_case(k, l_pre, cshift):
        h = t.host(gpu_lib)
        y, want = t.arrays()
        got = h.occ_planes(y)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, [(t.queries[i].cls, t.queries[i].sub, int(got[i]), int(want[i])) for i in bad[:5]]
        sizes, slots = h.export_sorted()
        assert np.array_equal(sizes, t.l1()[0]) and np.array_equal(slots, t.l1()[1])
        h.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_tables(gpu_lib, name, form):
    """a relaid or filled fixture holds the fixture's keys at the intended cshift in a legal layout; a filled one has at least three
    regions exactly full (d15's is more than 4/7 full overall), and its fillers are keys like any other"""
    t, d, full = table(gpu_lib, name, form)
    b = base(gpu_lib, name)
    cshift, slots = t.raw()
    regs = (slots != 0).reshape(1 << t.l_pre, -1)
    assert legal(slots, cshift) and (t.k, t.l_pre) == (b.k, b.l_pre)
    pairs = lambda x: set(zip(np.repeat(np.arange(1 << x.l_pre), x.export_sorted()[0]).tolist(), x.export_sorted()[1].tolist()))
    have = pairs(t)
    assert have >= pairs(b) and len(have) == t.count() == len(d.d) // 2
    if form == "relaid":
        assert cshift == RELAID[name] != b.raw()[0] and t.count() == b.count()
    else:
        sizes = b.export_sorted()[0]
        assert (1 << cshift) >= int(sizes.max()) > (1 << cshift) // 2 or cshift == 1
        assert len(full) == 3 and regs[full].all() and int(regs.all(axis=1).sum()) >= 3 and t.count() > b.count()
        print("filled %s: cshift %d, load %.3f" % (name, cshift, regs.mean()))
        if name == "d15":
            assert regs.mean() > 4 / 7


@pytest.mark.parametrize("name", FIXTURES)
def test_filled_twins_equal_the_string_oracles(gpu_lib, name):
    """on the filled fixtures the host twins unitigs, clip and pop_bubbles give the string oracles' results on the filled table's own dict"""
    t, d, full = table(gpu_lib, name, "filled")
    for min_cnt in (1, 2):
        assert gpu_lib.unitig_rows(*t.unitigs(min_cnt)) == want_unitigs(d, min_cnt)
    for kw in clip_sets(name):
        surv, stats, units = want_clip(d, key_of(kw))
        res, got = t.clip(**kw)
        assert clip_oracle.survivors_of_table(res) == surv and stats_of(got) == stats and gpu_lib.unitig_rows(*res.unitigs(1)) == units
        res.close()
    for kw in POP_SETS:
        surv, stats, units = want_pop(d, key_of(kw))
        res, got = t.pop_bubbles(**kw)
        assert bubble_oracle.survivors_of_table(res) == surv and stats_of(got) == stats and gpu_lib.unitig_rows(*res.unitigs(1)) == units
        res.close()


@pytest.mark.parametrize("how", ["clip", "pop"])
@pytest.mark.parametrize("name", FULL)
def test_full_result_region_of_a_cleaning(gpu_lib, name, how):
    """fillers that survive make one sub-table's survivors exactly 2^c: the host twin's result has cshift c and that region full, holds
    the oracle's survivors, and answers for them, for the removed nodes and for absent k-mers of every part of the full region"""
    inp, d, c, sub = full_input(gpu_lib, name, how)
    kw = FULL_KW[how]
    surv, stats, units = (want_clip if how == "clip" else want_pop)(d, key_of(kw))
    res, got = inp.clip(**kw) if how == "clip" else inp.pop_bubbles(**kw)
    cshift, slots = res.raw()
    assert cshift == c and (slots[sub << c:(sub + 1) << c] != 0).all() and legal(slots, c) and int(res.export_sorted()[0].max()) == 1 << c
    assert clip_oracle.survivors_of_table(res) == surv and stats_of(got) == stats and len(surv) < inp.count()
    assert gpu_lib.unitig_rows(*res.unitigs(1)) == units
    y, want = result_queries(gpu_lib, name, how)
    assert np.array_equal(res.occ_planes(y), want) and (want == -1).sum() >= 4 and (want >= 0).sum() == len(surv)
    res.close()


@functools.lru_cache(maxsize=None)
def result_queries(gpu_lib, name, how):
    """(planes, expected values) on the result of a full-region cleaning: every survivor, every removed node, absent k-mers of the full
    region (up to 64 homes spread over it)"""
    import graph_oracle
    inp, d, c, sub = full_input(gpu_lib, name, how)
    surv = (want_clip if how == "clip" else want_pop)(d, key_of(FULL_KW[how]))[0]
    nodes = sorted(s for s in d.d if s <= revcomp(s))
    y = graph_oracle.planes_of_strs(nodes, inp.k)
    want = np.array([surv.get(s, -1) for s in nodes], dtype=np.int16)
    extra = pc.absent_of_region(inp, sub, c, 64, 5)
    return np.concatenate([y, extra]), np.concatenate([want, np.full(len(extra), -1, dtype=np.int16)])


@pytest.mark.parametrize("name", FULL)
def test_full_result_region_of_a_union(gpu_lib, name):
    """bfc_ch_union of two tables whose keys of one sub-table number 2^c together: cshift c, that region full, the numpy union's slots"""
    import ctypes as C
    import tabcmp_oracle
    a, b, c, sub = full_input(gpu_lib, name, "union")
    L = gpu_lib._lib.load()
    u = gpu_lib.HostTable(L.bfc_ch_union((C.c_void_p * 2)(a.ptr, b.ptr), 2))
    cshift, slots = u.raw()
    assert cshift == c and (slots[sub << c:(sub + 1) << c] != 0).all() and legal(slots, c)
    sizes, want = tabcmp_oracle.Join(a.export_sorted(), b.export_sorted()).union()
    assert np.array_equal(u.export_sorted()[0], sizes) and np.array_equal(u.export_sorted()[1], want) and int(sizes.max()) == 1 << c
    u.close()
