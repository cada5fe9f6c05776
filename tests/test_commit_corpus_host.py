"""commit_corpus.py held to what it says it contains.  No GPU: the placements against the library's host instances of the functions that place a
k-mer (bfcg_seg_id_host: seg_id, seg_home, seg_unpack; bfcg_kmer_decode_host; the oracle's ch_subkey), the per-call key counts against the
oracle counted prefix by prefix, the final tables against the multiplicities the cases chose, and three cases through the live reference
where oracle/_ref has it.  test_gpu_commit.py then has one expectation per case: commit_corpus.expected()."""
import collections
import ctypes as C

import numpy as np
import pytest

import commit_corpus as cc
import oracle
from packed_corpus import kmer_of_hash

U = np.uint64
needs_ref = pytest.mark.skipif(not oracle.have_ref(), reason="oracle/_ref/libbfcref.so not built")


def _L():
    from bfc_amd import _lib
    return _lib.load()


def _slot(case, key, seg_shift=None):
    return cc.slot_of(key.home, case.blk_shift, case.seg_shift if seg_shift is None else seg_shift)


@pytest.mark.parametrize("k, b, rs, want", [(21, 16, 0, (7, 0, 0, 0, 7, 7)), (21, 22, 4, (4, 9, 4, 5, 4, 13)), (21, 24, 4, (4, 11, 5, 6, 4, 15)), (21, 28, 0, (8, 11, 5, 6, 8, 19)),
                                            (33, 16, 0, (7, 0, 0, 0, 7, 7)), (47, 16, 0, (7, 0, 0, 0, 7, 7)), (31, 33, 0, (8, 16, 8, 8, 8, 24)), (33, 37, 0, (8, 20, 10, 10, 8, 28))])
def test_geometry_restated(k, b, rs, want):
    """R, F, F1, F2, seg_lo, seg_hi of bfcg_create, by hand from bfcg_ctx.hip for the corpus's geometries and two of BASELINE.json's"""
    g = cc.geometry(k, b, rs)
    assert (g.R, g.F, g.F1, g.F2, g.seg_lo, g.seg_hi) == want


@pytest.mark.parametrize("k, b, rs", [(21, 16, 0), (21, 22, 4), (21, 24, 4), (33, 16, 0), (47, 16, 0), (31, 33, 0), (33, 37, 0), (21, 28, 0)])
def test_numpy_placement_is_the_librarys(gpu_lib, k, b, rs):
    """seg_id, seg_home and the unpack round trip of kmer_dev.h as the host compiles them, on random hashes and on the edges of the fields"""
    L, g = _L(), cc.geometry(k, b, rs)
    rng = np.random.default_rng(k * b)
    y0 = rng.integers(0, 1 << k, 400, dtype=np.uint64)
    y1 = rng.integers(0, 1 << k, 400, dtype=np.uint64)
    y0[:4], y1[:4] = [0, (1 << k) - 1, 0, (1 << k) - 1], [0, 0, (1 << k) - 1, (1 << k) - 1]
    sid, home, region = cc.seg_id(g, y0, y1), cc.seg_home(cc.seg_id(g, y0, y1)), cc.fine_id(g, y0, y1)
    out = (C.c_uint64 * 4)()
    for i in range(len(y0)):
        assert L.bfcg_seg_id_host(k, g.seg_lo, g.seg_hi, int(region[i]), int(y0[i]), int(y1[i]), out) == 0
        assert (int(out[0]), int(out[1])) == (int(sid[i]), int(home[i])) and int(home[i]) < 1 << 26
        if 2 * k - (g.seg_hi - g.seg_lo) <= 50:  # (the identity fits a slot's key: the geometries that keep segments at all)
            assert (int(out[2]), int(out[3])) == (int(y0[i]), int(y1[i])) == cc.seg_unpack(g, int(region[i]), int(sid[i]))
        if k >= b - 9:  # the region is the bit field [R, bf_shift - 9) of Y0 (what Picker._draw sets)
            assert int(region[i]) == (int(y0[i]) & ((1 << (b - 9)) - 1)) >> g.R
    assert L.bfcg_seg_id_host(k, 5, 4, 0, 0, 0, out) == -1


@pytest.mark.parametrize("k", [21, 33, 37])
def test_inverse_hash_is_the_librarys_decode(gpu_lib, k):
    """planes_of_hash (any k) against bfcg_kmer_decode_host (k <= 37)"""
    rng = np.random.default_rng(k)
    for _ in range(100):
        Y = int(rng.integers(0, 1 << k)), int(rng.integers(0, 1 << k))
        assert cc.planes_of_hash(k, *Y) == kmer_of_hash(k, *Y)


@pytest.mark.parametrize("k", [21, 33, 47, 63])
def test_inverse_hash_round_trip(k):
    """at every k: the k-mer of a hash is hashed back to it by the oracle, on the strand the hash chose (about half of the hashes)"""
    rng = np.random.default_rng(k)
    Ys = [(int(rng.integers(0, 1 << k)), int(rng.integers(0, 1 << k))) for _ in range(200)]
    rows = np.array([cc.row_of_planes(k, *cc.planes_of_hash(k, *Y)) for Y in Ys], dtype=np.uint8)
    back = cc.forward(k, rows)
    same = [(int(a), int(b)) == Y for (a, b), Y in zip(back, Ys)]
    assert 60 <= sum(same) <= 140


@pytest.mark.parametrize("name", list(cc.CASES))
def test_case_is_legal_and_counts_as_it_says(name):
    """every placement is the one asked for, every call fits its context, and the per-call key counts are the oracle's prefix by prefix; the
    oracle's final table holds every k-mer with the count its multiplicity gives (saturating) and no absent one"""
    case, exp = cc.case(name), cc.expected(name)
    g = cc.geometry(case.geom.k, case.geom.bf_shift, case.geom.kw.get("region_shift", 0))
    keys = case.keys()
    assert len(set(key.Y for key in keys + case.absent)) == len(keys) + len(case.absent)
    assert not set(key.Y for key in case.absent) & set(key.Y for key in keys)
    for key in keys + case.absent:
        y0, y1 = np.array([key.Y[0]], dtype=U), np.array([key.Y[1]], dtype=U)
        assert key.region == int(cc.fine_id(g, y0, y1)[0]) < 1 << g.F and key.id == int(cc.seg_id(g, y0, y1)[0]) and key.home == int(cc.seg_home(key.id))
        assert len(key.row) == case.geom.k
    back = cc.forward(case.geom.k, np.frombuffer(b"".join(key.row for key in keys + case.absent), dtype=np.uint8))
    assert [(int(a), int(b)) for a, b in back] == [key.Y for key in keys + case.absent]
    assert all(0 < case.positions(i) <= case.geom.max_batch_pos for i in range(len(case.calls))) and len(case.calls) <= 63
    assert case.sync_after <= set(range(1, len(case.calls) + 1))
    assert exp["keys_after"] == case.keys_after(), name
    assert sum(exp["table"][0]) == exp["keys_after"][-1]
    tot = case.totals()
    for key in keys:
        n, h = tot[key.Y]
        got = exp["get"][key.Y]
        if getattr(case, "shared_bits", False):
            assert got == -1 or (got & 0xff) in (min(255, n - 1), min(255, n)), (name, key, n, got)
            continue
        assert got == (-1 if n < 2 else got) and (n < 2 or got & 0xff == min(255, n - 1)), (name, key, n, got)
        if n >= 2:  # the first read of a k-mer is not inserted: of high quality or not
            assert min(63, h - 1) <= got >> 8 <= min(63, h, n - 1), (name, key, n, h, got)
    assert all(exp["get"][key.Y] == -1 for key in case.absent)


def _names(prefix):
    return [n for n in cc.CASES if n.startswith(prefix)]


def test_inventory_one_home():
    """2^4 - 1, 2^4 and 2^4 + 1 keys of an even home, an odd home and the last slot, in one, two and three calls; the creating call one batch"""
    seen = set()
    for name in _names("home_"):
        case = cc.case(name)
        _, tag, fill, calls = name.split("_")
        (role, keys), = case.roles.items()
        home = {"even": 6, "odd": 9, "last": 15}[tag]
        assert all(key.region == 0 and _slot(case, key) == (0, home) for key in keys + case.absent) and home % 2 == (tag != "even")
        assert len(keys) == 16 + {"less": -1, "full": 0, "more": 1}[fill] and len(case.calls) == int(calls[0])
        assert (case.seg_shift, case.blk_shift) == (4, 12) and case.geom.kw["tab_cshift"] == 1
        creating = 0 if len(case.calls) == 1 else 1
        assert case.positions(creating) <= cc.ONE_BATCH and cc.expected(name)["keys_after"][creating] == len(keys)
        per_key = collections.Counter(it.n for it in case.calls[creating])
        assert len(per_key) == 1   # every key as often as every other: whichever finds no slot is parked the same number of times
        assert case.want["seg_replayed"] == (list(per_key)[0] - (1 if creating == 0 else 0) if fill == "more" else 0)
        assert case.full_homes == ([home] if fill != "less" else []) and len(case.absent) == 1
        seen.add((tag, fill, calls))
    assert len(seen) == 27


def test_inventory_chains_and_pairs():
    for name, homes in (("interleaved_2", (15, 4)), ("interleaved_3", (15, 0, 1))):
        case = cc.case(name)
        assert [int(r[4:]) for r in case.roles] == list(homes) and sum(len(v) for v in case.roles.values()) == 16
        assert all(_slot(case, key) == (0, int(r[4:])) for r, v in case.roles.items() for key in v)
        assert [_slot(case, key)[1] for key in case.absent] == list(homes) and case.positions(1) <= cc.ONE_BATCH
    case = cc.case("pair_read")
    r = case.roles
    assert [_slot(case, key)[1] for key in r["even"] + r["odd"] + r["hot"]] == [2, 2, 7, 7, 10, 10]
    hot = [it for it in case.calls[1] if it.key in r["hot"]]
    assert [it.n for it in hot] == [65, 65] and not any(it.key in r["hot"] for it in case.calls[0]) and case.positions(1) <= cc.ONE_BATCH


def test_inventory_saturation():
    for name in ("saturation_whole", "saturation_split"):
        case, exp = cc.case(name), cc.expected(name)
        tot = case.totals()
        got = {}
        for role, (key,) in case.roles.items():
            seen, high = int(role.split("_")[0][4:]), int(role.split("_")[1][4:])
            n, h = tot[key.Y]
            extra = 2 if name.endswith("split") else 0   # (the last call comes on every key twice more)
            assert n == seen + 1 + extra and (h == high + extra or name.endswith("split"))
            got[(seen, high)] = exp["get"][key.Y]
            assert got[(seen, high)] & 0xff == min(255, seen + extra)
        assert set(s for s, h in got) == set(cc.SAT_SEEN) and all(set(h for s, h in got if s == seen) >= {0, 1, seen} for seen in cc.SAT_SEEN)
        assert all(set(h for s, h in got if s == seen) >= {62, 63, 64} for seen in cc.SAT_SEEN if seen >= 64)
        assert {v >> 8 for v in got.values()} >= {0, 1, 62, 63} and {v & 0xff for v in got.values()} >= ({2, 3, 254, 255} if extra == 0 else {4, 5, 255})
        assert case.seg_shift == 10
    split = cc.case("saturation_split")
    assert cc.expected("saturation_split")["keys_after"][:2] == [0, 36] and max(split.positions(i) for i in (2, 3)) > 20 * cc.ONE_BATCH
    assert any(cc.expected("saturation_split")["get"][it.key.Y] == (63 << 8 | 255) for it in split.calls[4])
    case = cc.case("park_then_saturate")
    assert len(case.roles["home5"]) == 17 and case.positions(0) <= cc.ONE_BATCH and case.sync_after == {1} and case.want["seg_replayed"] == 7
    assert sorted(set(v & 0xff for v in cc.expected("park_then_saturate")["get"].values())) == [7, 254, 255]


def test_inventory_ways_and_blocks():
    case = cc.case("way_in_place")
    assert case.seg_shift == 10 and case.entries == [0, 32, 13] and all(e * 16 < 1 << 10 for e in case.entries)
    assert [sum(it.n for it in items) for items in case.calls][1:] == case.entries[1:]   # (behind the first call every read is an entry)
    assert [it.n for it in case.calls[1] if it.key in case.roles["twice"]] == [2]
    case = cc.case("way_in_place_full_block")
    assert (case.seg_shift, case.blk_shift) == (10, 5) and all(_slot(case, key) == (7, 20) for key in case.keys() + case.absent) and len(case.roles["home20"]) == 32
    assert [sum(it.n for it in items) for items in case.calls[2:]] == [1] * 33 and 1 * 16 < 1 << 5 and cc.expected(case.name)["keys_after"][1] == 32
    assert case.checks == {34: dict(seg_replayed=0, seg_growths=0, seg_shift=10)} and 34 in case.sync_after
    assert [items[0].key for items in case.calls[2:]] == case.roles["home20"] + case.roles["late"] and 33 * 2 <= 0.62 * (1 << 10)
    case = cc.case("way_cas")
    hot, = case.roles["hot"]
    assert [it.n for it in case.calls[0] if it.key == hot] == [65600] and len(case.roles["plain"]) == 40
    assert len({key.region for key in case.keys()}) == 1 and sum(it.n for it in case.calls[0]) - 41 >= 65536
    assert len(case.keys()) * 2 <= 1 << case.seg_shift                 # (nothing is parked: the segment of 2^7 slots takes the 41 keys)
    case = cc.case("block_full_low_load")
    assert (case.seg_shift, case.blk_shift) == (6, 3)
    assert [_slot(case, key)[0] for key in case.roles["stay"] + case.roles["move"]] == [2] * 9
    assert [_slot(case, key, 7)[0] for key in case.roles["stay"] + case.roles["move"]] == [2] * 5 + [10] * 4
    assert 9 * 7 <= 1 << 6                                             # (a seventh of the segment and less)
    case = cc.case("block_three_growths")
    for stage, (shift, blk) in enumerate(((6, 5), (7, 3), (8, 17))):
        mine = [_slot(case, key, shift)[0] for key in case.roles["stage%d" % stage]]
        others = [_slot(case, key, shift)[0] for s in range(stage) for key in case.roles["stage%d" % s]]
        assert mine == [blk] * 9 and blk not in others
    assert case.sync_after == {1, 2, 3} and case.want["seg_growths"] == 3


def test_inventory_windows():
    for name in _names("windows_"):
        case, exp = cc.case(name), cc.expected(name)
        K = int(name[-1])
        assert case.geom.env == dict(BFCG_ONEPASS_MIN_TILES="0", BFCG_COMMIT_K=str(K)) and cc.geometry(21, 22, 4).F == 9 and case.seg_shift == 4
        cap2 = (case.geom.max_batch_pos + case.geom.max_batch_pos // 8) // 512 + 64
        for items in case.calls:   # a region's share of a batch stays below its slab
            share = collections.Counter()
            for it in items:
                share[it.key.region] += it.n
            assert max(share.values()) < cap2 // 2
        for r in cc.W_REGIONS:
            assert len(case.roles["fill%d" % r]) == 16 and len(case.roles["late%d" % r]) == 3
            assert all(key.region == r for key in case.roles["fill%d" % r] + case.roles["late%d" % r])
        after = exp["keys_after"]
        assert after[0] == 0 and after[2] == after[1] and after[3] == after[2]      # pages that create nothing
        p = case.parking_call
        late = [key for r in cc.W_REGIONS for key in case.roles["late%d" % r]]
        assert {it.key for it in case.calls[p - 1]} >= set(late) and after[p - 1] - after[p - 2] == 9
        assert (p == len(case.calls) and not case.sync_after) if "tail" in name else case.sync_after == (set() if "nodrain" in name else {p})
        assert case.short_calls == ({p} if K == 1 else {p, p + 1}) if "nodrain" in name else not case.short_calls
        sat, = case.roles["sat"]
        assert exp["get"][sat.Y] & 0xff == 255 and sum(1 for items in case.calls if any(it.key == sat for it in items)) >= 4
    assert {int(n[-1]) for n in _names("windows_K")} == {1, 2, 4}


def test_inventory_leaving_and_host_layout():
    case = cc.case("leave_segments")
    assert case.geom.env == dict(BFCG_SEG_BLOCK="4", BFCG_SEG_TOTAL="5") and len(case.roles["home3"]) == 17 and len(case.calls) == 3 and case.sync_after == {1}
    assert all(_slot(case, key) == (0, 3) for key in case.roles["home3"]) and case.positions(0) <= cc.ONE_BATCH
    assert cc.case("after_reset").geom == case.geom and len(cc.case("after_reset").roles["home12"]) == 12
    seen = set()
    for name in _names("host_chain"):
        case = cc.case(name)
        k, lp, cs = case.geom.k, case.P.l_pre, case.geom.kw["tab_cshift"]
        assert case.geom.kw["table_layout"] == 1 and lp == oracle.lib().orc_ch_clamp_lpre(k, case.geom.l_pre) == case.geom.l_pre
        R, n_sub, m = 1 << cs, 1 << lp, (1 << cs) - 1
        want = [("wrap", 0, R - 1, R), ("odd", n_sub // 2, 1, R)] + ([("over", n_sub - 1, 0, R + 1)] if name.endswith("park") else [])
        assert list(case.roles) == [w[0] for w in want]
        for role, sub, home, n in want:
            assert len(case.roles[role]) == n and all(key.sub == sub and key.skey & m == home for key in case.roles[role])
        assert cc.expected(name)["keys_after"][:2] == [0, len(case.keys())]
        seen.add((k, lp, cs))
    assert seen == {(21, 4, 1), (21, 8, 3), (33, 16, 3), (47, 24, 1)}
    case = cc.case("host_aggregated")
    assert [sum(it.n for it in case.calls[0] if it.key in keys) - 1 for keys in case.roles.values()] == list(cc.AGG_SEEN) and max(cc.AGG_SEEN) > 0xffff
    for name, k in (("host_same_y0_k33", 33), ("host_same_y0_k47", 47)):
        case = cc.case(name)
        two, three = case.roles["two"], case.roles["three"]
        assert case.geom.k == k and len({key.Y[0] for key in two}) == 1 and len({key.Y[1] for key in two}) == 2
        assert len({key.Y[0] for key in three}) == 1 and len({key.Y[1] for key in three}) == 3 and two[0].Y[0] != three[0].Y[0]
        first = {it.key: it.n for it in case.calls[0]}
        assert [first.get(key, 0) for key in three] == [1, 300, 0] and [first[key] for key in two] == [3, 3]
        assert len({(key.sub, key.region) for key in three}) == 1


@needs_ref
@pytest.mark.parametrize("name", ["home_last_more_3calls", "saturation_split", "host_same_y0_k33"])
def test_live_reference_counts_the_case_alike(name):
    case, exp = cc.case(name), cc.expected(name)
    after, r = cc.count_case(case, lambda *a, **kw: oracle.Counter(*a, impl="ref", **kw))
    assert after == exp["keys_after"]
    assert np.array_equal(r.bloom_bytes(), exp["bloom"])
    sizes, slots = r.export()
    assert np.array_equal(sizes, exp["table"][0]) and np.array_equal(slots, exp["table"][1])
    r.close()
