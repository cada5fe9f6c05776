"""The count table's write path on placed k-mers (-m gpu): every case of commit_corpus.py counted call by call and held to the oracle --
statistics, the filter's bytes, the table in L1 form, the distinct keys bfcg_progress reports for every call -- and to what the case was
built for: how many k-mers were parked and replayed where (bfcg_commit_info), how the table is held (bfcg_table_info), which partition the
batches took.  Before anything is counted, every placed k-mer is held to bfcg_seg_place: the context's own region, identity, home and block
of its hash must be the corpus's restatement, or "placed" would mean "random" and the parity checks would still pass.

Which way a block took through k_commit_seg (in place, counter pairs, compare-and-swap) follows from the number of entries and the block's
size, which the case fixes and table_info confirms; it is not observed.

bfcg_progress after a park: the keys that a replay of parked k-mers creates were counted by no page of the hand-over log.  They belong to
the call at which the replay runs -- the one the context drains at -- so a case drains behind a call that parks (Case.sync_after) where it
goes on counting afterwards, and the no-drain runs park in their last call."""
import numpy as np
import pytest

import commit_corpus as cc
import oracle

pytestmark = pytest.mark.gpu

KNOBS = ("BFCG_SEG_BLOCK", "BFCG_SEG_TOTAL", "BFCG_COMMIT_K", "BFCG_ONEPASS_MIN_TILES", "BFCG_R", "BFCG_F1", "BFCG_SEG", "BFCG_ONEPASS", "BFCG_COLD_FRAC")


def _counter(gpu_lib, geom, monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in geom.env.items():
        monkeypatch.setenv(name, v)
    return gpu_lib.GpuCounter(geom.k, geom.bf_shift, l_pre=geom.l_pre, max_batch_pos=geom.max_batch_pos, **geom.kw)


def _placement(g, case):
    """the context's own placement of every k-mer of the case is the corpus's"""
    segments = g.table_info()["segments"]
    for key in case.keys() + case.absent:
        region, sid, home, block = g.seg_place(*key.Y)
        assert (region, sid, home) == (key.region, key.id, key.home), (case.name, key)
        if segments:
            assert block == cc.slot_of(key.home, case.blk_shift, case.seg_shift)[0], (case.name, key)


def _count(gpu_lib, g, case, ask=None):
    """the case call by call, drained where it says; `ask` (a list) receives bfcg_progress's answer after every call, not drained"""
    for i in range(len(case.calls)):
        seq, qual, off = case.stream(i)
        g.count_host(gpu_lib.to_stream(seq, off), gpu_lib.to_stream(qual, off))
        if ask is not None:
            ask.append(g.progress())
        elif i + 1 in case.sync_after:
            g.sync()
            rep = _report(g)
            assert {name: rep[name] for name in case.checks.get(i + 1, {})} == case.checks.get(i + 1, {}), (case.name, i + 1, rep)
    g.sync()


def _report(g):
    """commit_info, table_info and partition_info in one dict"""
    out = dict(g.commit_info())
    out.update(g.table_info())
    out.update(g.partition_info())
    return out


def _keys_want(case, exp):
    """the distinct keys bfcg_progress must give for every call: the oracle's after the same prefix -- but for the calls between one whose
    k-mers parked and the one the context drained at, where a run does not drain itself (Case.short_calls): those lack the parked keys"""
    short = getattr(case, "short_calls", set())
    return [v - (case.short_by if i + 1 in short else 0) for i, v in enumerate(exp["keys_after"])]


def _check(gpu_lib, g, case, exp, base=None, attach=True):
    """everything the context shows after the case against the oracle and the case's own claims; base: commit_info before the case"""
    tag = case.name
    calls, final, keys = g.progress()
    assert calls == final == len(case.calls), (tag, calls, final)
    assert keys[::-1] == _keys_want(case, exp), (tag, keys[::-1], exp["keys_after"])
    rep = _report(g)
    for name, want in case.want.items():
        got = rep[name] - (base or {}).get(name, 0) if name in ("seg_replayed", "table_replayed", "to_host_layout") else rep[name]
        if isinstance(want, tuple):
            assert got >= want[1], (tag, name, got, want, rep)
        else:
            assert got == want, (tag, name, got, want, rep)
    st = g.stats()
    assert (st["n_kmers"], st["n_high"], st["n_seen"]) == (exp["stats"]["n_kmers"], exp["stats"]["n_high"], exp["stats"]["n_seen"]), tag
    assert st["n_keys"] == exp["keys_after"][-1], tag
    assert np.array_equal(g.bloom_bytes(), exp["bloom"]), tag
    if rep["segments"] and attach:  # the table as the lookup kernels find it where the segments were converted for them, not for the export
        km = gpu_lib.GpuKmers(g)
        ask = case.keys() + case.absent
        got = km.lookup_strings([key.row.decode() for key in ask])
        assert [int(v) for v in got] == [exp["get"][key.Y] for key in ask], tag
        assert all(exp["get"][key.Y] == -1 for key in case.absent) and (not case.full_homes or len(case.absent) == len(case.full_homes)), tag
        km.close()
    sizes, slots = g.export_table().export_sorted()
    assert np.array_equal(sizes, exp["table"][0]) and np.array_equal(slots, exp["table"][1]), tag
    return rep


RESET_PAIR = ("leave_segments", "after_reset")   # counted on one context, below
WHOLE = [n for n in cc.CASES if n not in RESET_PAIR and not n.startswith(("windows_tail", "windows_nodrain"))]


@pytest.mark.parametrize("name", WHOLE)
def test_case(gpu_lib, name, monkeypatch):
    case, exp = cc.case(name), cc.expected(name)
    g = _counter(gpu_lib, case.geom, monkeypatch)
    _placement(g, case)
    _count(gpu_lib, g, case)
    _check(gpu_lib, g, case, exp)
    g.close()


@pytest.mark.parametrize("name", ["home_last_full_1calls", "way_in_place_full_block", "block_three_growths", "windows_K2"])
def test_export_straight_from_the_segments(gpu_lib, name, monkeypatch):
    """the cases above attach the lookup first, which converts the segments for a context that counts on; here bfcg_export_table converts them
    itself, sized for the export (seg_to_legacy with for_export), from a full block, blocks of 2^3 and 2^5 slots and 512 regions"""
    case, exp = cc.case(name), cc.expected(name)
    g = _counter(gpu_lib, case.geom, monkeypatch)
    _count(gpu_lib, g, case)
    rep = _check(gpu_lib, g, case, exp, attach=False)
    assert rep["segments"] and rep["to_host_layout"] == 0 and g.commit_info()["to_host_layout"] == 1 and not g.table_info()["segments"], name
    g.close()


@pytest.mark.parametrize("name", ["home_odd_more_2calls", "block_full_low_load", "windows_K4"])
def test_progress_counts_the_keys_a_replay_created(gpu_lib, name, monkeypatch):
    """drain() took the distinct keys of the call it drains at BEFORE seg_maintain replayed the parked k-mers, and the following window's pages
    were added to that stale figure: the call that parked reported too few keys, and so did every call of the next window but the last.
    The figure is now taken again after a replay."""
    case, exp = cc.case(name), cc.expected(name)
    g = _counter(gpu_lib, case.geom, monkeypatch)
    park = min(case.sync_after)
    for i in range(len(case.calls)):
        seq, qual, off = case.stream(i)
        g.count_host(gpu_lib.to_stream(seq, off), gpu_lib.to_stream(qual, off))
        if i + 1 == park:
            g.sync()
            assert g.commit_info()["seg_replayed"] > 0, name
            assert g.progress()[2][0] == exp["keys_after"][i], (name, "the call that parked", g.progress(), exp["keys_after"])
    calls, final, keys = g.progress()   # not drained: the calls the context knows to be complete
    assert keys[::-1] == exp["keys_after"][:final], (name, keys[::-1], exp["keys_after"])
    g.sync()
    assert g.progress()[2][::-1] == exp["keys_after"], name
    g.close()


@pytest.mark.parametrize("name", ["windows_tail_K2", "windows_tail_K4"])
def test_progress_asked_between_calls_without_draining(gpu_lib, name, monkeypatch):
    """bfcg_progress after every call of a run that is never drained before its end: whatever call it names as complete, the keys it gives
    for that call and the calls before are the oracle's after the same prefix; the last call parks, and the drain at the end replays"""
    case, exp = cc.case(name), cc.expected(name)
    g = _counter(gpu_lib, case.geom, monkeypatch)
    _placement(g, case)
    asked = []
    _count(gpu_lib, g, case, ask=asked)
    for i, (calls, final, keys) in enumerate(asked):
        assert calls == i + 1 and final <= calls, (name, i, calls, final)
        assert keys[::-1] == exp["keys_after"][final - len(keys):final], (name, i, final, keys, exp["keys_after"])
    assert max(final for calls, final, keys in asked) >= 2, (name, asked)   # (some answer named a call that had created keys)
    _check(gpu_lib, g, case, exp)
    g.close()


@pytest.mark.parametrize("name", ["windows_nodrain_K1", "windows_nodrain_K4"])
def test_progress_of_a_call_that_parks_and_is_not_drained(gpu_lib, name, monkeypatch):
    """what remains of the fault above by construction, pinned: call 5 parks every entry of its page and the run goes on undrained.  The
    parked entries carry no call, so the 9 keys their replay creates go to the call the context drains at; the calls from the parking one up
    to that one report exactly 9 keys fewer than the oracle, for good; every call from the draining one on is the oracle's, asked between
    the calls and at the end; statistics, filter and table are the oracle's"""
    case, exp = cc.case(name), cc.expected(name)
    assert case.short_calls and case.short_by == 9 and not case.sync_after
    want = _keys_want(case, exp)
    assert [exp["keys_after"][i - 1] - want[i - 1] for i in sorted(case.short_calls)] == [9] * len(case.short_calls) and want[-1] == exp["keys_after"][-1]
    g = _counter(gpu_lib, case.geom, monkeypatch)
    _placement(g, case)
    asked = []
    _count(gpu_lib, g, case, ask=asked)
    for i, (calls, final, keys) in enumerate(asked):
        assert calls == i + 1 and final <= calls and keys[::-1] == want[final - len(keys):final], (name, i, final, keys, want)
    assert max(final for calls, final, keys in asked) > max(case.short_calls), (name, asked)   # (a short call and a later, exact one were named complete mid-run)
    _check(gpu_lib, g, case, exp)
    g.close()


def test_segments_left_with_parked_kmers_then_reset(gpu_lib, monkeypatch):
    """the segments leave for the host's layout while k-mers are parked (seg_to_legacy with ST_TAB_OVF != 0, k_table_replay), two more calls
    are counted there; after bfcg_reset the same context counts a second case in segments again"""
    first, second = cc.case("leave_segments"), cc.case("after_reset")
    g = _counter(gpu_lib, first.geom, monkeypatch)
    _placement(g, first)
    _count(gpu_lib, g, first)
    rep = _check(gpu_lib, g, first, cc.expected("leave_segments"))
    g.reset()
    assert g.table_info()["segments"] and g.progress()[:2] == (0, 0)
    _placement(g, second)
    _count(gpu_lib, g, second)
    _check(gpu_lib, g, second, cc.expected("after_reset"), base=rep)
    g.close()


def test_crowded_region_trips_stream_mode(gpu_lib, monkeypatch):
    """more than ag_cap = 256 distinct seen k-mers of one region in one batch: the aggregation table overflows (agg_add gives up, the k-mer is
    committed on its own), the region counts as crowded, and the next batches are streamed to k_commit_stream"""
    geom = cc.HOST(21, 8, 3)
    g = _counter(gpu_lib, geom, monkeypatch)
    oc = oracle.Counter(geom.k, geom.bf_shift, l_pre=geom.l_pre)
    seq, qual, off = cc.crowded_reads()
    placed = cc.case("host_chain_k21_l8_c3_park")
    batches = [(seq, qual, off), placed.stream(0), placed.stream(1), (seq, qual, off)]
    for s, q, o in batches:
        oc.count(s, q, o)
        g.count_host(gpu_lib.to_stream(s, o), gpu_lib.to_stream(q, o))
        g.sync()
    st, ost = g.stats(), oc.stats()
    assert st["stream_batches"] >= 1 and not g.table_info()["segments"], st
    assert (st["n_kmers"], st["n_high"], st["n_seen"], st["n_keys"]) == (ost["n_kmers"], ost["n_high"], ost["n_seen"], oc.table_count())
    assert np.array_equal(g.bloom_bytes(), oc.bloom_bytes())
    sizes, slots = g.export_table().export_sorted()
    osz, osl = oc.export()
    assert np.array_equal(sizes, osz) and np.array_equal(slots, osl)
    g.close(); oc.close()
