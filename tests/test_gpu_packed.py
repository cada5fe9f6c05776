"""GPU tests (-m gpu) of every read-out of the count table on the tables of tests/packed_corpus.py: regions exactly full, chains that wrap
round a region's end, probes that only the bound `probe <= cmask` stops -- laid out slot by slot (chain_case), graph fixtures relaid and
filled up, inputs whose clip / pop_bubbles / union result has a full region, and random slots for the passes that stream.  Every table
is GpuKmers(HostTable.from_slots(...)).  The reference side is the recorded answer of every query, numpy on the chosen slots, the host
twin on the same HostTable, and the string oracles on its dict; tests/test_packed_host.py holds the twins to the same oracles without a
GPU and makes the tables."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import packed_corpus as pc
import tabcmp_oracle
import test_packed_host as PH
from graph_oracle import census_of_nb, in_mask, paths, strs_of_planes
from test_gpu_kmers import _rows
from test_gpu_pop import _census_lines, _unitig_lines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64


def _decode(L, k, l_pre, subs, vals):
    """the host's instance of the slot decode (bfcg_kdec.h) on (sub-table, slot value) pairs: planes (n, 2) u64"""
    y, out = np.zeros((len(vals), 2), dtype=U), (C.c_uint64 * 2)()
    for i, (s, v) in enumerate(zip(subs, vals)):
        assert L.bfcg_kmer_decode_host(k, l_pre, int(s), int(v), out) == 0
        y[i] = out[0], out[1]
    return y


def _listing_of(L, k, l_pre, cshift, slots, min_cnt, min_diff, sub_lo=0, sub_hi=None):
    """what list() must give, in its order (slot order): (y, count, high) of the slots of sub-tables [sub_lo, sub_hi) that pass the filter"""
    sub_hi = (len(slots) >> cshift) if sub_hi is None else sub_hi
    at = np.flatnonzero(slots)
    at = at[(at >> cshift >= sub_lo) & (at >> cshift < sub_hi)]
    at = at[tabcmp_oracle.keep(slots[at], min_cnt, min_diff)]
    v = slots[at]
    return _decode(L, k, l_pre, at >> cshift, v), (v & U(0xff)).astype(np.uint8), (v >> U(8) & U(0x3f)).astype(np.uint8)


def _same_listing(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)


def _hist_of(slots):
    v = slots[slots != 0]
    cnt, high = np.bincount((v & U(0xff)).astype(np.int64), minlength=256), np.bincount((v >> U(8) & U(0x3f)).astype(np.int64), minlength=64)
    top = int(cnt[3:].max()) if len(v) else 0
    return (3 + int(cnt[3:].argmax()) if top else -1), cnt.astype(U), high.astype(U)   # bfc_ch_hist: the first of the largest bins from 3 on


def _check_streams(km, slots, cshift):
    """hist, sub_sizes and hist_sizes against numpy on the slots"""
    mode, cnt, high = _hist_of(slots)
    sizes = (slots != 0).reshape(-1, 1 << cshift).sum(axis=1)
    got = km.hist()
    assert got[0] == mode and np.array_equal(got[1], cnt) and np.array_equal(got[2], high)
    assert np.array_equal(km.sub_sizes(), sizes)
    got = km.hist_sizes()
    assert got[0] == mode and np.array_equal(got[1], cnt) and np.array_equal(got[2], high) and np.array_equal(got[3], sizes)


def _stream_of(y, k):
    """the k-mers as reads of exactly k bases: (stream u8, offsets u64)"""
    strs = strs_of_planes(y, k)
    return np.frombuffer(b"".join(s + b"\n" for s in strs), dtype=np.uint8), np.arange(len(strs) + 1, dtype=U) * U(k + 1)


# ---- chain_case: tables laid out slot by slot --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,l_pre,cshift", PH.CASES)
def test_chain_lookup_profile_neighbors(gpu_lib, k, l_pre, cshift):
    """lookup of every query is the recorded answer and the host twin's -- keys displaced by every distance in full regions, absent keys
    that walk a whole region, near misses -- on both strands; profile and read_stats of the queries as reads of k bases, and neighbors,
    equal the host twin; extend finds every present seed"""
    for t in pc.chain_case(k, l_pre, cshift):
        h = t.host(gpu_lib)
        km = gpu_lib.GpuKmers(h)
        assert (km.k, km.l_pre, km.cshift) == (k, l_pre, cshift)
        y, want = t.arrays()
        got = km.lookup(y)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, [(t.variant, t.queries[i].cls, t.queries[i].sub, int(got[i]), int(want[i])) for i in bad[:8]]
        assert np.array_equal(got, h.occ_planes(y)) and km.n_found == int((want >= 0).sum())
        stream, off = _stream_of(y, k)
        prof = np.full(len(stream), -2, dtype=np.int16)
        prof[k - 1::k + 1] = want
        assert np.array_equal(km.profile(stream), prof)
        for min_cov in (1, 2, 255):
            assert np.array_equal(km.read_stats(stream, off, min_cov), h.read_stats(stream, off, min_cov))
        assert np.array_equal(km.neighbors(y), h.neighbors(y))
        got, twin = km.extend(y, 1, 4), h.extend(y, 1, 4)   # the seed's own probe: 4 = the seed is absent
        assert all(np.array_equal(a, b) for a, b in zip(got, twin)) and np.array_equal(got[2] == 4, want < 0)
        km.close()
        h.close()


@pytest.mark.parametrize("k,l_pre,cshift", PH.CASES)
def test_chain_list_and_spectrum(gpu_lib, k, l_pre, cshift):
    """list of the whole table and of sub-table ranges at min_cnt 2 and 255 (and unfiltered) is the chosen slots in slot order, decoded by
    the host's instance of the decode -- at k = 21 these are the k-mers the builder chose; hist, sub_sizes, hist_sizes are numpy's"""
    L, n_sub = gpu_lib._lib.load(), 1 << l_pre
    for t in pc.chain_case(k, l_pre, cshift):
        h = t.host(gpu_lib)
        km = gpu_lib.GpuKmers(h)
        _check_streams(km, t.slots, cshift)
        for min_cnt, min_diff, lo, hi in ((2, 0, 0, n_sub), (255, 0, 0, n_sub), (0, -63, 0, n_sub), (2, 0, n_sub // 2 - 2, n_sub // 2 + 3), (255, -63, 0, 1), (2, -63, n_sub - 1, n_sub),
                                          (1, -63, 1, n_sub - 1)):
            want = _listing_of(L, k, l_pre, cshift, t.slots, min_cnt, min_diff, lo, hi)
            assert _same_listing(km.list(min_cnt, min_diff, lo, hi), want), (t.variant, min_cnt, min_diff, lo, hi)
        if k <= 32:
            chosen = {(p.sub, p.key): p.y for p in sorted(t.placed, key=lambda p: (p.sub, p.pos))}
            y = km.list(0, -63)[0]
            assert [tuple(int(v) for v in r) for r in y] == list(chosen.values()) and len(y) == len(t.placed)
        km.close()
        h.close()


@pytest.mark.parametrize("k,l_pre,cshift", PH.CASES)
def test_chain_two_tables(gpu_lib, k, l_pre, cshift):
    """joint_hist and list_vs in both directions -- the packed table is probed in one of them -- and union both ways, against
    tabcmp_oracle on the chosen slots; the second table holds every other key of the first and others, at cshift + 2.  Then the results
    that carry a full region over: clip(max_rounds=0) and the union with an empty table hold the same keys at the same cshift and answer
    every query"""
    L = gpu_lib._lib.load()
    for t in pc.chain_case(k, l_pre, cshift):
        cb, sb = pc.second_table(k, l_pre, cshift, t.variant)
        ha, hb = t.host(gpu_lib), gpu_lib.HostTable.from_slots(k, l_pre, cb, sb)
        ka, kb = gpu_lib.GpuKmers(ha), gpu_lib.GpuKmers(hb)
        la, lb = t.l1(), pc.l1_of_slots(sb, cb)
        for x, y, lx, ly in ((ka, kb, la, lb), (kb, ka, lb, la)):
            J = tabcmp_oracle.Join(lx, ly)
            joint, shared, only_x, only_y = J.joint()
            got = x.joint_hist(y)
            assert np.array_equal(got[0], joint) and got[1:] == (shared, only_x, only_y) and shared > 0 and only_x > 0 and only_y > 0
            subs = np.repeat(np.arange(len(lx[0])), lx[0])
            want = np.empty((len(lx[1]), 5), dtype=np.int64)
            want[:, :2] = _decode(L, k, l_pre, subs, lx[1]).astype(np.int64)
            want[:, 2], want[:, 3], want[:, 4] = lx[1] & U(0xff), lx[1] >> U(8) & U(0x3f), J.other_of_a()
            for o_min, o_max in ((0, 255), (0, 0), (1, 255)):
                gy, cnt, high, oth = x.list_vs(y, 0, -63, o_min, o_max)
                rows = np.column_stack([gy.astype(np.int64), cnt, high, oth]).reshape(-1, 5)
                oc = np.where(want[:, 4] < 0, 0, want[:, 4] & 0xff)
                w = want[(oc >= o_min) & (oc <= o_max)]
                assert np.array_equal(rows[np.lexsort((rows[:, 1], rows[:, 0]))], w[np.lexsort((w[:, 1], w[:, 0]))]), (t.variant, o_min, o_max)
            u = x.union(y)
            host = u.to_host()
            sizes, slots = J.union()
            assert np.array_equal(host.export_sorted()[0], sizes) and np.array_equal(host.export_sorted()[1], slots) and PH.legal(host.raw()[1], u.cshift)
            assert np.array_equal(u.sub_sizes(), sizes)
            host.close()
            u.close()
        # results that keep a full region full: the threshold filter at min_cnt 1 and the union with an empty table copy every key, so
        # the keys of one home fill their new region again and the last of them is upserted at the largest displacement
        y, want = t.arrays()
        he = gpu_lib.HostTable.from_slots(k, l_pre, 2, np.zeros(4 << l_pre, dtype=U))
        ke = gpu_lib.GpuKmers(he)
        c = pc.result_cshift(l_pre, len(t.placed), int(la[0].max()))
        assert c == cshift   # (chain_case refuses to build a table of which this does not hold)
        for res in (ka.clip(min_cnt=1, max_rounds=0)[0], ka.union(ke), ke.union(ka)):
            host = res.to_host()
            assert res.cshift == c and np.array_equal(host.export_sorted()[0], la[0]) and np.array_equal(host.export_sorted()[1], la[1]) and PH.legal(host.raw()[1], c)
            assert np.array_equal(res.lookup(y), want) and np.array_equal(host.occ_planes(y), want)
            host.close()
            res.close()
        for o in (ka, kb, ke, ha, hb, he):
            o.close()


# ---- graph fixtures relaid and filled --------------------------------------------------------------------------------------------------------

def _graph_rows(y, cnt, high, nb):
    r = np.column_stack([np.asarray(y, dtype=U).reshape(-1, 2), np.asarray(cnt, dtype=U), np.asarray(high, dtype=U), np.asarray(nb, dtype=U)]).reshape(-1, 5)
    return r[np.lexsort((r[:, 1], r[:, 0]))]


def _host_rows(t):
    slots = t.export_sorted()[1]
    return _rows(t.graph_nb(1)[0], slots & U(0xff), slots >> U(8) & U(0x3f))


@pytest.mark.parametrize("form", PH.FORMS)
@pytest.mark.parametrize("name", PH.FIXTURES)
def test_fixture_graph_reads(gpu_lib, name, form):
    """graph_census, list_graph, extend from every tip and unitigs on a relaid / filled fixture: the host twin's on the same table and the
    string oracles' on its dict"""
    t, d, full = PH.table(gpu_lib, name, form)
    km = gpu_lib.GpuKmers(t)
    k = t.k
    ys, nb1 = t.graph_nb(1)
    strs = strs_of_planes(ys, k)
    val = (t.export_sorted()[1] & U(0x3fff)).astype(np.int64)
    for min_cnt in (1, 2):
        want_nb = np.array([d.nb(s, min_cnt) if (v & 0xff) >= min_cnt else 0 for s, v in zip(strs, val)], dtype=np.uint8)
        assert np.array_equal(t.graph_nb(min_cnt)[1], want_nb)
        census = km.graph_census(min_cnt)
        assert np.array_equal(census, t.graph_census(min_cnt)) and np.array_equal(census, census_of_nb(want_nb[(val & 0xff) >= min_cnt]))
        for mask in ("all", "tips", "branching"):
            m = gpu_lib.GRAPH_MASKS[mask]
            got = _graph_rows(*km.list_graph(min_cnt, m))
            assert np.array_equal(got, _graph_rows(*t.list_graph(min_cnt, m)))
            keep = ((val & 0xff) >= min_cnt) & in_mask(want_nb, m)
            assert np.array_equal(got, _graph_rows(ys[keep], val[keep] & 0xff, val[keep] >> 8, want_nb[keep]))
        assert gpu_lib.unitig_rows(*km.unitigs(min_cnt)) == gpu_lib.unitig_rows(*t.unitigs(min_cnt)) == PH.want_unitigs(d, min_cnt)
    tips = ys[in_mask(nb1, gpu_lib.GRAPH_MASKS["tips"])]
    seeds = np.concatenate([tips, gpu_lib.kmer_revcomp(k, tips)])
    got, twin = km.extend(seeds, 1, 100), t.extend(seeds, 1, 100)
    assert all(np.array_equal(a, b) for a, b in zip(got, twin)) and len(tips) > 0
    want = [d.extend(s, 1, 100) for s in strs_of_planes(seeds, k)]
    assert paths(got[0], got[1]) == [w[0] for w in want] and got[2].tolist() == [w[1] for w in want]
    km.close()


@pytest.mark.parametrize("form", PH.FORMS)
@pytest.mark.parametrize("name", PH.FIXTURES)
def test_fixture_clip_and_pop(gpu_lib, name, form):
    """clip (test_gpu_clip.py's parameter sets) and pop_bubbles (max_diff = 2, and the defaults) on a relaid / filled fixture: listing,
    stats and the result's unitigs are the host twin's on the same table and the string oracle's on its dict"""
    t, d, full = PH.table(gpu_lib, name, form)
    km = gpu_lib.GpuKmers(t)
    for how, sets, oracle_of, surv_of in (("clip", PH.clip_sets(name), PH.want_clip, PH.clip_oracle.survivors_of_table), ("pop", PH.POP_SETS, PH.want_pop, PH.bubble_oracle.survivors_of_table)):
        for kw in sets:
            surv, stats, units = oracle_of(d, PH.key_of(kw))
            tw, tw_stats = t.clip(**kw) if how == "clip" else t.pop_bubbles(**kw)
            res, got_stats = km.clip(**kw) if how == "clip" else km.pop_bubbles(**kw)
            assert PH.stats_of(got_stats) == PH.stats_of(tw_stats) == stats and surv_of(tw) == surv
            assert np.array_equal(_rows(*res.list(1)), _host_rows(tw)) and len(surv) == int(res.sub_sizes().sum())
            assert gpu_lib.unitig_rows(*res.unitigs(1)) == units
            res.close()
            tw.close()
    km.close()


# ---- results with a full region ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["clip", "pop"])
@pytest.mark.parametrize("name", PH.FULL)
def test_full_result_region_of_a_cleaning(gpu_lib, name, how):
    """the survivors of one sub-table number exactly 2^c: the result has cshift c and that region full; on it, lookup of every survivor,
    every removed node and absent k-mers of the full region is right, unitigs and a second clip equal the twin's, to_host() is the twin's
    table"""
    inp, d, c, sub = PH.full_input(gpu_lib, name, how)
    kw = PH.FULL_KW[how]
    km = gpu_lib.GpuKmers(inp)
    res, stats = km.clip(**kw) if how == "clip" else km.pop_bubbles(**kw)
    tw, tw_stats = inp.clip(**kw) if how == "clip" else inp.pop_bubbles(**kw)
    sizes = res.sub_sizes()
    assert res.cshift == c and int(sizes.max()) == 1 << c and int(sizes[sub]) == 1 << c and PH.stats_of(stats) == PH.stats_of(tw_stats)
    y, want = PH.result_queries(gpu_lib, name, how)
    assert np.array_equal(res.lookup(y), want) and np.array_equal(tw.occ_planes(y), want) and (want == -1).sum() >= 4
    assert gpu_lib.unitig_rows(*res.unitigs(1)) == gpu_lib.unitig_rows(*tw.unitigs(1))
    again, ast = res.clip(min_cnt=1, max_tip=12, islands=True)
    tw_again, tw_ast = tw.clip(min_cnt=1, max_tip=12, islands=True)
    assert PH.stats_of(ast) == PH.stats_of(tw_ast) and len(ast) >= 1 and np.array_equal(_rows(*again.list(1)), _host_rows(tw_again))
    host = res.to_host()
    assert host.raw()[0] == c and all(np.array_equal(a, b) for a, b in zip(host.export_sorted(), tw.export_sorted())) and PH.legal(host.raw()[1], c)
    for o in (host, again, tw_again, tw, res, km):
        o.close()


@pytest.mark.parametrize("name", PH.FULL)
def test_full_result_region_of_a_union(gpu_lib, name):
    """two tables whose keys of one sub-table number 2^c together: the union, either way round, has cshift c and that region full, is
    bfc_ch_union's table, answers for every key of either input and for absent k-mers of the full region, and its unitigs and clip are the
    twin's"""
    a, b, c, sub = PH.full_input(gpu_lib, name, "union")
    L = gpu_lib._lib.load()
    tw = gpu_lib.HostTable(L.bfc_ch_union((C.c_void_p * 2)(a.ptr, b.ptr), 2))
    ka, kb = gpu_lib.GpuKmers(a), gpu_lib.GpuKmers(b)
    extra = pc.absent_of_region(tw, sub, c, 64, 6)
    y = np.concatenate([a.graph_nb(1)[0], b.graph_nb(1)[0], extra])
    want = tw.occ_planes(y)
    assert (want[-len(extra):] == -1).all() and (want[:-len(extra)] >= 0).all() and len(extra) >= 4
    for x, z in ((ka, kb), (kb, ka)):
        u = x.union(z)
        assert u.cshift == c and int(u.sub_sizes().max()) == 1 << c == int(u.sub_sizes()[sub])
        assert np.array_equal(u.lookup(y), want)
        host = u.to_host()
        assert all(np.array_equal(p, q) for p, q in zip(host.export_sorted(), tw.export_sorted())) and PH.legal(host.raw()[1], c)
        assert gpu_lib.unitig_rows(*u.unitigs(1)) == gpu_lib.unitig_rows(*tw.unitigs(1))
        res, stats = u.clip(min_cnt=2, islands=True)
        tw_res, tw_stats = tw.clip(min_cnt=2, islands=True)
        assert PH.stats_of(stats) == PH.stats_of(tw_stats) and np.array_equal(_rows(*res.list(1)), _host_rows(tw_res))
        for o in (res, tw_res, host, u):
            o.close()
    for o in (ka, kb, tw):
        o.close()


# ---- random slots: the passes that stream ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l_pre", [1, 4, 8])
def test_sweep_of_geometries(gpu_lib, l_pre):
    """cshift 1 .. 8 -- tables from 4 slots up, regions of one lane up to a whole wave -- with a full and an empty region: hist, sub_sizes
    and list against numpy, and clip(max_rounds=0) at min_cnt 1 and 2, the two streaming passes alone, against the numpy filter"""
    L, k = gpu_lib._lib.load(), pc.SWEEP_K
    for cshift in range(1, 9):
        slots = pc.sweep_case(l_pre, cshift)
        h = gpu_lib.HostTable.from_slots(k, l_pre, cshift, slots)
        km = gpu_lib.GpuKmers(h)
        _check_streams(km, slots, cshift)
        n_sub = 1 << l_pre
        for min_cnt, lo, hi in ((0, 0, n_sub), (2, 0, n_sub), (255, 1, n_sub), (1, 0, 1)):
            assert _same_listing(km.list(min_cnt, 0, lo, hi), _listing_of(L, k, l_pre, cshift, slots, min_cnt, 0, lo, hi)), (cshift, min_cnt, lo, hi)
        for min_cnt in (1, 2):
            res, stats = km.clip(min_cnt=min_cnt, max_rounds=0)
            keep = slots * ((slots & U(0xff)) >= U(min_cnt))
            sizes, want = pc.l1_of_slots(keep, cshift)
            assert len(stats) == 0 and np.array_equal(res.sub_sizes(), sizes), (cshift, min_cnt)
            assert res.cshift == pc.result_cshift(l_pre, len(want), int(sizes.max()))
            host = res.to_host()
            assert np.array_equal(host.export_sorted()[1], want) and np.array_equal(host.export_sorted()[0], sizes) and PH.legal(host.raw()[1], res.cshift)
            host.close()
            res.close()
        km.close()
        h.close()


# ---- one tool run ----------------------------------------------------------------------------------------------------------------------------------

def test_kmergraph_on_a_dump_with_full_regions(gpu_lib, tmp_path):
    """`python -m bfc_amd.kmergraph -u` on a dump of d15 filled (16 sub-tables; bfc_ch_restore grows a region only when it overflows, so
    the three full sub-tables restore to full regions) prints the string oracle's census and unitig lines"""
    t, d, full = PH.table(gpu_lib, "d15", "filled")
    dump = str(tmp_path / "d15.dump")
    assert t.dump(dump) == 0
    back = gpu_lib.HostTable.restore(dump)
    cshift, slots = back.raw()
    assert (slots != 0).reshape(16, -1)[full].all() and cshift == t.raw()[0]
    back.close()
    r = subprocess.run([sys.executable, "-m", "bfc_amd.kmergraph", "-u", dump], capture_output=True, env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()
    strs = strs_of_planes(t.graph_nb(1)[0], t.k)
    census = census_of_nb(np.array([d.nb(s, 1) for s in strs], dtype=np.uint8))
    assert r.stdout.decode().splitlines() == _census_lines(census) + _unitig_lines(PH.want_unitigs(d, 1))
