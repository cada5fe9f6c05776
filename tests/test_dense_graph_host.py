"""The host twins of every graph read-out (neighbors, graph_census, graph_nb, list_graph, extend, unitigs, clip: bfcg_graph.hip,
bfcg_unitigs.hip, bfcg_clip.hip) on the DENSE draws of tests/dense_corpus.py: k = 9..19 with 2 % errors, where the graph has several
cycles (one of two nodes), nodes of degree 3 and 4, tips and islands that cascade over three clipping rounds, and tables of 16 to 2^20
sub-tables.  Odd k: held to the string oracles (graph_oracle.DictGraph, unitig_oracle.unitigs, clip_oracle.clip), which never touch the
library's hash.  Even k: there is no string oracle (the strand rule leaves k-mers undecided), so the twins are held to
bfcg_kmer_occ_host, one k-mer at a time.  What the corpus must contain is asserted here on the oracle alone, so that a change of the
generator cannot quietly empty a case; test_gpu_dense_graph.py takes its expected values from this file.  No GPU."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import clip_oracle
import dense_corpus
import oracle
import unitig_oracle
from dense_corpus import EVEN, ODD, draw
from graph_oracle import DictGraph, census_of_nb, in_mask, paths, planes_of_strs, revcomp, strs_of_planes
from test_kmers_host import HASH2CNT, _forward, decode_slots, format_lines

U = np.uint64
MASKS = ["all", "tips", "isolated", "branching", "simple"]
MAX_LENS = (1, 7, 300)          # max_len 0 is outside the call's range: test_max_len_zero_is_refused


def clip_sets(k):
    """the three parameter sets of the clipping comparisons"""
    return [dict(min_cnt=1, max_tip=2 * k), dict(min_cnt=2, max_tip=k, islands=True), dict(min_cnt=1, max_tip=3, max_mean=2, islands=True, max_rounds=20)]


class OccGraph(DictGraph):
    """DictGraph's neighbours and extension with every value looked up by bfcg_kmer_occ_host on the strand given: the route for even k"""

    def __init__(self, t):
        self.k, self.t, self.d = t.k, t, {}

    def value(self, s):
        if s not in self.d:
            self.d[s] = int(self.t.occ_planes(planes_of_strs([s], self.k))[0])
        return self.d[s]


@functools.lru_cache(maxsize=None)
def counted(name):
    """the oracle's (sizes, slots) of a draw at -b 20 and its dump -- made once"""
    d = draw(name)
    c = oracle.Counter(d.k, dense_corpus.B, l_pre=d.l_pre)
    c.count(*d.reads)
    with tempfile.TemporaryDirectory() as tmp:
        fn = os.path.join(tmp, "t.hash")
        assert c.dump(fn) == 0
        raw = open(fn, "rb").read()
    sizes, slots = c.export()
    c.close()
    return sizes, slots, raw


@functools.lru_cache(maxsize=None)
def tab(gpu_lib, name):
    """a draw counted by the oracle, dumped and restored into this library's host table -- made once, never changed"""
    d = draw(name)
    with tempfile.TemporaryDirectory() as tmp:
        fn = os.path.join(tmp, "t.hash")
        with open(fn, "wb") as fh:
            fh.write(counted(name)[2])
        t = gpu_lib.HostTable.restore(fn)
    assert t is not None and (t.k, t.l_pre) == (d.k, d.l_pre), "the library refused k=%d l_pre=%d" % (d.k, d.l_pre)
    return t


@functools.lru_cache(maxsize=None)
def nodes(gpu_lib, name):
    """(y, strings, high << 8 | count) of every slot, in export_sorted()'s order"""
    t = tab(gpu_lib, name)
    y = t.graph_nb(1)[0]
    return y, strs_of_planes(y, t.k), (t.export_sorted()[1] & U(0x3fff)).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def graph(gpu_lib, name):
    """the reference graph of a draw: the dict over both strands' strings (odd k), bfcg_kmer_occ_host one by one (even k)"""
    t = tab(gpu_lib, name)
    if t.k % 2 == 0:
        return OccGraph(t)
    y, strs, ch = nodes(gpu_lib, name)
    return DictGraph(t.k, strs, ch)


@functools.lru_cache(maxsize=None)
def want_nb(gpu_lib, name, min_cnt):
    """the reference's neighbour bits of every slot, 0 where the count is below min_cnt"""
    y, strs, ch = nodes(gpu_lib, name)
    g = graph(gpu_lib, name)
    return np.array([g.nb(s, min_cnt) if (c & 0xff) >= min_cnt else 0 for s, c in zip(strs, ch)], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def absent(gpu_lib, name, n):
    """n random k-mers that the table holds on neither strand, as strings"""
    y, strs, ch = nodes(gpu_lib, name)
    have, rng, out = set(strs), np.random.default_rng(len(strs)), []
    while len(out) < n:
        s = dense_corpus._rand(rng, draw(name).k)
        if s not in have and revcomp(s) not in have:
            out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def nb_queries(gpu_lib, name):
    """(strings, planes) of the neighbour queries: every node, every seventh node's reverse complement, 200 absent k-mers"""
    y, strs, ch = nodes(gpu_lib, name)
    q = strs + [revcomp(s) for s in strs[::7]] + absent(gpu_lib, name, 200)
    return q, planes_of_strs(q, draw(name).k)


@functools.lru_cache(maxsize=None)
def want_neighbors(gpu_lib, name):
    """the reference's eight values of every neighbour query"""
    g = graph(gpu_lib, name)
    return np.array([g.neighbors(s) for s in nb_queries(gpu_lib, name)[0]], dtype=np.int16)


@functools.lru_cache(maxsize=None)
def seeds(gpu_lib, name):
    """(strings, planes) of the extension seeds: 300 nodes and 20 absent k-mers, each followed by its reverse complement; the planes of
    the reverse complements come from bfcg_kmer_revcomp"""
    k = draw(name).k
    y, strs, ch = nodes(gpu_lib, name)
    pick = np.random.default_rng(k).permutation(len(strs))[:300]
    fw = [strs[i] for i in pick] + absent(gpu_lib, name, 20)
    yf = planes_of_strs(fw, k)
    both = np.stack([yf, gpu_lib.kmer_revcomp(k, yf)], axis=1).reshape(-1, 2)
    return [s for f in fw for s in (f, revcomp(f))], both


@functools.lru_cache(maxsize=None)
def want_extend(gpu_lib, name, min_cnt, max_len):
    """the reference's [(path, stop)] of the seeds"""
    g = graph(gpu_lib, name)
    return [g.extend(s, min_cnt, max_len) for s in seeds(gpu_lib, name)[0]]


@functools.lru_cache(maxsize=None)
def want_unitigs(gpu_lib, name, min_cnt):
    return unitig_oracle.unitigs(graph(gpu_lib, name), min_cnt)


@functools.lru_cache(maxsize=None)
def want_clip(gpu_lib, name, i, twice=False):
    """clip_oracle.clip of a draw with parameter set i: (survivors, stats, the survivors' unitigs at min_cnt 1); twice: the survivors
    clipped again with the same set and islands"""
    kw = clip_sets(draw(name).k)[i]
    surv, stats = clip_oracle.clip(graph(gpu_lib, name), **kw)
    if twice:
        k = draw(name).k
        both = dict(surv)
        both.update({revcomp(s): v for s, v in surv.items()})
        surv, stats = clip_oracle.clip(clip_oracle._graph(k, both), **dict(kw, islands=True))
    return surv, stats, clip_oracle.unitigs_of(draw(name).k, surv, 1)


def stats_of(s):
    return [tuple(int(v) for v in r) for r in s]


# ---- odd draws: the twins against the string oracles -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ODD)
def test_neighbors_equal_the_dict(gpu_lib, name):
    """the eight values of every node and of 200 absent k-mers, on both strands"""
    n = len(nodes(gpu_lib, name)[1])
    got = tab(gpu_lib, name).neighbors(nb_queries(gpu_lib, name)[1])
    assert np.array_equal(got, want_neighbors(gpu_lib, name))
    assert (got[:n] >= 0).any(axis=1).sum() > n // 2 and (got[-200:] >= 0).sum() < 200


@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("name", ODD)
def test_census_nb_and_listing_equal_the_dict(gpu_lib, name, min_cnt):
    """graph_nb is the oracle's neighbour bits on the nodes and 0 on the others; graph_census is their census; list_graph under the five
    masks is the oracle's subset, with counts and neighbour bits"""
    t = tab(gpu_lib, name)
    y, strs, ch = nodes(gpu_lib, name)
    want = want_nb(gpu_lib, name, min_cnt)
    node = (ch & 0xff) >= min_cnt
    y2, nb = t.graph_nb(min_cnt)
    assert np.array_equal(y2, y) and np.array_equal(nb, want) and not nb[~node].any()
    assert np.array_equal(t.graph_census(min_cnt), census_of_nb(want[node]))
    for m in MASKS:
        keep = node & in_mask(want, gpu_lib.GRAPH_MASKS[m])
        ly, lc, lh, lnb = t.list_graph(min_cnt, gpu_lib.GRAPH_MASKS[m])
        assert (min_cnt == 2 or 0 < keep.sum()) and (m == "all") == (keep.sum() == node.sum())
        assert np.array_equal(ly, y[keep]) and np.array_equal(lnb, want[keep]) and np.array_equal(lc.astype(np.uint16) | lh.astype(np.uint16) << 8, ch[keep])


@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("name", ODD)
def test_extend_equals_the_dict(gpu_lib, name, min_cnt):
    """300 nodes and 20 absent k-mers, from both strands, for max_len 1, 7 and 300: paths and stop codes"""
    t = tab(gpu_lib, name)
    strs, y = seeds(gpu_lib, name)
    for max_len in MAX_LENS:
        bases, length, stop = t.extend(y, min_cnt, max_len)
        want = want_extend(gpu_lib, name, min_cnt, max_len)
        assert paths(bases, length) == [w[0] for w in want] and list(stop) == [w[1] for w in want]


def test_max_len_zero_is_refused(gpu_lib):
    """max_len 0 names no walk: the call's range is [1, 65535] (include/bfc_gpu.h), and the twin says so instead of answering"""
    strs, y = seeds(gpu_lib, "d11")
    with pytest.raises(gpu_lib.BfcGpuError, match=r"max_len 0 is outside \[1, 65535\]"):
        tab(gpu_lib, "d11").extend(y, 1, 0)


@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("name", ODD)
def test_unitigs_equal_the_oracle(gpu_lib, name, min_cnt):
    t = tab(gpu_lib, name)
    got = gpu_lib.unitig_rows(*t.unitigs(min_cnt))
    assert got == want_unitigs(gpu_lib, name, min_cnt) and len(got) > 40
    assert sum(r[1] for r in got) == int(t.graph_census(min_cnt).sum())


@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("name", ODD)
def test_clip_equals_the_oracle(gpu_lib, name, i):
    """survivors with their counts, and the per-round stats, for the three parameter sets"""
    surv, stats, units = want_clip(gpu_lib, name, i)
    res, got = tab(gpu_lib, name).clip(**clip_sets(draw(name).k)[i])
    assert stats_of(got) == stats and len(stats) >= 1
    assert clip_oracle.survivors_of_table(res) == surv and gpu_lib.unitig_rows(*res.unitigs(1)) == units
    res.close()


# ---- what the corpus must contain, on the oracle alone -----------------------------------------------------------------------------

def test_corpus_unitig_stop_codes_and_cycles(gpu_lib):
    """over the odd draws, the stop codes 1, 2, 3 and 6 of unitigs all occur; every odd draw with k >= 11 has at least four cycles at
    min_cnt 2; some draw has a cycle of two k-mers, some one of 64, some one of 65"""
    codes, cyc = set(), set()
    for name in ODD:
        rows = want_unitigs(gpu_lib, name, 2)
        codes |= {r[3] for r in rows} | {r[4] for r in rows}
        lens = [r[1] for r in rows if r[5]]
        cyc |= set(lens)
        assert draw(name).k < 11 or len(lens) >= 4, (name, lens)
    assert codes >= {1, 2, 3, 6} and cyc >= {2, 64, 65}, (codes, cyc)


def test_corpus_low_count_circle(gpu_lib):
    """d11 at min_cnt 1 has a cycle of 33 k-mers more than at min_cnt 2: a unitigs(1) call after a unitigs(2) call finds more cycle nodes"""
    one, two = (sorted(r[1] for r in want_unitigs(gpu_lib, "d11", m) if r[5]) for m in (1, 2))
    assert sorted(two + [dense_corpus.LOW_CIRC]) == one and sum(two) > 64


def test_corpus_two_node_cycle_is_the_planted_one(gpu_lib):
    """the two-node cycle is AC repeated: ACAC..A and CACA..C are each other's only neighbour on both sides"""
    for name in ODD:
        k = draw(name).k
        if any(r[1] == 2 and r[5] for r in want_unitigs(gpu_lib, name, 2)):
            a, b = dense_corpus.cycle_nodes(draw(name).planted.circ[2], k)
            d = graph(gpu_lib, name)
            assert (d.nb(a, 2), d.nb(b, 2)) == (0x22, 0x11)   # (succ and pred of a by C, of b by A)
            assert unitig_oracle.link(d, a, 2)[0] == b and unitig_oracle.link(d, b, 2)[0] == a


def test_corpus_extension_stop_codes(gpu_lib):
    """over the extension seeds of the odd draws every stop code 0 to 5 occurs"""
    seen = set()
    for name in ODD:
        for max_len in MAX_LENS:
            seen |= {w[1] for w in want_extend(gpu_lib, name, 2, max_len)}
    assert seen == {0, 1, 2, 3, 4, 5}


def test_corpus_degrees_three_and_four(gpu_lib):
    """at min_cnt 1 every draw with k <= 13 has a node in census row or column 4, and at least five in rows or columns 3 and above"""
    for name in ODD:
        if draw(name).k > 13:
            continue
        deg = census_of_nb(want_nb(gpu_lib, name, 1))
        four = int(deg[4, :].sum() + deg[:, 4].sum() - deg[4, 4])
        three = int(deg.sum() - deg[:3, :3].sum())
        assert four >= 1 and three >= 5, (name, four, three)


def test_corpus_clipping_rounds_tips_and_islands(gpu_lib):
    """with the first parameter set some draw needs at least three rounds and two others at least two; at min_cnt 2 every draw's
    clipping removes at least one island and at least one tip"""
    rounds = sorted(len(want_clip(gpu_lib, name, 0)[1]) for name in ODD)
    assert rounds[-1] >= 3 and rounds[-3] >= 2, rounds
    for name in ODD:
        k = draw(name).k
        gone = [u for u in want_unitigs(gpu_lib, name, 2) if clip_oracle.clippable(u, k, 255, True)]
        dead = [(u[3] in clip_oracle.DEAD) + (u[4] in clip_oracle.DEAD) for u in gone]
        assert 1 in dead and 2 in dead, (name, dead)


def test_corpus_sixteen_sub_tables(gpu_lib):
    """d15 is a table of 16 sub-tables of several hundred keys each: long probe chains, a cshift of 7 and more on the device"""
    sizes = counted("d15")[0]
    assert len(sizes) == 16 and sizes.min() > 64


# ---- even draws: the twins against bfcg_kmer_occ_host ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", EVEN)
def test_even_twins_equal_occ_lookups(gpu_lib, name):
    """neighbors, graph_nb, graph_census and extend against values looked up one k-mer at a time, on the strand given; the table lists
    at least five k-mers that equal their own reverse complement, and their neighbours are among what is compared"""
    t, g = tab(gpu_lib, name), graph(gpu_lib, name)
    y, strs, ch = nodes(gpu_lib, name)
    pal = [s for s in strs if s == revcomp(s)]
    assert len(pal) >= 5, (name, len(pal))
    assert np.array_equal(t.neighbors(nb_queries(gpu_lib, name)[1]), want_neighbors(gpu_lib, name))
    for min_cnt in (1, 2):
        want = want_nb(gpu_lib, name, min_cnt)
        node = (ch & 0xff) >= min_cnt
        y2, nb = t.graph_nb(min_cnt)
        assert np.array_equal(y2, y) and np.array_equal(nb, want)
        assert np.array_equal(t.graph_census(min_cnt), census_of_nb(want[node]))
        sy = seeds(gpu_lib, name)[1]
        for max_len in MAX_LENS:
            bases, length, stop = t.extend(sy, min_cnt, max_len)
            w = want_extend(gpu_lib, name, min_cnt, max_len)
            assert paths(bases, length) == [v[0] for v in w] and list(stop) == [v[1] for v in w]
    for call in (t.unitigs, t.clip):
        with pytest.raises(gpu_lib.BfcGpuError, match="k=%d is even" % t.k):
            call()


# ---- the decode at small k -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["d9", "d15"])
def test_decode_at_small_k(gpu_lib, name, tmp_path):
    """2k - l_pre = 10 (d9) and a table of 16 sub-tables (d15): every slot decoded by bfcg_kmer_decode_host hashes forward to its own
    sub-table and key; every decoded string, or its reverse complement, is in a read; where the reference's hash2cnt is built, the
    formatted listing is its output on the dump"""
    L, O = gpu_lib._lib.load(), oracle.lib()
    d = draw(name)
    sizes, slots, raw = counted(name)
    y, ch = decode_slots(L, d.k, d.l_pre, sizes, slots)
    strs = strs_of_planes(y, d.k)
    sub = np.repeat(np.arange(len(sizes)), sizes)
    key = C.c_uint64()
    for s, sb, slot in zip(strs, sub, slots):
        Y = _forward(d.k, [b"ACGT".index(c) for c in s])
        assert O.orc_ch_subkey(d.k, d.l_pre, (C.c_uint64 * 2)(*Y), C.byref(key)) == sb and key.value >> 14 == int(slot) >> 14
    in_reads = set(r[i:i + d.k] for r in d.planted.reads for i in range(len(r) - d.k + 1))
    assert all(s in in_reads or revcomp(s) in in_reads for s in strs) and len(strs) > 1000
    if os.path.exists(HASH2CNT):
        fn = str(tmp_path / "t.hash")
        with open(fn, "wb") as fh:
            fh.write(raw)
        ref = subprocess.run([HASH2CNT, fn], capture_output=True, check=True).stdout.splitlines()
        assert sorted(format_lines(L, d.k, y, ch)) == sorted(ref)
