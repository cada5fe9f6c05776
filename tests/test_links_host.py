"""The host twin of the linked unitigs (bfcg_unitig_graph_host, bfc_amd/csrc/bfcg_unitigs.hip) -- the reference side of the GPU
comparisons in test_gpu_links.py -- held to the oracle of tests/link_oracle.py: the edges between the oriented unitigs found on strings
with a dict, which asserts the definition of include/bfc_gpu.h on itself (what each kind of end produces, the mirror rule, the overlap,
the degree identity).  Also the GFA 1 writer of `python -m bfc_amd.kmergraph -g`, on a host table.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import link_oracle
import test_dense_graph_host as dense
import unitig_oracle
from dense_corpus import ODD, draw
from graph_oracle import revcomp
from test_unitig_host import _tab, _want

U = np.uint64
FILL = 77


def raw_graph(L, fn, obj, min_cnt, seq_cap, n_cap, null_links=False):
    """one call through the C ABI into buffers filled with 77: (rc, n0, n1, n2, seq, off, n_kmers, cnt_sum, ends, links)"""
    seq, off = np.full(max(seq_cap, 1), FILL, dtype=np.uint8), np.full(n_cap + 1, FILL, dtype=U)
    nk, cs, ends = np.full(max(n_cap, 1), FILL, dtype=np.uint32), np.full(max(n_cap, 1), FILL, dtype=U), np.full(max(n_cap, 1), FILL, dtype=np.uint8)
    links = np.full((max(n_cap, 1), 2, 4), FILL, dtype=np.int64)
    n = (C.c_uint64 * 3)(FILL, FILL, FILL)
    rc = fn(obj, min_cnt, seq.ctypes.data, seq_cap, off.ctypes.data, nk.ctypes.data, cs.ctypes.data, ends.ctypes.data, None if null_links else links.ctypes.data, n_cap, n)
    return rc, int(n[0]), int(n[1]), int(n[2]), seq, off, nk, cs, ends, links


def untouched(r):
    return all((a == FILL).all() for a in r[4:])


def degree_identity(deg, n_kmers):
    """the edges that a census and the unitigs' sizes leave: every neighbour of every node, less the two ends of every link inside a unitig"""
    deg = np.asarray(deg).astype(np.int64)
    o, i = np.meshgrid(np.arange(5), np.arange(5), indexing="ij")
    return int((deg * (o + i)).sum()) - 2 * int((np.asarray(n_kmers).astype(np.int64) - 1).sum())


def check_graph(gpu_lib, k, got, plain, deg, want_rows, want_links):
    """unitig_graph()'s six arrays against unitigs()'s rows, the census and the oracle's rows and links"""
    seq, off, nk, cs, ends, links = got
    assert links.shape == (len(nk), 2, 4) and links.dtype == np.int64
    assert off[0] == 0 and off[-1] == len(seq) and np.array_equal(np.diff(off).astype(np.int64), nk.astype(np.int64) + k - 1)
    assert gpu_lib.unitig_rows(seq, off, nk, cs, ends) == want_rows == gpu_lib.unitig_rows(*plain)
    assert ((links >= -1) & (links < 2 * len(nk))).all()
    assert gpu_lib.unitig_link_rows(seq, off, links) == want_links
    assert int((links >= 0).sum()) == len(want_links) == degree_identity(deg, nk)


def test_the_definition_on_string_graphs():
    """without the library: a genome with one-base errors, a circle and an A-run as a dict of k-mer strings, k = 5 to 21 at min_cnt 1
    and 2 -- the oracle's own assertions hold in every graph, and every kind of end occurs among them"""
    codes = set()
    for k in (5, 7, 9, 11, 15, 21):
        for seed in (0, 1):
            rng = np.random.default_rng(100 * k + seed)
            rand = lambda n: bytes(b"ACGT"[c] for c in rng.integers(0, 4, n))
            genome, circ = rand(300), rand(40)
            reads = [genome, genome, circ * 3, circ * 3, b"A" * (k + 2), b"A" * (k + 2)]
            for _ in range(12):
                at = int(rng.integers(0, 300 - 2 * k))
                r = bytearray(genome[at:at + 2 * k])
                r[int(rng.integers(0, 2 * k))] = b"ACGT"[int(rng.integers(0, 4))]
                reads += [bytes(r)] * int(rng.integers(1, 3))
            for min_cnt in (1, 2):
                d = link_oracle.dict_of_reads(k, reads)
                rows = unitig_oracle.unitigs(d, min_cnt)
                got = link_oracle.links(d, rows, min_cnt)
                assert len(got) > 0
                codes |= {r[3] for r in rows} | {r[4] for r in rows} | {64 for r in rows if r[5]}
    assert codes >= {0, 1, 2, 3, 6, 64}


@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("k", [21, 33, 37])
def test_host_twin_equals_the_oracle(gpu_lib, k, min_cnt):
    """on the unitig fixture: the sorted link rows are the oracle's, the first five outputs are HostTable.unitigs's, the degree
    identity holds against the census; and what the generator knows: the cycle links to itself on both strands, the A-run to itself
    on both strands by A and T, the hairpin's closed end to its own reverse complement once, the bubble's arms hang between its flanks"""
    t, f = _tab(gpu_lib, k), unitig_oracle.fixture(k)
    d = unitig_oracle.dict_of_table(t)
    want_rows = _want(gpu_lib, k, min_cnt)
    want = link_oracle.links(d, want_rows, min_cnt)
    got = t.unitig_graph(min_cnt)
    plain = t.unitigs(min_cnt)
    assert all(np.array_equal(a, b) for a, b in zip(got[:5], plain))
    check_graph(gpu_lib, k, got, plain, t.graph_census(min_cnt), want_rows, want)
    by = {}
    for s, o, c, v, p in want:
        by.setdefault(s, []).append((o, c, v, p))
    cyc = [r[0] for r in want_rows if r[5]][0]
    assert by[cyc] == [(0, b"ACGT".index(cyc[k - 1]), cyc, 0), (1, b"ACGT".index(revcomp(cyc)[k - 1]), cyc, 1)]
    assert by[f.base.a_run] == [(0, 0, f.base.a_run, 0), (1, 3, f.base.a_run, 1)]
    hp = min(f.hairpin[:k], revcomp(f.hairpin[:k]))
    row = [r for r in want_rows if r[0] == hp][0]
    o = int(row[3] == 6)   # the side with code 6 is the right one of (hp, o); beyond it lies the same node read the other way
    assert sorted(row[3:5]) == [1, 6] and by[hp] == [(o, b"ACGT".index(link_oracle.oriented(hp, 1 - o)[k - 1]), hp, 1 - o)]
    iso = min(f.base.isolated, revcomp(f.base.isolated))
    assert iso not in by
    arms = [r[0] for r in want_rows if (r[3], r[4]) == (3, 3)]
    assert len(arms) == 2 and all(len(by[a]) == 2 and {e[0] for e in by[a]} == {0, 1} for a in arms)


@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("name", ODD)
def test_dense_draws_equal_the_oracle(gpu_lib, name, min_cnt):
    """the odd dense draws: three- and four-way branches, several cycles including the one of two nodes, hairpins"""
    t, d = dense.tab(gpu_lib, name), dense.graph(gpu_lib, name)
    want_rows = dense.want_unitigs(gpu_lib, name, min_cnt)
    want = link_oracle.links(d, want_rows, min_cnt)
    check_graph(gpu_lib, t.k, t.unitig_graph(min_cnt), t.unitigs(min_cnt), t.graph_census(min_cnt), want_rows, want)
    assert len(want) > 8


def test_corpus_links_hold_every_kind(gpu_lib):
    """over the odd draws: at min_cnt 2 a cycle of two nodes links to itself on both strands and some hairpin's edge is its own mirror;
    at min_cnt 1 some end has three edges and some has four (test_dense_graph_host.py asserts the nodes of degree 3 and 4)"""
    own, two, fans = 0, 0, set()
    for name in ODD:
        rows = dense.want_unitigs(gpu_lib, name, 2)
        want = link_oracle.links(dense.graph(gpu_lib, name), rows, 2)
        own += sum(1 for s, o, c, v, p in want if s == v and p == 1 - o)
        small = [r[0] for r in rows if r[5] and r[1] == 2]
        two += sum(1 for s, o, c, v, p in want if s in small and v == s and p == o)
        fan = {}
        for s, o, c, v, p in link_oracle.links(dense.graph(gpu_lib, name), dense.want_unitigs(gpu_lib, name, 1), 1):
            fan[s, o] = fan.get((s, o), 0) + 1
        fans |= set(fan.values())
    assert own >= 1 and two >= 2 and fans == {1, 2, 3, 4}


def test_refusals_leave_the_outputs_untouched(gpu_lib):
    """an even k, k = 39, min_cnt 0 and 256 and a NULL links with n_cap > 0 are refused with bfcg_unitigs_host's messages; nothing is
    written, n[] and links included"""
    L = gpu_lib._lib.load()
    for k, min_cnt, msg in ((32, 2, "k=32 is even"), (39, 2, "k=39"), (21, 0, "min_cnt 0 is outside [1, 255]"), (21, 256, "min_cnt 256 is outside [1, 255]")):
        r = raw_graph(L, L.bfcg_unitig_graph_host, _tab(gpu_lib, k).ptr, min_cnt, 1 << 16, 1 << 10)
        assert r[0] == -1 and r[1:4] == (FILL, FILL, FILL) and untouched(r)
        assert msg in L.bfcg_last_error().decode()
    r = raw_graph(L, L.bfcg_unitig_graph_host, _tab(gpu_lib, 21).ptr, 2, 1 << 16, 1 << 10, null_links=True)
    assert r[0] == -1 and r[1:4] == (FILL, FILL, FILL) and untouched(r) and "needs output buffers" in L.bfcg_last_error().decode()
    with pytest.raises(gpu_lib.BfcGpuError, match="k=32 is even"):
        _tab(gpu_lib, 32).unitig_graph(2)
    with pytest.raises(gpu_lib.BfcGpuError, match="k=39.*k <= 37"):
        _tab(gpu_lib, 39).unitig_graph(2)


@pytest.mark.parametrize("k", [21, 37])
def test_cap_protocol(gpu_lib, k):
    """caps of 0 size the call and leave n[2] alone; a seq_cap one short and an n_cap one short return 1 with the right n[0], n[1] and
    write nothing, links and n[2] included; exact caps write, and n[2] is the number of entries >= 0"""
    L, t = gpu_lib._lib.load(), _tab(gpu_lib, k)
    rows = _want(gpu_lib, k, 2)
    want = link_oracle.links(unitig_oracle.dict_of_table(t), rows, 2)
    n0, n1 = len(rows), sum(len(r[0]) for r in rows)
    n = (C.c_uint64 * 3)(FILL, FILL, FILL)
    assert L.bfcg_unitig_graph_host(t.ptr, 2, None, 0, None, None, None, None, None, 0, n) == 1 and list(n) == [n0, n1, FILL]
    for seq_cap, n_cap in ((0, 0), (n1 - 1, n0), (n1, n0 - 1)):
        r = raw_graph(L, L.bfcg_unitig_graph_host, t.ptr, 2, seq_cap, n_cap)
        assert r[:4] == (1, n0, n1, FILL) and untouched(r)
    r = raw_graph(L, L.bfcg_unitig_graph_host, t.ptr, 2, n1, n0)
    assert r[:4] == (0, n0, n1, len(want)) and int((r[9] >= 0).sum()) == len(want)
    assert gpu_lib.unitig_rows(*r[4:9]) == rows and gpu_lib.unitig_link_rows(r[4], r[5], r[9]) == want


@pytest.mark.parametrize("k,min_cnt", [(21, 1), (21, 2), (37, 2)])
def test_gfa_of_a_host_table_round_trips(gpu_lib, k, min_cnt):
    """kmergraph.gfa on the host twin's arrays, parsed back: the k-mers of the S lines are the graph's nodes; the k-mer edges inside
    the segments plus one per L line are the graph's edges on both strands; segments in unitig_rows's order with their sums and means"""
    from bfc_amd import kmergraph
    t = _tab(gpu_lib, k)
    d = unitig_oracle.dict_of_table(t)
    rows = _want(gpu_lib, k, min_cnt)
    seq, off, nk, cs, ends, links = t.unitig_graph(min_cnt)
    text, n_links = kmergraph.gfa(k, seq, off, nk, cs, links)
    segs, ls, nodes, edges = link_oracle.read_gfa(text, k)
    assert n_links == len(ls) == int((links >= 0).sum())
    assert [(s[0], s[1]) for s in segs.values()] == [(r[0], r[2]) for r in rows]
    assert (nodes, edges) == link_oracle.kmer_edges(d, min_cnt)
    want = link_oracle.links(d, rows, min_cnt)
    sid = {r[0]: i + 1 for i, r in enumerate(rows)}
    assert ls == sorted((sid[s], o, sid[v], p) for s, o, c, v, p in want)
