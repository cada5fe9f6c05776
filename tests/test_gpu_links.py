"""GPU tests (-m gpu) of the linked unitigs (bfcg_kmers_unitig_graph, bfc_amd/csrc/bfcg_unitigs.hip) through GpuKmers and the C ABI, and
of `python -m bfc_amd.kmergraph -g`.  The reference side is twofold: the host twin on the exported table (HostTable.unitig_graph), and
the string oracle of tests/link_oracle.py on the export's dict, which asserts the definition on itself.  The unitigs of two calls may be
numbered differently, so every comparison is of api.unitig_link_rows: the edges with their ends named by their spellings, sorted.  The
inputs are those of test_gpu_unitigs.py, the dense draws, a packed table with full regions and the bubble fixture."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_oracle
import graph_oracle
import link_oracle
import test_dense_graph_host as H
import test_packed_host as PH
import unitig_oracle
from graph_oracle import revcomp
from test_gpu_dense_graph import _case as _dense_case
from test_gpu_kmers import _count
from test_gpu_pop import _case as _bubble_case
from test_gpu_tabcmp import FORMS
from test_gpu_unitigs import TABLES, _case
from test_links_host import FILL, degree_identity, raw_graph, untouched

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _want(gpu_lib, which, form, min_cnt):
    """(the unitig rows, the host twin's link rows) of a case of test_gpu_unitigs.py -- made once"""
    c = _case(gpu_lib, which, form)
    g = c.host.unitig_graph(min_cnt)
    assert gpu_lib.unitig_rows(*g[:5]) == c.want[min_cnt]
    return c.want[min_cnt], gpu_lib.unitig_link_rows(g[0], g[1], g[5])


@functools.lru_cache(maxsize=None)
def _oracle(gpu_lib, which, form, min_cnt):
    """the string oracle's link rows of a case's export -- made once"""
    c = _case(gpu_lib, which, form)
    return link_oracle.links(unitig_oracle.dict_of_table(c.host), c.want[min_cnt], min_cnt)


def _check(gpu_lib, km, min_cnt, rows, want):
    """km.unitig_graph(min_cnt) against the unitig rows and link rows expected; its first five outputs against km.unitigs(); n[2]
    (which api._unitig_graph holds to the entries >= 0) and the degree identity against the device's census"""
    seq, off, nk, cs, ends, links = km.unitig_graph(min_cnt)
    assert km.last_ms() > 0
    assert links.shape == (len(nk), 2, 4) and ((links >= -1) & (links < 2 * len(nk))).all()
    assert off[0] == 0 and off[-1] == len(seq) and np.array_equal(np.diff(off).astype(np.int64), nk.astype(np.int64) + km.k - 1)
    assert gpu_lib.unitig_rows(seq, off, nk, cs, ends) == rows == gpu_lib.unitig_rows(*km.unitigs(min_cnt))
    assert gpu_lib.unitig_link_rows(seq, off, links) == want
    assert int((links >= 0).sum()) == len(want) == degree_identity(km.graph_census(min_cnt), nk)
    return links


@pytest.mark.parametrize("which,form", TABLES)
def test_links_equal_host_twin_and_oracle(gpu_lib, which, form):
    """on the attached table and on the upload of its export, at min_cnt 1 and 2 (k = 21 runs the 32-bit windows, 33 and 37 the 64-bit
    ones): the link rows are the host twin's and the string oracle's"""
    c = _case(gpu_lib, which, form)
    for min_cnt in (1, 2):
        rows, want = _want(gpu_lib, which, form, min_cnt)
        assert want == _oracle(gpu_lib, which, form, min_cnt)
        assert len(want) > (8 if which == "fixture" else 0)   # (g1 at min_cnt 2 is an almost linear graph)
        for km in (c.att, c.up):
            _check(gpu_lib, km, min_cnt, rows, want)


@pytest.mark.parametrize("name", ["d9", "d11", "d15"])
def test_dense_draws(gpu_lib, name):
    """d9 grown from two slots per sub-table, d11 on converted segments, d15 a table of 16 sub-tables, against the string oracle
    directly: ends with three and four edges, several cycles (one of two nodes), hairpins"""
    c = _dense_case(gpu_lib, name)
    for min_cnt in (1, 2):
        rows = H.want_unitigs(gpu_lib, name, min_cnt)
        want = link_oracle.links(H.graph(gpu_lib, name), rows, min_cnt)
        for km in (c.att, c.up):
            _check(gpu_lib, km, min_cnt, rows, want)


@pytest.mark.parametrize("cap", [1, 7, 64])
def test_launch_seams(gpu_lib, monkeypatch, cap):
    """BFCG_UNITIG_CAP (read when the object is made) of 1, 7 and 64 cuts k_ut_links into many launches -- a launch of one lane is half a
    unitig; d11 has more than 64 sides at either threshold --: the result is unchanged, with the 32-bit windows (d11) and the 64-bit
    ones (the fixture at k = 33)"""
    d, c = _dense_case(gpu_lib, "d11"), _case(gpu_lib, "fixture", "33host")
    monkeypatch.setenv("BFCG_UNITIG_CAP", str(cap))
    small_d, small_c = gpu_lib.GpuKmers(d.g), gpu_lib.GpuKmers(c.g)
    monkeypatch.delenv("BFCG_UNITIG_CAP")
    for min_cnt in (1, 2):
        rows = H.want_unitigs(gpu_lib, "d11", min_cnt)
        assert 2 * len(rows) > 64
        _check(gpu_lib, small_d, min_cnt, rows, link_oracle.links(H.graph(gpu_lib, "d11"), rows, min_cnt))
        _check(gpu_lib, small_c, min_cnt, *_want(gpu_lib, "fixture", "33host", min_cnt))
    small_d.close()
    small_c.close()


def map_load(rows, smallest=True):
    """(entries, words) of the end map for these unitig rows, by the rule of include/bfc_gpu.h: a path enters its two end nodes, one
    entry where they are one node, a cycle nothing; the words are the smallest power of two above 2 x the paths under
    BFCG_LINK_MAP_MIN=1, else the smallest one >= 4 x the paths"""
    paths = [r for r in rows if not r[5]]
    need, words = (2 * len(paths) + 1 if smallest else 4 * len(paths)), 1
    while words < need:
        words *= 2
    return 2 * len(paths) - sum(1 for r in paths if r[1] == 1), words


@pytest.mark.parametrize("where", ["d15", "fixture"])
def test_crowded_map(gpu_lib, monkeypatch, where):
    """BFCG_LINK_MAP_MIN=1 (read when the object is made): the end map is the smallest power of two above 2 x the paths, never larger
    than the usual one, which is at most half full, and the rows are equal.  How full it gets depends on the number of paths:
    test_map_filled_to_the_brim chooses it"""
    monkeypatch.setenv("BFCG_LINK_MAP_MIN", "1")
    km = gpu_lib.GpuKmers(_dense_case(gpu_lib, "d15").g if where == "d15" else _case(gpu_lib, "fixture", "21grown").g)
    monkeypatch.delenv("BFCG_LINK_MAP_MIN")
    for min_cnt in (1, 2):
        if where == "d15":
            rows = H.want_unitigs(gpu_lib, "d15", min_cnt)
            want = link_oracle.links(H.graph(gpu_lib, "d15"), rows, min_cnt)
        else:
            rows, want = _want(gpu_lib, "fixture", "21grown", min_cnt)
        entries, words = map_load(rows)
        assert entries < words <= map_load(rows, False)[1] and 2 * entries <= map_load(rows, False)[1]
        _check(gpu_lib, km, min_cnt, rows, want)
    km.close()


def test_map_filled_to_the_brim(gpu_lib, monkeypatch):
    """the unitig fixture at k = 33 with as many reads of k + 2 random bases (three times each: a dead-ended unitig of three k-mers at
    either threshold) as bring it to 1023 paths: under BFCG_LINK_MAP_MIN=1 the end map has 2048 words for 2 x 1023 entries less the few
    one-node paths, more than 0.99 full at min_cnt 1 and 2, so the fixture's edges are looked up through chains of hundreds of words
    that wrap round the map's end; the rows are the host twin's and the string oracle's, and equal those from the usual map"""
    k, rng = 33, np.random.default_rng(1023)
    f = unitig_oracle.fixture(k)
    base = [f.seq[int(f.off[i]):int(f.off[i + 1])].tobytes() for i in range(len(f.off) - 1)]
    p0 = sum(1 for r in _want(gpu_lib, "fixture", "33host", 1)[0] if not r[5])
    more = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, k + 2)) for _ in range(1023 - p0)]
    reads = base + [r for r in more for _ in range(3)]
    seq = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    g = _count(gpu_lib, k, (seq, np.full(len(seq), ord("I"), dtype=np.uint8), off), **FORMS["33host"][1])
    g.sync()
    host = g.export_table()
    monkeypatch.setenv("BFCG_LINK_MAP_MIN", "1")
    full = gpu_lib.GpuKmers(g)
    monkeypatch.delenv("BFCG_LINK_MAP_MIN")
    usual = gpu_lib.GpuKmers(g)
    d = unitig_oracle.dict_of_table(host)
    for min_cnt in (1, 2):
        tw = host.unitig_graph(min_cnt)
        rows, want = gpu_lib.unitig_rows(*tw[:5]), gpu_lib.unitig_link_rows(tw[0], tw[1], tw[5])
        entries, words = map_load(rows)
        assert words == 2048 and entries > 0.99 * words and (min_cnt == 2 or sum(1 for r in rows if not r[5]) == 1023)
        assert rows == unitig_oracle.unitigs(d, min_cnt) and want == link_oracle.links(d, rows, min_cnt) and len(want) > 8
        for km in (full, usual):
            _check(gpu_lib, km, min_cnt, rows, want)
    for o in (full, usual, host, g):
        o.close()


def test_more_entries_than_one_block_of_the_scan(gpu_lib, monkeypatch):
    """test_gpu_unitigs.py's 5000 reads of k + 2 bases: 5000 unitigs of three k-mers with both ends dead, 10000 entries of the end map
    from winners in more than one block of the scan; no edge at all -- every entry of links is -1, n[2] == 0 --, with the map at its
    usual size and at its smallest"""
    L = gpu_lib._lib.load()
    k, rng = 33, np.random.default_rng(33)
    reads = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, k + 2)) for _ in range(5000)]
    seq = np.frombuffer(b"".join(r + r for r in reads), dtype=np.uint8).copy()
    off = np.arange(0, len(seq) + 1, k + 2, dtype=np.uint64)
    g = _count(gpu_lib, k, (seq, np.full(len(seq), ord("I"), dtype=np.uint8), off), **FORMS["33host"][1])
    g.sync()
    host = g.export_table()
    want = gpu_lib.unitig_rows(*host.unitigs(1))
    assert len(want) == 5000 and all(r[1:] == (3, 3, 1, 1, 0) for r in want)
    for smallest in (None, "1"):
        if smallest:
            monkeypatch.setenv("BFCG_LINK_MAP_MIN", smallest)
        km = gpu_lib.GpuKmers(g)
        monkeypatch.delenv("BFCG_LINK_MAP_MIN", raising=False)
        out = km.unitig_graph(1)
        assert gpu_lib.unitig_rows(*out[:5]) == want and out[5].shape == (5000, 2, 4) and (out[5] == -1).all()
        r = raw_graph(L, L.bfcg_kmers_unitig_graph, km.t, 1, 5000 * (k + 2), 5000)
        assert r[:4] == (0, 5000, 5000 * (k + 2), 0) and (r[9] == -1).all()
        km.close()
    host.close()
    g.close()


def test_full_regions(gpu_lib):
    """d15 filled (test_packed_host.py): three sub-tables exactly full, so an absent successor of an end is probed round its whole region
    before the lane knows; the rows are the host twin's on the same table and the string oracle's on its dict"""
    t, d, full = PH.table(gpu_lib, "d15", "filled")
    assert len(full) == 3
    km = gpu_lib.GpuKmers(t)
    for min_cnt in (1, 2):
        rows = PH.want_unitigs(d, min_cnt)
        want = link_oracle.links(d, rows, min_cnt)
        g = t.unitig_graph(min_cnt)
        assert gpu_lib.unitig_link_rows(g[0], g[1], g[5]) == want
        _check(gpu_lib, km, min_cnt, rows, want)
    km.close()


def _has(rows, s):
    return [r for r in rows if s in r[0] or revcomp(s) in r[0]]


def test_chaining(gpu_lib):
    """a clip result answers unitig_graph as the host twin does on its to_host(); after pop_bubbles on the bubble fixture the tie
    bubble's two arms, which had two links each, are no unitigs any more, and its flanks lie on one unitig with the arm that stayed"""
    c = _bubble_case(gpu_lib, "21grown")
    k, f = c.k, bubble_oracle.fixture(c.k)
    clipped, st = c.att.clip(min_cnt=1, max_tip=12, islands=True)
    host = clipped.to_host()
    g = host.unitig_graph(1)
    rows, want = gpu_lib.unitig_rows(*g[:5]), gpu_lib.unitig_link_rows(g[0], g[1], g[5])
    assert len(st) >= 1 and want == link_oracle.links(unitig_oracle.dict_of_table(host), rows, 1)
    _check(gpu_lib, clipped, 1, rows, want)
    host.close()
    clipped.close()
    # the bubble of graph_oracle's genome and variant: the k-mer that ends before SUB, the two arms, the k-mer that starts after it
    sub, genome = graph_oracle.SUB, f.base.genome
    entry, exit_ = genome[sub - k:sub], genome[sub + 1:sub + 1 + k]
    arms = [g_[sub - k + 1:sub + k] for g_ in (f.base.genome, f.base.variant)]
    before = c.att.unitig_graph(1)
    rows0, links0 = gpu_lib.unitig_rows(*before[:5]), gpu_lib.unitig_link_rows(before[0], before[1], before[5])
    names = [r[0] for r in rows0]
    arm_names = [a if a in names else revcomp(a) for a in arms]
    assert all(a in names for a in arm_names) and _has(rows0, entry)[0][0] != _has(rows0, exit_)[0][0]
    assert sorted(e[0] for e in links0 if e[0] in arm_names) == sorted(arm_names * 2)
    popped, pst = c.att.pop_bubbles()
    after = popped.unitig_graph(1)
    rows1, links1 = gpu_lib.unitig_rows(*after[:5]), gpu_lib.unitig_link_rows(after[0], after[1], after[5])
    names1 = [r[0] for r in rows1]
    assert len(pst) >= 1 and not any(a in names1 or revcomp(a) in names1 for a in arms)
    assert not any(e[0] in arm_names or e[3] in arm_names for e in links1)
    one = _has(rows1, entry)
    assert len(one) == 1 and one == _has(rows1, exit_) and sum(1 for a in arms if _has(one, a)) == 1
    tw = popped.to_host()
    g = tw.unitig_graph(1)
    assert rows1 == gpu_lib.unitig_rows(*g[:5]) and links1 == gpu_lib.unitig_link_rows(g[0], g[1], g[5])
    tw.close()
    popped.close()


@pytest.mark.parametrize("form", ["21grown", "33host"])
def test_cap_protocol(gpu_lib, form):
    """caps of 0 size the call and leave n[2] alone; a seq_cap one short and an n_cap one short return 1 with the right n[0], n[1] and
    leave the outputs, links and n[2] included, as they were; exact caps write, and n[2] is the number of entries >= 0"""
    L, c = gpu_lib._lib.load(), _case(gpu_lib, "fixture", form)
    rows, want = _want(gpu_lib, "fixture", form, 2)
    n0, n1 = len(rows), sum(len(r[0]) for r in rows)
    n = (C.c_uint64 * 3)(FILL, FILL, FILL)
    assert L.bfcg_kmers_unitig_graph(c.att.t, 2, None, 0, None, None, None, None, None, 0, n) == 1 and list(n) == [n0, n1, FILL]
    for seq_cap, n_cap in ((0, 0), (n1 - 1, n0), (n1, n0 - 1)):
        r = raw_graph(L, L.bfcg_kmers_unitig_graph, c.att.t, 2, seq_cap, n_cap)
        assert r[:4] == (1, n0, n1, FILL) and untouched(r)
    r = raw_graph(L, L.bfcg_kmers_unitig_graph, c.att.t, 2, n1, n0)
    assert r[:4] == (0, n0, n1, len(want)) and int((r[9] >= 0).sum()) == len(want)
    assert gpu_lib.unitig_rows(*r[4:9]) == rows and gpu_lib.unitig_link_rows(r[4], r[5], r[9]) == want


def test_refusals(gpu_lib):
    """an even k, k = 39, min_cnt 0 and 256 and a NULL links with n_cap > 0 are refused before any launch with bfcg_kmers_unitigs's
    messages; nothing is written, n[] and links included, and the object stays usable"""
    L = gpu_lib._lib.load()
    c = _case(gpu_lib, "fixture", "21grown")
    for k, msg in ((32, "k=32 is even"), (39, "k=39.*k <= 37")):
        g = _count(gpu_lib, k, graph_oracle.fixture(k).reads)
        g.sync()
        km = gpu_lib.GpuKmers(g)
        with pytest.raises(gpu_lib.BfcGpuError, match=msg):
            km.unitig_graph(2)
        r = raw_graph(L, L.bfcg_kmers_unitig_graph, km.t, 2, 1 << 16, 1 << 10)
        assert r[0] == -1 and r[1:4] == (FILL, FILL, FILL) and untouched(r)
        assert km.hist()[1].sum() > 0
        km.close()
        g.close()
    for bad in (0, 256):
        with pytest.raises(gpu_lib.BfcGpuError, match="min_cnt %d is outside" % bad):
            c.att.unitig_graph(bad)
        r = raw_graph(L, L.bfcg_kmers_unitig_graph, c.att.t, bad, 1 << 16, 1 << 10)
        assert r[0] == -1 and r[1:4] == (FILL, FILL, FILL) and untouched(r)
    r = raw_graph(L, L.bfcg_kmers_unitig_graph, c.att.t, 2, 1 << 16, 1 << 10, null_links=True)
    assert r[0] == -1 and r[1:4] == (FILL, FILL, FILL) and untouched(r) and "needs output buffers" in L.bfcg_last_error().decode()
    rows, want = _want(gpu_lib, "fixture", "21grown", 2)
    _check(gpu_lib, c.att, 2, rows, want)


def test_kmergraph_tool(gpu_lib, tmp_path):
    """`python -m bfc_amd.kmergraph -m 2 -u dump` is byte for byte what the string oracle says it was before; with -g FILE the same lines
    with links<TAB>N after the n50 line, and FILE parses back to the oracle's graph -- its nodes, its k-mer edges, its link rows; -c 0
    -p 0 -g runs and its file is the graph of the table that -o wrote; a FILE that cannot be written is exit status 1"""
    c = _case(gpu_lib, "fixture", "21grown")
    k = c.k
    dump, gfa = str(tmp_path / "f.dump"), str(tmp_path / "f.gfa")
    assert c.host.dump(dump) == 0
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "bfc_amd.kmergraph", *a], capture_output=True, env=env, cwd=ROOT)
    d = unitig_oracle.dict_of_table(c.host)
    rows = unitig_oracle.unitigs(d, 2)
    want = link_oracle.links(d, rows, 2)
    plain, r = run("-m", "2", "-u", dump), run("-m", "2", "-u", "-g", gfa, dump)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr.decode()
    deg = c.att.graph_census(2)
    tips = int(deg[0, 1:].sum() + deg[1:, 0].sum())
    today = ["deg\t%d\t%s" % (o, "\t".join(str(int(v)) for v in deg[o])) for o in range(5)]
    today += ["nodes\t%d" % deg.sum(), "isolated\t%d" % deg[0, 0], "tips\t%d" % tips, "simple\t%d" % deg[1, 1], "branching\t%d" % (deg.sum() - deg[:2, :2].sum())]
    lens = sorted((len(w[0]) for w in rows), reverse=True)
    n50 = next(v for i, v in enumerate(lens) if 2 * sum(lens[:i + 1]) >= sum(lens))
    today += ["unitigs\t%d" % len(rows), "cycles\t1", "n50\t%d" % n50]
    units = ["unitig\t%s\t%d\t%.2f\t%d\t%d\t%d" % (s.decode(), n, cs / n, left, right, cyc) for s, n, cs, left, right, cyc in rows]
    assert plain.stdout.decode() == "".join(ln + "\n" for ln in today + units)
    assert r.stdout.decode() == "".join(ln + "\n" for ln in today + ["links\t%d" % len(want)] + units)
    segs, ls, nodes, edges = link_oracle.read_gfa(open(gfa, "rb").read(), k)
    sid = {s[0]: i + 1 for i, s in enumerate(rows)}
    assert [(s[0], s[1]) for s in segs.values()] == [(w[0], w[2]) for w in rows]
    assert (nodes, edges) == link_oracle.kmer_edges(d, 2) and ls == sorted((sid[s], o, sid[v], p) for s, o, cc, v, p in want)
    # cleaned first: the file describes the table that -o wrote
    gfa2, out2 = str(tmp_path / "c.gfa"), str(tmp_path / "c.dump")
    r = run("-c", "0", "-p", "0", "-g", gfa2, "-o", out2, dump)
    assert r.returncode == 0, r.stderr.decode()
    t = gpu_lib.HostTable.restore(out2)
    d2 = unitig_oracle.dict_of_table(t)
    rows2 = unitig_oracle.unitigs(d2, 1)
    want2 = link_oracle.links(d2, rows2, 1)
    segs, ls, nodes, edges = link_oracle.read_gfa(open(gfa2, "rb").read(), k)
    assert [s[0] for s in segs.values()] == [w[0] for w in rows2] and (nodes, edges) == link_oracle.kmer_edges(d2, 1) and len(ls) == len(want2)
    lines = r.stdout.decode().splitlines()
    assert "links\t%d" % len(want2) in lines and lines[lines.index("links\t%d" % len(want2)) - 1].startswith("n50\t") and not any(ln.startswith("unitig\t") for ln in lines)
    assert any(ln.startswith("clip\t") for ln in lines)
    t.close()
    r = run("-u", "-g", str(tmp_path / "no" / "such" / "dir.gfa"), dump)
    assert r.returncode == 1 and "cannot write" in r.stderr.decode()
