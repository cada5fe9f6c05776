"""GPU tests (-m gpu) of the count table read as a de Bruijn graph (bfcg_kmers_neighbors / _graph_census / _list_graph / _extend,
bfc_amd/csrc/bfcg_graph.hip) through GpuKmers, and of `python -m bfc_amd.kmergraph`.  The reference side is the host twins on the
exported table (HostTable.neighbors / graph_census / graph_nb / extend), which tests/test_graph_host.py holds to bfcg_kmer_occ_host and
to a Python dict over the table's strings; the inputs are the constructed fixture of tests/graph_oracle.py, in which every class of node
is there by design, and g1 at -b 24."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from graph_oracle import census_of_nb, fixture, in_mask, paths, planes_of_strs, revcomp
from test_gpu_kmers import _count, _g1
from test_gpu_tabcmp import FORMS
from test_lookup_host import stream_kmers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64
NAMED = ["tips", "isolated", "branching", "simple", "all"]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(gpu_lib, which, k, form=None):
    """a table counted on the GPU: attached, exported to the host, the export uploaded again -- made once, never changed"""
    c = Case()
    c.k = k
    kw = FORMS[form][1] if form else dict(table_layout=0) if k == 21 else {}
    c.reads = fixture(k).reads if which == "fixture" else _g1()
    c.g = _count(gpu_lib, k, c.reads, n_batches=3 if which == "g1" else 1, **kw)
    c.g.sync()
    c.segments = bool(c.g.table_info()["segments"])
    c.att = gpu_lib.GpuKmers(c.g)
    c.host = c.g.export_table()
    c.up = gpu_lib.GpuKmers(c.host)
    return c


@functools.lru_cache(maxsize=None)
def _read_kmers(which, k, n_reads):
    """the distinct k-mers rolled from the first reads, as planes"""
    seq, qual, off = fixture(k).reads if which == "fixture" else _g1()
    n = min(n_reads, len(off) - 1)
    stream = np.concatenate([np.append(seq[int(off[r]):int(off[r + 1])], 10) for r in range(n)]).astype(np.uint8)
    ends, y = stream_kmers(stream, k)
    return np.unique(y[ends], axis=0)


@functools.lru_cache(maxsize=None)
def _host_nb(gpu_lib, which, k, form, min_cnt):
    """the twin of a listing: sub-table, planes, high << 8 | count and neighbour bits of every slot of the export"""
    c = _case(gpu_lib, which, k, form)
    sizes, slots = c.host.export_sorted()
    y, nb = c.host.graph_nb(min_cnt)
    return np.repeat(np.arange(len(sizes), dtype=np.uint64), sizes), y, (slots & U(0x3fff)).astype(np.uint16), nb


def _rows(sub, y, ch, nb):
    """rows (sub-table, y0, y1, high << 8 | count, nb) sorted inside a sub-table, sub-tables ascending"""
    r = np.empty((len(ch), 5), dtype=np.uint64)
    r[:, 0], r[:, 1:3], r[:, 3], r[:, 4] = sub, y, ch, nb
    return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]


# ---- neighbours ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["fixture", "g1"])
@pytest.mark.parametrize("k", [21, 32, 33, 37, 38, 55, 63])
def test_neighbors_equal_host_twin(gpu_lib, which, k):
    """every listed k-mer (k <= 37) or the k-mers rolled from the reads (k > 37), and 1000 random ones: eight values each, entry for entry
    the host twin's on the exported table -- on the attached table (at k = 21 one whose segments the attach converts) and on the upload"""
    c = _case(gpu_lib, which, k)
    assert c.segments or k != 21
    q = c.att.list()[0] if k <= 37 else _read_kmers(which, k, 200)
    rnd = np.random.default_rng(k).integers(0, 1 << k, (1000, 2), dtype=np.uint64)
    q = np.concatenate([q, rnd])
    want = c.host.neighbors(q)
    assert len(q) > 1500 and (want[:-1000] >= 0).any(axis=1).sum() > 500 and (want[-1000:] == -1).all()
    for km in (c.att, c.up):
        got = km.neighbors(q)
        assert got.dtype == np.int16 and got.shape == (len(q), 8) and np.array_equal(got, want)
        assert km.last_ms() > 0
        assert km.neighbors(np.zeros((0, 2), dtype=np.uint64)).shape == (0, 8) and km.last_ms() == 0
    assert np.array_equal(c.att.neighbors(q[:3000] | U(1) << U(k)), want[:3000])   # bits at and above k are ignored


def test_neighbors_staging_seams(gpu_lib, monkeypatch):
    """BFCG_LOOKUP_CAP = 1000 (read when the object is made) and n = 2501: two full pieces and a ragged last one"""
    c = _case(gpu_lib, "g1", 33)
    q = c.att.list()[0][:2501]
    monkeypatch.setenv("BFCG_LOOKUP_CAP", "1000")
    small = gpu_lib.GpuKmers(c.g)
    monkeypatch.delenv("BFCG_LOOKUP_CAP")
    want = c.host.neighbors(q)
    for n in (1, 999, 1000, 1001, 2000, 2501):
        assert np.array_equal(small.neighbors(q[:n]), want[:n]), n
    small.close()


# ---- census -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["21seg", "21grown", "32host", "33host", "37grown"])
def test_census_equals_host_twin(gpu_lib, form):
    """graph_census on g1 for the forms of test_gpu_tabcmp.py's table A -- segments converted at attach, grown from two slots per
    sub-table, the host's layout -- and min_cnt 1, 2, 3, 255: the host twin's census of the export, on the attached table and on the
    upload; its sum is the number of keys with count >= min_cnt that hist() counts"""
    k = FORMS[form][0]
    c = _case(gpu_lib, "g1", k, form)
    cnt = c.att.hist()[1]
    for min_cnt in (1, 2, 3, 255):
        want = c.host.graph_census(min_cnt)
        for km in (c.att, c.up):
            got = km.graph_census(min_cnt)
            assert got.shape == (5, 5) and np.array_equal(got, want) and km.last_ms() > 0
        assert int(want.sum()) == int(cnt[min_cnt:].sum())
    assert c.host.graph_census(1)[1, 1] > 10000 and c.host.graph_census(255).sum() == 0


@pytest.mark.parametrize("k", [21, 32, 33, 37])
def test_census_of_the_fixture(gpu_lib, k):
    """the constructed classes are counted: isolated k-mers, tips, simple nodes and the bubble's branch nodes, as the host twin does"""
    c = _case(gpu_lib, "fixture", k)
    for min_cnt in (1, 2, 3, 255):
        want = c.host.graph_census(min_cnt)
        assert np.array_equal(c.att.graph_census(min_cnt), want) and np.array_equal(c.up.graph_census(min_cnt), want)
    deg = c.att.graph_census(2)
    assert deg[0, 0] > 0 and deg[1, 0] + deg[0, 1] > 0 and deg[1, 1] > 100 and deg[2, 1] + deg[1, 2] > 0


def test_refusals(gpu_lib):
    """k = 51: the census and the listing are refused with the listing's message; min_cnt, cell_mask and max_len out of range are
    refused; the object stays usable"""
    c51, c = _case(gpu_lib, "fixture", 51), _case(gpu_lib, "fixture", 21)
    with pytest.raises(gpu_lib.BfcGpuError, match="k=51.*k <= 37"):
        c51.att.graph_census(2)
    with pytest.raises(gpu_lib.BfcGpuError, match="k=51.*k <= 37"):
        c51.att.list_graph(2)
    for bad in (0, 256):
        for call in (lambda: c.att.graph_census(bad), lambda: c.att.list_graph(bad), lambda: c.att.extend(np.zeros((1, 2), dtype=U), bad, 5)):
            with pytest.raises(gpu_lib.BfcGpuError, match="min_cnt %d is outside" % bad):
                call()
    for bad in (0, 1 << 25):
        with pytest.raises(gpu_lib.BfcGpuError, match="cell_mask"):
            c.att.list_graph(2, bad)
    for bad in (0, 65536):
        with pytest.raises(gpu_lib.BfcGpuError, match="max_len %d is outside" % bad):
            c.att.extend(np.zeros((1, 2), dtype=U), 2, bad)
    # through the C ABI: a refusal writes nothing
    import ctypes as C
    L = gpu_lib._lib.load()
    deg, n, out = np.full(25, 77, dtype=U), C.c_uint64(77), np.full(64, 77, dtype=np.uint8)
    seed = np.zeros((1, 2), dtype=U)
    assert L.bfcg_kmers_graph_census(c.att.t, 0, deg.ctypes.data_as(C.POINTER(C.c_uint64))) == -1
    assert L.bfcg_kmers_graph_census(c51.att.t, 2, deg.ctypes.data_as(C.POINTER(C.c_uint64))) == -1
    assert L.bfcg_kmers_list_graph(c.att.t, 2, 0, 0, 1 << c.att.l_pre, out.ctypes.data, out.ctypes.data, out.ctypes.data, 2, C.byref(n)) == -1
    assert L.bfcg_kmers_extend(c.att.t, seed.ctypes.data, 1, 2, 65536, out.ctypes.data, out.ctypes.data) == -1
    assert L.bfcg_kmers_extend(c.att.t, seed.ctypes.data, 1, 256, 8, out.ctypes.data, out.ctypes.data) == -1
    assert (deg == 77).all() and n.value == 77 and (out == 77).all()
    assert c51.att.neighbors(_read_kmers("fixture", 51, 10)).shape[1] == 8
    assert np.array_equal(c.att.graph_census(2), c.host.graph_census(2))


# ---- listing by degree cell ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["fixture", "g1"])
@pytest.mark.parametrize("k", [21, 32, 33, 37])
def test_list_graph_equals_host_twin(gpu_lib, which, k):
    """rows (sub-table run, planes, high << 8 | count, nb) equal the twin's under every named mask and under all 25 bits, at min_cnt 1
    and 2; the census recomputed from a full listing's nb is graph_census"""
    c = _case(gpu_lib, which, k)
    for min_cnt in (1, 2):
        sub, hy, hch, hnb = _host_nb(gpu_lib, which, k, None, min_cnt)
        node = (hch & 0xff) >= min_cnt
        for name in NAMED:
            mask = gpu_lib.GRAPH_MASKS[name]
            keep = node & in_mask(hnb, mask)
            y, cnt, high, nb = (c.att if name != "simple" else c.up).list_graph(min_cnt, mask)
            assert len(cnt) == int(keep.sum()) and (which == "g1" or name == "all" or 0 < len(cnt) < node.sum())
            want = _rows(sub[keep], hy[keep], hch[keep], hnb[keep])
            assert np.array_equal(_rows(np.sort(sub[keep]), y, cnt.astype(np.uint16) | high.astype(np.uint16) << 8, nb), want)
            if name == "all":
                assert np.array_equal(census_of_nb(nb), c.att.graph_census(min_cnt))
    assert c.att.last_ms() > 0


@pytest.mark.parametrize("k", [21, 37])
def test_list_graph_ranges_pieces_and_cap(gpu_lib, k):
    """sub-table ranges and pieces of a few thousand k-mers concatenate to the whole; a cap one short writes nothing and reports the
    number needed"""
    c = _case(gpu_lib, "g1", k)
    n_sub = 1 << c.att.l_pre
    cuts = [0, 1, n_sub // 3, n_sub // 3 + 1, n_sub - 7, n_sub]
    for mask in (gpu_lib.GRAPH_MASKS["all"], gpu_lib.GRAPH_MASKS["all"] & ~gpu_lib.GRAPH_MASKS["simple"]):   # everything; what the filter leaves of g1: a few hundred
        whole = c.att.list_graph(1, mask)
        assert (len(whole[1]) == c.host.count()) == (mask == gpu_lib.GRAPH_MASKS["all"]) and len(whole[1]) > 100
        parts = [c.att.list_graph(1, mask, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
        for j in range(4):
            assert np.array_equal(np.concatenate([p[j] for p in parts]), whole[j])
        small = c.att.list_graph(1, mask, piece=3000)
        assert all(np.array_equal(a, b) for a, b in zip(small, whole))
        n = len(whole[1])
        rc, need, y, ch, nb = c.att.list_graph_raw(1, mask, 0, n_sub, n - 1)
        assert (rc, need) == (1, n) and not y.any() and not ch.any() and not nb.any()
        rc, got, y, ch, nb = c.att.list_graph_raw(1, mask, 0, n_sub, n)
        assert (rc, got) == (0, n) and np.array_equal(y, whole[0]) and np.array_equal(nb, whole[3])


# ---- extension ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [21, 32, 33, 55])
def test_extend_equals_host_twin(gpu_lib, k):
    """every k-mer of the fixture's reads, and 50 random ones, as seeds, and 2000 k-mers of g1's reads: paths, lengths and stop codes are
    the host twin's for max_len 1, 7 and 300; every stop code 0 to 5 occurs on the fixture"""
    seen = set()
    for which in ("fixture", "g1"):
        c = _case(gpu_lib, which, k)
        q = _read_kmers(which, k, 10 ** 6 if which == "fixture" else 40)[:2000 if which == "g1" else None]
        q = np.concatenate([q, np.random.default_rng(k).integers(0, 1 << k, (50, 2), dtype=np.uint64)])
        for max_len in (1, 7, 300):
            want = c.host.extend(q, 2, max_len)
            for km in (c.att, c.up):
                got = km.extend(q, 2, max_len)
                assert got[0].shape == (len(q), max_len) and all(np.array_equal(a, b) for a, b in zip(got, want))
                assert km.last_ms() > 0
            paths(want[0], want[1])   # zero beyond every length
            if which == "fixture":
                seen |= set(int(s) for s in want[2])
        assert (want[1] > 0).any()
    assert seen == {0, 1, 2, 3, 4, 5}
    assert all(len(a) == 0 for a in _case(gpu_lib, "fixture", k).att.extend(np.zeros((0, 2), dtype=U), 2, 9))


@pytest.mark.parametrize("k", [21, 33, 55])
def test_left_and_right_spell_the_unitig(gpu_lib, k):
    """around a mid-genome seed the walk to the right ends before the bubble (code 2), the walk to the left -- the same call on the
    reverse complement -- before the node the tip hangs off (code 3): together they spell the generator's genome between the two.  Odd
    k: the reads give one strand, and for even k the strand rule hashes an undecided k-mer as given, so a reverse complement is another
    key"""
    c, f = _case(gpu_lib, "fixture", k), fixture(k)
    seed = planes_of_strs([f.seed], k)
    rb, rl, rs = c.att.extend(seed, 2, 300)
    lb, ll, ls = c.att.extend(gpu_lib.kmer_revcomp(k, seed), 2, 300)
    assert (rs[0], ls[0]) == (2, 3)
    assert revcomp(paths(lb, ll)[0]) + f.seed + paths(rb, rl)[0] == f.unitig and len(f.unitig) > 150


def test_extend_staging_seams(gpu_lib, monkeypatch):
    """BFCG_LOOKUP_CAP = 100 leaves room for five paths of 300 bases a piece, and for one of 3000: pieces and a ragged last piece"""
    c = _case(gpu_lib, "fixture", 33)
    q = _read_kmers("fixture", 33, 10 ** 6)[:203]
    monkeypatch.setenv("BFCG_LOOKUP_CAP", "100")
    small = gpu_lib.GpuKmers(c.g)
    monkeypatch.delenv("BFCG_LOOKUP_CAP")
    for max_len, n in ((300, 203), (3000, 7), (16, 203)):
        want = c.host.extend(q[:n], 2, max_len)
        got = small.extend(q[:n], 2, max_len)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), max_len
    small.close()


# ---- the tool -------------------------------------------------------------------------------------------------------------------------

def test_kmergraph_tool(gpu_lib, tmp_path):
    """`python -m bfc_amd.kmergraph -m 2 -t -x seeds dump` on a dump of the fixture prints the census the test computed, the folded
    summary, the tips with their neighbour bases, and the unitig around the seed"""
    k = 21
    c, f = _case(gpu_lib, "fixture", k), fixture(k)
    dump, seeds = str(tmp_path / "f.dump"), str(tmp_path / "seeds.txt")
    assert c.host.dump(dump) == 0
    with open(seeds, "wb") as fh:
        fh.write(b">a seed\n" + f.seed + b"\n" + f.a_run + b"\n")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "bfc_amd.kmergraph", "-m", "2", "-t", "-x", seeds, dump], capture_output=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()
    lines = r.stdout.decode().splitlines()
    deg = c.att.graph_census(2)
    assert lines[:5] == ["deg\t%d\t%s" % (o, "\t".join(str(int(v)) for v in deg[o])) for o in range(5)]
    y, cnt, high, nb = c.att.list_graph(2, gpu_lib.GRAPH_MASKS["tips"])
    tips = int(deg[0, 1:].sum() + deg[1:, 0].sum())
    assert lines[5:10] == ["nodes\t%d" % deg.sum(), "isolated\t%d" % deg[0, 0], "tips\t%d" % tips, "simple\t%d" % deg[1, 1],
                           "branching\t%d" % (deg.sum() - deg[:2, :2].sum())]
    assert len(cnt) == tips > 0
    assert lines[10:10 + tips] == ["%s\t%d\t%d\t%s" % (s, a, b, gpu_lib.nb_text(v)) for s, a, b, v in zip(c.att.strings(y), cnt, high, nb)]
    assert lines[10 + tips].split("\t") == [f.seed.decode(), f.unitig.decode(), str(160 - (147 - k)), "3", str(300 - 160 - k), "2"]
    assert lines[11 + tips].split("\t") == [f.a_run.decode(), f.a_run.decode(), "0", "5", "0", "5"] and len(lines) == 12 + tips
