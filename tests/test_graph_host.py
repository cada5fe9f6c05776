"""The host twins of the de Bruijn graph calls (bfcg_neighbors_host / _graph_census_host / _graph_nb_host / _extend_host, bfcg_kmer_revcomp:
bfc_amd/csrc/bfcg_graph.hip) -- the reference side of every GPU comparison in test_gpu_graph.py -- held to bfcg_kmer_occ_host on k-mers
built by string surgery and, for odd k, to a Python dict over the exported table's strings that never touches the library's hash
(tests/graph_oracle.py).  The properties of the constructed fixture that the GPU tests rely on are asserted here.  No GPU."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import oracle
from graph_oracle import DictGraph, census_of_nb, fixture, paths, planes_of_strs, revcomp, strs_of_planes


@functools.lru_cache(maxsize=None)
def _g1():
    from bfc_amd import gen
    return gen.fixture("g1").reads()


@functools.lru_cache(maxsize=None)
def _tab(gpu_lib, which, k):
    """the fixture or g1 counted by the oracle at -b 24, dumped and restored into this library's host table -- made once, never changed"""
    reads = fixture(k).reads if which == "fixture" else _g1()
    c = oracle.Counter(k, 24)
    c.count(*reads)
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "t.hash")
        assert c.dump(fn) == 0
        t = gpu_lib.HostTable.restore(fn)
    c.close()
    assert t is not None and t.k == k
    return t


@functools.lru_cache(maxsize=None)
def _nodes(gpu_lib, which, k):
    """(y, strings, high << 8 | count) of every slot, in export_sorted()'s order"""
    t = _tab(gpu_lib, which, k)
    y, nb = t.graph_nb(1)
    ch = (t.export_sorted()[1] & np.uint64(0x3fff)).astype(np.uint16)
    return y, strs_of_planes(y, k), ch


@functools.lru_cache(maxsize=None)
def _dict(gpu_lib, which, k):
    y, strs, ch = _nodes(gpu_lib, which, k)
    return DictGraph(k, strs, ch)


def _surgery(s):
    return [s[1:] + bytes([c]) for c in b"ACGT"] + [bytes([c]) + s[:-1] for c in b"ACGT"]


@pytest.mark.parametrize("which", ["fixture", "g1"])
@pytest.mark.parametrize("k", [21, 32, 33, 37, 55])
def test_neighbors_host_is_eight_occ(gpu_lib, which, k):
    """neighbors_host equals eight bfcg_kmer_occ_host on k-mers built by slicing strings: k-mers of the reads on either strand and random
    ones; some neighbours are present, most of a random k-mer's are not"""
    t = _tab(gpu_lib, which, k)
    seq, qual, off = fixture(k).reads if which == "fixture" else _g1()
    rng = np.random.default_rng(k)
    strs = []
    while len(strs) < 150:
        r = int(rng.integers(0, len(off) - 1))
        read = seq[int(off[r]):int(off[r + 1])].tobytes()
        p = int(rng.integers(0, len(read) - k + 1))
        s = read[p:p + k].upper()
        if set(s) <= set(b"ACGT"):
            strs.append(s if rng.integers(0, 2) else revcomp(s))
    strs += [bytes(b"ACGT"[c] for c in rng.integers(0, 4, k)) for _ in range(50)]
    got = t.neighbors(planes_of_strs(strs, k))
    want = t.occ_planes(planes_of_strs([n for s in strs for n in _surgery(s)], k)).reshape(-1, 8)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert (want[:150] >= 0).any() and (want[150:] == -1).all()
    junk = np.uint64(1) << np.uint64(k)   # bits at and above k are ignored
    assert np.array_equal(t.neighbors(planes_of_strs(strs, k) | junk), want)


@pytest.mark.parametrize("which", ["fixture", "g1"])
@pytest.mark.parametrize("k", [21, 33, 37])
def test_twins_equal_the_dict_route(gpu_lib, which, k):
    """odd k: neighbours, the neighbour bits of every slot, the census and the extensions equal the dict over both strands' strings"""
    t, d = _tab(gpu_lib, which, k), _dict(gpu_lib, which, k)
    y, strs, ch = _nodes(gpu_lib, which, k)
    pick = np.random.default_rng(k).permutation(len(strs))[:300] if which == "g1" else np.arange(len(strs))
    assert np.array_equal(t.neighbors(y[pick]), np.array([d.neighbors(strs[i]) for i in pick], dtype=np.int16))
    for min_cnt in (1, 2, 3, 255):
        y2, nb = t.graph_nb(min_cnt)
        node = (ch & 0xff) >= min_cnt
        want = np.array([d.nb(s, min_cnt) if n else 0 for s, n in zip(strs, node)], dtype=np.uint8)
        assert np.array_equal(y2, y) and np.array_equal(nb, want)
        assert np.array_equal(t.graph_census(min_cnt), census_of_nb(want[node]))
        ly, lc, lh, lnb = t.list_graph(min_cnt, gpu_lib.GRAPH_MASKS["tips"])
        tip = node & ((want & 15 == 0) != (want >> 4 == 0))
        assert np.array_equal(ly, y[tip]) and np.array_equal(lnb, want[tip]) and np.array_equal(lc.astype(np.uint16) | lh.astype(np.uint16) << 8, ch[tip])
    for min_cnt, max_len in ((2, 1), (2, 7), (1, 300), (3, 300)):
        bases, length, stop = t.extend(y[pick], min_cnt, max_len)
        want = [d.extend(strs[i], min_cnt, max_len) for i in pick]
        assert paths(bases, length) == [w[0] for w in want] and list(stop) == [w[1] for w in want]


@pytest.mark.parametrize("k", [21, 33, 37, 55])
def test_reverse_complement_swaps_the_sides(gpu_lib, k):
    """odd k: neighbors(revcomp(x))[c] == neighbors(x)[4 + (3 - c)] and the other way round"""
    t = _tab(gpu_lib, "fixture", k)
    if k <= 37:
        y = _nodes(gpu_lib, "fixture", k)[0]
    else:
        f = fixture(k)
        y = planes_of_strs([f.genome[p:p + k] for p in range(0, 500, 3)] + [f.isolated, f.a_run], k)
    a, b = t.neighbors(y), t.neighbors(gpu_lib.kmer_revcomp(k, y))
    assert (a >= 0).any()
    assert np.array_equal(b[:, :4], a[:, 7:3:-1]) and np.array_equal(b[:, 4:], a[:, 3::-1])


@pytest.mark.parametrize("k", [21, 32, 33, 37, 55, 63])
def test_revcomp_is_an_involution_and_agrees_with_strings(gpu_lib, k):
    rng = np.random.default_rng(k)
    strs = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, k)) for _ in range(200)]
    y = planes_of_strs(strs, k)
    r = gpu_lib.kmer_revcomp(k, y)
    assert strs_of_planes(r, k) == [revcomp(s) for s in strs]
    assert np.array_equal(gpu_lib.kmer_revcomp(k, r), y)
    assert np.array_equal(gpu_lib.kmer_revcomp(k, y | np.uint64(1) << np.uint64(k)), r)   # bits at and above k are ignored
    out = (C.c_uint64 * 2)(5, 6)
    for bad in (0, 64, -1):
        assert gpu_lib._lib.load().bfcg_kmer_revcomp(bad, (C.c_uint64 * 2)(1, 2), out) == -1 and (out[0], out[1]) == (5, 6)


@pytest.mark.parametrize("k", [21, 32, 33, 37, 55])
def test_the_fixture_holds_every_class(gpu_lib, k):
    """what the GPU tests rely on: at min_cnt = 2 the census has isolated k-mers, tips, simple and branching nodes, the A-run is its own
    successor and predecessor, and the extensions named by the issue stop where the construction says, with every stop code 0 to 5"""
    t, f = _tab(gpu_lib, "fixture", k), fixture(k)
    if k <= 37:
        deg = t.graph_census(2)
        assert deg[0, 0] > 0 and deg[1, 0] + deg[0, 1] > 0 and deg[1, 1] > 100 and deg[2, 1] + deg[1, 2] > 0
        y, strs, ch = _nodes(gpu_lib, "fixture", k)
        nb = t.graph_nb(2)[1]
        assert (ch & 0xff).min() >= 2
        assert nb[strs.index(f.a_run)] == 0x11
        iso = strs.index(f.isolated) if f.isolated in strs else strs.index(revcomp(f.isolated))
        assert nb[iso] == 0
    seeds = [f.isolated, f.left_of_bubble, f.in_branch, f.a_run, f.seed, b"ACGT" * (k // 4) + b"ACG"[:k % 4]]
    bases, length, stop = t.extend(planes_of_strs(seeds, k), 2, 300)
    p = paths(bases, length)
    assert (p[0], stop[0]) == (b"", 1)
    assert (p[1], stop[1]) == (f.genome[300 - 5:300], 2)
    assert (p[2], stop[2]) == (f.genome[300 - 3 + k:300 + k], 3)
    assert (p[3], stop[3]) == (b"", 5)
    assert (p[4], stop[4]) == (f.genome[160 + k:300], 2)
    assert (p[5], stop[5]) == (b"", 4)
    bases, length, stop = t.extend(planes_of_strs([f.seed], k), 2, 10)
    assert (paths(bases, length)[0], stop[0]) == (f.genome[160 + k:170 + k], 0)
    # to the left: the same call on the reverse complement; both walks spell the unitig the generator knows.  Odd k only: the reads give
    # one strand, and for even k the strand rule hashes an undecided k-mer as given, so its reverse complement is another key
    if k % 2 == 0:
        return
    bases, length, stop = t.extend(gpu_lib.kmer_revcomp(k, planes_of_strs([f.seed], k)), 2, 300)
    assert stop[0] == 3 and revcomp(paths(bases, length)[0]) + f.seed + p[4] == f.unitig


def test_refusals_leave_the_outputs_untouched(gpu_lib):
    """min_cnt outside [1, 255], max_len outside [1, 65535], a cell mask of 0 or beyond 2^25, k > 37 for the census and the listing's twin:
    refused with a message, nothing written"""
    L = gpu_lib._lib.load()
    t, t55 = _tab(gpu_lib, "fixture", 21), _tab(gpu_lib, "fixture", 55)
    y = planes_of_strs([fixture(21).seed], 21)
    deg = np.full(25, 77, dtype=np.uint64)
    bases, ls, nb = np.full(8, 77, dtype=np.uint8), np.full(2, 77, dtype=np.int32), np.full(4096, 77, dtype=np.uint8)
    u64p = C.POINTER(C.c_uint64)
    for bad in (0, 256, -3):
        assert L.bfcg_graph_census_host(t.ptr, bad, deg.ctypes.data_as(u64p)) == -1
        assert "min_cnt %d is outside [1, 255]" % bad in L.bfcg_last_error().decode()
        assert L.bfcg_graph_nb_host(t.ptr, bad, None, nb.ctypes.data) == -1
        assert L.bfcg_extend_host(t.ptr, y.ctypes.data, 1, bad, 8, bases.ctypes.data, ls.ctypes.data) == -1
    for bad in (0, 65536, -1):
        assert L.bfcg_extend_host(t.ptr, y.ctypes.data, 1, 2, bad, bases.ctypes.data, ls.ctypes.data) == -1
        assert "max_len %d is outside [1, 65535]" % bad in L.bfcg_last_error().decode()
    assert L.bfcg_graph_census_host(t55.ptr, 2, deg.ctypes.data_as(u64p)) == -1
    assert "k=55" in L.bfcg_last_error().decode() and "k <= 37" in L.bfcg_last_error().decode()
    assert L.bfcg_graph_nb_host(t55.ptr, 2, None, nb.ctypes.data) == -1
    for bad in (0, 1 << 25):
        with pytest.raises(gpu_lib.BfcGpuError, match="cell_mask"):
            t.list_graph(2, bad)
    assert (deg == 77).all() and (bases == 77).all() and (ls == 77).all() and (nb == 77).all()
    assert L.bfcg_extend_host(t55.ptr, y.ctypes.data, 0, 2, 8, None, None) == 0   # n = 0
