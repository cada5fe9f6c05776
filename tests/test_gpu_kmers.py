"""GPU tests (-m gpu) of the table read-out (bfcg_kmers_*, bfc_amd/csrc/bfcg_kmers.hip) through the C ABI and GpuKmers: the spectrum and
the sub-table sizes against the oracle, the listing against the host instance of the decode and against the reference's hash2cnt, and
the command-line tool `python -m bfc_amd.hash2cnt` against the reference tool byte for byte."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from test_kmers_host import HASH2CNT, decode_slots

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
need_ref = pytest.mark.skipif(not os.path.exists(HASH2CNT), reason="oracle/_ref/hash2cnt not built (needs the reference's sources)")
B = 24


@functools.lru_cache(maxsize=None)
def _g1():
    from bfc_amd import gen
    return gen.fixture("g1").reads()


@functools.lru_cache(maxsize=None)
def _want(k, l_pre=20):
    """the oracle on g1 at -b 24: (mode, cnt, high), sizes, slots -- computed once per k"""
    seq, qual, off = _g1()
    c = oracle.Counter(k, B, l_pre=l_pre)
    c.count(seq, qual, off)
    hist, (sizes, slots) = c.table_hist(), c.export()
    c.close()
    return hist, sizes, slots


def _count(gpu_lib, k, reads=None, n_batches=1, **kw):
    seq, qual, off = reads if reads is not None else _g1()
    n = len(off) - 1
    per = (n + n_batches - 1) // n_batches
    g = gpu_lib.GpuCounter(k, B, max_batch_pos=int(off[min(per, n)]) + per + 64, **kw)
    for i in range(0, n, per):
        j = min(n, i + per)
        o = off[i:j + 1] - off[i]
        g.count_host(gpu_lib.to_stream(seq[int(off[i]):int(off[j])], o), gpu_lib.to_stream(qual[int(off[i]):int(off[j])], o))
    return g


def _same_hist(got, want):
    return got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def _rows(y, cnt, high):
    """the listing as sorted rows (y0, y1, count, high)"""
    r = np.empty((len(cnt), 4), dtype=np.uint64)
    r[:, :2], r[:, 2], r[:, 3] = y, cnt, high
    return r[np.lexsort((r[:, 1], r[:, 0]))]


def _host_rows(L, k, l_pre, sizes, slots):
    """the host instance of the decode on a table in L1 form: planes, high << 8 | count, sub-table of every slot"""
    y, ch = decode_slots(L, k, l_pre, sizes, slots)
    return y, ch, np.repeat(np.arange(len(sizes)), sizes)


def _keep(slots, min_cnt, min_diff):
    """hash2cnt's -m / -d on the slots' fields"""
    cnt, high = (slots & np.uint64(0xff)).astype(np.int64), (slots >> np.uint64(8) & np.uint64(0x3f)).astype(np.int64)
    return (cnt >= min_cnt) & (np.minimum(cnt, 63) - high >= min_diff)


@pytest.mark.parametrize("k", [21, 32, 33, 35, 37, 51])
def test_hist_and_sizes_attached_and_uploaded(gpu_lib, k):
    """hist() and sub_sizes() equal the oracle's bfc_ch_hist and sub-table sizes, read in place from the counting context (nothing
    exported) and from the exported table uploaded again; k = 51: they need no decode.  list() refuses k > 37 with a clear message."""
    hist, sizes, slots = _want(k)
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    assert (km.k, km.l_pre) == (k, int(np.log2(len(sizes))))
    assert _same_hist(km.hist(), hist)
    assert np.array_equal(km.sub_sizes(), sizes)
    assert km.last_ms() > 0
    both = km.hist_sizes()   # one pass for both
    assert _same_hist(both[:3], hist) and np.array_equal(both[3], sizes)
    if k > 37:
        with pytest.raises(gpu_lib.BfcGpuError, match="k <= 37"):
            km.list()
        assert "k=51" in gpu_lib._lib.load().bfcg_last_error().decode()
    km.close()
    t = g.export_table()
    g.close()
    km = gpu_lib.GpuKmers(t)
    assert _same_hist(km.hist(), hist)
    assert np.array_equal(km.sub_sizes(), sizes)
    km.close(); t.close()


@pytest.mark.parametrize("k", [21, 32, 33, 35, 37])
def test_list_equals_host_decode(gpu_lib, k):
    """list() as a set of (y0, y1, count, high) equals the host instance of the decode on export_sorted()'s slots; sub-tables ascending;
    several sub-table ranges, and pieces of a few thousand k-mers, concatenate to the whole; a cap one short writes nothing"""
    L = gpu_lib._lib.load()
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    y, cnt, high = km.list()
    assert km.last_ms() > 0
    t = g.export_table()
    sizes, slots = t.export_sorted()
    assert np.array_equal(slots, _want(k)[2])
    hy, hch, hsub = _host_rows(L, k, km.l_pre, sizes, slots)
    want = _rows(hy, hch & 0xff, hch >> 8)
    assert len(cnt) == len(slots) and np.array_equal(_rows(y, cnt, high), want)
    # sub-tables ascending: the sub-table of every listed k-mer, looked up by its planes
    sub_of = {(int(a), int(b)): int(s) for (a, b), s in zip(hy, hsub)}
    subs = np.array([sub_of[(int(a), int(b))] for a, b in y])
    assert np.all(np.diff(subs) >= 0) and np.array_equal(np.bincount(subs, minlength=len(sizes)), sizes)
    # ranges (also odd bounds) and small pieces
    n_sub = len(sizes)
    cuts = [0, 1, n_sub // 3 + 1, n_sub // 2, n_sub - 1, n_sub]
    parts = [km.list(sub_lo=cuts[i], sub_hi=cuts[i + 1]) for i in range(len(cuts) - 1)]
    for i, p in enumerate(parts):
        assert len(p[1]) == int(sizes[cuts[i]:cuts[i + 1]].sum())
    assert np.array_equal(_rows(*[np.concatenate([p[j] for p in parts]) for j in range(3)]), want)
    py, pc, ph = km.list(piece=5000)
    assert np.array_equal(_rows(py, pc, ph), want)
    per = n_sub // 7 + 1
    km.MAX_SLOTS = per << km.cshift   # pieces are bounded by slots too: here at most `per` sub-tables a call (sizes handed in)
    assert sum(1 for _ in km.pieces(sizes=sizes)) == (n_sub + per - 1) // per
    assert np.array_equal(_rows(*km.list()), want)
    del km.MAX_SLOTS
    # cap one below the need: 1, *n = the need, nothing written (a guard pattern fills the whole buffer)
    need = len(slots)
    by, bch = np.full((need, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(need, 0xA5A5, dtype=np.uint16)
    n = C.c_uint64()
    assert L.bfcg_kmers_list(km.t, 0, 0, 0, n_sub, by.ctypes.data, bch.ctypes.data, need - 1, C.byref(n)) == 1
    assert n.value == need and np.all(by == 0xA5A5A5A5A5A5A5A5) and np.all(bch == 0xA5A5)
    assert L.bfcg_kmers_list(km.t, 0, 0, 0, n_sub, by.ctypes.data, bch.ctypes.data, need, C.byref(n)) == 0 and n.value == need
    assert np.array_equal(_rows(by, bch & 0xff, bch >> 8), want)
    assert L.bfcg_kmers_list(km.t, 0, 0, 5, 5, None, None, 0, C.byref(n)) == 0 and n.value == 0   # an empty range
    assert L.bfcg_kmers_list(km.t, 0, 0, 0, n_sub + 1, None, None, 0, C.byref(n)) == -1             # a range beyond the table
    km.close(); t.close(); g.close()


FILTERS = [(0, 0), (3, 0), (0, 1), (3, 1), (2, 1)]   # (-m, -d); g1 has no k-mer seen three times with a low-quality copy: -m 3 -d 1 keeps nothing


def _filter_case(gpu_lib, k):
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    t = g.export_table()
    return g, km, t


@pytest.mark.parametrize("k", [21, 33, 37])
def test_filters(gpu_lib, k):
    """-m / -d: the listing equals the rule applied to the exported slots, and -m 3, -d 1 and -m 2 -d 1 each keep some k-mers and
    drop others"""
    L = gpu_lib._lib.load()
    g, km, t = _filter_case(gpu_lib, k)
    sizes, slots = t.export_sorted()
    hy, hch, _ = _host_rows(L, k, km.l_pre, sizes, slots)
    for m, d in FILTERS:
        y, cnt, high = km.list(min_cnt=m, min_diff=d)
        keep = _keep(slots, m, d)
        assert len(cnt) == int(keep.sum())
        if (m, d) in [(3, 0), (0, 1), (2, 1)]:
            assert 0 < len(cnt) < len(slots)
        assert np.array_equal(_rows(y, cnt, high), _rows(hy[keep], hch[keep] & 0xff, hch[keep] >> 8)), (m, d)
    km.close(); t.close(); g.close()


@need_ref
@pytest.mark.parametrize("k", [21, 33, 37])
def test_filters_vs_reference_hash2cnt(gpu_lib, tmp_path, k):
    """the listing's sorted lines equal `hash2cnt [-m INT] [-d INT] dump | sort` on this library's dump, for every filter of FILTERS"""
    g, km, t = _filter_case(gpu_lib, k)
    fn = str(tmp_path / "t.hash")
    assert t.dump(fn) == 0
    for m, d in FILTERS:
        y, cnt, high = km.list(min_cnt=m, min_diff=d)
        ref = subprocess.run([HASH2CNT, "-m", str(m), "-d", str(d), fn], capture_output=True, check=True).stdout.splitlines()
        ch = cnt.astype(np.uint16) | high.astype(np.uint16) << 8
        assert sorted(km.format(y, ch).splitlines()) == sorted(ref), (m, d)
        assert km.strings(y[:3]) == [ln.split(b"\t")[0].decode() for ln in km.format(y[:3], ch[:3]).splitlines()]
    km.close(); t.close(); g.close()


def test_empty_table(gpu_lib):
    """a context that counted nothing: no k-mers, an all-zero histogram, mode -1, all sizes 0"""
    g = gpu_lib.GpuCounter(31, B, max_batch_pos=1 << 16)
    km = gpu_lib.GpuKmers(g)
    mode, cnt, high = km.hist()
    assert mode == -1 and not cnt.any() and not high.any()
    sizes = km.sub_sizes()
    assert len(sizes) == 1 << 20 and not sizes.any()
    y, c, h = km.list()
    assert y.shape == (0, 2) and len(c) == 0 and len(h) == 0
    km.close(); g.close()


def test_saturated_counts(gpu_lib):
    """the same reads thousands of times (tests/test_gpu_parity.py: test_massive_duplicates_saturate_exactly): count 255 and high 63 in
    the spectrum and the listing, and min(count, 63) - high at the cap -- 63 - 63 = 0 passes -d 0 and fails -d 1"""
    Lr = 150
    rng = np.random.default_rng(3)
    other = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, Lr)]
    n = 6000
    seq = np.concatenate([np.frombuffer(b"A" * Lr, dtype=np.uint8) if i % 3 else other for i in range(n)])
    qual = np.full(len(seq), ord("I"), dtype=np.uint8)
    qual[10::75] = ord("#")
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(Lr)
    oc = oracle.Counter(31, B)
    oc.count(seq, qual, off)
    hist, (sizes, slots) = oc.table_hist(), oc.export()
    oc.close()
    L = gpu_lib._lib.load()
    g = _count(gpu_lib, 31, (seq, qual, off), 3)
    km = gpu_lib.GpuKmers(g)
    assert _same_hist(km.hist(), hist) and hist[1][255] > 0 and hist[2][63] > 0
    assert np.array_equal(km.sub_sizes(), sizes)
    sat = (slots & np.uint64(0x3fff)) == np.uint64(63 << 8 | 255)
    assert sat.any()
    hy, hch, _ = _host_rows(L, 31, km.l_pre, sizes, slots)
    for d in (0, 1):
        y, cnt, high = km.list(min_diff=d)
        keep = _keep(slots, 0, d)
        assert not (keep & sat).any() if d else (keep & sat).any()
        assert np.array_equal(_rows(y, cnt, high), _rows(hy[keep], hch[keep] & 0xff, hch[keep] >> 8))
        assert bool(((cnt == 255) & (high == 63)).any()) == (d == 0)
    km.close(); g.close()


@pytest.mark.parametrize("case", ["segments", "host_layout", "grown"])
def test_table_layouts(gpu_lib, case):
    """the context's table in region-owned segments (converted in place by attach, nothing exported), in the host's layout from the
    start, and in the host's layout grown from two slots per sub-table: the same spectrum, sizes and k-mers"""
    L = gpu_lib._lib.load()
    k, l_pre = 21, (10 if case == "grown" else 20)
    hist, sizes, slots = _want(k, l_pre)
    kw = dict(segments=dict(table_layout=0), host_layout=dict(table_layout=1), grown=dict(table_layout=1, l_pre=10, tab_cshift=1))[case]
    g = _count(gpu_lib, k, n_batches=3, **kw)
    g.sync()
    ti = g.table_info()
    assert ti["segments"] == (case == "segments"), ti
    km = gpu_lib.GpuKmers(g)
    assert not g.table_info()["segments"]
    if case == "grown":
        assert km.cshift > 1
    assert _same_hist(km.hist(), hist)
    assert np.array_equal(km.sub_sizes(), sizes)
    y, cnt, high = km.list()
    hy, hch, _ = _host_rows(L, k, km.l_pre, sizes, slots)
    assert np.array_equal(_rows(y, cnt, high), _rows(hy, hch & 0xff, hch >> 8))
    km.close(); g.close()


def _tool(*args):
    return subprocess.run([sys.executable, "-m", "bfc_amd.hash2cnt", *args], capture_output=True, cwd=ROOT, timeout=300)


@need_ref
def test_tool_matches_reference(gpu_lib, tmp_path):
    """python -m bfc_amd.hash2cnt in a fresh process on this library's dump of g1 (k = 33): -s, -h and -s -h byte-identical to the
    reference's hash2cnt, the listings identical after sort"""
    g = _count(gpu_lib, 33)
    t = g.export_table()
    fn = str(tmp_path / "t.hash")
    assert t.dump(fn) == 0
    t.close(); g.close()
    for flags in (["-s"], ["-h"], ["-s", "-h"]):
        r, ref = _tool(*flags, fn), subprocess.run([HASH2CNT, *flags, fn], capture_output=True)
        assert r.returncode == 0 == ref.returncode, r.stderr[-500:]
        assert r.stdout == ref.stdout, flags
    for flags in ([], ["-m", "3"], ["-m", "2", "-d", "1"]):
        r, ref = _tool(*flags, fn), subprocess.run([HASH2CNT, *flags, fn], capture_output=True)
        assert r.returncode == 0 == ref.returncode, r.stderr[-500:]
        assert len(ref.stdout) > 0 and sorted(r.stdout.splitlines()) == sorted(ref.stdout.splitlines()), flags


def test_tool_refuses_k39_listing(gpu_lib, tmp_path):
    """k = 39: the listing prints the reference's error line and exits 1 before any output; -s and -h still work"""
    seq, qual, off = _g1()
    n = 2000
    g = _count(gpu_lib, 39, (seq[:int(off[n])], qual[:int(off[n])], off[:n + 1]))
    t = g.export_table()
    fn = str(tmp_path / "t39.hash")
    assert t.dump(fn) == 0
    hist, (sizes, _) = t.hist(), t.export_sorted()
    t.close(); g.close()
    r = _tool(fn)
    assert r.returncode == 1 and r.stdout == b"" and b"ERROR: hash2cnt does not work for k>37\n" in r.stderr
    r = _tool("-s", "-h", fn)
    assert r.returncode == 0, r.stderr[-500:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(sizes) + 256 and [int(v) for v in lines[:len(sizes)]] == sizes.tolist()
    assert lines[len(sizes) + 3] == b"3\t%d\t%d" % (hist[1][3], hist[2][3]) and lines[-1] == b"255\t%d" % hist[1][255]
    assert _tool().returncode == 1
