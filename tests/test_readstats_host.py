"""Per-read statistics of a count profile on the host (bfc_amd/csrc/bfc_host.c: bfcg_read_stats_host, the twin of bfcg_kmers_read_stats
and the reference side of every GPU comparison; bfcg_read_stats_format; the refusals both share) and the -t rule of
`python -m bfc_amd.readstats`.  The expected words come by a third route: the profile from stream_kmers and HostTable.occ_planes
(test_lookup_host.py), the eight words per read in plain numpy -- np.sort for the median, a Python loop for the run.  No GPU."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import oracle
from test_lookup_host import _g1_reads, stream_kmers

KS = [21, 32, 33, 51]
MIN_COVS = [1, 3, 255]
L1 = 149   # bases of the read with two equally long runs: odd, so that its middle base has as many k-mers on either side


def np_profile(table, stream, k):
    """bfcg_kmers_profile restated: -2 where no k-mer ends, else bfc_ch_kmer_occ of the k-mer ending there"""
    ends, y = stream_kmers(stream, k)
    return np.where(ends, table.occ_planes(y), -2).astype(np.int16)


def np_stats(prof, off, k, min_cov):
    """the eight words per read of a profile, as include/bfc_gpu.h defines them"""
    out = np.zeros((len(off) - 1, 8), dtype=np.int32)
    for r in range(len(off) - 1):
        v = prof[int(off[r]):int(off[r + 1]) - 1].astype(np.int64)
        defined, present = v != -2, v >= 0
        c = np.where(present, v & 0xff, 0)
        solid = present & (c >= min_cov)
        cs = np.sort(c[defined])
        n = len(cs)
        best, start, run = 0, -1, 0
        for p in range(len(v)):
            run = run + 1 if solid[p] else 0
            if run and run >= best:   # of equally long runs the last
                best, start = run, p - run + 1 - (k - 1)
        out[r, :4] = n, present.sum(), solid.sum(), np.uint32(cs.sum() & 0xffffffff).astype(np.int32)
        out[r, 4] = int(cs[0]) | int(cs[(n - 1) >> 1]) << 8 | int(cs[-1]) << 16 if n else 0
        out[r, 5:] = best, start, start + best + k - 1 if best else -1
    return out


@functools.lru_cache(maxsize=None)
def g1_table(gpu_lib, k):
    """g1's table at -b 24: the oracle's dump restored (as test_occ_host_vs_oracle does)"""
    seq, qual, off = _g1_reads()
    c = oracle.Counter(k, 24)
    c.count(seq, qual, off)
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "g1.hash")
        assert c.dump(fn) == 0
        t = gpu_lib.HostTable.restore(fn)
    c.close()
    return t


def to_stream_off(reads):
    """a list of reads (bytes) -> the batch stream (a separator behind each) and off[n + 1]"""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) + 1 for s in reads])
    return np.frombuffer(b"".join(s + b"\n" for s in reads), dtype=np.uint8), off


def damaged(read, d):
    """the read with base d replaced by the next one of ACGT"""
    return read[:d] + b"CGTA"[b"ACGT".index(read[d:d + 1].upper())].to_bytes(1, "little") + read[d + 1:]


@functools.lru_cache(maxsize=None)
def hand_reads(gpu_lib, k):
    """(reads, the index of the read with two equally long runs): the hand-made stream of the issue.  The clean read behind that one is
    the first of g1's reads whose first L1 bases have every k-mer in the table, and stay in two runs of present k-mers when the middle
    base is damaged (found with the numpy profile, on the host)."""
    seq, qual, off = _g1_reads()
    L = int(off[1])
    read = lambda r: seq[r * L:(r + 1) * L].tobytes()  # noqa: E731
    cat = lambda r0, n: b"".join(read(r) for r in range(r0, r0 + (n + L - 1) // L))[:n]  # noqa: E731
    t = g1_table(gpu_lib, k)
    reads = [b"", read(0)[:1], read(1)[:k - 1], read(2)[:k], read(3)[:k + 1]]
    reads += [cat(10 + 2 * i, n + k - 1) for i, n in enumerate((63, 64, 65, 127, 128, 129))]   # this many k-mers
    reads.append(cat(100, 20001))
    r = read(30)
    reads += [b"N" + r[1:], r[:75] + b"N" + r[76:], r[:-1] + b"N", b"N" * 70, read(31).lower()]
    rng = np.random.default_rng(5)
    reads.append(bytes(b"ACGT"[c] for c in rng.integers(0, 4, 100)))   # k-mers the table does not hold
    d, twin = (L1 - 1) // 2, None
    for i in range(300, 700):
        dmg = damaged(read(i)[:L1], d)
        s, o = to_stream_off([read(i)[:L1], dmg])
        p = np_profile(t, s, k)
        if (p[k - 1:L1] >= 0).all() and (p[L1 + 1 + d:L1 + 1 + d + k] < 0).all() and (p[L1 + 1 + k - 1:L1 + 1 + d] >= 0).all() and (p[L1 + 1 + d + k:-1] >= 0).all():
            twin = len(reads)
            reads += [read(i)[:L1], dmg]
            break
    assert twin is not None, "no read of g1 has all its %d-mers in the table" % k
    reads += [damaged(damaged(read(r), 40), 120) for r in range(40, 44)] + [read(r) for r in range(44, 60)]
    return reads, twin + 1


@functools.lru_cache(maxsize=None)
def hand_case(gpu_lib, k):
    """(stream, off, the numpy profile, the index of the read with two equally long runs)"""
    reads, twin = hand_reads(gpu_lib, k)
    stream, off = to_stream_off(reads)
    prof = np_profile(g1_table(gpu_lib, k), stream, k)
    for a in (stream, off, prof):
        a.flags.writeable = False
    return stream, off, prof, twin


@pytest.mark.parametrize("k", KS)
def test_host_twin_equals_numpy(gpu_lib, k):
    """bfcg_read_stats_host == the numpy route, word for word, for min_cov 1, 3, 255; the read with two equally long runs of present
    k-mers reports the later one at min_cov = 1; and the input is not degenerate"""
    stream, off, prof, twin = hand_case(gpu_lib, k)
    t = g1_table(gpu_lib, k)
    lens = np.diff(off.astype(np.int64)) - 1
    assert {0, 1, k - 1, k, k + 1, 20001}.issubset(set(lens.tolist()))
    for min_cov in MIN_COVS:
        want = np_stats(prof, off, k, min_cov)
        got = t.read_stats(stream, off, min_cov)
        assert got.dtype == np.int32 and got.shape == (len(off) - 1, 8)
        assert np.array_equal(got, want), (min_cov, np.flatnonzero((got != want).any(axis=1))[:10])
        n_kmers, n_present, n_solid, streak = want[:, 0], want[:, 1], want[:, 2], want[:, 5]
        assert {63, 64, 65, 127, 128, 129}.issubset(set(n_kmers.tolist()))
        assert ((n_kmers > 0) & (n_present == 0)).any() and (n_kmers == 0).sum() >= 4
        if min_cov == 1:
            d = (L1 - 1) // 2
            assert tuple(want[twin - 1, [0, 2, 5, 6, 7]]) == (L1 - k + 1, L1 - k + 1, L1 - k + 1, 0, L1)          # the clean read: one run
            assert tuple(want[twin, [2, 5, 6, 7]]) == (L1 - 2 * k + 1, d - k + 1, d + 1, L1) and d - k + 1 == L1 - d - k  # the LATER of two equal runs
        if min_cov < 255:
            assert ((0 < n_solid) & (n_solid < n_kmers)).any() and ((streak == n_kmers) & (n_kmers > 0)).any()
            assert (want[:, 4] >> 8 & 0xff != want[:, 4] & 0xff).any() and (want[:, 4] >> 16 != want[:, 4] >> 8 & 0xff).any()   # min < median < max somewhere
        else:
            assert (n_solid <= n_present).all()


def test_refusals(gpu_lib):
    """min_cov outside [1, 255], offsets that do not ascend, off[n_reads] != n_pos and a read of 2^24 positions are refused with a
    message that names the read, and nothing is written; n_reads = 0 and n_pos = 0 return 0 and write nothing"""
    L = gpu_lib._lib.load()
    t = g1_table(gpu_lib, 21)
    stream, off = to_stream_off([b"ACGT" * 10, b"ACGTT" * 9, b"A" * 30])
    out = np.full((3, 8), 77, dtype=np.int32)
    call = lambda s, n_pos, o, n, mc: L.bfcg_read_stats_host(t.ptr, s.ctypes.data, n_pos, o.ctypes.data, n, mc, out.ctypes.data)  # noqa: E731
    for mc in (0, -1, 256):
        assert call(stream, len(stream), off, 3, mc) == -1 and b"min_cov" in L.bfcg_last_error() and b"[1, 255]" in L.bfcg_last_error()
    bad = off.copy(); bad[2] = bad[1]
    assert call(stream, len(stream), bad, 3, 3) == -1 and b"read 1:" in L.bfcg_last_error() and b"ascend" in L.bfcg_last_error()
    bad = off.copy(); bad[1], bad[2] = off[2], off[1]
    assert call(stream, len(stream), bad, 3, 3) == -1 and b"read 1:" in L.bfcg_last_error()
    assert call(stream, len(stream) - 1, off, 3, 3) == -1 and b"read 2, the last" in L.bfcg_last_error()
    assert call(stream, len(stream), off, 2, 3) == -1 and b"read 1, the last" in L.bfcg_last_error()
    big = np.array([0, 41, 41 + (1 << 24) + 1], dtype=np.uint64)   # refused before a byte of the stream is read
    assert call(stream, int(big[2]), big, 2, 3) == -1 and b"read 1 has 16777216 positions" in L.bfcg_last_error()
    assert (out == 77).all()
    assert call(stream, len(stream), off, 0, 3) == 0 and call(stream, 0, off, 3, 3) == 0 and (out == 77).all()
    with pytest.raises(gpu_lib.BfcGpuError, match="min_cov 0 is outside"):
        t.read_stats(stream, off, 0)
    assert call(stream, len(stream), off, 3, 3) == 0 and (out[:, 0] == [40 - 20, 45 - 20, 30 - 20]).all()


def test_format(gpu_lib):
    """bfcg_read_stats_format on a hand-written array: ten tab-separated fields, word 4 split into min, median, max"""
    st = np.array([[130, 120, 100, 1234, 0 | 9 << 8 | 255 << 16, 57, 3, 3 + 57 + 20, ],
                   [0, 0, 0, 0, 0, 0, -1, -1],
                   [(1 << 24) - 1, 16777215, 16777215, -16777471, 255 | 255 << 8 | 255 << 16, 16777215, 0, 16777215 + 62]], dtype=np.int32)
    want = b"130\t120\t100\t1234\t0\t9\t255\t57\t3\t80\n0\t0\t0\t0\t0\t0\t0\t0\t-1\t-1\n16777215\t16777215\t16777215\t-16777471\t255\t255\t255\t16777215\t0\t16777277\n"
    assert gpu_lib.format_read_stats(st) == want and max(len(ln) for ln in want.split(b"\n")) < 110
    buf = C.create_string_buffer(16)
    assert gpu_lib._lib.load().bfcg_read_stats_format(st.ctypes.data, 0, buf) == 0


def test_trim_rule():
    """the tool's -t rule on hand-written words: correct.c:557 -- streak > 0 and (streak + k) / l_seq > min_frac, min_frac a float"""
    from bfc_amd.readstats import keep
    k = 33
    w = lambda streak, start: np.array([0, 0, 0, 0, 0, streak, start, start + streak + k - 1 if streak else -1], dtype=np.int32)  # noqa: E731
    assert keep(w(0, -1), k, 150, 0.9) is None
    assert keep(w(118, 0), k, 150, 0.9) == (0, 150)            # 151 / 150
    assert keep(w(103, 5), k, 150, 0.9) == (5, 140)            # 136 / 150 = 0.9067
    assert keep(w(102, 5), k, 150, 0.9) == (5, 139)            # 135 / 150 = 0.9 is above the float 0.9 = 0.89999997...
    assert keep(w(101, 5), k, 150, 0.9) is None                # 134 / 150
    assert keep(w(1, 0), k, 33, 0.9) == (0, 33) and keep(w(1, 0), k, 40, 0.9) is None
    assert keep(w(57, 10), k, 100, 0.5) == (10, 99) and keep(w(17, 10), k, 100, 0.5) is None   # 50 / 100 is not above 0.5
