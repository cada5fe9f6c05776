"""The trim pass of `bfc -1` on the GPU (bfcg_trim_*: run_query's six kernels and k_streak) on built filters and built reads
(tests/trim_corpus.py, held to the oracle in test_trim_corpus_host.py).  The filter is a HostBloom whose bytes the test writes itself, so
what each queried k-mer finds is decided bit by bit; the expectation is always the oracle's answer on those very bytes (orc_max_streak +
orc_trim_decide reading the HostBloom through its bfc_bf_t), never another GPU path.

Which kernel a test runs (run_query, bfcg_kernels.hip): k_query<*, COOP = false> below 4 GiB; k_query4 for four hashes at 4 GiB and more,
or anywhere with BFCG_QUERY4=1; k_query<*, COOP = true> at 4 GiB and more for any other number of hashes, or with BFCG_QUERY4=0.  The word
width follows k (<= 32 or above)."""
import ctypes as C

import numpy as np
import pytest

import oracle
import trim_corpus as tc

pytestmark = pytest.mark.gpu


def _set_q4(monkeypatch, q4):
    if q4 is None:
        monkeypatch.delenv("BFCG_QUERY4", raising=False)
    else:
        monkeypatch.setenv("BFCG_QUERY4", q4)


def _windows(tr, stream, off, min_frac, d_seq=None):
    st, en = tr.trim(stream, off, min_frac, d_seq=d_seq)
    return np.stack([st, en], axis=1)


def _query(gpu_lib, hb, qc):
    """one trim context over the filter, the case's stream as one batch of exactly the context's capacity: every read's window is the oracle's"""
    want = tc.orc_windows(hb, qc.k, qc.stream, qc.off, [0.5])[0]
    one = qc.kmer >= 0
    assert (want[one, 0] == 0).sum() > 100 and (want[one, 0] < 0).sum() > 200
    tr = gpu_lib.GpuTrimmer(qc.k, hb, max_pos=len(qc.stream), max_reads=len(qc.off) - 1)
    assert not tr.adopted
    got = _windows(tr, qc.stream, qc.off, 0.5)
    tr.close()
    bad = np.flatnonzero((got != want).any(axis=1))
    where = [(int(r), tc.CLASS_NAMES[qc.cells[qc.cell[r]][0]] + "/" + qc.cells[qc.cell[r]][1] if qc.cell[r] >= 0 else "2k", got[r].tolist(), want[r].tolist()) for r in bad[:8]]
    assert len(bad) == 0, (len(bad), where)


@pytest.mark.parametrize("k,n_shift,n_hashes,q4", [c + (None,) for c in tc.SMALL] + [c + ("1",) for c in tc.SMALL if c[2] == 4],
                         ids=lambda v: "unset" if v is None else str(v))
def test_bit_states_small_filter(gpu_lib, monkeypatch, k, n_shift, n_hashes, q4):
    """a 32 MiB filter holding, for 40 k-mers of every walk class, all, none, the first and all but one of their bits: k_query<*, false>, and
    for four hashes also k_query4 (BFCG_QUERY4=1), whose closed form of the positions must take a skipped candidate at every step and fall
    back on two, and whose four lanes each test one of the bits"""
    _set_q4(monkeypatch, q4)
    qc = tc.query_case(k, n_shift, n_hashes)
    hb = gpu_lib.HostBloom.init(n_shift, n_hashes)
    tc.set_bits(hb.bytes(), qc.blk, qc.bit)
    _query(gpu_lib, hb, qc)
    hb.close()


@pytest.fixture(scope="module")
def big_filter(gpu_lib):
    """the 4 GiB host filter for 3 or 4 hashes, carrying the bits of both k; one at a time (the tests below ask for 3 first, then 4)"""
    held = {}

    def get(n_hashes):
        if n_hashes not in held:
            for hb in held.values():
                hb.close()
            held.clear()
            hb = gpu_lib.HostBloom.init(35, n_hashes)
            for k, b, nh in tc.BIG:
                if nh == n_hashes:
                    qc = tc.query_case(k, b, nh)
                    tc.set_bits(hb.bytes(), qc.blk, qc.bit)
            held[n_hashes] = hb
        return held[n_hashes]

    yield get
    for hb in held.values():
        hb.close()


@pytest.mark.parametrize("k,n_hashes,q4", [(31, 3, None), (33, 3, None), (31, 4, None), (33, 4, None), (31, 4, "0"), (33, 4, "0")],
                         ids=lambda v: "unset" if v is None else str(v))
def test_bit_states_4gib_filter(gpu_lib, monkeypatch, big_filter, k, n_hashes, q4):
    """-b35, where run_query changes kernels: three hashes run k_query<*, true> -- four lanes load the four quarters of a block, each counts the
    positions in its own, two shuffles add the parts: a k-mer with exactly one bit clear tells a wrong quarter or source lane -- and four hashes
    k_query4 at its native size, or k_query<*, true> with BFCG_QUERY4=0.  The filter is uploaded, not adopted."""
    _set_q4(monkeypatch, q4)
    _query(gpu_lib, big_filter(n_hashes), tc.query_case(k, 35, n_hashes))


@pytest.fixture(scope="module")
def saturated(gpu_lib):
    """every byte 0xff: a position's hit bit is "a k-mer ends here\""""
    hb = gpu_lib.HostBloom.init(20, 4)
    hb.bytes()[:] = 0xff
    yield hb
    hb.close()


@pytest.mark.parametrize("k", tc.STREAK_KS)
def test_streaks(gpu_lib, saturated, k):
    """k_streak on built runs (trim_corpus.streak_case: every read at every bit offset of a result word; runs of 1..200 hits, equal runs,
    the keep rule at equality and at the float 0.9) -- batches of 17, 9, 8, 7 and 1 tiles as calls of their own on ONE context, longest
    first, so that a shorter batch finds the longer one's result words behind its own"""
    sc = tc.streak_case(k)
    tr = gpu_lib.GpuTrimmer(k, saturated, max_pos=len(sc.batches[0].stream), max_reads=max(len(b.off) - 1 for b in sc.batches))
    assert sorted({b.tiles for b in sc.batches}) == [1, 7, 8, 9, 17]
    for b in sc.batches:
        for mf, want in zip(tc.MIN_FRACS, tc.orc_windows(saturated, k, b.stream, b.off, tc.MIN_FRACS)):
            got = _windows(tr, b.stream, b.off, mf)
            bad = np.flatnonzero((got != want).any(axis=1))
            where = [(int(r), sc.names[b.src[r, 1]] if b.src[r, 0] >= 0 else "pad", int(b.src[r, 0]), got[r].tolist(), want[r].tolist()) for r in bad[:8]]
            assert len(bad) == 0, (b.tiles, mf, len(bad), where)
    tr.close()


def test_device_stream_unaligned(gpu_lib, saturated):
    """the stream given as d_seq at an address 0, 1, 5 and 15 bytes off a 16-byte boundary (the kernels' byte-wise load path): the windows
    of the host call, which are the oracle's"""
    k = 31
    b = next(b for b in tc.streak_case(k).batches if b.tiles == 9)
    want = tc.orc_windows(saturated, k, b.stream, b.off, [0.9])[0]
    tr = gpu_lib.GpuTrimmer(k, saturated, max_pos=len(b.stream), max_reads=len(b.off) - 1)
    host = _windows(tr, b.stream, b.off, 0.9)
    assert np.array_equal(host, want) and (want[:, 0] >= 0).sum() > 100
    g = gpu_lib.GpuCounter(k, 20, max_batch_pos=1 << 16)
    d = g.dev_alloc(len(b.stream) + 64)
    assert d % 16 == 0
    for o in (0, 1, 5, 15):
        g.h2d(d + o, b.stream)
        g.sync()
        assert np.array_equal(_windows(tr, None, b.off, 0.9, d_seq=d + o), host), o
    g.dev_free(d)
    g.close(); tr.close()


def test_capacity(gpu_lib, saturated):
    """a batch of more positions or more reads than the context was made for is refused with a message that names the capacity and writes
    nothing; the next batch of exactly the capacity is right; no reads: 0"""
    k = 31
    b = next(b for b in tc.streak_case(k).batches if b.tiles == 1)
    reads = [b.stream[int(b.off[r]):int(b.off[r + 1]) - 1].tobytes() for r in range(len(b.off) - 1)]
    n, n_pos = len(reads), len(b.stream)
    assert len(reads[-1]) > 1
    tr = gpu_lib.GpuTrimmer(k, saturated, max_pos=n_pos, max_reads=n)
    L = tr.L
    i32p = C.POINTER(C.c_int32)

    def call(stream, off, n_reads):
        st, en = np.full(n + 2, 77, dtype=np.int32), np.full(n + 2, 77, dtype=np.int32)
        rc = L.bfcg_trim_batch(tr.t, stream.ctypes.data, None, int(off[n_reads]), off.ctypes.data_as(oracle.u64p), n_reads, C.c_float(0.9),
                               st.ctypes.data_as(i32p), en.ctypes.data_as(i32p))
        return rc, st, en

    longer = tc.to_stream_off(reads[:-1] + [reads[-1] + b"A"])             # one position too many, as many reads
    more = tc.to_stream_off(reads[:-1] + [reads[-1][:-1], b""])            # one read too many, as many positions
    assert len(longer[0]) == n_pos + 1 and len(more[0]) == n_pos and len(more[1]) == n + 2
    for (s, o), nr in ((longer, n), (more, n + 1)):
        rc, st, en = call(s, o, nr)
        assert rc != 0 and b"capacity" in L.bfcg_last_error() and (st == 77).all() and (en == 77).all()
        with pytest.raises(gpu_lib.BfcGpuError, match="capacity"):
            tr.trim(s, o, 0.9)
    want = tc.orc_windows(saturated, k, b.stream, b.off, [0.9])[0]
    rc, st, en = call(np.ascontiguousarray(b.stream), np.ascontiguousarray(b.off), n)
    assert rc == 0 and np.array_equal(np.stack([st[:n], en[:n]], axis=1), want) and (st[n:] == 77).all() and (want[:, 0] >= 0).any()
    rc, st, en = call(np.ascontiguousarray(b.stream), np.zeros(1, dtype=np.uint64), 0)
    assert rc == 0 and (st == 77).all() and (en == 77).all()
    tr.close()


@pytest.mark.parametrize("k", [31, 63])
def test_kcov_same_tiles(gpu_lib, k, tmp_path):
    """the coverage pass (k_occ + k_cov, the same tiles and xcd_tile) on clean reads of 4000, 4096 and 9000 bases whose every k-mer the table
    holds with count 1, min_occ = 1, in batches of 9, 8, 7 and 1 tiles: every value is orc_kcov's, and lcov inside a read is the number of
    k-mers over a base, min(i + 1, k, len - i, len - k + 1)"""
    rng = np.random.default_rng(500 + k)
    reads = [tc.ACGT[rng.integers(0, 4, n)] for n in (4000, 4096, 9000)]
    off = np.zeros(4, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    c = oracle.Counter(k, 24)
    for _ in range(3):   # the filter takes the first sight of a k-mer, the table the second with count 0: the third leaves count 1
        c.count(np.concatenate(reads), None, off)
    want = []
    for r in reads:
        w = np.zeros(len(r), dtype=np.uint16)
        oracle.lib().orc_kcov(oracle.lib().orc_state_ch(c.st), 1, r.ctypes.data, len(r), w.ctypes.data)
        i, n = np.arange(len(r)), len(r)
        assert np.array_equal(w & 0x3f, np.minimum(np.minimum(i + 1, k), np.minimum(n - i, n - k + 1)))
        assert np.array_equal(w >> 12 & 1, i >= k - 1)
        want.append(np.append(w, np.uint16(0)))
    fn = str(tmp_path / "t.hash")
    assert c.dump(fn) == 0
    t = gpu_lib.HostTable.restore(fn)
    c.close()
    kc = gpu_lib.GpuKcov(t, max_pos=9 * tc.TILE)
    sep = np.array([10], dtype=np.uint8)
    for tiles, pick in ((9, [2, 2, 2, 1, 0]), (8, [2, 2, 2, 1]), (7, [2, 2, 1, 0]), (1, [0])):
        stream = np.concatenate([a for i in pick for a in (reads[i], sep)])
        assert (len(stream) + tc.TILE - 1) // tc.TILE == tiles
        got = kc.kcov(stream, 1)
        assert np.array_equal(got, np.concatenate([want[i] for i in pick])), tiles
    kc.close(); t.close()
