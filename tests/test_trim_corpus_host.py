"""The built inputs of the trim pass (tests/trim_corpus.py) held to the oracle alone: bloom_addr against orc_bf_positions, every cell of
every query_case that tests/test_gpu_trim.py uses against orc_bf_get, the shape of every streak_case under orc_max_streak and
orc_trim_decide on a saturated filter -- and, where oracle/_ref is built, the reference's own trim pass on the same bytes.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle
import trim_corpus as tc

SMALL, BIG, STREAK_KS = tc.SMALL, tc.BIG, tc.STREAK_KS
needs_ref = pytest.mark.skipif(not oracle.have_ref_ec(), reason="oracle/_ref/libbfcref_ec.so not built")


def _ref_windows(bf, k, stream, off, min_frac):
    seq, o = tc.unstream(stream, off)
    st, en = oracle.ref_trim(tc.bf_ptr(bf), k, seq, o, min_frac)
    return np.stack([st, en], axis=1)


@pytest.mark.parametrize("n_hashes", [1, 3, 4, 5, 12])
@pytest.mark.parametrize("n_shift", [20, 28, 35])
def test_bloom_addr_equals_oracle(n_shift, n_hashes):
    """block, positions and -- recomputed here from the oracle's positions -- the walk class of 10 000 hashes"""
    L = oracle.lib()
    hs = tc.hashes(33)[:10000]
    blk, pos, cls = tc.bloom_addr(hs, n_shift, n_hashes)
    buf = (C.c_int * 64)()
    for i, h in enumerate(hs):
        assert int(blk[i]) == L.orc_bf_positions(n_shift, n_hashes, int(h), buf) and pos[i].tolist() == buf[:n_hashes], i
        h1, h2 = int(h) >> (n_shift - 9) & 511, int(h) >> n_shift & 511
        if h2 & 31 == 0:
            want = tc.ADJ
        else:
            z, skips, got = h1, [], 0
            for step in range(64):
                if z < 8:
                    skips.append(step)
                else:
                    got += 1
                    if got == n_hashes:
                        break
                z = (z + h2) & 511
            want = tc.NONE if not skips else (tc.SKIP if n_hashes != 4 else tc.MULTI if len(skips) > 1 else tc.SKIP0 + skips[0])
        assert cls[i] == want, i
    assert set(cls.tolist()) == set(tc.walk_classes(n_hashes))


def test_hashes_are_the_oracles():
    """hash = ((y0 - y1 & m) ^ y1) << k | y0 from the trace's planes is orc_hash_from_y, at both word widths and at k = 63"""
    L = oracle.lib()
    for k in (21, 32, 33, 63):
        c = oracle.Counter(k, 20)
        tr = c.count(tc.sequence()[:2000], None, np.array([0, 2000], dtype=np.uint64), trace=True)
        c.close()
        hs = tc.hashes(k)[:len(tr)]
        assert np.array_equal(hs, tr[:, 0])
        for i in range(0, len(tr), 97):
            assert int(hs[i]) == L.orc_hash_from_y(k, (C.c_uint64 * 2)(int(tr[i, 1]), int(tr[i, 2])))


def _check_query_case(qc, bf):
    """every cell has at least 20 reads that the oracle answers as intended with just the bits of the cell's state set, on all four members of a group of lanes; the result word's
    64 bits all occur; the reads of 2k bases are mostly as intended and have windows inside the read"""
    cnt = tc.orc_gets(bf, tc.hashes(qc.k)[qc.kmer[qc.kmer >= 0]])
    one = np.flatnonzero(qc.kmer >= 0)
    as_intended = (cnt == qc.n_hashes) == (qc.want[one, 0] == 0)
    qpos = qc.off[one].astype(np.int64) + qc.k - 1   # where the read's one k-mer ends
    for c, (cl, state) in enumerate(qc.cells):
        n_set = dict(all=qc.n_hashes, none=0, first=1).get(state, qc.n_hashes - 1)   # "but j": exactly one bit clear
        sel = (qc.cell[one] == c) & as_intended & (cnt == n_set)
        assert sel.sum() >= 20, (tc.CLASS_NAMES[cl], state, int(sel.sum()))
        assert set((qpos[sel] & 3).tolist()) == {0, 1, 2, 3}, (tc.CLASS_NAMES[cl], state)
    assert set((qpos & 63).tolist()) == set(range(64))
    win = tc.orc_windows(bf, qc.k, qc.stream, qc.off, [0.5])[0]
    assert np.array_equal(win[one][as_intended], qc.want[one][as_intended])
    assert (win[one][~as_intended][:, 0] == np.where(cnt[~as_intended] == qc.n_hashes, 0, -1)).all()
    two = np.flatnonzero((qc.kmer < 0) & (np.diff(qc.off.astype(np.int64)) > 1))
    assert len(two) == 50 and (win[two] == qc.want[two]).all(axis=1).sum() >= 40
    inner = win[two][(win[two, 0] > 0) & (win[two, 1] < 2 * qc.k)]
    assert len(inner) >= 10 and len(set((inner[:, 1] - inner[:, 0]).tolist())) >= 4
    return win


@pytest.mark.parametrize("k,n_shift,n_hashes", SMALL)
def test_query_cases_small(k, n_shift, n_hashes):
    qc = tc.query_case(k, n_shift, n_hashes)
    bf = tc.OrcFilter(n_shift, n_hashes)
    tc.set_bits(bf.bytes(), qc.blk, qc.bit)
    _check_query_case(qc, bf)
    bf.close()


@pytest.mark.parametrize("n_hashes", [3, 4])
def test_query_cases_4gib(n_hashes):
    """one filter carries the bits of both k, as on the GPU"""
    cases = [tc.query_case(k, b, nh) for k, b, nh in BIG if nh == n_hashes]
    bf = tc.OrcFilter(35, n_hashes)
    for qc in cases:
        tc.set_bits(bf.bytes(), qc.blk, qc.bit)
    for qc in cases:
        _check_query_case(qc, bf)
    bf.close()


@pytest.fixture(scope="module")
def saturated():
    bf = tc.OrcFilter(20, 4)
    bf.bytes()[:] = 0xff
    yield bf
    bf.close()


@pytest.mark.parametrize("k", STREAK_KS)
def test_streak_case_shape(saturated, k):
    sc = tc.streak_case(k)
    T, L = sc.tags, sc.keep_len
    assert sorted({b.tiles for b in sc.batches}) == [1, 7, 8, 9, 17]
    assert [len(b.stream) for b in sc.batches] == sorted((len(b.stream) for b in sc.batches), reverse=True)
    offsets_seen, seam_end, seam_start, long_seen = set(), False, False, 0
    for b in sc.batches:
        w05, w09, w10 = tc.orc_windows(saturated, k, b.stream, b.off, tc.MIN_FRACS)
        lens = np.diff(b.off.astype(np.int64)) - 1
        for r in np.flatnonzero(b.src[:, 0] >= 0):
            s, i = int(b.src[r, 0]), int(b.src[r, 1])
            p0, name = int(b.off[r]), sc.names[i]
            if i == 0:
                assert p0 & 63 == s   # the copy stands at bit offset s
                offsets_seen.add(s)
            a05, a09, a10 = (tuple(int(v) for v in w[r]) for w in (w05, w09, w10))
            if a05[0] >= 0:   # the kept run's last hit is bit 63 of a result word / its first hit is bit 0
                seam_end |= (p0 + a05[1]) & 63 == 0
                seam_start |= (p0 + a05[0] + k - 1) & 63 == 0
            if name.startswith("run"):
                assert a05 == (1, int(name[3:]) + k), (name, s)
            elif name == "twin":
                assert a05 == (30 + k, 2 * (30 + k - 1) + 1)
            elif name == "twin64":
                assert a05 == (64 + k, 2 * (64 + k - 1) + 1)
            elif name == "first":
                assert a05 == (0, 100 + k - 1)
            elif name == "middle":
                assert a05 == (3 + k, 3 + k + 100 + k - 1)
            elif name == "last":
                assert a05[1] == lens[r] and a05[1] - a05[0] == 100 + k - 1
            elif name == "tail":
                assert a05 == (2, lens[r]) and a09 == a05
            elif name in ("len0", "len1", "lenk-1", "allN", "empty_a", "empty_b", "empty_c"):
                assert a05 == (-1, -1) and lens[r] == dict(len0=0, len1=1, allN=70).get(name, k - 1 if name == "lenk-1" else 0)
            elif name in ("lenk", "lenk+1", "lower", "mixed", "full"):
                assert a05 == a10 == (0, lens[r])
            elif name == "keep_eq":
                assert lens[r] == L and a05 == (-1, -1)          # (streak + k) / L = 0.5, not above
            elif name == "keep_above":
                assert lens[r] == L and a05 == (0, L // 2)   # one hit more: a window of streak + k - 1 bases
            elif name == "keep_09":
                assert lens[r] == L and a09 == (0, 9 * L // 10 - 1) and a10 == (-1, -1)   # 0.9 is above the float 0.9
            elif name == "notfull":
                assert a10 == (-1, -1) and a09 == (0, L - 1)
            elif name == "long":
                assert lens[r] == 20001 and a05 == (9000 + k - 1 + 130, 9000 + k - 1 + 130 + 10100 + k - 1)   # whole words of ones and of zeros on the way
                long_seen += 1
    assert offsets_seen == set(range(64)) and seam_end and seam_start and long_seen == 1
    assert set(T) == set(sc.names) and any(len(b.stream) % 64 for b in sc.batches if b.tiles > 1)


@needs_ref
@pytest.mark.parametrize("k,n_shift,n_hashes", SMALL + BIG)
def test_query_cases_vs_reference(k, n_shift, n_hashes):
    """the reference's own worker_ec on the built filter's bytes gives the oracle's windows"""
    qc = tc.query_case(k, n_shift, n_hashes)
    bf = tc.OrcFilter(n_shift, n_hashes)
    tc.set_bits(bf.bytes(), qc.blk, qc.bit)
    assert np.array_equal(_ref_windows(bf, k, qc.stream, qc.off, 0.5), tc.orc_windows(bf, k, qc.stream, qc.off, [0.5])[0])
    bf.close()


@needs_ref
@pytest.mark.parametrize("k", STREAK_KS)
def test_streak_case_vs_reference(saturated, k):
    for b in tc.streak_case(k).batches:
        for mf, w in zip(tc.MIN_FRACS, tc.orc_windows(saturated, k, b.stream, b.off, tc.MIN_FRACS)):
            assert np.array_equal(_ref_windows(saturated, k, b.stream, b.off, mf), w), (b.tiles, mf)
