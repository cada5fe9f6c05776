"""The host side of the lookups by k-mer (bfc_amd/csrc/bfc_host.c; the kernels are bfcg_lookup.hip's): text <-> planes, the line grammar
of a query file, and bfcg_kmer_occ_host -- the reference side of every GPU comparison -- against the oracle's table and, where
oracle/_ref has it, the reference's own bfc_ch_kmer_occ.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle

u64p = C.POINTER(C.c_uint64)
CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = CODE[_c | 0x20] = _i


def planes_of_codes(codes, k):
    """base codes (n, k), 5' to 3' -> listing-style planes (n, 2) u64: bit l = the base l from the 3' end, low / high code bit"""
    codes = np.asarray(codes).reshape(-1, k)
    y = np.zeros((len(codes), 2), dtype=np.uint64)
    for l in range(k):
        c = codes[:, k - 1 - l].astype(np.uint64)
        y[:, 0] |= (c & np.uint64(1)) << np.uint64(l)
        y[:, 1] |= (c >> np.uint64(1)) << np.uint64(l)
    return y


def revcomp_planes(y, k):
    """the planes of the reverse complements: every plane complemented and bit-reversed over k"""
    y = np.asarray(y, dtype=np.uint64).reshape(-1, 2)
    r = np.zeros_like(y)
    for l in range(k):
        r |= ((y >> np.uint64(l)) & np.uint64(1)) << np.uint64(k - 1 - l)
    return ~r & np.uint64((1 << k) - 1)


def stream_kmers(stream, k):
    """(ends, y): ends[p] = a k-mer ends at position p of a batch stream (k bytes of ACGTacgt in a row), y[p] = its planes (else 0)"""
    c = CODE[np.asarray(stream, dtype=np.uint8)]
    ok = c < 4
    run, n = np.zeros(len(c), dtype=np.int64), 0
    for p in range(len(c)):
        n = n + 1 if ok[p] else 0
        run[p] = n
    ends = run >= k
    y = np.zeros((len(c), 2), dtype=np.uint64)
    cc = np.where(ok, c, 0).astype(np.uint64)
    for l in range(k):
        y[l:, 0] |= (cc[:len(c) - l] & np.uint64(1)) << np.uint64(l)
        y[l:, 1] |= (cc[:len(c) - l] >> np.uint64(1)) << np.uint64(l)
    y[~ends] = 0
    return ends, y


def _str(L, k, y):
    buf = C.create_string_buffer(k + 1)
    L.bfcg_kmer_2str(k, (C.c_uint64 * 2)(int(y[0]), int(y[1])), buf)
    return buf.value


@pytest.mark.parametrize("k", [21, 32, 33, 37, 51, 63])
def test_from_str_inverts_2str(gpu_lib, k):
    """bfcg_kmer_from_str o bfcg_kmer_2str is the identity on random k-mers (lower case too); lengths k +- 1, an N and the empty string
    are refused"""
    L = gpu_lib._lib.load()
    rng = np.random.default_rng(k)
    codes = rng.integers(0, 4, (300, k))
    ys = planes_of_codes(codes, k)
    out = (C.c_uint64 * 2)()
    for i in range(len(ys)):
        s = _str(L, k, ys[i])
        assert s == bytes(b"ACGT"[c] for c in codes[i])
        assert L.bfcg_kmer_from_str(k, s if i & 1 else s.lower(), out) == 0 and (out[0], out[1]) == (int(ys[i, 0]), int(ys[i, 1]))
    s = _str(L, k, ys[0])
    out[0] = out[1] = 77
    for bad in (s[:-1], s + b"A", s[:k // 2] + b"N" + s[k // 2 + 1:], b"", s[:-1] + b" "):
        assert L.bfcg_kmer_from_str(k, bad, out) == -1
    assert (out[0], out[1]) == (77, 77)


def _parse(L, k, text, cap):
    y, bad = np.full((cap + 1, 2), 0xA5, dtype=np.uint64), C.c_uint64(99)
    n = L.bfcg_kmers_parse(k, text, len(text), y.ctypes.data, cap, C.byref(bad))
    assert np.all(y[n:] == 0xA5)   # nothing written beyond the k-mers returned
    return int(n), int(bad.value), y[:n]


def test_parse_line_grammar(gpu_lib):
    """bfcg_kmers_parse: '>' lines and empty lines skipped, the first field up to tab / space / CR taken, CRLF, a last line without a
    newline, cap, and the 1-based number of the first malformed line"""
    L = gpu_lib._lib.load()
    k = 5
    a, b, c = b"ACGTA", b"ttgca", b"GGGGC"
    want = planes_of_codes([[CODE[x] for x in s] for s in (a, b, c)], k)
    text = b">header ACGTA\n\n" + a + b"\t12\t3\n\r\n" + b + b" trailing words\r\n>another\n" + c
    n, bad, y = _parse(L, k, text, 10)
    assert (n, bad) == (3, 0) and np.array_equal(y, want)
    assert _parse(L, k, text + b"\n", 10)[0] == 3 and _parse(L, k, text + b"\r\n\n", 10)[0] == 3
    for cap in (0, 1, 2):                      # stops at cap, before it looks at the next line
        n, bad, y = _parse(L, k, text + b"\nACGTN\n", cap)
        assert (n, bad) == (cap, 0) and np.array_equal(y, want[:cap])
    n, bad, y = _parse(L, k, text + b"\nACGTN\n" + a + b"\n", 10)   # line 8: an N
    assert (n, bad) == (3, 8) and np.array_equal(y, want)
    assert _parse(L, k, a + b"\n" + a + b"C\n", 10)[:2] == (1, 2)    # k + 1 bases
    assert _parse(L, k, a[:-1] + b"\n", 10)[:2] == (0, 1)            # k - 1 bases
    assert _parse(L, k, b"", 10)[:2] == (0, 0) and _parse(L, k, b"\n\n>x\n", 10)[:2] == (0, 0)
    # the answers' text walks the same lines
    occ = np.array([5 << 8 | 200, -1, 63 << 8 | 255], dtype=np.int16)
    buf = C.create_string_buffer(len(text) + 8 * 3 + 16)
    m = L.bfcg_lookup_format(text, len(text), occ.ctypes.data, 3, buf)
    assert buf.raw[:m] == a + b"\t200\t5\n" + b + b"\t0\t0\n" + c + b"\t255\t63\n"
    prof = np.array([-2, -2, 7, -1, 3 << 8 | 12, -2], dtype=np.int16)
    m = L.bfcg_profile_format(prof.ctypes.data, len(prof), buf)
    assert buf.raw[:m] == b". . 7 0 12 .\n"


@functools.lru_cache(maxsize=None)
def _g1_reads():
    from bfc_amd import gen
    return gen.fixture("g1").reads()


@pytest.mark.parametrize("k", [21, 32, 33, 51])
def test_occ_host_vs_oracle(gpu_lib, tmp_path, k):
    """Every k-mer ending at every position of g1's first 200 reads, on both strands: bfcg_kmer_occ_host on our restore of the oracle's
    dump equals the oracle's bfc_ch_get on the oracle's own hash (the four rolled planes, kmer.h:79-88) of that strand's k-mer -- for
    odd k one hash for both strands; for even k the strand rule reads two different bases and the two strands may hash apart, which the
    twin must reproduce.  Where the reference is built, its bfc_ch_kmer_occ on its restore of the same dump is held against both."""
    L, O = gpu_lib._lib.load(), oracle.lib()
    seq, qual, off = _g1_reads()
    c = oracle.Counter(k, 24)
    c.count(seq, qual, off)
    fn = str(tmp_path / "g1.hash")
    assert c.dump(fn) == 0
    t = gpu_lib.HostTable.restore(fn)
    R = rt = None
    if oracle.have_ref():
        R = oracle.ref()
        R.bfc_ch_kmer_occ.argtypes = [C.c_void_p, u64p]
        rt = R.bfc_ch_restore(fn.encode())
        assert rt
    ys, want, apart = [], [], 0
    x, y, xr = (C.c_uint64 * 4)(), (C.c_uint64 * 2)(), (C.c_uint64 * 4)()
    for r in range(200):
        codes = CODE[seq[int(off[r]):int(off[r + 1])]]
        n = 0
        for i in range(4):
            x[i] = 0
        for p, cd in enumerate(codes):
            if cd > 3:
                n = 0
                for i in range(4):
                    x[i] = 0
                continue
            O.orc_kmer_push(k, x, int(cd))
            n += 1
            if n < k:
                continue
            xr[0], xr[1], xr[2], xr[3] = x[2], x[3], x[0], x[1]   # the reverse complement's planes are the same four, swapped
            O.orc_kmer_hash(k, x, y)
            fw = (int(y[0]), int(y[1]))
            O.orc_kmer_hash(k, xr, y)
            rv = (int(y[0]), int(y[1]))
            assert k % 2 == 0 or fw == rv
            apart += fw != rv
            w = [c.table_get(*fw), c.table_get(*rv)]
            if R:
                assert [R.bfc_ch_kmer_occ(rt, x), R.bfc_ch_kmer_occ(rt, xr)] == w
            want += w
            ys.append(codes[p - k + 1:p + 1])
    yf = planes_of_codes(np.array(ys), k)
    both = np.stack([yf, revcomp_planes(yf, k)], axis=1).reshape(-1, 2)
    got = t.occ_planes(both)
    want = np.array(want, dtype=np.int16)
    assert len(want) > 200 * 2 * (150 - k) * 0.9 and np.array_equal(got, want)
    assert (want >= 0).any() and (want == -1).any() and (k % 2 == 1) == (apart == 0)   # (the table holds the k-mers seen twice)
    one = (C.c_uint64 * 2)(int(both[5, 0]) | 1 << 63, int(both[5, 1]) | 1 << 63)   # bits at and above k are ignored
    assert L.bfcg_kmer_occ_host(t.ptr, one) == want[5]
    if R:
        R.bfc_ch_destroy(rt)
    t.close(); c.close()
