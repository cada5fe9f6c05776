"""The decode of a count-table slot back to its k-mer (bfc_amd/csrc/bfcg_kdec.h), through its host instance bfcg_kmer_decode_host:
round trip against the oracle's forward functions, and line for line against the reference's hash2cnt where oracle/_ref has it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle

HASH2CNT = os.path.join(oracle.REF_DIR, "hash2cnt")
u64p = C.POINTER(C.c_uint64)


def _forward(k, bases):
    """the oracle's hash (Y0, Y1) of a k-mer given as base codes, 5' to 3'"""
    L = oracle.lib()
    p, y = (C.c_uint64 * 4)(), (C.c_uint64 * 2)()
    for c in bases:
        L.orc_kmer_push(k, p, int(c))
    L.orc_kmer_hash(k, p, y)
    return int(y[0]), int(y[1])


def decode_slots(L, k, l_pre, sizes, slots):
    """bfcg_kmer_decode_host on every slot of a table in L1 form -> (y (n, 2) u64, cnt_high u16)"""
    sub = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    y = np.zeros((len(slots), 2), dtype=np.uint64)
    out = (C.c_uint64 * 2)()
    for i in range(len(slots)):
        assert L.bfcg_kmer_decode_host(k, l_pre, int(sub[i]), int(slots[i]), out) == 0
        y[i] = out[0], out[1]
    return y, (slots & np.uint64(0x3fff)).astype(np.uint16)


def format_lines(L, k, y, cnt_high):
    buf = C.create_string_buffer(max(1, len(cnt_high) * (k + 8)))
    n = L.bfcg_kmers_format(k, np.ascontiguousarray(y).ctypes.data, np.ascontiguousarray(cnt_high).ctypes.data, len(cnt_high), buf)
    return buf.raw[:n].splitlines()


@pytest.mark.parametrize("l_pre_req", [20, 10])
@pytest.mark.parametrize("k", [21, 31, 32, 33, 35, 37])
def test_decode_round_trip(gpu_lib, k, l_pre_req):
    """random k-mers -> oracle hash -> (sub-table, key) -> decode -> text -> oracle hash again: the same hash, and the text is the k-mer
    or its reverse complement.  k = 32: the largest k of the first key form (a request of l_pre 10 is clamped to 14 there);
    k = 37: the last lossless k, l_pre 24."""
    from bfc_amd import _lib
    L, O = _lib.load(), oracle.lib()
    l_pre = O.orc_ch_clamp_lpre(k, l_pre_req)
    assert l_pre == min(max(l_pre_req, 2 * k - 50), 24) and (k, l_pre_req, l_pre) not in [(32, 10, 10), (37, 20, 20)]  # htab.c:24-25
    rng = np.random.default_rng(k)
    buf = C.create_string_buffer(k + 1)
    for it in range(200):
        bases = rng.integers(0, 4, k)
        Y = _forward(k, bases)
        key = C.c_uint64()
        sub = O.orc_ch_subkey(k, l_pre, (C.c_uint64 * 2)(*Y), C.byref(key))
        slot = (key.value & ~0x3fff) | int(rng.integers(0, 64)) << 8 | int(rng.integers(1, 256))
        y = (C.c_uint64 * 2)()
        assert L.bfcg_kmer_decode_host(k, l_pre, sub, slot, y) == 0
        L.bfcg_kmer_2str(k, y, buf)
        s = buf.value
        assert len(s) == k
        fw = bytes(b"ACGT"[c] for c in bases)
        rc = bytes(b"TGCA"[c] for c in bases[::-1])
        assert s in (fw, rc)
        assert _forward(k, [b"ACGT".index(c) for c in s]) == Y


@pytest.mark.parametrize("k", [38, 39, 51, 63])
def test_decode_refuses_lossy_keys(gpu_lib, k):
    from bfc_amd import _lib
    y = (C.c_uint64 * 2)()
    assert _lib.load().bfcg_kmer_decode_host(k, 24, 5, (12345 << 14) | 3, y) == -1


@pytest.mark.skipif(not os.path.exists(HASH2CNT), reason="oracle/_ref/hash2cnt not built (needs the reference's sources)")
@pytest.mark.parametrize("k", [21, 33, 37])
def test_host_decode_vs_reference_hash2cnt(gpu_lib, g1, tmp_path, k):
    """g1 counted by the oracle at -b 24, dumped: every slot decoded and formatted on the host, sorted, equals `hash2cnt dump | sort`"""
    from bfc_amd import _lib
    L = _lib.load()
    rs, (seq, qual, off) = g1
    c = oracle.Counter(k, 24)
    c.count(seq, qual, off)
    fn = str(tmp_path / "t.hash")
    c.dump(fn)
    c.close()
    kk, l_pre, sizes, slots = oracle.parse_dump(fn)
    assert kk == k and len(slots) > 50000
    y, ch = decode_slots(L, k, l_pre, sizes, slots)
    want = subprocess.run([HASH2CNT, fn], capture_output=True, check=True).stdout.splitlines()
    assert sorted(format_lines(L, k, y, ch)) == sorted(want)
