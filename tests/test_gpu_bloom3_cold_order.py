"""k_bloom3<.., COLD>'s ordering of a region's list by (block, file index) -- grouped in place, ranked from contiguous reads, moved to its
ranks, walked by returning ORs -- against the CPU oracle, exactly as tests/test_gpu_parity.py::test_vs_oracle_full compares: filter bytes,
per-k-mer seen flags (debug_seen), the counters and the sorted table export.  Bit-exact is the bar.

Which kernel a shape takes (bfcg_ctx.hip).  -b26 / -b24 give 2^9 / 2^7 regions of 256 blocks (R = 8).  k_bloom3 needs `b3_ok` (line 208):
region-owned table segments (`seg_ok`, lines 200-204: a k-mer's identity inside its region, 2k - (min(k, b - 9) - R) bits, must fit the 50 key
bits of a slot), four hashes, 12-byte records (2k - rec_n + 33 <= 96 bits) and bloom3_geometry_ok.
  * k = 27: 54 - 9 = 45 bits at -b26, 54 - 7 = 47 at -b24; 87 record bits; the bloom address is a bit field of the record (k >= b - 9, b + 9 <= 2k):
    `b3_ok` holds.  bfcg_create then sets `list_cap_c` (lines 249-256) unless BFCG_B3_COLD=0, a fresh context is `cold`, and warm_tables()
    (lines 494-495) gives every batch of a cold context `b3_cold = 1`: k_bloom3<512, 4, true>.  A context stays cold while fewer than 40 % of a
    batch's k-mers were seen (line 685).  THESE are the cases that run the new ordering.
  * k = 33, the shapes as first written down for this file: 66 - 9 = 57 > 50 bits, so `seg_ok` fails, `b3_ok` with it, and every batch takes
    k_bloom whatever BFCG_B3_COLD says.  They stay as a check that the same inputs give the oracle's answers on the path beside k_bloom3.
With BFCG_B3_COLD=0 the k = 27 batches take the first-setter protocol (k_bloom3 warm / k_bloom): the answers must be the same either way."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

def _shape(name, g1, g42):
    """(seq, qual, off, bf_shift) of a named shape; reads of equal length, so `off` is a plain ramp."""
    if name in ("full", "overflow"):  # 8 000 reads of g42 (g1 holds 6 600): ~950 K k-mers, 1 860 per region at -b26, 7 400 at -b24
        rs, (seq, qual, off) = g42
        n = 8000
        return seq[:n * rs.L], qual[:n * rs.L], off[:n + 1], 26 if name == "full" else 24
    rs, (seq, qual, off) = g1
    L = rs.L
    if name == "copies":  # all of g1, a 10x coverage: most k-mers of a block are copies of an earlier one -- the walk's `seen` branch
        return seq, qual, off, 26
    if name == "thin":  # 300 reads: ~70 k-mers per region, lists shorter than a wave, most blocks empty
        n = 300
        return seq[:n * L], qual[:n * L], off[:n + 1], 26
    assert name == "long_block"  # 3 000 copies of one read among 3 000 others: each of its k-mers' blocks holds its copies one after the other
    n = 3000
    s = np.empty((2 * n, L), dtype=seq.dtype); q = np.empty((2 * n, L), dtype=qual.dtype)
    s[0::2] = seq[:n * L].reshape(n, L); q[0::2] = qual[:n * L].reshape(n, L)
    s[1::2] = seq[7 * L:8 * L]; q[1::2] = qual[7 * L:8 * L]
    return s.reshape(-1), q.reshape(-1), np.arange(2 * n + 1, dtype=off.dtype) * L, 26


_ORACLE = {}


def _oracle(name, k, shape):
    """The oracle's answers for a shape, computed once and shared by the shape's cases."""
    if (name, k) not in _ORACLE:
        seq, qual, off, b = shape
        oc = oracle.Counter(k, b)
        tr = oc.count(seq, qual, off, trace=True)
        ost = oc.stats()
        _ORACLE[name, k] = dict(bloom=oc.bloom_bytes().copy(), seen=((tr[:, 3] >> 1) & 1 == 1).copy(),
                             stats=(ost["n_kmers"], ost["n_high"], ost["n_seen"]), table=tuple(a.copy() for a in oc.export()))
    return _ORACLE[name, k]


def _check(gpu_lib, name, k, shape, n_batches):
    seq, qual, off, b = shape
    want = _oracle(name, k, shape)
    n_reads = len(off) - 1
    L = int(off[1] - off[0])
    per = (n_reads + n_batches - 1) // n_batches
    g = gpu_lib.GpuCounter(k, b, max_batch_pos=per * (L + 1) + 64, debug_seen=True)
    seen = []
    for i in range(0, n_reads, per):  # (the flags are per batch: read after each one, in file order)
        j = min(n_reads, i + per)
        o = off[i:j + 1] - off[i]
        g.count_host(gpu_lib.to_stream(seq[int(off[i]):int(off[j])], o), gpu_lib.to_stream(qual[int(off[i]):int(off[j])], o))
        fl = g.seen_flags(int(off[j] - off[i]) + (j - i))
        seen.append(fl[fl > 0] == 2)
    assert np.array_equal(g.bloom_bytes(), want["bloom"]), "filter bytes differ"
    assert np.array_equal(np.concatenate(seen), want["seen"]), "seen flags differ from the sequential semantics"
    st = g.stats()
    assert (st["n_kmers"], st["n_high"], st["n_seen"]) == want["stats"]
    sizes, slots = g.export_table().export_sorted()
    assert np.array_equal(sizes, want["table"][0]) and np.array_equal(slots, want["table"][1])
    g.close()


_MODES = pytest.mark.parametrize("cold_env", [None, "0"], ids=["default", "B3_COLD=0"])
_BATCHES = pytest.mark.parametrize("n_batches", [1, 3])
_KS = pytest.mark.parametrize("k", [27, 33])


def _env(monkeypatch, cold_env):
    if cold_env is None:
        monkeypatch.delenv("BFCG_B3_COLD", raising=False)
    else:
        monkeypatch.setenv("BFCG_B3_COLD", cold_env)


@_MODES
@_BATCHES
@_KS
def test_nearly_full_lists(gpu_lib, g1, g42, monkeypatch, cold_env, n_batches, k):
    """(a) -b26 (512 regions of 256 blocks), 8 000 reads: ~1 900 listed k-mers per region in one batch, seven per block -- under the cold
    list's 2 879 entries, so every region is grouped, ranked and walked (no overflow), with several of a thread's eight positions in use.
    k = 27 is cold by bfcg_ctx.hip:200-208 (45 identity bits: seg_ok, b3_ok), 249-256 (list_cap_c is set) and 494-495 (a fresh context is
    cold; in three batches the reads of a 1.2x sample hardly repeat, so it stays cold).  k = 33 takes k_bloom (57 identity bits)."""
    _env(monkeypatch, cold_env)
    _check(gpu_lib, "full", k, _shape("full", g1, g42), n_batches)


@_MODES
@_BATCHES
@_KS
def test_blocks_of_copies(gpu_lib, g1, g42, monkeypatch, cold_env, n_batches, k):
    """(a') the same filter with all of g1 (10x coverage): ~1 530 listed k-mers per region of which most repeat an earlier k-mer of the same
    block -- the walk's `seen` verdict, the emit by permuted record index, and ranks among equal addresses.  k = 27 is cold as in (a) for the
    first batch (bfcg_ctx.hip:494-495); a later third of a 10x sample finds more than 40 % of its k-mers seen (line 685), so the batch after
    it takes the warm kernel: the answers cover the hand-over between the two.  k = 33 takes k_bloom."""
    _env(monkeypatch, cold_env)
    _check(gpu_lib, "copies", k, _shape("copies", g1, g42), n_batches)


@_MODES
@_BATCHES
@_KS
def test_thin_lists(gpu_lib, g1, g42, monkeypatch, cold_env, n_batches, k):
    """(b) the same filter with 300 reads: ~70 k-mers per region (23 in three batches) -- a list shorter than a wave and no multiple of 512,
    most of a thread's eight positions unused (they must read in bounds and count nothing), most blocks empty.  k = 27 is cold as in (a):
    bfcg_ctx.hip:200-208 and 249-256 set list_cap_c for this geometry, 494-495 pick it for a context whose batches bring nearly only new
    k-mers.  k = 33 takes k_bloom."""
    _env(monkeypatch, cold_env)
    _check(gpu_lib, "thin", k, _shape("thin", g1, g42), n_batches)


@_MODES
@_BATCHES
@_KS
def test_overflowing_lists(gpu_lib, g1, g42, monkeypatch, cold_env, n_batches, k):
    """(c) -b24 (128 regions) with the 8 000 reads: ~7 500 k-mers per region in one batch, ~2 500 in three -- in one batch every region's
    list overflows (`ovf_list`) and takes the HBM-pool path, in three most fit and some do not: both in one launch.  k = 27 takes the cold
    kernel as in (a) (bfcg_ctx.hip:200-208: 54 - 7 = 47 identity bits, 87 record bits; 249-256; 494-495); debug_seen keeps each batch whole.
    k = 33 takes k_bloom (59 identity bits)."""
    _env(monkeypatch, cold_env)
    _check(gpu_lib, "overflow", k, _shape("overflow", g1, g42), n_batches)


@_MODES
@_BATCHES
@_KS
def test_one_very_long_block(gpu_lib, g1, g42, monkeypatch, cold_env, n_batches, k):
    """(d) 3 000 copies of one read among 3 000 others at -b26: each k-mer of the repeated read brings its block 3 000 entries in one batch
    (that region's list overflows: 3 000 + ~700 > 2 879) and 1 000 in each of three (the list fits: a block of 1 000 entries is ranked by
    the long loop and walked by one lane, and must still be exact).  With k = 27 the first batch is cold by bfcg_ctx.hip:200-208, 249-256 and
    494-495; half of its k-mers are copies found seen (line 685: 40 %), so the batches behind it are no longer cold and take the warm kernel
    behind a cold one.  k = 33 takes k_bloom."""
    _env(monkeypatch, cold_env)
    _check(gpu_lib, "long_block", k, _shape("long_block", g1, g42), n_batches)
