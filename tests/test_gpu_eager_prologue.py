"""k_bloom3's eager prologue (BloomArgs.eager: the region's slice, the five words its exits test and -- from a one-pass slab -- a first round of
records are requested together before anything is decided; bfcg_bloom3.hip) against the CPU oracle, as tests/test_gpu_bloom3_cold_order.py::_check
compares: filter bytes, counters and the sorted table export, bit for bit.  Every case runs with BFCG_EAGER=1 and =0 (read at context creation;
the default rule, bfcg_ctx.hip: enqueue_stage_b, would leave most of these small batches on the old order), once more by that rule, and with and without debug_seen: the
per-k-mer flags are compared in the first run, and only the second hands the seen k-mers over through the log and its cursor (ho_cur).

Shapes (bfcg_ctx.hip: bfcg_create).  k = 27 takes k_bloom3 (tests/test_gpu_bloom3_cold_order.py says why).  -b26: 2^9 regions of 256 blocks,
F1 = 4, F2 = 5: the one-pass partition (region slabs, cap2 != 0, records requested ahead) from 16 x 8 x 1024 = 131 072 positions on.  -b24: 2^7
regions on ONE scatter level (F2 = 0): region_list's start[f] / start[f + 1] mode.  -b30: 2^13 regions, one pass from 2^19 positions on; below it
two passes with the regions' counts beside their starts (cnt_live)."""
import numpy as np
import pytest

import oracle
from bfc_amd import gen

pytestmark = pytest.mark.gpu

K = 27


def _cut(g, n):
    rs, (seq, qual, off) = g
    return seq[:n * rs.L], qual[:n * rs.L], off[:n + 1]


def _shape(name, g1, g42):
    """(seq, qual, off, bf_shift) of a named shape; reads of equal length."""
    if name.startswith("g42_"):  # "g42_<reads>_<b>"
        _, n, b = name.split("_")
        return _cut(g42, int(n)) + (int(b),)
    if name.startswith("g1_"):
        _, n, b = name.split("_")
        return _cut(g1, int(n)) + (int(b),)
    if name == "copies":  # all of g1, a 10x coverage, at -b26
        rs, (seq, qual, off) = g1
        return seq, qual, off, 26
    assert name == "one_read"  # 1 500 copies of one read among 1 500 others: each of its k-mers brings ONE region 1 500 records
    rs, (seq, qual, off) = g1
    L, n = rs.L, 1500
    s = np.empty((2 * n, L), dtype=seq.dtype); q = np.empty((2 * n, L), dtype=qual.dtype)
    s[0::2] = seq[:n * L].reshape(n, L); q[0::2] = qual[:n * L].reshape(n, L)
    s[1::2] = seq[7 * L:8 * L]; q[1::2] = qual[7 * L:8 * L]
    return s.reshape(-1), q.reshape(-1), np.arange(2 * n + 1, dtype=off.dtype) * L, 26


_ORACLE = {}


def _oracle(name, k, shape):
    """The oracle's answers for a shape, computed once and shared by the shape's cases (never changed)."""
    if (name, k) not in _ORACLE:
        seq, qual, off, b = shape
        oc = oracle.Counter(k, b)
        tr = oc.count(seq, qual, off, trace=True)
        ost = oc.stats()
        R = min(8, b - 9)
        loads = np.bincount(((tr[:, 1] >> np.uint64(R)) & np.uint64((1 << (b - 9 - R)) - 1)).astype(np.int64), minlength=1 << (b - 9 - R))
        _ORACLE[name, k] = dict(bloom=oc.bloom_bytes().copy(), seen=((tr[:, 3] >> 1) & 1 == 1).copy(), loads=loads,
                                stats=(ost["n_kmers"], ost["n_high"], ost["n_seen"]), table=tuple(a.copy() for a in oc.export()))
        oc.close()
    return _ORACLE[name, k]


def _count(gpu_lib, k, shape, n_batches, debug_seen, room=1):
    """The shape through a fresh context (sized for `room` times a batch) in n_batches host batches; the context (open) and the seen flags of all
    batches (or None)."""
    seq, qual, off, b = shape
    n_reads = len(off) - 1
    L = int(off[1] - off[0])
    per = (n_reads + n_batches - 1) // n_batches
    g = gpu_lib.GpuCounter(k, b, max_batch_pos=room * (per * (L + 1) + 64), debug_seen=debug_seen)
    seen = []
    for i in range(0, n_reads, per):
        j = min(n_reads, i + per)
        o = off[i:j + 1] - off[i]
        g.count_host(gpu_lib.to_stream(seq[int(off[i]):int(off[j])], o), gpu_lib.to_stream(qual[int(off[i]):int(off[j])], o))
        if debug_seen:  # (the flags are per batch: read after each one, in file order)
            fl = g.seen_flags(int(off[j] - off[i]) + (j - i))
            seen.append(fl[fl > 0] == 2)
    return g, (np.concatenate(seen) if debug_seen else None)


def _same(g, seen, want):
    assert np.array_equal(g.bloom_bytes(), want["bloom"]), "filter bytes differ"
    if seen is not None:
        assert np.array_equal(seen, want["seen"]), "seen flags differ from the sequential semantics"
    st = g.stats()
    assert (st["n_kmers"], st["n_high"], st["n_seen"]) == want["stats"]
    sizes, slots = g.export_table().export_sorted()
    assert np.array_equal(sizes, want["table"][0]) and np.array_equal(slots, want["table"][1])
    return st


def _set_eager(monkeypatch, eager):
    if eager is None:
        monkeypatch.delenv("BFCG_EAGER", raising=False)
    else:
        monkeypatch.setenv("BFCG_EAGER", eager)


def _check(gpu_lib, monkeypatch, eager, debug_seen, name, shape, n_batches=1, k=K, after=None, room=1):
    _set_eager(monkeypatch, eager)
    want = _oracle(name, k, shape)
    g, seen = _count(gpu_lib, k, shape, n_batches, debug_seen, room)
    st = _same(g, seen, want)
    if after:
        after(g, st)
    g.close()
    return want


# (the third setting: the rule of enqueue_stage_b itself -- eager from 16 positions per region on: the batches of 8 000 reads at -b26 / -b24 and
#  g1 in thirds are above it, the tiny ones below)
_EAGER = pytest.mark.parametrize("eager", ["1", "0", None], ids=["EAGER=1", "EAGER=0", "by_rule"])
_SEEN = pytest.mark.parametrize("debug_seen", [True, False], ids=["seen_flags", "handover_log"])


@_EAGER
@_SEEN
@pytest.mark.parametrize("name,onepass", [("g1_20_26", False), ("g1_300_30", False), ("g1_300_30", True)])
def test_empty_and_tiny_regions(gpu_lib, g1, g42, monkeypatch, eager, debug_seen, name, onepass):
    """(a) 20 reads into -b26: ~5 records per region, some regions none; 300 reads into -b30: 2^13 regions for 37 200 k-mers, most of them with a
    handful of records, some empty -- a forced eager launch requests every region's slice and takes the n == 0 exit with the loads in flight.  These
    batches are below the one-pass partition's minimum (two passes: start[f] and the live counts, nothing read ahead of rs); the third case lowers
    the minimum (BFCG_ONEPASS_MIN_TILES=1), so that the same -b30 batch lies in region slabs and a round of records is requested from EVERY slab,
    empty ones included (in bounds: a slab has cap2 records).  Its context is sized for eight such batches: a level-1 slab (~800 records) then
    holds all a bucket can bring (~580), so that however unevenly so few tiles fill the slabs, none overflows and the batch stays on the slabs."""
    if onepass:
        monkeypatch.setenv("BFCG_ONEPASS_MIN_TILES", "1")
    def after(g, st):
        if onepass:  # (the batch did lie in region slabs, and no slab overflowed: nothing was replayed through the two-pass partition)
            pi = g.partition_info()
            assert pi["one_pass"] and pi["level2_one_pass"] and pi["replayed_batches"] == 0, pi
    want = _check(gpu_lib, monkeypatch, eager, debug_seen, name, _shape(name, g1, g42), after=after, room=8 if onepass else 1)
    assert want["loads"].min() == 0 and np.median(want["loads"]) < 10


@_EAGER
@_SEEN
@pytest.mark.parametrize("n_reads,edge", [(4240, 1024), (8470, 2048)])
def test_round_boundaries(gpu_lib, g1, g42, monkeypatch, eager, debug_seen, n_reads, edge):
    """(b) one batch of g42's first 4 240 / 8 470 reads at -b26: 0.2418 k-mers per read and region (1 860 per region for 8 000 reads), so the regions'
    loads lie around 1 025 / 2 048 records with a spread of +-10 %: regions on either side of a round of BT x PF = 1 024 (PF = 2) and 2 048 (PF = 4)
    records in ONE launch -- the first round is what the eager prologue requests before the count is known, the second what it requests after.
    (The oracle's trace says how many regions lie on which side; at least a tenth must lie on each.)"""
    name = "g42_%d_26" % n_reads
    want = _check(gpu_lib, monkeypatch, eager, debug_seen, name, _shape(name, g1, g42))
    below = int((want["loads"] <= edge).sum())
    assert 51 <= below <= 512 - 51, (below, want["loads"].min(), want["loads"].max())


@_EAGER
@_SEEN
@pytest.mark.parametrize("mode", ["slabs", "two_pass", "one_level"])
def test_region_list_modes(gpu_lib, g1, g42, monkeypatch, eager, debug_seen, mode):
    """(c) 8 000 reads of g42 (1.2 M positions) in one batch.  `slabs`: -b26, above the one-pass minimum of 131 072 positions: region slabs, cap2 != 0,
    the first round of records requested with the slice.  `two_pass`: the same reads with the minimum out of reach: start[f] and the live counts
    (cnt_live) -- nothing may be read before rs is known.  `one_level`: -b24 (F2 = 0): start[f] / start[f + 1]; every region's list overflows there
    (7 400 k-mers per region), so the eager launch also enters k_bloom3's own slow path, which stages the slice again from memory."""
    if mode == "two_pass":
        monkeypatch.setenv("BFCG_ONEPASS_MIN_TILES", "1000000")
    name = "g42_8000_24" if mode == "one_level" else "g42_8000_26"

    def after(g, st):
        pi = g.partition_info()
        if mode == "slabs":
            assert g.mg_info()["nb1"] * 8 * 1024 <= 8000 * 151 and pi["one_pass"] and pi["level2_one_pass"] and pi["replayed_batches"] == 0
        if mode == "one_level":
            assert g.mg_info()["nb1"] == 128 and (st["slow_buckets"] > 0 or not debug_seen)  # (without debug_seen the library cuts the batch: no overflow)
    _check(gpu_lib, monkeypatch, eager, debug_seen, name, _shape(name, g1, g42), after=after)


@_EAGER
@_SEEN
def test_poisoned_batch(gpu_lib, g1, g42, monkeypatch, eager, debug_seen):
    """(d) 1 500 copies of one read among 1 500 others at -b26, one batch of 453 000 positions (one pass): a region's slab holds
    9/8 x 453 000 / 512 + 64 = 1 059 records, and each k-mer of the repeated read brings its region 1 500 -- a slab overflows, the launch is poisoned
    (its eager loads are dropped, nothing is stored) and the batch is replayed through the two-pass partition."""
    def after(g, st):
        assert g.partition_info()["replayed_batches"] > 0
    _check(gpu_lib, monkeypatch, eager, debug_seen, "one_read", _shape("one_read", g1, g42), after=after)


@_EAGER
@_SEEN
def test_tiny_bloom_slow_path(gpu_lib, g1, g42, monkeypatch, eager, debug_seen):
    """(e) tests/test_gpu_parity.py::test_tiny_bloom_forces_slow_path's -b14 shape (k = 31, 2 000 reads of g1, one region): with debug_seen, which
    keeps the batch whole, the HBM-pool path runs (slow_buckets > 0); without it the library cuts the batch into pieces the region takes, so only
    the answers are compared.  (k_bloom3's own slow path: test_region_list_modes.)"""
    def after(g, st):
        assert st["slow_buckets"] > 0 or not debug_seen
    _check(gpu_lib, monkeypatch, eager, debug_seen, "g1_2000_14", _shape("g1_2000_14", g1, g42), k=31, after=after)


@_EAGER
@_SEEN
def test_cold_to_warm(gpu_lib, g1, g42, monkeypatch, eager, debug_seen):
    """(f) all of g1 (10x coverage) at -b26 in three batches: the first is cold, a later third finds more than 40 % of its k-mers seen and the batch
    behind it takes the warm kernel (tests/test_gpu_bloom3_cold_order.py::test_blocks_of_copies): both prologues in one run, the log's cursor
    carried from one to the other."""
    _check(gpu_lib, monkeypatch, eager, debug_seen, "copies", _shape("copies", g1, g42), n_batches=3)


@_EAGER
def test_group_of_two_ranks(gpu_lib, g1, g42, monkeypatch, eager):
    """(h) the same reads through a group of two ranks emulated on one device (tests/test_gpu_group.py): a rank's stage B -- k_seg_setup_mg's segment
    arrays, level 2, the bloom insert over its half of the regions -- goes through the one stage-B entry that sets the flag.  (A group has no
    debug_seen -- bfcg_group_create takes no such parameter and a rank's flags are not exported --, so this case runs through the hand-over log only.)"""
    _set_eager(monkeypatch, eager)
    seq, qual, off, b = shape = _shape("copies", g1, g42)
    want = _oracle("copies", K, shape)
    rs = g1[0]
    n = rs.n_reads
    grp = gpu_lib.GpuGroup(K, b, [0, 0], max_batch_pos=(n // 3 + 2) * (rs.L + 1) // 2 + 4096)
    for a in range(0, n, n // 3 + 1):
        e = min(n, a + n // 3 + 1)
        grp.count_host(gen.to_stream(seq[a * rs.L:e * rs.L], rs.L, 10), gen.to_stream(qual[a * rs.L:e * rs.L], rs.L, 33))
    st = grp.stats()
    assert (st["n_kmers"], st["n_high"], st["n_seen"]) == want["stats"]
    bf = grp.export_bloom(0)
    assert np.array_equal(bf.bytes(), want["bloom"]), "filter bytes differ"
    bf.close()
    t = grp.export_table()
    sizes, slots = t.export_sorted()
    assert np.array_equal(sizes, want["table"][0]) and np.array_equal(slots, want["table"][1])
    t.close(); grp.close()
