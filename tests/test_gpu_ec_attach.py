"""GPU tests (-m gpu) of the corrector attached to a counting context (bfcg_ec_attach, GpuCorrector(GpuCounter, ...)): the count table is
read where the count kernels built it, nothing is exported, and the reads the first kernel leaves are corrected by the retry kernel
(k_ec_retry) instead of the host instance.  The expected side of every comparison is the host instance (bfcg_ec1_host) on an exported
table, or the reference's bytes (tests/golden/ec_goldens.json); never an attached corrector."""
import hashlib
import json
import os

import numpy as np
import pytest

import refine_inputs as RI
from bfc_amd import gen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ec_goldens.json")))
SMALL = {"BFCG_EC_HEAP": "2", "BFCG_EC_STACK": "40"}              # as test_gpu_fallback_forced: many reads overflow in the first kernel


def _equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert x == y


def _head(res, n):
    return res[0][:n], res[1][:n] if res[1] is not None else None, res[2][:n], res[3][:n]


def _opt(gpu_lib, k=31, **kw):
    o = gpu_lib.bfc_opt_init(); o.k = k
    for name, v in kw.items():
        setattr(o, name, v)
    return o


def _pos(seqs):
    return sum(len(s) + 1 for s in seqs)


def _count_g1(gpu_lib, g1, lo=0.0, hi=1.0, counter=None, **kw):
    """reads [lo, hi) of g1 (fractions) counted as one batch with k = 31, -b26"""
    rs, (seq, qual, off) = g1
    a, b = int(rs.n_reads * lo), int(rs.n_reads * hi)
    o = off[a:b + 1] - off[a]
    s = gpu_lib.to_stream(seq[int(off[a]):int(off[b])], o)
    q = gpu_lib.to_stream(qual[int(off[a]):int(off[b])], o)
    g = counter or gpu_lib.GpuCounter(31, 26, max_batch_pos=len(seq) + rs.n_reads + 64, **kw)
    g.count_host(s, q)
    return g


@pytest.fixture(scope="module")
def g1_reads(tmp_path_factory):
    fq = str(tmp_path_factory.mktemp("ec_attach") / "g1.fq")
    gen.fixture("g1").fastq(fq)
    lines = open(fq, "rb").read().split(b"\n")
    return ([lines[i][1:] for i in range(0, len(lines) - 1, 4)], [lines[i] for i in range(1, len(lines) - 1, 4)],
            [lines[i] for i in range(3, len(lines) - 1, 4)])


@pytest.fixture(scope="module")
def env(gpu_lib, g1, g1_reads):
    """g1 counted once: the counter (kept, for the attached correctors), its exported table, the host instance's twin on that table and
    what it makes of every read of g1 (FASTQ) and of the first 2000 (FASTA): computed once, never changed"""
    names, seqs, quals = g1_reads
    g = _count_g1(gpu_lib, g1)
    t = g.export_table()
    twin = gpu_lib.GpuCorrector(t, _opt(gpu_lib), gpu=False)
    e = dict(g=g, t=t, twin=twin, fq=twin.host_correct(seqs, quals), fa=twin.host_correct(seqs[:2000]))
    yield e
    g.close(); t.close()


@pytest.mark.parametrize("layout", ["segments", "host_layout"])
def test_attached_equals_host_on_both_layouts(gpu_lib, g1, g1_reads, layout):
    """g1 corrected on the counter's own table: equal to the host instance on the table exported afterwards, and the reference's bytes"""
    names, seqs, quals = g1_reads
    # k = 31 at -b26 takes the region-owned segments with regions of 16 blocks (13 region bits: 49 identity bits)
    g = _count_g1(gpu_lib, g1, **(dict(region_shift=4) if layout == "segments" else dict(table_layout=1)))
    g.sync()
    assert g.table_info()["segments"] == (layout == "segments"), g.table_info()
    o = _opt(gpu_lib)
    with pytest.raises(gpu_lib.BfcGpuError):                       # refused before the context is drained or converted
        gpu_lib.GpuCorrector(g, _opt(gpu_lib, k=33))
    assert g.table_info()["segments"] == (layout == "segments")
    c = gpu_lib.GpuCorrector(g, o, max_pos=_pos(seqs), max_reads=len(seqs))
    assert not g.table_info()["segments"] and not c.adopted
    dev = c.correct(seqs, quals)
    fa = c.correct(seqs[:2000])
    assert c.host_reads() == 0 and c.last_ms() > 0 and c.last_lookups() > 0
    t = g.export_table()
    twin = gpu_lib.GpuCorrector(t, o, gpu=False)
    _equal(dev, twin.host_correct(seqs, quals))
    _equal(fa, twin.host_correct(seqs[:2000]))
    assert hashlib.md5(gpu_lib.format_ec(names, *dev, o)).hexdigest() == GOLD["g1"]["stdout_md5"]
    assert c.mode == t.hist()[0] == twin.mode
    c.close(); t.close(); g.close()


@pytest.mark.parametrize("lmax", [None, "64"])
def test_retry_kernel(gpu_lib, env, g1_reads, monkeypatch, lmax):
    """a heap of 2 entries and a stack of 40 on 2048 lanes: the reads the first kernel leaves take rounds of 512, 128, ... lanes with 4x
    the capacities each; with a read bound of 64 bases every longer read takes them, and the round's bound grows to the longest"""
    names, seqs, quals = g1_reads
    n = 2000
    for name, v in SMALL.items():
        monkeypatch.setenv(name, v)
    if lmax:
        monkeypatch.setenv("BFCG_EC_LMAX", lmax)
    c = gpu_lib.GpuCorrector(env["g"], _opt(gpu_lib), max_pos=_pos(seqs[:n]), max_reads=n)
    dev = c.correct(seqs[:n], quals[:n])
    print("retry_reads %d of %d (lmax %s), last_ms %.3f, lookups %d" % (c.retry_reads(), n, lmax, c.last_ms(), c.last_lookups()))
    assert c.retry_reads() > 0 and c.host_reads() == 0
    if lmax:
        assert c.retry_reads() >= sum(len(s) > 64 for s in seqs[:n])
    _equal(dev, _head(env["fq"], n))
    first = c.retry_reads()
    _equal(c.correct(seqs[:n]), _head(env["fa"], n))              # FASTA, and the counters add up over batches
    assert c.retry_reads() >= first and c.host_reads() == 0
    c.close()


def test_retry_kernel_refine(gpu_lib, env, g1_reads, monkeypatch):
    """`-R` on the first 300 reads' first pass rewritten by recipe (b) (every read refined, rf 2 and 3), forced capacities: the attached
    refinement corrector equals the host refine instance"""
    names, seqs, quals = g1_reads
    n = 300
    first = gpu_lib.format_ec(names[:n], *_head(env["fq"], n), _opt(gpu_lib))
    rnames, comments, rseqs, rquals = RI.read_records(RI.recipe_b(first))
    assert len(rnames) == n
    o = _opt(gpu_lib, refine_ec=1)
    want, want_a2 = RI.refine(gpu_lib.GpuCorrector(env["t"], o, gpu=False), rnames, comments, rseqs, rquals, o, gpu=False)
    for name, v in SMALL.items():
        monkeypatch.setenv(name, v)
    c = gpu_lib.GpuCorrector(env["g"], o, max_pos=_pos(rseqs), max_reads=n)
    got, got_a2 = RI.refine(c, rnames, comments, rseqs, rquals, o, gpu=True)
    assert c.retry_reads() > 0 and c.host_reads() == 0
    assert got == want and np.array_equal(got_a2, want_a2)
    c.close()


def test_edge_shapes(gpu_lib, env, g1_reads, monkeypatch):
    """a read, a read shorter than k, an empty read and a read of all N in one batch; then each of them, and a few more reads, as a batch
    of one on the smallest grid (256 lanes) with a heap and a stack of one entry: the rounds shrink to a single lane and move on to a
    larger workspace"""
    names, seqs, quals = g1_reads
    bs = [seqs[0], seqs[1][:20], b"", b"N" * 100]
    bq = [quals[0], quals[1][:20], b"", quals[2][:100]]
    want = env["twin"].host_correct(bs, bq)
    c = gpu_lib.GpuCorrector(env["g"], _opt(gpu_lib), max_pos=_pos(bs), max_reads=len(bs))
    _equal(c.correct(bs, bq), want)
    _equal(c.correct(bs), env["twin"].host_correct(bs))
    c.close()
    monkeypatch.setenv("BFCG_EC_HEAP", "1")
    monkeypatch.setenv("BFCG_EC_STACK", "1")
    c = gpu_lib.GpuCorrector(env["g"], _opt(gpu_lib), max_pos=1024, max_reads=1)
    for i in range(len(bs)):
        _equal(c.correct(bs[i:i + 1], bq[i:i + 1]), _head((want[0][i:], want[1][i:], want[2][i:], want[3][i:]), 1))
    for i in range(3, 11):
        one = c.correct(seqs[i:i + 1], quals[i:i + 1])
        _equal(one, (env["fq"][0][i:i + 1], env["fq"][1][i:i + 1], env["fq"][2][i:i + 1], env["fq"][3][i:i + 1]))
    assert c.retry_reads() > 0 and c.host_reads() == 0
    c.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_options_attached_equal_host(gpu_lib, seed, monkeypatch):
    """the reads, k and options of test_gpu_random_options_equal_host (k in {21 .. 63}: the lossy key too), attached, with forced small
    capacities, against the host instance on the table exported from the same counter"""
    rng = np.random.default_rng(seed)
    k = int(rng.choice([21, 31, 33, 47, 55, 63]))
    genome = rng.integers(0, 4, 6000)
    n = 1500
    seqs, quals = [], []
    for _ in range(n):
        L = int(rng.integers(1, 300))
        p = int(rng.integers(0, 6000 - 300))
        s = bytearray(b"ACGT"[c] for c in genome[p:p + L])
        for _ in range(int(rng.poisson(L * 0.01))):
            s[int(rng.integers(0, L))] = b"ACGT"[int(rng.integers(0, 4))]
        if rng.random() < 0.1:
            s[int(rng.integers(0, L))] = b"NRYacgtn"[int(rng.integers(0, 8))]
        if rng.random() < 0.1:
            s = bytearray(s.lower())
        seqs.append(bytes(s))
        quals.append(bytes(rng.integers(35, 75, L).astype(np.uint8)))
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    qual = np.frombuffer(b"".join(quals), dtype=np.uint8)
    st, qt = gpu_lib.to_stream(seq, off), gpu_lib.to_stream(qual, off)
    g = gpu_lib.GpuCounter(k, 22, max_batch_pos=len(st) + 64)
    g.count_host(st, qt)
    o = _opt(gpu_lib, k=k)
    o.min_cov = int(rng.integers(1, 5)); o.win_multi_ec = int(rng.integers(3, 15)); o.q = int(rng.integers(10, 40))
    o.max_heap = int(rng.integers(1, 12)); o.max_end_ext = int(rng.integers(1, 8)); o.max_path_diff = int(rng.integers(5, 20))
    for name, v in SMALL.items():
        monkeypatch.setenv(name, v)
    c = gpu_lib.GpuCorrector(g, o, max_pos=len(st), max_reads=n)
    fq, fa = c.correct(seqs, quals), c.correct(seqs)
    print("seed %d: k %d, retry_reads %d" % (seed, k, c.retry_reads()))
    assert c.host_reads() == 0
    t = g.export_table()
    twin = gpu_lib.GpuCorrector(t, o, gpu=False)
    assert c.mode == twin.mode
    _equal(fq, twin.host_correct(seqs, quals))
    _equal(fa, twin.host_correct(seqs))
    c.close(); t.close(); g.close()


def test_context_counts_on_afterwards(gpu_lib, g1, g1_reads):
    """half of g1 counted, corrected on the spot, the corrector closed, the other half counted: the table is that of a fresh counter
    given both batches"""
    names, seqs, quals = g1_reads
    g = _count_g1(gpu_lib, g1, 0.0, 0.5, region_shift=4)
    c = gpu_lib.GpuCorrector(g, _opt(gpu_lib), max_pos=_pos(seqs[:500]), max_reads=500)
    c.correct(seqs[:500], quals[:500])
    c.close()
    _count_g1(gpu_lib, g1, 0.5, 1.0, counter=g)
    fresh = _count_g1(gpu_lib, g1, 0.0, 0.5, region_shift=4)
    _count_g1(gpu_lib, g1, 0.5, 1.0, counter=fresh)
    t, tf = g.export_table(), fresh.export_table()
    for a, b in zip(t.export_sorted(), tf.export_sorted()):
        assert np.array_equal(a, b)
    t.close(); tf.close(); g.close(); fresh.close()


def test_refusals(gpu_lib, env, g1_reads):
    """a filter-mode context, another k, filter_mode in the options, the host instance of an attached corrector: BfcGpuError each"""
    names, seqs, quals = g1_reads
    fm = gpu_lib.GpuCounter(31, 26, filter_mode=1, max_batch_pos=1 << 16)
    with pytest.raises(gpu_lib.BfcGpuError, match="table-mode context"):
        gpu_lib.GpuCorrector(fm, _opt(gpu_lib))
    fm.close()
    with pytest.raises(gpu_lib.BfcGpuError, match="opt->k"):
        gpu_lib.GpuCorrector(env["g"], _opt(gpu_lib, k=33))
    with pytest.raises(gpu_lib.BfcGpuError):
        gpu_lib.GpuCorrector(env["g"], _opt(gpu_lib, filter_mode=1))
    c = gpu_lib.GpuCorrector(env["g"], _opt(gpu_lib), max_pos=1024, max_reads=4)
    with pytest.raises(gpu_lib.BfcGpuError, match="no host table"):
        c.host_correct(seqs[:1], quals[:1])
    assert c.retry_reads() == 0 and c.host_reads() == 0
    c.close()
