"""GPU tests (-m gpu) of the device corrector (k_ec, k_ec_retry, k_decode in bfcg_ec.hip, running bfcg_ec1.h) on every exit of bfc_ec1,
every k and every seam of its workspace.  The reads are tests/ec_corpus.py's (edge_reads + exit_reads: ec_code 0, 2, 3, 4, 5 and the brute
path; ec_code 1 is unreachable, see there); the table is the corpus's counting file (1500 reads of 120 bases) counted by GpuCounter at
-b22, bit-identical to the reference's by the parity tests.  The expected side of every comparison is the host instance
(GpuCorrector(table, o, gpu=False)) on an exported table, or the reference's md5 (tests/golden/ec_paths_goldens.json); never a GPU
corrector.  Every comparison is exact: bytes, qualities, aux and aux2."""
import hashlib
import json
import os

import numpy as np
import pytest

import ec_corpus as EC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ec_paths_goldens.json")))
SMALL = {"BFCG_EC_HEAP": "2", "BFCG_EC_STACK": "40"}              # as test_gpu_ec_attach: many reads overflow in the first kernel
# test_ec_host.py's test_options_vs_reference, and max_end_ext = 0
OPTIONS = [{"discard": 1}, {"no_qual": 1}, {"min_cov": 2}, {"min_cov": 5}, {"win_multi_ec": 4}, {"win_multi_ec": 20}, {"q": 10}, {"q": 35},
           {"max_heap": 1}, {"max_heap": 2}, {"max_heap": 3}, {"max_heap": 4}, {"max_end_ext": 1, "max_path_diff": 3},
           {"w_ec": 2, "w_ec_high": 3, "w_absent": 1, "w_absent_high": 2}, {"max_end_ext": 0}]


def _equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert x == y


def _head(res, n):
    return res[0][:n], res[1][:n] if res[1] is not None else None, res[2][:n], res[3][:n]


def _opt(gpu_lib, k, **kw):
    o = gpu_lib.bfc_opt_init(); o.k = k
    for name, v in kw.items():
        setattr(o, name, v)
    return o


def _pos(seqs):
    return sum(len(s) + 1 for s in seqs)


def _names(n):
    return [b"r%d" % i for i in range(n)]                       # ec_corpus.write_reads's, which the goldens were made with


@pytest.fixture(scope="module")
def cset(gpu_lib):
    """the genome, the counting file's reads and their streams"""
    _, genome, reads, quals = EC.count_set()
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in reads])
    st = gpu_lib.to_stream(np.frombuffer(b"".join(reads), dtype=np.uint8), off)
    qt = gpu_lib.to_stream(np.frombuffer(b"".join(quals), dtype=np.uint8), off)
    return dict(genome=genome, reads=reads, quals=quals, st=st, qt=qt)


def _count(gpu_lib, cset, k, **kw):
    g = gpu_lib.GpuCounter(k, 22, max_batch_pos=len(cset["st"]) + 64, **kw)
    g.count_host(cset["st"], cset["qt"])
    return g


@pytest.fixture(scope="module")
def tables(gpu_lib, cset):
    """per k, made when first asked for and kept: the counter (for attached correctors), its exported table, the host instance on it
    and what that makes of the corpus as FASTQ and as FASTA.  Nothing here is changed by a test."""
    made = {}

    def get(k):
        if k not in made:
            g = _count(gpu_lib, cset, k)
            t = g.export_table()
            twin = gpu_lib.GpuCorrector(t, _opt(gpu_lib, k), gpu=False)
            seqs, quals = EC.corpus(cset["genome"], k)
            made[k] = dict(g=g, t=t, twin=twin, seqs=seqs, quals=quals, fq=twin.host_correct(seqs, quals), fa=twin.host_correct(seqs))
        return made[k]
    yield get
    for e in made.values():
        e["t"].close(); e["g"].close()


def _check_expected(k, want_fq, want_fa):
    """the conditions on the expected side (ec_corpus.conditions) and the reference's numbers for it"""
    for fmt, want in (("fq", want_fq), ("fa", want_fa)):
        g = GOLD["k%d_%s" % (k, fmt)]
        EC.conditions(want[2])
        hist, brute = EC.histogram(want[2])
        print("k %d %s expected: ec_code histogram %s, brute %d" % (k, fmt, hist, brute))
        assert hist == g["ec_code_hist"]
        assert int(((want[2] >> 3 & 1 == 1) & (want[2] & 7 == 0)).sum()) == g["brute_code0"]


# region-owned segments need a k-mer's identity inside its region to fit a slot's 50 key bits: 2k - (13 - region_shift) bits at -b22 (13
# block bits), so of the corpus's k only 21 can take them
FORMS = [(k, f) for k in EC.KS for f in ("uploaded", "host_layout")] + [(21, "segments")]


@pytest.mark.parametrize("k,form", FORMS, ids=["k%d_%s" % kf for kf in FORMS])
def test_every_exit_every_k_every_table_form(gpu_lib, cset, k, form):
    """the corpus of k, FASTQ and FASTA, on a corrector that looks k-mers up in (a) the exported table uploaded by bfcg_ec_create, (b) the
    context's table in the host layout (table_layout = 1), (c) the context's region-owned segments, converted on attaching (k = 21 only,
    see FORMS).  Equal to the host instance on the table exported from the same counter; the formatted output is the reference's
    (golden md5); the expected side has every reachable ec_code and a brute read with ec_code 0.  Attached: nothing went to the host,
    and the mode of the brute path (from the device histogram) is the host table's."""
    seqs, quals = EC.corpus(cset["genome"], k)
    o = _opt(gpu_lib, k)
    g = _count(gpu_lib, cset, k, **(dict(region_shift=4) if form == "segments" else dict(table_layout=1) if form == "host_layout" else {}))
    g.sync()
    if form != "uploaded":
        assert g.table_info()["segments"] == (form == "segments"), g.table_info()
        c = gpu_lib.GpuCorrector(g, o, max_pos=_pos(seqs), max_reads=len(seqs))
        assert not g.table_info()["segments"]
        fq, fa = c.correct(seqs, quals), c.correct(seqs)
        t = g.export_table()
    else:
        t = g.export_table()
        c = gpu_lib.GpuCorrector(t, o, max_pos=_pos(seqs), max_reads=len(seqs))
        fq, fa = c.correct(seqs, quals), c.correct(seqs)
    twin = gpu_lib.GpuCorrector(t, o, gpu=False)
    want_fq, want_fa = twin.host_correct(seqs, quals), twin.host_correct(seqs)
    _check_expected(k, want_fq, want_fa)
    _equal(fq, want_fq)
    _equal(fa, want_fa)
    names = _names(len(seqs))
    assert hashlib.md5(gpu_lib.format_ec(names, *fq, o)).hexdigest() == GOLD["k%d_fq" % k]["stdout_md5"]
    assert hashlib.md5(gpu_lib.format_ec(names, *fa, o)).hexdigest() == GOLD["k%d_fa" % k]["stdout_md5"]
    assert c.last_lookups() > 0
    if form != "uploaded":
        assert c.host_reads() == 0 and c.mode == twin.mode == t.hist()[0]
    c.close(); t.close(); g.close()


@pytest.mark.parametrize("form", ["uploaded", "attached_small"])
@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "_".join("%s%d" % kv for kv in o.items()))
def test_options_on_the_device(gpu_lib, tables, monkeypatch, opts, form):
    """k = 33, the option sets the host instance is held to the reference with (test_options_vs_reference) and max_end_ext = 0, on the
    uploaded table and attached with a heap of 2 and a stack of 40 entries (the retry kernel takes what overflows)"""
    e = tables(33)
    seqs, quals = e["seqs"], e["quals"]
    o = _opt(gpu_lib, 33, **opts)
    twin = gpu_lib.GpuCorrector(e["t"], o, gpu=False)
    want_fq, want_fa = twin.host_correct(seqs, quals), twin.host_correct(seqs)
    if form == "attached_small":
        for name, v in SMALL.items():
            monkeypatch.setenv(name, v)
    c = gpu_lib.GpuCorrector(e["g"] if form == "attached_small" else e["t"], o, max_pos=_pos(seqs), max_reads=len(seqs))
    fq, fa = c.correct(seqs, quals), c.correct(seqs)
    _equal(fq, want_fq)
    _equal(fa, want_fa)
    names = _names(len(seqs))
    assert gpu_lib.format_ec(names, *fq, o) == gpu_lib.format_ec(names, *want_fq, o)
    if form == "attached_small":
        assert c.retry_reads() > 0 and c.host_reads() == 0 and c.mode == twin.mode
    c.close()


@pytest.mark.parametrize("form", ["uploaded", "attached"])
def test_a_lane_takes_several_reads(gpu_lib, cset, tables, monkeypatch, form):
    """256 lanes (the smallest grid) for the corpus and the counting file's reads, about 1650 reads: every lane takes reads from the queue
    again and again and reuses its slices of the workspace.  The first 255, 256, 257 reads and all of them, FASTQ then FASTA on the same
    corrector: each result is the head of the host instance's answer"""
    k = 31
    e = tables(k)
    seqs, quals = e["seqs"] + cset["reads"], e["quals"] + cset["quals"]
    more_fq, more_fa = e["twin"].host_correct(cset["reads"], cset["quals"]), e["twin"].host_correct(cset["reads"])
    want_fq = (e["fq"][0] + more_fq[0], e["fq"][1] + more_fq[1], np.concatenate([e["fq"][2], more_fq[2]]), np.concatenate([e["fq"][3], more_fq[3]]))
    want_fa = (e["fa"][0] + more_fa[0], None, np.concatenate([e["fa"][2], more_fa[2]]), np.concatenate([e["fa"][3], more_fa[3]]))
    EC.conditions(want_fq[2]); EC.conditions(want_fa[2])
    monkeypatch.setenv("BFCG_EC_LANES", "256")
    c = gpu_lib.GpuCorrector(e["g"] if form == "attached" else e["t"], _opt(gpu_lib, k), max_pos=_pos(seqs), max_reads=len(seqs))
    for n in (255, 256, 257, len(seqs)):
        _equal(c.correct(seqs[:n], quals[:n]), _head(want_fq, n))
        _equal(c.correct(seqs[:n]), _head(want_fa, n))
    if form == "attached":
        assert c.host_reads() == 0
    c.close()


def _erroneous(rng, genome, L, n_err):
    p = int(rng.integers(0, len(genome) - 120 - L))
    s = bytearray(genome[p:p + L])
    for j in rng.integers(0, L, n_err):
        s[j] = b"ACGT"[(b"ACGT".index(s[j]) + 1 + int(rng.integers(0, 3))) % 4]
    return s


@pytest.mark.parametrize("form", ["uploaded", "attached"])
def test_reads_on_the_length_bound(gpu_lib, cset, tables, monkeypatch, form):
    """BFCG_EC_LMAX = 100 and 600 erroneous genome reads of 99, 100 and 101 bases, interleaved, so neighbouring lanes hold full result
    slices (2 x lmax bytes a lane, next to each other) at the same time.  Every third read of a length has an error in its last base and
    every third in its first: the two bytes at the slices' seam.  A heap of 256 entries (the search holds at most max_heap + 4 = 104)
    and a stack of 16384, so that the length is the only reason to leave the device: the 101-base reads go to the host instance
    (uploaded) or the retry kernel (attached), the 100-base reads are corrected where they are."""
    k = 31
    e = tables(k)
    rng = np.random.default_rng(77)
    seqs, quals = [], []
    for i in range(600):
        L = 99 + i % 3
        s = _erroneous(rng, cset["genome"], L, int(rng.integers(1, 4)))
        q = bytearray(rng.integers(33, 74, L).astype(np.uint8))
        if i // 3 % 3 == 0:
            s[L - 1] = b"ACGT"[(b"ACGT".index(s[L - 1]) + 1) % 4]; q[L - 1] = 40
        elif i // 3 % 3 == 1:
            s[0] = b"ACGT"[(b"ACGT".index(s[0]) + 1) % 4]; q[0] = 40
        seqs.append(bytes(s)); quals.append(bytes(q))
    want_fq, want_fa = e["twin"].host_correct(seqs, quals), e["twin"].host_correct(seqs)
    for name, v in {"BFCG_EC_LMAX": "100", "BFCG_EC_HEAP": "256", "BFCG_EC_STACK": "16384"}.items():
        monkeypatch.setenv(name, v)
    c = gpu_lib.GpuCorrector(e["g"] if form == "attached" else e["t"], _opt(gpu_lib, k), max_pos=_pos(seqs), max_reads=len(seqs))
    fq = c.correct(seqs, quals)
    left = c.retry_reads() if form == "attached" else c.host_reads()
    print("%s: %d of 600 reads left the first kernel (200 are longer than lmax)" % (form, left))
    _equal(fq, want_fq)
    _equal(c.correct(seqs), want_fa)
    if form == "attached":
        assert left >= 200 and c.host_reads() == 0
    else:
        assert left >= 200
    on = np.nonzero([len(s) == 100 for s in seqs])[0]            # the reads of exactly lmax bases are corrected, first and last base too
    assert (fq[2][on] & 7 == 0).all() and (fq[3][on] != 0xffffffff).all()
    assert all(fq[0][i].upper() != seqs[i] for i in on)
    assert sum(fq[0][i][-1:].islower() for i in on) > 50 and sum(fq[0][i][:1].islower() for i in on) > 50
    c.close()


def test_retry_rounds_under_load_then_an_ordinary_batch(gpu_lib, cset, tables, monkeypatch):
    """attached, 256 lanes, a heap and a stack of one entry, a read bound of 64 bases; 200 reads of 600 bases with about 1 % errors.  No
    read fits before the first retry round (lmax grows to 600 there and the result buffer with it, for good); the rounds shrink to one
    lane of 256 entries, which a 600-base read's stack outgrows, so the larger workspace (64 lanes) starts with more reads than lanes.
    Then the corpus on the same corrector: k_ec on the grown buffer with the original bound"""
    k = 31
    e = tables(k)
    rng = np.random.default_rng(78)
    seqs = [bytes(_erroneous(rng, cset["genome"], 600, int(rng.poisson(6)))) for _ in range(200)]
    quals = [bytes(rng.integers(33, 74, 600).astype(np.uint8)) for _ in seqs]
    want = e["twin"].host_correct(seqs, quals)
    assert (want[2] & 7 == 0).sum() > 150 and (want[2] >> 18).sum() > 300
    for name, v in {"BFCG_EC_LANES": "256", "BFCG_EC_HEAP": "1", "BFCG_EC_STACK": "1", "BFCG_EC_LMAX": "64"}.items():
        monkeypatch.setenv(name, v)
    n = max(len(seqs), len(e["seqs"]))
    c = gpu_lib.GpuCorrector(e["g"], _opt(gpu_lib, k), max_pos=max(_pos(seqs), _pos(e["seqs"])), max_reads=n)
    _equal(c.correct(seqs, quals), want)
    print("retry_reads %d, host_reads %d" % (c.retry_reads(), c.host_reads()))
    assert c.retry_reads() == 200 and c.host_reads() == 0
    EC.conditions(e["fq"][2]); EC.conditions(e["fa"][2])
    _equal(c.correct(e["seqs"], e["quals"]), e["fq"])
    _equal(c.correct(e["seqs"]), e["fa"])
    assert c.retry_reads() > 200 and c.host_reads() == 0
    _equal(c.correct(seqs), e["twin"].host_correct(seqs))       # and the long reads again, as FASTA, on the buffers as they are now
    c.close()


REFINE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 300)


def refine_batches(genome, k, seed):
    """batches of 1, 3, 4 and 5 reads (k_decode takes four reads a workgroup, 64 bases a stride) whose lengths are drawn from
    REFINE_LENGTHS, every length in every batch size: genome stretches with errors, Ns and a few random bases in a row (k-mers absent
    from any path: rf_code 2 where the earlier stats claim none), bases written in quality bytes 34 .. 38, '!' and '~' bytes; earlier
    stats as test_gpu_refine_random_equals_host makes them.  [(seqs, quals, (ori_aux, ori_aux2))]"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (1, 3, 4, 5):
        lengths = list(REFINE_LENGTHS) * 2
        rng.shuffle(lengths)
        lengths += [300] * (-len(lengths) % n)
        for b in range(0, len(lengths), n):
            seqs, quals = [], []
            for L in lengths[b:b + n]:
                p = int(rng.integers(0, len(genome) - 120 - 300))
                s = bytearray(genome[p:p + L])
                for _ in range(int(rng.poisson(L * 0.01))):
                    s[int(rng.integers(0, L))] = b"ACGTN"[int(rng.integers(0, 5))]
                if L > 2 * k and rng.random() < 0.5:
                    j = int(rng.integers(k, L - 6))
                    s[j:j + 6] = bytes(b"ACGT"[c] for c in rng.integers(0, 4, 6))
                q = bytearray(rng.integers(39, 75, L).astype(np.uint8))
                for j in rng.integers(0, max(L, 1), int(rng.poisson(L * 0.03))):
                    if L:
                        q[j] = int(rng.choice([33, 34, 35, 36, 37, 38, 126]))
                seqs.append(bytes(s)); quals.append(bytes(q))
            ori = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0xfffffcf8),
                   rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0x3ff))
            out.append((seqs, quals, ori))
    return out


@pytest.mark.parametrize("form", ["uploaded", "attached"])
@pytest.mark.parametrize("k", [31, 33, 47, 63])
def test_refinement_seams(gpu_lib, cset, tables, k, form):
    """`-R` (refine_ec = 1) on refine_batches, FASTQ and FASTA, for the k the refine fuzz of test_gpu_ec_refine.py does not draw: equal to
    the host refine instance, whose answers hold both rf_code 2 (the earlier stats stand) and rf_code 3 (corrected again)"""
    e = tables(k)
    o = _opt(gpu_lib, k, refine_ec=1)
    twin = gpu_lib.GpuCorrector(e["t"], o, gpu=False)
    c = gpu_lib.GpuCorrector(e["g"] if form == "attached" else e["t"], o, max_pos=5 * 301, max_reads=5)
    rf = set()
    for seqs, quals, ori in refine_batches(cset["genome"], k, 500 + k):
        want_fq, want_fa = twin.host_correct(seqs, quals, ori=ori), twin.host_correct(seqs, ori=ori)
        rf |= set(int(v) for v in want_fq[3] >> 8 & 3) | set(int(v) for v in want_fa[3] >> 8 & 3)
        _equal(c.correct(seqs, quals, ori=ori), want_fq)
        _equal(c.correct(seqs, ori=ori), want_fa)
    assert {2, 3} <= rf, rf
    if form == "attached":
        assert c.host_reads() == 0
    c.close()
