"""GPU tests (-m gpu) of error correction on the device (bfcg_ec_*, bfcg_ec.hip): bfc_ec1 (correct.c:388-476) for whole batches,
read for read equal to the host instance of the same code (bfcg_ec1_host, held to the reference by tests/test_ec_host.py), and the
reference's whole pipeline through the drop-in binary with BFC_GPU_EC=1."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
from bfc_amd import gen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "ec_goldens.json")))
GPUTRIM = os.path.join(oracle.REF_DIR, "bfc-dropin-gputrim")


def _need(path):
    if not os.path.exists(path):
        pytest.skip("%s not built (make -C oracle where the reference is present)" % path)


def _fastq_records(fn):
    lines = open(fn, "rb").read().split(b"\n")
    return ([lines[i][1:] for i in range(0, len(lines) - 1, 4)], [lines[i] for i in range(1, len(lines) - 1, 4)],
            [lines[i] for i in range(3, len(lines) - 1, 4)])


@pytest.fixture(scope="module")
def g1_table(gpu_lib, g1, tmp_path_factory):
    """g1's count table from the GPU counter (bit-identical to the reference's: test_gpu_parity), and g1's reads as bytes"""
    rs, (seq, qual, off) = g1
    s, q = gpu_lib.to_stream(seq, off), gpu_lib.to_stream(qual, off)
    g = gpu_lib.GpuCounter(31, 26, max_batch_pos=len(s) + 64)
    g.count_host(s, q)
    t = g.export_table()
    g.close()
    d = tmp_path_factory.mktemp("ec")
    fq = str(d / "g1.fq")
    gen.fixture("g1").fastq(fq)
    yield t, _fastq_records(fq)
    t.close()


def _equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert x == y


def test_gpu_equals_host_on_g1(gpu_lib, g1_table):
    t, (names, seqs, quals) = g1_table
    o = gpu_lib.bfc_opt_init(); o.k = 31
    c = gpu_lib.GpuCorrector(t, o, max_pos=sum(len(s) + 1 for s in seqs), max_reads=len(seqs))
    dev = c.correct(seqs, quals)
    host = c.host_correct(seqs, quals)
    _equal(dev, host)
    assert hashlib.md5(gpu_lib.format_ec(names, *dev, o)).hexdigest() == GOLD["g1"]["stdout_md5"]
    assert c.last_ms() > 0 and c.last_lookups() > len(seqs) * 100
    # FASTA: the same reads without quality strings
    _equal(c.correct(seqs[:2000]), c.host_correct(seqs[:2000]))
    c.close()


def test_gpu_equals_host_on_g42(gpu_lib, g42):
    rs, (seq, qual, off) = g42
    s, q = gpu_lib.to_stream(seq, off), gpu_lib.to_stream(qual, off)
    g = gpu_lib.GpuCounter(33, 24, max_batch_pos=len(s) + 64)
    g.count_host(s, q)
    t = g.export_table()
    g.close()
    n = min(rs.n_reads, 6000)
    seqs = [seq[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    quals = [qual[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    o = gpu_lib.bfc_opt_init(); o.k = 33
    c = gpu_lib.GpuCorrector(t, o, max_pos=sum(len(x) + 1 for x in seqs), max_reads=n)
    dev = c.correct(seqs, quals)
    _equal(dev, c.host_correct(seqs, quals))
    assert (dev[2] & 7 == 0).sum() > n // 2
    c.close(); t.close()


def test_gpu_fallback_forced(gpu_lib, g1_table, monkeypatch):
    """a device heap of 2 entries and a stack of 40: many reads go to the host instance, the output is the same"""
    t, (names, seqs, quals) = g1_table
    monkeypatch.setenv("BFCG_EC_HEAP", "2")
    monkeypatch.setenv("BFCG_EC_STACK", "40")
    o = gpu_lib.bfc_opt_init(); o.k = 31
    c = gpu_lib.GpuCorrector(t, o, max_pos=sum(len(s) + 1 for s in seqs), max_reads=len(seqs))
    dev = c.correct(seqs, quals)
    assert c.host_reads() > 0
    assert hashlib.md5(gpu_lib.format_ec(names, *dev, o)).hexdigest() == GOLD["g1"]["stdout_md5"]
    c.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gpu_random_options_equal_host(gpu_lib, seed, tmp_path):
    """seeded random k and options on ragged reads with Ns, IUPAC codes, lower case and FASTA / FASTQ batches: device == host"""
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
    t = g.export_table()
    g.close()
    o = gpu_lib.bfc_opt_init(); o.k = k
    o.min_cov = int(rng.integers(1, 5)); o.win_multi_ec = int(rng.integers(3, 15)); o.q = int(rng.integers(10, 40))
    o.max_heap = int(rng.integers(1, 12)); o.max_end_ext = int(rng.integers(1, 8)); o.max_path_diff = int(rng.integers(5, 20))
    c = gpu_lib.GpuCorrector(t, o, max_pos=len(st), max_reads=n)
    _equal(c.correct(seqs, quals), c.host_correct(seqs, quals))
    _equal(c.correct(seqs), c.host_correct(seqs))
    c.close(); t.close()


def test_dropin_gpu_ec(tmp_path):
    """`bfc -k31 -b26 g1.fq` with both phases on the GPU (BFC_GPU_EC=1): the reference's bytes and the GPU line; two emulated devices too"""
    _need(GPUTRIM)
    fq = str(tmp_path / "g1.fq")
    gen.fixture("g1").fastq(fq)
    for devices in (None, "0,0"):
        env = dict(os.environ, BFC_GPU_EC="1")
        if devices:
            env["BFC_GPU_DEVICES"] = devices
        r = subprocess.run([GPUTRIM, "-k", "31", "-b", "26", "-t", "4", fq], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        assert hashlib.md5(r.stdout).hexdigest() == GOLD["g1"]["stdout_md5"]
        assert b"error correction ran on the GPU" in r.stderr
    r = subprocess.run([GPUTRIM, "-k", "31", "-b", "26", "-t", "4", fq], capture_output=True, timeout=300)  # default: the reference's corrector
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == GOLD["g1"]["stdout_md5"]
    assert b"error correction ran on the GPU" not in r.stderr


def test_dropin_gpu_ec_ecoli30x(tmp_path):
    """E. coli 30x (920 000 reads of 150 bp, 1 % errors), -k31 -b30: the whole pipeline's stdout is the reference's"""
    _need(GPUTRIM)
    e = GOLD["ecoli30x"]
    fq = str(tmp_path / "ecoli.fq")
    gen.ReadSet(**e["gen"]).fastq_parallel(fq, threads=8)
    assert oracle.md5_file(fq) == e["fastq_md5"]
    env = dict(os.environ, BFC_GPU_EC="1")
    r = subprocess.run([GPUTRIM] + e["args"] + ["-t", "8", fq], capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert hashlib.md5(r.stdout).hexdigest() == e["stdout_md5"]
    assert b"error correction ran on the GPU" in r.stderr
