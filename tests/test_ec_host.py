"""Error correction's host instance (bfcg_ec1_host: bfcg_ec1.h, the code the device runs too) against the reference (-m "not gpu").

The reference is the corrector of oracle/_ref/: `bfc-ref` for the whole pipeline, and libbfcref_ec.so's own bfc_correct (correct.c:620),
called in a child process with any bfc_opt_t on a table that bfc_ch_restore read from a reference `-d` dump.  Both sides correct the same
file with the same table; stdout must be byte-identical."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from ec_corpus import KS, conditions, corpus, count_set, edge_reads, histogram, write_reads

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "ec_goldens.json")))
PATHS_GOLD = os.path.join(HERE, "golden", "ec_paths_goldens.json")  # read by its test: make_ec_paths_goldens.py imports this module to write it
BFC_REF = os.path.join(oracle.REF_DIR, "bfc-ref")
REF_EC = os.path.join(oracle.REF_DIR, "libbfcref_ec.so")
needs_ref = pytest.mark.skipif(not (os.path.exists(BFC_REF) and os.path.exists(REF_EC)),
                               reason="oracle/_ref/bfc-ref and libbfcref_ec.so not built (needs the reference sources)")

# the reference's bfc_correct in a fresh process: its stdout is the corrected file
_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from bfc_amd.api import bfc_opt_init
R = C.CDLL(sys.argv[2])
R.bfc_ch_restore.restype = C.c_void_p
R.bfc_ch_restore.argtypes = [C.c_char_p]
R.bfc_correct.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
o = bfc_opt_init()
for k, v in json.loads(sys.argv[5]).items():
    setattr(o, k, v)
ch = R.bfc_ch_restore(sys.argv[3].encode())
R.bfc_correct(sys.argv[4].encode(), C.byref(o), C.c_void_p(ch))
"""


def ref_correct(dump, fn, opts):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, REF_EC, dump, fn, json.dumps(opts)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def ref_dump(fq, k, dump, b=22):
    r = subprocess.run([BFC_REF, "-t1", "-E", "-k", str(k), "-b", str(b), "-d", dump, fq], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]


def read_records(fn):
    """FASTQ (4 lines a record) or FASTA (2 lines) as the tests write them: names (first word), sequences, qualities or None"""
    lines = open(fn, "rb").read().split(b"\n")
    step = 4 if lines[0].startswith(b"@") else 2
    names = [lines[i][1:].split()[0] for i in range(0, len(lines) - 1, step)]
    seqs = [lines[i + 1] for i in range(0, len(lines) - 1, step)]
    quals = [lines[i + 3] for i in range(0, len(lines) - 1, step)] if step == 4 else None
    return names, seqs, quals


def host_correct(dump, fn, opts):
    import bfc_amd
    t = bfc_amd.HostTable.restore(dump)
    o = bfc_amd.bfc_opt_init()
    for k, v in opts.items():
        setattr(o, k, v)
    c = bfc_amd.GpuCorrector(t, o, gpu=False)
    names, seqs, quals = read_records(fn)
    s, q, a, a2 = c.host_correct(seqs, quals)
    out = bfc_amd.format_ec(names, s, q, a, a2, o)
    t.close()
    return out, a, a2


@pytest.fixture(scope="module")
def edge_env(tmp_path_factory):
    """one genome, one counting file, one dump per k, one file of edge reads per k"""
    d = tmp_path_factory.mktemp("ec_host")
    rng, genome, reads, quals = count_set()
    cnt = str(d / "count.fq")
    write_reads(cnt, reads, quals)
    return d, rng, genome, cnt


def _edge_files(edge_env, k, fasta=False):
    d, _, genome, cnt = edge_env
    dump = str(d / ("k%d.hash" % k))
    if not os.path.exists(dump):
        ref_dump(cnt, k, dump)
    rng = np.random.default_rng(100 + k)
    seqs = edge_reads(rng, genome, k)
    quals = [bytes(rng.integers(33, 74, len(s)).astype(np.uint8)) for s in seqs]
    fn = str(d / ("edge_k%d%s" % (k, ".fa" if fasta else ".fq")))
    write_reads(fn, seqs, None if fasta else quals)
    return dump, fn


@needs_ref
def test_g1_whole_file_golden(g1, tmp_path):
    """table of `bfc-ref -t1 -E -k31 -b26 -d` on g1, every read through bfcg_ec1_host: `bfc -k31 -b26 -t1 g1.fq`'s md5"""
    from bfc_amd import gen
    fq, dump = str(tmp_path / "g1.fq"), str(tmp_path / "g1.hash")
    gen.fixture("g1").fastq(fq)
    ref_dump(fq, 31, dump, b=26)
    out, aux, aux2 = host_correct(dump, fq, {"k": 31})
    assert hashlib.md5(out).hexdigest() == GOLD["g1"]["stdout_md5"]
    assert (aux & 7 == 0).sum() > 6000 and (aux >> 18).sum() > 1000


@needs_ref
@pytest.mark.parametrize("k", [21, 31, 33, 47, 55, 63])
def test_edge_reads_vs_reference(edge_env, k):
    dump, fn = _edge_files(edge_env, k)
    want = ref_correct(dump, fn, {"k": k})
    got, aux, aux2 = host_correct(dump, fn, {"k": k})
    assert got == want
    codes = set(int(c) for c in aux & 7)
    assert {0, 2, 3} <= codes, codes                            # corrected, MANY_N, NO_SOLID
    assert (aux >> 3 & 1).any()                                 # the brute path took a read
    assert (aux >> 18).sum() > 20                               # bases changed


@pytest.fixture(scope="module")
def corpus_tables(tmp_path_factory):
    """the counting file's table per k without the reference: counted by the CPU restatement (oracle.Counter, held to the reference's
    table by tests/test_oracle.py), dumped in bfc_ch_dump's format"""
    d = tmp_path_factory.mktemp("ec_paths")
    _, genome, reads, quals = count_set()
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in reads])
    seq, qual = np.frombuffer(b"".join(reads), dtype=np.uint8), np.frombuffer(b"".join(quals), dtype=np.uint8)
    made = {}

    def get(k):
        if k not in made:
            c = oracle.Counter(k, 22)
            c.count(seq, qual, off)
            made[k] = str(d / ("k%d.hash" % k))
            c.dump(made[k])
            c.close()
        return made[k]
    return d, genome, get


@pytest.mark.parametrize("fmt", ["fq", "fa"])
@pytest.mark.parametrize("k", KS)
def test_corpus_paths_golden(corpus_tables, edge_env, k, fmt):
    """edge_reads + exit_reads (ec_corpus.corpus) through the host instance: the bytes of the reference's bfc_correct as recorded in
    tests/golden/ec_paths_goldens.json, its reads per ec_code and its brute count; the corpus reaches ec_code 0, 2, 3, 4 and 5 and the
    brute path (ec_corpus.conditions).  Where oracle/_ref is built, the live reference on its own table gives the same bytes."""
    d, genome, table = corpus_tables
    g = json.load(open(PATHS_GOLD))["k%d_%s" % (k, fmt)]
    seqs, quals = corpus(genome, k)
    fn = str(d / ("corpus_k%d.%s" % (k, fmt)))
    write_reads(fn, seqs, quals if fmt == "fq" else None)
    got, aux, aux2 = host_correct(table(k), fn, {"k": k})
    hist, brute = histogram(aux)
    print("k %d %s: ec_code histogram %s, brute %d" % (k, fmt, hist, brute))
    assert hashlib.md5(got).hexdigest() == g["stdout_md5"]
    conditions(aux)
    assert len(seqs) == g["n_reads"] and hist == g["ec_code_hist"]
    assert int(((aux >> 3 & 1 == 1) & (aux & 7 == 0)).sum()) == g["brute_code0"]
    if os.path.exists(BFC_REF) and os.path.exists(REF_EC):
        dump = str(edge_env[0] / ("k%d.hash" % k))
        if not os.path.exists(dump):
            ref_dump(edge_env[3], k, dump)
        assert got == ref_correct(dump, fn, {"k": k})


@needs_ref
def test_edge_reads_fasta(edge_env):
    dump, fn = _edge_files(edge_env, 31, fasta=True)
    assert host_correct(dump, fn, {"k": 31})[0] == ref_correct(dump, fn, {"k": 31})


@needs_ref
@pytest.mark.parametrize("opts", [{"discard": 1}, {"no_qual": 1}, {"min_cov": 2}, {"min_cov": 5}, {"win_multi_ec": 4}, {"win_multi_ec": 20},
                                  {"q": 10}, {"q": 35}, {"max_heap": 1}, {"max_heap": 2}, {"max_heap": 3}, {"max_heap": 4},
                                  {"max_end_ext": 1, "max_path_diff": 3}, {"w_ec": 2, "w_ec_high": 3, "w_absent": 1, "w_absent_high": 2}],
                         ids=lambda o: "_".join("%s%d" % kv for kv in o.items()))
def test_options_vs_reference(edge_env, opts):
    opts = dict(opts, k=33)
    dump, fn = _edge_files(edge_env, 33)
    assert host_correct(dump, fn, opts)[0] == ref_correct(dump, fn, opts)


@needs_ref
@pytest.mark.parametrize("seed", range(6))
def test_seeded_fuzz_vs_reference(edge_env, tmp_path, seed):
    """random read sets (ragged, errors, Ns, case) and random options against the reference's bfc_correct"""
    d, _, genome, cnt = edge_env
    rng = np.random.default_rng(1000 + seed)
    k = int(rng.choice([21, 25, 31, 33, 41, 47, 55, 63]))
    dump = str(tmp_path / "t.hash")
    ref_dump(cnt, k, dump)
    seqs = edge_reads(rng, genome, k)
    rng.shuffle(seqs)
    quals = [bytes(rng.integers(33, 80, len(s)).astype(np.uint8)) for s in seqs]
    fn = str(tmp_path / "r.fq")
    write_reads(fn, seqs, quals)
    opts = {"k": k, "min_cov": int(rng.integers(1, 6)), "win_multi_ec": int(rng.integers(2, 16)), "q": int(rng.integers(5, 45)),
            "max_heap": int(rng.integers(1, 40)), "max_end_ext": int(rng.integers(0, 9)), "max_path_diff": int(rng.integers(1, 25)),
            "w_ec": int(rng.integers(1, 4)), "w_ec_high": int(rng.integers(1, 9)), "w_absent": int(rng.integers(1, 5)),
            "w_absent_high": int(rng.integers(0, 3)), "discard": int(rng.integers(0, 2)), "no_qual": int(rng.integers(0, 2))}
    assert host_correct(dump, fn, opts)[0] == ref_correct(dump, fn, opts)
