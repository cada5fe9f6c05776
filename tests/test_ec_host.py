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

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "ec_goldens.json")))
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


def write_reads(fn, seqs, quals=None):
    with open(fn, "wb") as f:
        for i, s in enumerate(seqs):
            if quals is None:
                f.write(b">r%d\n%s\n" % (i, s))
            else:
                f.write(b"@r%d c%d\n%s\n+\n%s\n" % (i, i, s, quals[i]))


def _genome(rng, G):
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, G))


def count_file(rng, genome, n, L=120, err=0.004):
    """reads from both strands at high coverage: the table the corrections are checked with"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    out = []
    for _ in range(n):
        p = int(rng.integers(0, len(genome) - L))
        s = bytearray(genome[p:p + L])
        for j in np.nonzero(rng.random(L) < err)[0]:
            s[j] = b"ACGT"[int(rng.integers(0, 4))]
        s = bytes(s)
        out.append(s.translate(comp)[::-1] if rng.random() < 0.5 else s)
    return out


def edge_reads(rng, genome, k):
    """every path of bfc_ec1: clean and erroneous reads, reads shorter than k, N-rich reads, N runs inside solid stretches, reads with no
    solid k-mer (errors every k/2 bases: the brute path), lower case and IUPAC codes, random reads"""
    G = len(genome)
    reads = []

    def pick(L):
        p = int(rng.integers(0, G - L))
        return bytearray(genome[p:p + L])
    for _ in range(60):                                         # sequencing errors, 0-6 per read, some close together
        s = pick(int(rng.integers(k + 5, 250)))
        for _ in range(int(rng.integers(0, 7))):
            s[int(rng.integers(0, len(s)))] = b"ACGT"[int(rng.integers(0, 4))]
        reads.append(s)
    for _ in range(10):
        reads.append(pick(int(rng.integers(1, k))))             # shorter than k
    for _ in range(10):                                         # N-rich
        s = pick(150)
        for j in rng.integers(0, 150, 12):
            s[j] = ord("N")
        reads.append(s)
    for _ in range(15):                                         # one N or a short N run inside
        s = pick(200)
        j = int(rng.integers(k, 200 - k))
        s[j:j + int(rng.integers(1, 4))] = b"N" * 3
        reads.append(s[:200])
    for _ in range(20):                                         # no solid k-mer: an error every k/2 bases
        s = pick(int(rng.integers(k + 2, 2 * k + 10)))
        for j in range(int(rng.integers(0, k // 2)), len(s), max(2, k // 2)):
            s[j] = b"ACGT"[(b"ACGT".index(s[j]) + 1) % 4]
        reads.append(s)
    for _ in range(10):                                         # lower case, IUPAC codes
        s = pick(180)
        s[int(rng.integers(0, 180))] = b"RYKMSWBDHVN"[int(rng.integers(0, 11))]
        if rng.random() < 0.5:
            s = bytearray(bytes(s).lower())
        else:
            s[10:60] = bytes(s[10:60]).lower()
        reads.append(s)
    for _ in range(5):
        reads.append(bytearray(b"ACGT"[c] for c in rng.integers(0, 4, 150)))
    return [bytes(s) for s in reads]


@pytest.fixture(scope="module")
def edge_env(tmp_path_factory):
    """one genome, one counting file, one dump per k, one file of edge reads per k"""
    d = tmp_path_factory.mktemp("ec_host")
    rng = np.random.default_rng(11)
    genome = _genome(rng, 4000)
    cnt = str(d / "count.fq")
    reads = count_file(rng, genome, 1500)
    write_reads(cnt, reads, [bytes(rng.integers(40, 74, len(s)).astype(np.uint8)) for s in reads])
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
