"""`bfc -R` (refine_ec) on the host instance of the corrector (bfcg_ec1_host_refine: bfcg_ec1.h's RF instance, the code the device runs
too) and the ec:Z: parser (bfcg_ec_parse_stats) against the reference (-m "not gpu").

The reference is libbfcref_ec.so's own bfc_correct (correct.c:620) with refine_ec = 1, in a child process on a table bfc_ch_restore read
from a `bfc-ref -d` dump (as tests/test_ec_host.py).  Our side: tests/refine_inputs.refine -- worker_ec's skip and ori_st in stream
order, the corrector, bfc_ec_cb's output.  stdout must be byte-identical.  Quality bytes <= 33 (undefined in the reference) are kept out."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import refine_inputs as RI

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "ec_goldens.json")))
RGOLD = json.load(open(os.path.join(HERE, "golden", "ec_refine_goldens.json")))
BFC_REF = os.path.join(oracle.REF_DIR, "bfc-ref")
REF_EC = os.path.join(oracle.REF_DIR, "libbfcref_ec.so")
needs_ref = pytest.mark.skipif(not (os.path.exists(BFC_REF) and os.path.exists(REF_EC)),
                               reason="oracle/_ref/bfc-ref and libbfcref_ec.so not built (needs the reference sources)")

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
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, REF_EC, dump, fn, json.dumps(dict(opts, refine_ec=1))], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def ref_dump(fq, k, dump, b=24):
    r = subprocess.run([BFC_REF, "-t1", "-E", "-k", str(k), "-b", str(b), "-d", dump, fq], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]


def host_refine(dump, fn, opts):
    import bfc_amd
    t = bfc_amd.HostTable.restore(dump)
    o = bfc_amd.bfc_opt_init()
    for k, v in dict(opts, refine_ec=1).items():
        setattr(o, k, v)
    c = bfc_amd.GpuCorrector(t, o, gpu=False)
    out, a2 = RI.refine(c, *RI.read_records(open(fn, "rb").read()), o)
    t.close()
    return out, a2


# ------------------------------------------------------------------------------------------------ the parser

@pytest.mark.parametrize("comment,want", [
    ("ec:Z:0_3:60_1_12:4_0", (0, 1, 12, 4, 3, 60)),            # (ec_code, brute, n_ec, n_ec_high, n_absent, max_heap)
    ("ec:Z:0_3:9_0_2:1_3", (0, 0, 2, 1, 3, 9)),                 # rf_code in the tag is not read
    ("ec:Z:0_1:300_0_0:0_0", (0, 0, 0, 0, 1, 44)),              # max_heap: 8 bits
    ("ec:Z:0_1:306_0_0:0_0", (0, 0, 0, 0, 1, 50)),
    ("ec:Z:0_4194304:1_3_16384:16385_0", (0, 1, 0, 1, 0, 1)),   # n_absent 22 bits, brute 1, n_ec / n_ec_high 14
    ("ec:Z:8_5:7_1_2:3_0", (0, 1, 2, 3, 5, 7)),                 # ec_code 3 bits: 8 is 0 and the fields are parsed
    ("ec:Z:9_5:7_1_2:3_0", (1, 0, 0, 0, 0, 0)),                 # 9 is 1: nothing else
    ("ec:Z:3", (3, 0, 0, 0, 0, 0)),
    ("ec:Z:-1", (7, 0, 0, 0, 0, 0)),
    ("ec:Z:0", (0, 0, 0, 0, 0, 0)),                             # truncated: what is missing is 0 (the reference reads past the NUL)
    ("ec:Z:0_7", (0, 0, 0, 0, 7, 0)),
    ("ec:Z:0_7:", (0, 0, 0, 0, 7, 0)),
    ("ec:Z:", (0, 0, 0, 0, 0, 0)),
    ("ec:Z:0 12 13 1 4 5", (0, 1, 4, 5, 12, 13)),               # any separator byte: strtol(p + 1)
])
def test_parse_stats(gpu_lib, comment, want):
    a, a2 = gpu_lib.parse_ec_stats(comment)
    assert (a & 7, a >> 3 & 1, a >> 18, a >> 4 & 0x3fff, a2 >> 10, a2 & 0xff) == want
    assert a2 >> 8 & 3 == 1                                     # parse_stats sets rf_code 1


@pytest.mark.parametrize("comment", ["", "foo", "ec:z:0_1:2_0_0:0_0", " ec:Z:0", "EC:Z:0", "ec:Z"])
def test_parse_stats_not_ec(gpu_lib, comment):
    assert gpu_lib.parse_ec_stats(comment) is None


def test_refine_needs_a_refine_corrector(gpu_lib):
    """earlier stats are refused by a table-mode corrector, and the host instance of table mode refuses refine_ec"""
    t = gpu_lib.HostTable.init(21, 12)
    o = gpu_lib.bfc_opt_init(); o.k = 21
    c = gpu_lib.GpuCorrector(t, o, gpu=False)
    with pytest.raises(gpu_lib.BfcGpuError):
        c.host_correct([b"ACGT"], None, ori=(np.zeros(1, np.uint32), np.zeros(1, np.uint32)))
    import ctypes as C
    from bfc_amd import _lib
    o.refine_ec = 1
    a, a2 = C.c_uint32(), C.c_uint32()
    assert _lib.load().bfcg_ec1_host(t.ptr, C.byref(o), c.mode, C.create_string_buffer(b"ACGT"), None, C.byref(a), C.byref(a2)) != 0
    assert b"refine" in _lib.load().bfcg_last_error()
    t.close()


# ------------------------------------------------------------------------------------------------ against the reference

@pytest.fixture(scope="module")
def g1_inputs(tmp_path_factory):
    """g1, its first pass (`bfc-ref -k31 -b26 -t1`, the golden of ec_goldens.json), and the recipes' inputs (a)-(d)"""
    if not (os.path.exists(BFC_REF) and os.path.exists(REF_EC)):
        pytest.skip("oracle/_ref not built")
    from bfc_amd import gen
    d = tmp_path_factory.mktemp("refine")
    g1 = str(d / "g1.fq")
    gen.fixture("g1").fastq(g1)
    r = subprocess.run([BFC_REF, "-k31", "-b26", "-t1", g1], capture_output=True, timeout=300)
    assert r.returncode == 0 and hashlib.md5(r.stdout).hexdigest() == GOLD["g1"]["stdout_md5"]
    a = r.stdout
    files = {"a": a, "b": RI.recipe_b(a), "c": RI.recipe_c(a), "d": open(g1, "rb").read()}
    out = {}
    for name, data in files.items():
        fn = str(d / ("in_%s.fq" % name))
        open(fn, "wb").write(data)
        out[name] = fn
    out["c_fa"] = str(d / "in_c.fa")
    open(out["c_fa"], "wb").write(RI.recipe_fasta(files["c"]))
    return d, out


def _dump(d, fn, k):
    dump = str(d / ("%s.k%d.hash" % (os.path.basename(fn), k)))
    if not os.path.exists(dump):
        ref_dump(fn, k, dump)
    return dump


@needs_ref
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_goldens_are_the_references(g1_inputs, name):
    """the recipes make the files the goldens were recorded on: `bfc-ref -R -k31 -b26 -t1` gives the recorded md5"""
    _, files = g1_inputs
    r = subprocess.run([BFC_REF, "-R", "-k31", "-b26", "-t1", files[name]], capture_output=True, timeout=300)
    assert r.returncode == 0
    assert hashlib.md5(r.stdout).hexdigest() == RGOLD["g1"][name]["stdout_md5"]


@needs_ref
@pytest.mark.parametrize("k", [21, 31, 33, 55, 63])
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "c_fa"])
def test_host_refine_vs_reference(g1_inputs, name, k):
    d, files = g1_inputs
    fn = files[name]
    dump = _dump(d, fn, k)
    got, a2 = host_refine(dump, fn, {"k": k})
    assert got == ref_correct(dump, fn, {"k": k})
    if name in ("b", "d"):                                      # every read refined: both ends of correct.c:438-470 taken
        rf = set(int(v) for v in a2 >> 8 & 3)
        assert {2, 3} <= rf if name == "b" else 2 in rf, rf


@needs_ref
@pytest.mark.parametrize("opts", [{"discard": 1}, {"no_qual": 1}, {"discard": 1, "no_qual": 1}])
def test_host_refine_options_vs_reference(g1_inputs, opts):
    """(e): -D and -Q on the mixture"""
    d, files = g1_inputs
    opts = dict(opts, k=31)
    dump = _dump(d, files["c"], 31)
    assert host_refine(dump, files["c"], opts)[0] == ref_correct(dump, files["c"], opts)


def _genome(rng, G):
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, G))


@needs_ref
@pytest.mark.parametrize("seed", range(5))
def test_seeded_fuzz_vs_reference(tmp_path, seed):
    """ragged reads with errors and Ns, quality bytes 34..45 (bases read from 34..38), random ec:Z: comments and options"""
    rng = np.random.default_rng(500 + seed)
    k = int(rng.choice([21, 31, 33, 55, 63]))
    genome = _genome(rng, 5000)
    cnt = str(tmp_path / "count.fq")
    reads = []
    for _ in range(1500):
        p = int(rng.integers(0, len(genome) - 120))
        reads.append(genome[p:p + 120])
    open(cnt, "wb").write(b"".join(b"@c%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(reads)))
    dump = str(tmp_path / "t.hash")
    ref_dump(cnt, k, dump)
    names, comments, seqs, quals = [], [], [], []
    for i in range(300):
        L = int(rng.integers(1, 260))
        p = int(rng.integers(0, len(genome) - L))
        s = bytearray(genome[p:p + L])
        for j in rng.integers(0, L, int(rng.poisson(L * 0.015))):
            s[j] = b"ACGTN"[int(rng.integers(0, 5))]
        q = bytearray(rng.integers(39, 46, L).astype(np.uint8))
        for j in rng.integers(0, L, int(rng.poisson(L * 0.03))):
            q[j] = int(rng.integers(34, 39))
        u = rng.random()
        c = (None if u < 0.2 else b"x y" if u < 0.25 else b"ec:Z:%d" % int(rng.integers(1, 6)) if u < 0.35
             else b"ec:Z:0_%d:%d_%d_%d:%d_%d" % (int(rng.integers(0, 6)), int(rng.choice([0, 49, 50, 60, 300])), int(rng.integers(0, 2)),
                                                 int(rng.integers(0, 9)), int(rng.integers(0, 4)), int(rng.integers(0, 4))))
        names.append(b"r%d" % i); comments.append(c); seqs.append(bytes(s)); quals.append(bytes(q))
    fn = str(tmp_path / "r.fq")
    open(fn, "wb").write(RI.write_records(names, comments, seqs, quals))
    opts = {"k": k, "min_cov": int(rng.integers(1, 5)), "win_multi_ec": int(rng.integers(2, 16)), "q": int(rng.integers(0, 40)),
            "max_heap": int(rng.integers(1, 40)), "max_end_ext": int(rng.integers(0, 9)), "max_path_diff": int(rng.integers(1, 25)),
            "discard": int(rng.integers(0, 2)), "no_qual": int(rng.integers(0, 2))}
    assert host_refine(dump, fn, opts)[0] == ref_correct(dump, fn, opts)
