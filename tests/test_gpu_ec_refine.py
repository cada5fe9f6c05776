"""GPU tests (-m gpu) of `bfc -R` (refine_ec) on the device: bfcg_ec_batch_refine read for read equal to the host instance of the same code
(bfcg_ec1_host_refine, held to the reference by tests/test_ec_refine_host.py), and the whole pipeline through the drop-in binary and through
the library alone against the reference's md5s (tests/golden/ec_refine_goldens.json; inputs made by tests/refine_inputs.py)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import refine_inputs as RI
from bfc_amd import gen

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = json.load(open(os.path.join(HERE, "golden", "ec_goldens.json")))
RGOLD = json.load(open(os.path.join(HERE, "golden", "ec_refine_goldens.json")))
GPUTRIM = os.path.join(oracle.REF_DIR, "bfc-dropin-gputrim")
GPU_LINE = b"error correction ran on the GPU"


def _need(path):
    if not os.path.exists(path):
        pytest.skip("%s not built (make -C oracle where the reference is present)" % path)


def _run(args, env=None, timeout=300):
    r = subprocess.run([GPUTRIM] + args, capture_output=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """g1's first pass on the GPU (the reference's bytes: ec_goldens.json) and the recipes' inputs (a)-(d) of ec_refine_goldens.json"""
    _need(GPUTRIM)
    d = tmp_path_factory.mktemp("refine_gpu")
    g1 = str(d / "g1.fq")
    gen.fixture("g1").fastq(g1)
    a = _run(["-k31", "-b26", "-t1", g1], env={"BFC_GPU_EC": "1"}).stdout
    assert hashlib.md5(a).hexdigest() == GOLD["g1"]["stdout_md5"]
    files = {}
    for name, data in {"a": a, "b": RI.recipe_b(a), "c": RI.recipe_c(a), "d": open(g1, "rb").read()}.items():
        files[name] = str(d / ("in_%s.fq" % name))
        open(files[name], "wb").write(data)
    return d, files


def _table(gpu_lib, seqs, quals, k=31, b=26):
    """the table `bfc -k31 -b26` counts on these reads (the GPU counter is bit-identical to the reference's: test_gpu_parity)"""
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    s = gpu_lib.to_stream(np.frombuffer(b"".join(seqs), dtype=np.uint8), off)
    q = gpu_lib.to_stream(np.frombuffer(b"".join(quals), dtype=np.uint8), off)
    g = gpu_lib.GpuCounter(k, b, max_batch_pos=len(s) + 64)
    g.count_host(s, q)
    t = g.export_table()
    g.close()
    return t


def _equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert x == y


def _corrector(gpu_lib, t, seqs, **kw):
    o = gpu_lib.bfc_opt_init(); o.k = t.k; o.refine_ec = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return o, gpu_lib.GpuCorrector(t, o, max_pos=sum(len(s) + 1 for s in seqs), max_reads=len(seqs))


@pytest.mark.parametrize("name", ["b", "c"])
def test_gpu_refine_equals_host_and_golden(gpu_lib, inputs, name):
    """every read of (b) / (c) through the device and the host instance with its earlier stats; the device's whole output is the
    reference's `bfc -R` (same table: counted on the file itself).  FASTA: the same reads without quality strings, device == host."""
    _, files = inputs
    names, comments, seqs, quals = RI.read_records(open(files[name], "rb").read())
    t = _table(gpu_lib, seqs, quals)
    o, c = _corrector(gpu_lib, t, seqs)
    rng = np.random.default_rng(3)
    ori = (rng.integers(0, 1 << 32, len(seqs), dtype=np.uint64).astype(np.uint32) & np.uint32(0xfffffcf8),
           rng.integers(0, 1 << 32, len(seqs), dtype=np.uint64).astype(np.uint32))
    ori[1][::3] &= np.uint32(0x3ff)                             # small n_absent: rf 2 and 3 both
    dev = c.correct(seqs, quals, ori=ori)
    _equal(dev, c.host_correct(seqs, quals, ori=ori))
    assert {2, 3} <= set(int(v) for v in dev[3] >> 8 & 3)
    assert c.last_ms() > 0
    out, _ = RI.refine(c, names, comments, seqs, quals, o, gpu=True)
    assert hashlib.md5(out).hexdigest() == RGOLD["g1"][name]["stdout_md5"]
    _equal(c.correct(seqs, None, ori=ori), c.host_correct(seqs, None, ori=ori))
    c.close(); t.close()


def test_gpu_refine_fallback_forced(gpu_lib, inputs, monkeypatch):
    """a device heap of 2 entries and a stack of 40: many reads go to the host instance with their stats, the output is the same"""
    _, files = inputs
    monkeypatch.setenv("BFCG_EC_HEAP", "2")
    monkeypatch.setenv("BFCG_EC_STACK", "40")
    names, comments, seqs, quals = RI.read_records(open(files["c"], "rb").read())
    t = _table(gpu_lib, seqs, quals)
    o, c = _corrector(gpu_lib, t, seqs)
    out, _ = RI.refine(c, names, comments, seqs, quals, o, gpu=True)
    assert c.host_reads() > 0
    assert hashlib.md5(out).hexdigest() == RGOLD["g1"]["c"]["stdout_md5"]
    c.close(); t.close()


@pytest.mark.parametrize("seed", [1, 2])
def test_gpu_refine_random_equals_host(gpu_lib, seed):
    """seeded k, options and reads (ragged, errors, Ns, bases in quality bytes 34..38, '!' / '~' bytes) with random earlier stats"""
    rng = np.random.default_rng(40 + seed)
    k = int(rng.choice([21, 31, 33, 55, 63]))
    genome = rng.integers(0, 4, 6000)
    seqs, quals = [], []
    for _ in range(1500):
        L = int(rng.integers(1, 300))
        p = int(rng.integers(0, 6000 - 300))
        s = bytearray(b"ACGT"[c] for c in genome[p:p + L])
        for _ in range(int(rng.poisson(L * 0.01))):
            s[int(rng.integers(0, L))] = b"ACGTN"[int(rng.integers(0, 5))]
        q = bytearray(rng.integers(39, 75, L).astype(np.uint8))
        for j in rng.integers(0, L, int(rng.poisson(L * 0.03))):
            q[j] = int(rng.choice([33, 34, 35, 36, 37, 38, 126]))
        seqs.append(bytes(s)); quals.append(bytes(q))
    t = _table(gpu_lib, seqs, [bytes(b"I" * len(s)) for s in seqs], k=k, b=22)
    o, c = _corrector(gpu_lib, t, seqs, min_cov=int(rng.integers(1, 5)), win_multi_ec=int(rng.integers(3, 15)), q=int(rng.integers(0, 40)),
                      max_heap=int(rng.integers(1, 12)), max_end_ext=int(rng.integers(1, 8)), max_path_diff=int(rng.integers(5, 20)))
    n = len(seqs)
    ori = (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0xfffffcf8),
           rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0x3ff))
    _equal(c.correct(seqs, quals, ori=ori), c.host_correct(seqs, quals, ori=ori))
    _equal(c.correct(seqs, ori=ori), c.host_correct(seqs, ori=ori))
    c.close(); t.close()


@pytest.mark.parametrize("name,extra", [("a", []), ("b", []), ("c", []), ("d", []), ("c_D", ["-D"]), ("c_Q", ["-Q"])])
def test_dropin_refine_gpu(inputs, name, extra):
    """`bfc -R -k31 -b26` with BFC_GPU_EC=1: the reference's bytes and the GPU line with the refine counts; two emulated devices; small
    batches (-L: the earlier stats carry across batches)"""
    _, files = inputs
    fn = files[name[0]]
    want = RGOLD["g1"][name]["stdout_md5"]
    for env, more in (({"BFC_GPU_EC": "1"}, []), ({"BFC_GPU_EC": "1", "BFC_GPU_DEVICES": "0,0"}, []), ({"BFC_GPU_EC": "1"}, ["-L", "40000"])):
        r = _run(["-R", "-k31", "-b26", "-t1"] + extra + more + [fn], env=env)
        assert hashlib.md5(r.stdout).hexdigest() == want, (env, more)
        assert GPU_LINE in r.stderr and b"reads refined" in r.stderr
        if more:
            assert r.stderr.count(b"[M::bfc_ec_cb] read ") > 10


def test_dropin_refine_default_is_reference(inputs):
    """without BFC_GPU_EC a binary that links the reference's corrector keeps it for -R"""
    _, files = inputs
    r = _run(["-R", "-k31", "-b26", "-t1", files["c"]])
    assert hashlib.md5(r.stdout).hexdigest() == RGOLD["g1"]["c"]["stdout_md5"]
    assert GPU_LINE not in r.stderr


_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from bfc_amd import _lib
from bfc_amd.api import bfc_opt_init
L = C.CDLL(_lib.SO)
L.bfc_ch_restore.restype = C.c_void_p
L.bfc_ch_restore.argtypes = [C.c_char_p]
L.bfc_correct.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p]
o = bfc_opt_init()
o.k = 31; o.refine_ec = 1
ch = L.bfc_ch_restore(sys.argv[2].encode())
L.bfc_correct(sys.argv[3].encode(), C.byref(o), C.c_void_p(ch))
"""


def test_library_alone_refine(gpu_lib, inputs):
    """libbfc_gpu.so's bfc_correct with refine_ec = 1 and no bfc_correct_cpu linked: the GPU path, the reference's bytes"""
    d, files = inputs
    names, comments, seqs, quals = RI.read_records(open(files["b"], "rb").read())
    t = _table(gpu_lib, seqs, quals)
    dump = str(d / "b.hash")
    t.dump(dump)
    t.close()
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, dump, files["b"]], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-1500:]
    assert hashlib.md5(r.stdout).hexdigest() == RGOLD["g1"]["b"]["stdout_md5"]
    assert GPU_LINE in r.stderr


def test_dropin_refine_gpu_ecoli30x(tmp_path):
    """E. coli 30x: the first pass on the GPU, every ec:Z:0 comment's max_heap set to 60, `-R` on the GPU: the reference's md5"""
    _need(GPUTRIM)
    e, g = GOLD["ecoli30x"], RGOLD["ecoli30x"]
    fq = str(tmp_path / "ecoli.fq")
    gen.ReadSet(**e["gen"]).fastq_parallel(fq, threads=8)
    r = _run(e["args"] + ["-t", "8", fq], env={"BFC_GPU_EC": "1"})
    assert hashlib.md5(r.stdout).hexdigest() == e["stdout_md5"]
    os.unlink(fq)
    fb = str(tmp_path / "in_b.fq")
    open(fb, "wb").write(RI.rewrite_all_refined(r.stdout))
    del r
    assert oracle.md5_file(fb) == g["input_md5"]
    r = _run(["-R"] + e["args"] + ["-t", "8", fb], env={"BFC_GPU_EC": "1"})
    assert hashlib.md5(r.stdout).hexdigest() == g["stdout_md5"]
    assert GPU_LINE in r.stderr and b"reads refined" in r.stderr
