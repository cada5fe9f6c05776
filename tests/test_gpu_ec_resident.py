"""GPU tests (-m gpu) of the count table that bfc_count leaves resident in HBM (bfcg_export_table_resident) and the corrector adopts
(bfcg_kcov_create behind bfcg_ec_create): the first corrector on the returned table takes the copy instead of uploading, a second one
uploads, a host insert or BFC_GPU_NO_RESIDENT=1 makes everyone upload -- and the output is the host instance's (bfcg_ec1_host) on that
table, or the reference's bytes (tests/golden/ec_goldens.json), every time."""
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
N = 2000                                                         # reads of g1 each corrector is given


def _equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert x == y


def _opt(gpu_lib):
    o = gpu_lib.bfc_opt_init(); o.k = 31; o.bf_shift = 26
    return o


@pytest.fixture(scope="module")
def g1_fq(tmp_path_factory):
    fq = str(tmp_path_factory.mktemp("ec_resident") / "g1.fq")
    gen.fixture("g1").fastq(fq)
    lines = open(fq, "rb").read().split(b"\n")
    return fq, [lines[i] for i in range(1, len(lines) - 1, 4)][:N], [lines[i] for i in range(3, len(lines) - 1, 4)][:N]


def _corrector(gpu_lib, t, seqs):
    return gpu_lib.GpuCorrector(t, _opt(gpu_lib), max_pos=sum(len(s) + 1 for s in seqs), max_reads=len(seqs))


def test_first_corrector_adopts_second_uploads(gpu_lib, g1_fq):
    fq, seqs, quals = g1_fq
    t = gpu_lib.bfc_count(fq, _opt(gpu_lib))
    c1 = _corrector(gpu_lib, t, seqs)
    assert c1.adopted and c1.retry_reads() == 0
    want = c1.host_correct(seqs, quals)
    _equal(c1.correct(seqs, quals), want)
    c2 = _corrector(gpu_lib, t, seqs)                             # the first taker owns the copy
    assert not c2.adopted
    _equal(c2.correct(seqs, quals), want)
    c1.close(); c2.close(); t.close()


def test_host_insert_drops_the_copy(gpu_lib, g1_fq):
    """the k-mers of a read that is not in g1, inserted on the host six times each: a corrector made afterwards uploads the table it is
    given, and corrects that read with an error in it as the host instance on the changed table does (and not as before the inserts)"""
    fq, seqs, quals = g1_fq
    t = gpu_lib.bfc_count(fq, _opt(gpu_lib))
    rng = np.random.default_rng(5)
    read = bytes(b"ACGT"[c] for c in rng.integers(0, 4, 150))
    bad = bytearray(read); bad[75] = ord("A") if read[75] != ord("A") else ord("C")
    rs, rq = seqs[:50] + [bytes(bad)], quals[:50] + [b"I" * 75 + b"#" + b"I" * 74]
    twin = gpu_lib.GpuCorrector(t, _opt(gpu_lib), gpu=False)
    before = twin.host_correct(rs, rq)
    h = gpu_lib.GpuCounter(31, 26, max_batch_pos=1 << 12)
    y = h.hash_positions(np.frombuffer(read + b"\n", dtype=np.uint8))
    h.close()
    ends = y[(y[:, 2] & 1) == 1]
    assert len(ends) == 150 - 31 + 1
    for y0, y1, _ in ends:
        for _ in range(6):
            t.insert(int(y0), int(y1), 1)
    c = _corrector(gpu_lib, t, rs)
    assert not c.adopted
    after = c.host_correct(rs, rq)
    assert after[0][-1].upper() == read and before[0][-1].upper() != read   # the inserts decide this read's correction (lower case: corrected)
    _equal(c.correct(rs, rq), after)
    c.close(); t.close()


def test_opt_out(gpu_lib, g1_fq, monkeypatch):
    fq, seqs, quals = g1_fq
    monkeypatch.setenv("BFC_GPU_NO_RESIDENT", "1")
    t = gpu_lib.bfc_count(fq, _opt(gpu_lib))
    c = _corrector(gpu_lib, t, seqs)
    assert not c.adopted
    _equal(c.correct(seqs, quals), c.host_correct(seqs, quals))
    c.close(); t.close()


def test_dropin_adopts_the_resident_table(tmp_path, g1_fq):
    """`bfc -k31 -b26 g1.fq` with both phases on the GPU: the corrector finds the table in HBM, or uploads it when told to; same bytes"""
    if not os.path.exists(GPUTRIM):
        pytest.skip("%s not built (make -C oracle where the reference is present)" % GPUTRIM)
    fq = g1_fq[0]
    for no_resident, say in ((None, b"count table found in HBM"), ("1", b"count table uploaded")):
        env = dict(os.environ, BFC_GPU_EC="1")
        env.pop("BFC_GPU_NO_RESIDENT", None)
        if no_resident:
            env["BFC_GPU_NO_RESIDENT"] = no_resident
        r = subprocess.run([GPUTRIM, "-k", "31", "-b", "26", "-t", "4", fq], capture_output=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr.decode()[-1500:]
        assert hashlib.md5(r.stdout).hexdigest() == GOLD["g1"]["stdout_md5"]
        line = [ln for ln in r.stderr.split(b"\n") if b"error correction ran on the GPU (" in ln]
        assert len(line) == 1 and say in line[0], r.stderr.decode()[-1500:]
