"""GPU tests (-m gpu) of creations that fail half way: every kind of device object gives back what it had made, leaves no stale HIP
error behind, and the device goes on working.

The failures are hipMalloc calls for more bytes than any device has (a 256 TiB count table, buffers for 2^50 positions): the runtime
refuses them by size with hipErrorOutOfMemory and starts nothing on the GPU.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from test_gpu_ec import _equal, _fastq_records
from test_kcov import KCOV, _summary, _unstream

pytestmark = pytest.mark.gpu

# a table of 8 << (l_pre + tab_cshift) = 256 TiB in one allocation (table_layout=1), made after the streams, the events, the record
# buffers of both levels, the filter and the one-pass buffers
BIG = dict(k=33, bf_shift=26, l_pre=20, table_layout=1, tab_cshift=25, max_batch_pos=1 << 24)
N_FAILS = 4
# What four failed creations may cost.  Not measured: the two level-1 record buffers alone are 2 x 2^24 x 12 bytes = 384 MiB per call, so
# four creations that kept them take more than 1.5 GiB; 256 MiB leaves room for the runtime's pools and other tenants' small allocations.
LEAK_BOUND = 256 << 20


def _hip():
    """the HIP runtime the library has already loaded (no second runtime, no torch context beside it)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("libbfc_gpu.so is loaded but no libamdhip64 is mapped")


def _free_bytes(hip):
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.fixture(scope="module")
def failed_creations(gpu_lib):
    """N_FAILS failed bfcg_create calls in this process and thread: (free bytes before, free bytes after, the messages)"""
    gpu_lib.GpuCounter(31, 20, max_batch_pos=1 << 16).close()  # the runtime is up and has its pools before the first reading
    hip = _hip()
    before = _free_bytes(hip)
    msgs = []
    for _ in range(N_FAILS):
        with pytest.raises(gpu_lib.BfcGpuError) as ei:
            gpu_lib.GpuCounter(**BIG)
        msgs.append(str(ei.value))
    return before, _free_bytes(hip), msgs


def test_failed_create_gives_its_memory_back(failed_creations):
    before, after, msgs = failed_creations
    assert all("hipMalloc" in m for m in msgs), msgs
    drop = before - after
    print("free device memory: %d -> %d bytes, drop %.1f MiB after %d failed creations" % (before, after, drop / 2.0 ** 20, N_FAILS))
    assert drop < LEAK_BOUND, "%d failed creations kept %.1f MiB of device memory" % (N_FAILS, drop / 2.0 ** 20)


def test_no_stale_error_after_failed_creations(gpu_lib, g1, failed_creations):
    """the same geometry with a table that fits counts g1 as the oracle does: a bail-out that left HIP's last error set would make the
    first check behind a kernel launch report that out-of-memory as its own"""
    rs, (seq, qual, off) = g1
    g = gpu_lib.GpuCounter(**dict(BIG, tab_cshift=0))
    g.count_host(gpu_lib.to_stream(seq, off), gpu_lib.to_stream(qual, off))
    oc = oracle.Counter(BIG["k"], BIG["bf_shift"])
    oc.count(seq, qual, off)
    st, ost = g.stats(), oc.stats()
    assert (st["n_kmers"], st["n_high"], st["n_seen"]) == (ost["n_kmers"], ost["n_high"], ost["n_seen"])
    t = g.export_table()
    assert t.count() == oc.table_count() == st["n_keys"]
    t.close(); g.close(); oc.close()


# ---- the satellites: trimmer, coverage pass, corrector

HUGE = 1 << 50  # positions: no device holds a buffer of a byte each


@pytest.fixture(scope="module")
def g1_k31(gpu_lib, g1, tmp_path_factory):
    """g1 counted with k = 31, -b26 (the geometry of KCOV's and the corrector's goldens): the counter, its streams, g1's reads as bytes"""
    from bfc_amd import gen
    rs, (seq, qual, off) = g1
    s, q = gpu_lib.to_stream(seq, off), gpu_lib.to_stream(qual, off)
    g = gpu_lib.GpuCounter(31, 26, max_batch_pos=len(s) + 64)
    g.count_host(s, q)
    fq = str(tmp_path_factory.mktemp("create_failure") / "g1.fq")
    gen.fixture("g1").fastq(fq)
    yield g, s, _fastq_records(fq)
    g.close()


def _trimmer_case(gpu_lib, g1, request):
    rs, (seq, qual, off) = g1
    n, k, b = 1000, 31, 20
    seq, qual, off = seq[:n * rs.L], qual[:n * rs.L], off[:n + 1]
    s_seq = gpu_lib.to_stream(seq, off)
    g = gpu_lib.GpuCounter(k, b, filter_mode=1, max_batch_pos=len(s_seq) + 64)
    g.count_host(s_seq, gpu_lib.to_stream(qual, off))
    bf = g.export_bloom(1, resident=True)  # the failed creation adopts the copy in HBM before its buffers do not fit
    g.close()
    with pytest.raises(gpu_lib.BfcGpuError, match="hipMalloc"):
        gpu_lib.GpuTrimmer(k, bf, max_pos=HUGE)
    tr = gpu_lib.GpuTrimmer(k, bf)
    assert not tr.adopted
    start, end = tr.trim(s_seq, off + np.arange(n + 1, dtype=np.uint64), 0.9)
    L = oracle.lib()
    oc = oracle.Counter(k, b, filter_mode=1)
    oc.count(seq, qual, off)
    obf = L.orc_state_bf_high(oc.st)
    kept = 0
    for r in range(n):  # tests/test_gpu_dropin.py: test_gpu_trim_pass_matches_reference
        rd = seq[int(off[r]):int(off[r + 1])]
        a, e = C.c_int(), C.c_int()
        if L.orc_trim_decide(L.orc_max_streak(k, obf, rd.ctypes.data, len(rd)), k, len(rd), 0.9, C.byref(a), C.byref(e)):
            assert (int(start[r]), int(end[r])) == (a.value, e.value), r
            kept += 1
        else:
            assert start[r] == -1, r
    assert kept > 0
    tr.close(); bf.close(); oc.close()


def _kcov_case(gpu_lib, g1, request):
    """the failed creation takes the table's copy out of the registry and frees it: whoever comes next uploads"""
    from bfc_amd.api import HostTable
    rs, (seq, qual, off) = g1
    g, s, _ = request.getfixturevalue("g1_k31")
    p = g.L.bfcg_export_table_resident(g.ctx)
    assert p, g.L.bfcg_last_error().decode()
    t = HostTable(p)
    with pytest.raises(gpu_lib.BfcGpuError, match="hipMalloc"):
        gpu_lib.GpuKcov(t, max_pos=HUGE)
    # (a coverage pass does not say whether it adopted; a corrector says it for the coverage pass it creates the same way)
    o = gpu_lib.bfc_opt_init(); o.k = 31
    c = gpu_lib.GpuCorrector(t, o)
    assert not c.adopted
    c.close()
    kc = gpu_lib.GpuKcov(t)
    e = KCOV[0]
    assert (e["k"], e["b"]) == (31, 26)
    vals = _unstream(kc.kcov(s, e["min_occ"]), off)
    assert [int(v) for v in vals[:int(off[1])][:48]] == e["read0_head"]
    got = _summary(vals)
    assert got == {k_: e[k_] for k_ in got}
    kc.close(); t.close()


def _corrector_case(gpu_lib, g1, request):
    g, s, (names, seqs, quals) = request.getfixturevalue("g1_k31")
    t = g.export_table()
    o = gpu_lib.bfc_opt_init(); o.k = 31
    with pytest.raises(gpu_lib.BfcGpuError, match="hipMalloc"):
        gpu_lib.GpuCorrector(t, o, max_pos=HUGE)
    c = gpu_lib.GpuCorrector(t, o)
    n = 2000
    _equal(c.correct(seqs[:n], quals[:n]), c.host_correct(seqs[:n], quals[:n]))  # tests/test_gpu_ec.py: device == host instance, read for read
    c.close(); t.close()


@pytest.mark.parametrize("case", [_trimmer_case, _kcov_case, _corrector_case], ids=["trimmer", "kcov", "corrector"])
def test_satellite_creation_fails_clean(gpu_lib, g1, request, case):
    """a creation that cannot get its buffers raises; the same object with the default capacity then works on one small batch"""
    case(gpu_lib, g1, request)
