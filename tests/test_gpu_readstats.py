"""GPU tests (-m gpu) of the per-read statistics (bfcg_kmers_read_stats, bfc_amd/csrc/bfcg_readstats.hip) through GpuKmers.read_stats:
the hand-made stream of test_readstats_host.py against the host twin on every form of the table and against the numpy reduction of
GpuKmers.profile, the read counts around a workgroup's seams, the stream given on the device, the refusals, and the command-line tool
`python -m bfc_amd.readstats`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_kmers import _count, _g1
from test_readstats_host import L1, MIN_COVS, damaged, hand_case, np_stats, to_stream_off

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = dict(segments=dict(table_layout=0), host_layout=dict(table_layout=1), uploaded={})


def _g1_stream(gpu_lib, n):
    """the first n reads of g1 as a stream with its offsets"""
    seq, qual, off = _g1()
    L = int(off[1])
    return gpu_lib.to_stream(seq[:n * L], off[:n + 1]), np.arange(n + 1, dtype=np.uint64) * np.uint64(L + 1)


@pytest.mark.parametrize("case", list(LAYOUTS))
@pytest.mark.parametrize("k", [21, 33, 51])
def test_equals_host_twin(gpu_lib, k, case):
    """the hand-made stream (reads of 0, 1, k - 1, k, k + 1 bases, of 63 .. 129 k-mers, of 20 001 bases, with N, lower case, two equally
    long runs): read_stats == HostTable.read_stats on the exported table, word for word, for min_cov 1, 3, 255 -- on a context whose
    table is in region-owned segments, in the host's layout, and on the exported table uploaded again"""
    stream, off, _, twin = hand_case(gpu_lib, k)
    g = _count(gpu_lib, k, **LAYOUTS[case])
    g.sync()
    t = g.export_table() if case == "uploaded" else None
    km = gpu_lib.GpuKmers(t if t is not None else g)
    got = {mc: km.read_stats(stream, off, mc) for mc in MIN_COVS}
    assert km.last_ms() > 0
    km.close()
    if t is None:
        t = g.export_table()
    for mc in MIN_COVS:
        want = t.read_stats(stream, off, mc)
        assert got[mc].dtype == np.int32 and got[mc].shape == want.shape == (len(off) - 1, 8)
        assert np.array_equal(got[mc], want), (mc, np.flatnonzero((got[mc] != want).any(axis=1))[:10])
    d = (L1 - 1) // 2
    assert tuple(got[1][twin, 5:]) == (d - k + 1, d + 1, L1) and (got[3][:, 2] > 0).any() and (got[1][:, 0] > 19000).any()
    t.close(); g.close()


@pytest.mark.parametrize("k", [21, 33, 51])
def test_equals_reduced_profile(gpu_lib, k):
    """the two GPU paths agree: read_stats == the numpy reduction per read of GpuKmers.profile of the same stream"""
    stream, off, _, _ = hand_case(gpu_lib, k)
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    prof = km.profile(stream)
    for mc in MIN_COVS:
        got, want = km.read_stats(stream, off, mc), np_stats(prof, off, k, mc)
        assert np.array_equal(got, want), (mc, np.flatnonzero((got != want).any(axis=1))[:10])
    assert np.array_equal(km.profile(stream), prof)   # the profile's own call is as it was
    km.close(); g.close()


def test_read_count_seams(gpu_lib):
    """the first n reads of g1 for n = 0, 1, 3, 4, 5, 255, 256, 257 (the workgroup seams of any number of waves per workgroup that
    divides 256): each result is the head of the answer for 1000 reads, on one object whose buffers grow and are used again"""
    k = 33
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    full = km.read_stats(*_g1_stream(gpu_lib, 1000))
    t = g.export_table()
    assert np.array_equal(full, t.read_stats(*_g1_stream(gpu_lib, 1000)))
    for n in (257, 0, 1, 3, 4, 5, 255, 256, 257):
        got = km.read_stats(*_g1_stream(gpu_lib, n))
        assert got.shape == (n, 8) and np.array_equal(got, full[:n]), n
        assert (km.last_ms() > 0) == (n > 0)
    t.close(); km.close(); g.close()


def test_stream_on_device(gpu_lib):
    """the stream staged on the device (bfcg_dev_alloc / bfcg_h2d) and given as d_seq: the same words"""
    k = 33
    stream, off, _, _ = hand_case(gpu_lib, k)
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    want = km.read_stats(stream, off)
    d = g.dev_alloc(len(stream))
    g.h2d(d, stream)
    assert np.array_equal(km.read_stats(None, off, d_seq=d), want) and (want[:, 5] > 0).any()
    g.dev_free(d)
    km.close(); g.close()


def test_refusals(gpu_lib):
    """min_cov outside [1, 255], offsets that do not ascend, off[n_reads] != n_pos, a read of 2^24 positions, both or none of h_seq /
    d_seq: -1, a message that names the read, out untouched; the next good call on the same object works"""
    k = 21
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    L = km.L
    stream, off = _g1_stream(gpu_lib, 3)
    out = np.full((3, 8), 77, dtype=np.int32)
    call = lambda h, d, n_pos, o, n, mc: L.bfcg_kmers_read_stats(km.t, h, d, n_pos, o.ctypes.data, n, mc, out.ctypes.data)  # noqa: E731
    h = stream.ctypes.data
    for mc in (0, 256):
        assert call(h, None, len(stream), off, 3, mc) == -1 and b"min_cov" in L.bfcg_last_error()
    bad = off.copy(); bad[2] = bad[1]
    assert call(h, None, len(stream), bad, 3, 3) == -1 and b"read 1:" in L.bfcg_last_error()
    assert call(h, None, len(stream) - 1, off, 3, 3) == -1 and b"read 2, the last" in L.bfcg_last_error()
    big = np.array([0, 151, 151 + (1 << 24) + 1], dtype=np.uint64)
    assert call(h, None, int(big[2]), big, 2, 3) == -1 and b"read 1 has 16777216 positions" in L.bfcg_last_error()
    assert call(None, None, len(stream), off, 3, 3) == -1 and b"exactly one" in L.bfcg_last_error()
    assert call(h, h, len(stream), off, 3, 3) == -1 and b"exactly one" in L.bfcg_last_error()
    assert (out == 77).all()
    with pytest.raises(gpu_lib.BfcGpuError, match="min_cov 0 is outside"):
        km.read_stats(stream, off, 0)
    t = g.export_table()
    assert call(h, None, len(stream), off, 3, 3) == 0 and np.array_equal(out, t.read_stats(stream, off, 3)) and (out[:, 0] > 100).all()
    t.close(); km.close(); g.close()


N_TOOL, K_TOOL = 2000, 33


@pytest.fixture(scope="module")
def tool_case(gpu_lib, tmp_path_factory):
    """a dump of g1 at k = 33, a FASTQ of its first 2000 reads -- every 100th damaged near its head, every 150th in the middle -- and
    the twin's words for them"""
    seq, qual, off = _g1()
    Lr = int(off[1])
    g = _count(gpu_lib, K_TOOL)
    t = g.export_table()
    d = tmp_path_factory.mktemp("readstats")
    fn, fq = str(d / "g1.hash"), str(d / "reads.fq")
    assert t.dump(fn) == 0
    recs = []
    for r in range(N_TOOL):
        s, q = seq[r * Lr:(r + 1) * Lr].tobytes(), qual[r * Lr:(r + 1) * Lr].tobytes()
        if b"N" not in s.upper():
            s = damaged(s, 4) if r % 100 == 0 else damaged(s, 75) if r % 150 == 0 else s
        recs.append((b"read%d" % r, s, q))
    with open(fq, "wb") as f:
        f.write(b"".join(b"@" + n + b" a comment\n" + s + b"\n+\n" + q + b"\n" for n, s, q in recs))
    words = {mc: t.read_stats(*to_stream_off([s for _, s, _ in recs]), mc) for mc in (3, 2)}
    t.close(); g.close()
    return fn, fq, recs, words


def _tool(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "bfc_amd.readstats", *args], capture_output=True, cwd=ROOT, timeout=300, input=stdin)


def test_tool_stats(gpu_lib, tool_case):
    """python -m bfc_amd.readstats in a fresh process: every record's name, a tab, and the twin's words as bfcg_read_stats_format
    prints them; -c is min_cov; no arguments: the usage and status 1"""
    fn, fq, recs, words = tool_case
    for args, mc in (((), 3), (("-c", "2"), 2)):
        lines = gpu_lib.format_read_stats(words[mc]).split(b"\n")
        want = b"".join(n + b"\t" + ln + b"\n" for (n, _, _), ln in zip(recs, lines))
        r = _tool(*args, fn, fq) if mc == 3 else _tool(*args, fn, "-", stdin=open(fq, "rb").read())
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == want and r.stdout.count(b"\n") == N_TOOL
    assert _tool().returncode == 1


def test_tool_trim(gpu_lib, tool_case):
    """-t: the records cut to [start, end), qualities too, kept under correct.c:557 -- streak > 0 and (streak + k) / l_seq > min_frac --
    computed here from the twin's words; -f is min_frac"""
    fn, fq, recs, words = tool_case
    for frac in (0.9, 0.6):
        want, kept, cut = [], 0, 0
        for (n, s, q), w in zip(recs, words[3]):
            streak, a, e = int(w[5]), int(w[6]), int(w[7])
            if streak > 0 and (streak + K_TOOL) / len(s) > float(np.float32(frac)):
                want.append(b"@" + n + b"\n" + s[a:e] + b"\n+\n" + q[a:e] + b"\n")
                kept += 1
                cut += (a, e) != (0, len(s))
        assert 0 < cut < kept < N_TOOL
        r = _tool("-t", fn, fq) if frac == 0.9 else _tool("-t", "-f", str(frac), fn, fq)
        assert r.returncode == 0, r.stderr[-500:]
        assert r.stdout == b"".join(want)
