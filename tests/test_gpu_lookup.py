"""GPU tests (-m gpu) of the lookups by k-mer (bfcg_kmers_lookup / bfcg_kmers_profile, bfc_amd/csrc/bfcg_lookup.hip) through GpuKmers:
a listing looked up again on every form of the table, random and read-derived queries against the host twin bfcg_kmer_occ_host, the
seams of the staging buffers, the count under every position of a stream, and the command-line tool `python -m bfc_amd.kmerquery`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_kmers import B, _count, _g1
from test_lookup_host import CODE, planes_of_codes, revcomp_planes, stream_kmers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096   # positions per workgroup of k_profile (BFCG_TILE1)


def _occ(cnt, high):
    return (high.astype(np.int16) << 8) | cnt.astype(np.int16)


def _tied(y, k):
    """k-mers whose two strands the reference's rule (kmer.h:81) does not order: it compares the high code bit of base k - 1 - t from
    the 3' end with the complemented one of base t, t = k >> 1 -- one base for odd k (never equal), two neighbours for even k"""
    t = np.uint64(k >> 1)
    return ((y[:, 1] >> t) & np.uint64(1)) != ((y[:, 1] >> np.uint64(k - 1 - (k >> 1))) & np.uint64(1))


LAYOUTS = dict(segments=dict(table_layout=0), host_layout=dict(table_layout=1), grown=dict(table_layout=1, l_pre=10, tab_cshift=1), uploaded={})


@pytest.mark.parametrize("case", list(LAYOUTS))
@pytest.mark.parametrize("k", [21, 32, 33, 37])
def test_round_trip(gpu_lib, k, case):
    """list() then lookup(): every answer is the listing's high << 8 | count and n_found the number of k-mers -- every probe chain the
    table holds is walked -- on an attached context whose table is in region-owned segments, in the host's layout, or grown from two
    slots per sub-table, and on the exported table uploaded again.  The reverse complements (planes complemented and bit-reversed in
    numpy) give the same answers wherever the strand rule orders the two strands, which is everywhere for odd k.  For k = 32 it reads
    two neighbouring bases and leaves half of all k-mers tied: there bfc_ch_kmer_occ hashes each strand as given, so the reverse
    complement of a listed k-mer is another key and a round trip through it cannot hold.  Measured on g1 at k = 32: 78 780 of the
    128 502 listed k-mers are tied, and 64 514 of them get another answer on the other strand (the rest have both strands in the
    table with equal counts).  Those answers are held to the host twin on the exported table instead, as every other answer is too."""
    g = _count(gpu_lib, k, n_batches=3, **LAYOUTS[case])
    g.sync()
    if k == 21 and case != "uploaded":
        assert g.table_info()["segments"] == (case == "segments")
    t = g.export_table() if case == "uploaded" else None
    km = gpu_lib.GpuKmers(t if t is not None else g)
    if case == "grown" and k < 37:   # (k = 37 has 2^24 sub-tables: two slots each hold g1)
        assert km.cshift > 1
    y, cnt, high = km.list()
    want = _occ(cnt, high)
    assert len(want) > 50000 and (want > 0).all()
    out = km.lookup(y)
    assert np.array_equal(out, want) and km.n_found == len(want) and km.last_ms() > 0
    rc = revcomp_planes(y, k)
    out_rc = km.lookup(rc)
    tied = _tied(y, k)
    print("k=%d %s: %d k-mers, %d tied, %d of them answered differently on the other strand" % (k, case, len(want), tied.sum(), (out_rc != want).sum()))
    assert tied.any() == (k % 2 == 0)
    assert np.array_equal(out_rc[~tied], want[~tied])
    km.close()
    if t is None:
        t = g.export_table()
    assert np.array_equal(out_rc, t.occ_planes(rc)) and np.array_equal(out, t.occ_planes(y))
    t.close(); g.close()


@functools.lru_cache(maxsize=None)
def _queries(k, n=20000):
    """n k-mers: half cut from g1's reads, on either strand at random, half uniform random"""
    seq, qual, off = _g1()
    rng = np.random.default_rng(100 + k)
    L, n_reads = int(off[1]), len(off) - 1
    st = rng.integers(0, n_reads, n // 2) * L + rng.integers(0, L - k + 1, n // 2)
    codes = np.minimum(CODE[seq[st[:, None] + np.arange(k)[None, :]]], 3)
    y = planes_of_codes(codes, k)
    flip = rng.integers(0, 2, len(y)).astype(bool)
    y[flip] = revcomp_planes(y[flip], k)
    rnd = rng.integers(0, 1 << k, (n - len(y), 2), dtype=np.uint64)
    return np.concatenate([y, rnd])


@pytest.mark.parametrize("k", [21, 32, 33, 37, 51, 63])
def test_lookup_equals_host_twin(gpu_lib, k):
    """20 000 k-mers, half from g1's reads on either strand, half uniform random (nearly all absent): entry for entry
    bfcg_kmer_occ_host on the exported table; garbage in the bits >= k of the planes changes nothing"""
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    q = _queries(k)
    out = km.lookup(q)
    assert out.dtype == np.int16 and len(out) == 20000
    t = g.export_table()
    assert np.array_equal(out, t.occ_planes(q))
    assert (out == -1).any() and (out >= 0).any() and (out[:10000] >= 0).sum() > 1000 and out.min() == -1
    assert km.n_found == int((out >= 0).sum())
    rng = np.random.default_rng(k)
    junk = rng.integers(0, 1 << 63, q.shape, dtype=np.uint64) * np.uint64(2) + np.uint64(1) << np.uint64(k)
    assert (junk != 0).all() and np.array_equal(km.lookup(q | junk), out)
    km.close(); t.close(); g.close()


def test_staging_seams(gpu_lib, monkeypatch):
    """n = 0, 1, 63, 64, 65, and n above the staging capacity (BFCG_LOOKUP_CAP = 1000, read when the object is made): 2000 is two full
    pieces, 2500 leaves a rest, 20 000 is twenty -- each equals the head of the answer an object with the default capacity gives"""
    k = 33
    g = _count(gpu_lib, k)
    q = _queries(k)
    km = gpu_lib.GpuKmers(g)
    full = km.lookup(q)
    monkeypatch.setenv("BFCG_LOOKUP_CAP", "1000")
    small = gpu_lib.GpuKmers(g)
    monkeypatch.delenv("BFCG_LOOKUP_CAP")
    for n in (0, 1, 63, 64, 65, 999, 1000, 1001, 2000, 2500, 20000):
        got = small.lookup(q[:n])
        assert len(got) == n and np.array_equal(got, full[:n]), n
        assert small.n_found == int((full[:n] >= 0).sum()) and (small.last_ms() > 0) == (n > 0)
    assert np.array_equal(km.lookup(q[:65]), full[:65])
    small.close(); km.close(); g.close()


def _profile_stream(k):
    """a stream longer than two tiles: g1 reads, one of them across the first tile boundary, and hand-made reads -- shorter than k,
    exactly k, with an N, lower case -- the last read ending at the stream's last position (no separator behind it)"""
    seq, qual, off = _g1()
    L = int(off[1])
    read = lambda r: seq[r * L:(r + 1) * L].tobytes()  # noqa: E731
    reads = [read(r) for r in range(26)] + [read(26)[:73]]     # 26 * 151 + 74 = 4000 positions
    reads.append(read(27))                                     # positions 4000 .. 4149: across 4096
    reads += [read(28)[:k - 1], read(29)[:k], read(30)[:70] + b"N" + read(30)[71:], read(31).lower(), b"ACGTNNACGT"]
    reads += [read(r) for r in range(32, 62)]
    reads.append(read(62)[:k + 9])
    stream = np.frombuffer(b"\n".join(reads), dtype=np.uint8)
    assert len(stream) > 2 * TILE + 64 and len(stream) % 16 != 0 and stream[3999] == 10 and stream[4150] == 10
    return stream


@pytest.mark.parametrize("k", [21, 33, 51])
def test_profile(gpu_lib, k):
    """out[p] of every position against the restatement in numpy: -2 unless the k bytes ending at p are ACGTacgt, else
    bfcg_kmer_occ_host of that window's k-mer on the exported table; the stream given on the host and on the device agree; and
    GpuKcov.kcov(min_occ=3) on the same stream has solid_end exactly where out[p] >= 0 and its count is >= 3"""
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    t = g.export_table()
    stream = _profile_stream(k)
    ends, y = stream_kmers(stream, k)
    want = np.where(ends, t.occ_planes(y), -2).astype(np.int16)
    assert ends[-1] and ends[TILE:TILE + k - 1].all() and not ends[:k - 1].any() and (want == -2).any() and (want == -1).any() and (want >= 0).any()
    got = km.profile(stream)
    assert got.dtype == np.int16 and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert km.last_ms() > 0
    d = g.dev_alloc(len(stream))
    g.h2d(d, stream)
    assert np.array_equal(km.profile(None, d_seq=d, n_pos=len(stream)), want)
    g.dev_free(d)
    with pytest.raises(gpu_lib.BfcGpuError, match="exactly one"):
        km.profile(None, d_seq=None, n_pos=5)
    kc = gpu_lib.GpuKcov(t, max_pos=len(stream))
    cov = kc.kcov(stream, min_occ=3)
    solid = (cov & kc.SOLID_END) != 0
    assert solid.any() and np.array_equal(solid, (got >= 0) & ((got & 0xff) >= 3))
    kc.close(); km.close(); t.close(); g.close()


def test_errors(gpu_lib):
    """a filter-mode context has no table to look up in: attach refuses it with its message, as before; lookup_strings names the
    entry that is not a k-mer, and answers like lookup() otherwise"""
    f = gpu_lib.GpuCounter(31, B, filter_mode=1, max_batch_pos=1 << 16)
    with pytest.raises(gpu_lib.BfcGpuError, match="bfcg_kmers_attach needs a table-mode context"):
        gpu_lib.GpuKmers(f)
    f.close()
    k = 21
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    y, cnt, high = km.list(sub_hi=1 << 13)
    assert len(y) >= 50
    strs = km.strings(y[:50])
    assert np.array_equal(km.lookup_strings(strs), _occ(cnt, high)[:50])
    assert np.array_equal(km.lookup_strings([s.lower() for s in strs]), _occ(cnt, high)[:50])
    for bad in ("ACGN" + "A" * (k - 4), "A" * (k - 1), "A" * (k + 1), ""):
        with pytest.raises(gpu_lib.BfcGpuError, match="entry 2 "):
            km.lookup_strings(strs[:2] + [bad] + strs[2:])
    km.close(); g.close()


def _tool(*args, stdin=None):
    return subprocess.run([sys.executable, "-m", "bfc_amd.kmerquery", *args], capture_output=True, cwd=ROOT, timeout=300, input=stdin)


def test_tool(gpu_lib, tmp_path):
    """python -m bfc_amd.kmerquery in fresh processes on a dump of g1 (k = 33): 1000 listed and 1000 random k-mers, with a header, an
    empty line and extra fields among them, answered with the lines formatted from the host twin; one record through -p against
    profile(); a malformed line ends the run with status 1 and its number"""
    k = 33
    g = _count(gpu_lib, k)
    km = gpu_lib.GpuKmers(g)
    t = g.export_table()
    fn, qf = str(tmp_path / "t.hash"), str(tmp_path / "q.txt")
    assert t.dump(fn) == 0
    y, cnt, high = km.list(sub_hi=1 << 15)
    assert len(y) >= 1000
    rng = np.random.default_rng(9)
    q = np.concatenate([y[:1000], rng.integers(0, 1 << k, (1000, 2), dtype=np.uint64)])[rng.permutation(2000)]
    strs = km.strings(q)
    occ = t.occ_planes(q)
    assert (occ >= 0).sum() >= 1000 and (occ == -1).sum() > 900
    want = b"".join(b"%s\t%d\t%d\n" % (s.encode(), max(int(o), 0) & 0xff, max(int(o), 0) >> 8) for s, o in zip(strs, occ))
    with open(qf, "w") as f:   # (no newline behind the last line)
        f.write(">queries\n\n" + "\n".join(s + "\t7" if i % 3 == 0 else s for i, s in enumerate(strs)))
    r = _tool(fn, qf)
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout == want
    r = _tool(fn, "-", stdin=open(qf, "rb").read())
    assert r.returncode == 0 and r.stdout == want
    # -p: one FASTA record, its sequence on two lines
    seq, qual, off = _g1()
    rd = seq[:150].tobytes()
    fa = str(tmp_path / "r.fa")
    with open(fa, "wb") as f:
        f.write(b">read0 some comment\n" + rd[:80] + b"\n" + rd[80:] + b"\n")
    prof = km.profile(np.frombuffer(rd + b"\n", dtype=np.uint8))[:150]
    line = b" ".join(b"." if v == -2 else b"%d" % (max(int(v), 0) & 0xff) for v in prof)
    r = _tool("-p", fn, fa)
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout == b">read0\n" + line + b"\n" and (prof >= 0).any() and (prof[:k - 1] == -2).all()
    # a malformed line
    with open(qf, "w") as f:
        f.write(strs[0] + "\n" + strs[1] + "\n" + strs[2][:-1] + "N\n" + strs[3] + "\n")
    r = _tool(fn, qf)
    assert r.returncode == 1 and b"line 3" in r.stderr
    assert _tool().returncode == 1
    km.close(); t.close(); g.close()
