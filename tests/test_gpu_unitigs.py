"""GPU tests (-m gpu) of the compacted graph (bfcg_kmers_unitigs, bfc_amd/csrc/bfcg_unitigs.hip) through GpuKmers and the C ABI, and of
`python -m bfc_amd.kmergraph -u`.  The reference side is the host twin on the exported table (HostTable.unitigs), which
tests/test_unitig_host.py holds to a Python dict over the table's strings; the inputs are the constructed fixture of
tests/unitig_oracle.py -- paths, a bubble, a tip, singletons, a self-loop, two hairpins and a cycle -- and g1 at -b 24."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import graph_oracle
import unitig_oracle
from test_gpu_kmers import _count, _g1
from test_gpu_tabcmp import FORMS
from test_unitig_host import _raw, untouched

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = [("fixture", "21seg"), ("fixture", "21grown"), ("fixture", "33host"), ("fixture", "37grown"), ("g1", "21seg"), ("g1", "33host")]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(gpu_lib, which, form):
    """a table counted on the GPU in one of test_gpu_tabcmp.py's forms: attached, exported to the host, the export uploaded again, and
    the host twin's unitigs of the export at min_cnt 1 and 2 -- made once, never changed"""
    c = Case()
    c.k = FORMS[form][0]
    c.reads = unitig_oracle.fixture(c.k).reads if which == "fixture" else _g1()
    c.g = _count(gpu_lib, c.k, c.reads, n_batches=3 if which == "g1" else 1, **FORMS[form][1])
    c.g.sync()
    assert bool(c.g.table_info()["segments"]) == (form == "21seg")   # (the attach converts them)
    c.att = gpu_lib.GpuKmers(c.g)
    c.host = c.g.export_table()
    c.up = gpu_lib.GpuKmers(c.host)
    c.want = {m: gpu_lib.unitig_rows(*c.host.unitigs(m)) for m in (1, 2)}
    return c


@pytest.mark.parametrize("which,form", TABLES)
def test_unitigs_equal_host_twin(gpu_lib, which, form):
    """on the attached table (segments converted at attach, grown from two slots per sub-table, the host's layout) and on the upload of its
    export, at min_cnt 1 and 2: the sorted unitigs are the host twin's, so both forms give the same set; their k-mers add up to the
    device's census; offsets, lengths and k-mers agree"""
    c = _case(gpu_lib, which, form)
    for min_cnt in (1, 2):
        want = c.want[min_cnt]
        assert len(want) > (8 if which == "fixture" else 100)
        for km in (c.att, c.up):
            seq, off, nk, cs, ends = km.unitigs(min_cnt)
            assert km.last_ms() > 0
            assert off[0] == 0 and off[-1] == len(seq) and np.array_equal(np.diff(off).astype(np.int64), nk.astype(np.int64) + c.k - 1)
            assert gpu_lib.unitig_rows(seq, off, nk, cs, ends) == want
            assert int(nk.sum()) == int(km.graph_census(min_cnt).sum())
    if which == "fixture":
        assert sum(r[5] for r in c.want[2]) == 1 and {r[3] for r in c.want[2]} | {r[4] for r in c.want[2]} == {0, 1, 2, 3, 6}


@pytest.mark.parametrize("form", ["21seg", "37grown"])
def test_union_with_itself_keeps_the_unitigs(gpu_lib, form):
    """a.union(a) holds the same keys in another layout with doubled counts: the same unitigs but for cnt_sum"""
    c = _case(gpu_lib, "fixture", form)
    u = c.att.union(c.att)
    strip = lambda rows: [r[:2] + r[3:] for r in rows]
    got = gpu_lib.unitig_rows(*u.unitigs(1))
    assert strip(got) == strip(c.want[1]) and [r[2] for r in got] == [2 * r[2] for r in c.want[1]]
    assert strip(gpu_lib.unitig_rows(*u.unitigs(3))) == strip(c.want[2])   # a count of 1 became 2, of 2 and more 4 and more
    u.close()


@pytest.mark.parametrize("form", ["21grown", "33host"])
def test_cap_protocol(gpu_lib, form):
    """caps of 0 size the call; a seq_cap one short and an n_cap one short return 1 with the right n[] and leave the outputs as they
    were; exact caps write"""
    L, c = gpu_lib._lib.load(), _case(gpu_lib, "fixture", form)
    want = c.want[2]
    n0, n1 = len(want), sum(len(r[0]) for r in want)
    for seq_cap, n_cap in ((0, 0), (n1 - 1, n0), (n1, n0 - 1)):
        r = _raw(L, L.bfcg_kmers_unitigs, c.att.t, 2, seq_cap, n_cap)
        assert r[:3] == (1, n0, n1) and untouched(r)
    r = _raw(L, L.bfcg_kmers_unitigs, c.att.t, 2, n1, n0)
    assert r[:3] == (0, n0, n1) and gpu_lib.unitig_rows(*r[3:]) == want


@pytest.mark.parametrize("cap", [1, 7, 64])
def test_launch_seams(gpu_lib, monkeypatch, cap):
    """BFCG_UNITIG_CAP (read when the object is made) below the fixture's starts: 1 and 7 cut the paths' counting and fill walks into
    many launches, 64 still cuts the walks of the cycle's 200 nodes; the result is unchanged"""
    c = _case(gpu_lib, "fixture", "33host")
    monkeypatch.setenv("BFCG_UNITIG_CAP", str(cap))
    small = gpu_lib.GpuKmers(c.g)
    monkeypatch.delenv("BFCG_UNITIG_CAP")
    assert sum(1 for r in c.want[1] if not r[5]) > 7 and unitig_oracle.CIRC > 64
    for min_cnt in (1, 2):
        assert gpu_lib.unitig_rows(*small.unitigs(min_cnt)) == c.want[min_cnt]
    small.close()


def test_more_starts_than_one_block_of_the_scan(gpu_lib, monkeypatch):
    """5000 random reads of k + 2 bases, each given twice: 5000 unitigs of three k-mers with two open ends each, 10000 starts -- the scan
    of the winners works in blocks of 8192 entries and carries its sums into the second; a launch cap of 4096 cuts the walks as well"""
    k, rng = 33, np.random.default_rng(33)
    reads = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, k + 2)) for _ in range(5000)]
    seq = np.frombuffer(b"".join(r + r for r in reads), dtype=np.uint8).copy()
    off = np.arange(0, len(seq) + 1, k + 2, dtype=np.uint64)
    g = _count(gpu_lib, k, (seq, np.full(len(seq), ord("I"), dtype=np.uint8), off), **FORMS["33host"][1])
    g.sync()
    host = g.export_table()
    want = gpu_lib.unitig_rows(*host.unitigs(1))
    assert len(want) == 5000 and all(r[1:] == (3, 3, 1, 1, 0) for r in want)
    for cap in (None, "4096"):
        if cap:
            monkeypatch.setenv("BFCG_UNITIG_CAP", cap)
        km = gpu_lib.GpuKmers(g)
        monkeypatch.delenv("BFCG_UNITIG_CAP", raising=False)
        assert gpu_lib.unitig_rows(*km.unitigs(1)) == want
        km.close()
    host.close()
    g.close()


def test_refusals(gpu_lib):
    """an even k, k = 39 and min_cnt 0 and 256 are refused before any launch with a message; nothing is written, n[] included, and the
    object stays usable"""
    L = gpu_lib._lib.load()
    c = _case(gpu_lib, "fixture", "21grown")
    for k, msg in ((32, "k=32 is even"), (39, "k=39.*k <= 37")):
        g = _count(gpu_lib, k, graph_oracle.fixture(k).reads)
        g.sync()
        km = gpu_lib.GpuKmers(g)
        with pytest.raises(gpu_lib.BfcGpuError, match=msg):
            km.unitigs(2)
        r = _raw(L, L.bfcg_kmers_unitigs, km.t, 2, 1 << 16, 1 << 10)
        assert r[0] == -1 and (r[1], r[2]) == (77, 77) and untouched(r)
        assert km.hist()[1].sum() > 0
        km.close()
        g.close()
    for bad in (0, 256):
        with pytest.raises(gpu_lib.BfcGpuError, match="min_cnt %d is outside" % bad):
            c.att.unitigs(bad)
        r = _raw(L, L.bfcg_kmers_unitigs, c.att.t, bad, 1 << 16, 1 << 10)
        assert r[0] == -1 and (r[1], r[2]) == (77, 77) and untouched(r)
    assert gpu_lib.unitig_rows(*c.att.unitigs(2)) == c.want[2]


def test_kmergraph_tool(gpu_lib, tmp_path):
    """`python -m bfc_amd.kmergraph -m 2 dump` prints the ten census lines as before; with -u the same lines, then the counts and one line
    per unitig as the string oracle has them; an even k with -u is refused with the library's message and exit status 1"""
    c = _case(gpu_lib, "fixture", "21grown")
    dump = str(tmp_path / "f.dump")
    assert c.host.dump(dump) == 0
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "bfc_amd.kmergraph", *a], capture_output=True, env=env, cwd=ROOT)
    plain, r = run("-m", "2", dump), run("-m", "2", "-u", dump)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr.decode()
    deg = c.att.graph_census(2)
    tips = int(deg[0, 1:].sum() + deg[1:, 0].sum())
    today = ["deg\t%d\t%s" % (o, "\t".join(str(int(v)) for v in deg[o])) for o in range(5)]
    today += ["nodes\t%d" % deg.sum(), "isolated\t%d" % deg[0, 0], "tips\t%d" % tips, "simple\t%d" % deg[1, 1], "branching\t%d" % (deg.sum() - deg[:2, :2].sum())]
    assert plain.stdout.decode().splitlines() == today
    lines = r.stdout.decode().splitlines()
    want = unitig_oracle.unitigs(unitig_oracle.dict_of_table(c.host), 2)
    lens = sorted((len(w[0]) for w in want), reverse=True)
    n50 = next(v for i, v in enumerate(lens) if 2 * sum(lens[:i + 1]) >= sum(lens))
    assert lines[:10] == today and lines[10:13] == ["unitigs\t%d" % len(want), "cycles\t1", "n50\t%d" % n50]
    assert lines[13:] == ["unitig\t%s\t%d\t%.2f\t%d\t%d\t%d" % (s.decode(), n, cs / n, left, right, cyc) for s, n, cs, left, right, cyc in want]
    g = _count(gpu_lib, 32, graph_oracle.fixture(32).reads)
    even = str(tmp_path / "even.dump")
    t = g.export_table()
    assert t.dump(even) == 0
    r = run("-u", even)
    assert r.returncode == 1 and r.stdout == b"" and "k=32 is even" in r.stderr.decode()
    t.close()
    g.close()
