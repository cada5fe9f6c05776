"""GPU tests (-m gpu) of the graph clipping (bfcg_kmers_clip, bfc_amd/csrc/bfcg_clip.hip) through GpuKmers and the C ABI, and of
`python -m bfc_amd.kmergraph -c`.  The reference side is the host twin on the exported table (HostTable.clip), which
tests/test_clip_host.py holds to the string oracle of tests/clip_oracle.py; the inputs are the forked-tip fixture of that file, the
fixture of tests/unitig_oracle.py and g1 at -b 24."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import clip_oracle
import graph_oracle
import unitig_oracle
from clip_oracle import kmers_of
from graph_oracle import planes_of_strs
from test_gpu_kmers import _count, _rows
from test_gpu_tabcmp import FORMS
from test_gpu_unitigs import _case as _base_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = [("fork", "21seg"), ("fork", "21grown"), ("fork", "33host"), ("fork", "37grown"), ("g1", "21seg"), ("g1", "33host")]
U = np.uint64


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(gpu_lib, which, form):
    """a table counted on the GPU in one of test_gpu_tabcmp.py's forms: attached, exported to the host, the export uploaded again -- made
    once, never changed.  "fork" is clip_oracle's fixture; "fixture" and "g1" are test_gpu_unitigs.py's cases"""
    if which != "fork":
        return _base_case(gpu_lib, which, form)
    c = Case()
    c.k = FORMS[form][0]
    c.reads = clip_oracle.fixture(c.k).reads
    c.g = _count(gpu_lib, c.k, c.reads, **FORMS[form][1])
    c.g.sync()
    c.att = gpu_lib.GpuKmers(c.g)
    c.host = c.g.export_table()
    c.up = gpu_lib.GpuKmers(c.host)
    return c


def _host_rows(t):
    """a HostTable's k-mers as sorted rows (y0, y1, count, high)"""
    slots = t.export_sorted()[1]
    return _rows(t.graph_nb(1)[0], slots & U(0xff), slots >> U(8) & U(0x3f))


def _stats(s):
    return [tuple(int(v) for v in r) for r in s]


@functools.lru_cache(maxsize=None)
def _twin(gpu_lib, which, form, kw):
    """HostTable.clip of a case's export: (sorted rows, stats, unitig rows) -- made once per parameter set, never changed"""
    res, stats = _case(gpu_lib, which, form).host.clip(**dict(kw))
    out = _host_rows(res), _stats(stats), gpu_lib.unitig_rows(*res.unitigs(1))
    res.close()
    return out


def _same(gpu_lib, km, want, **kw):
    """km.clip(**kw) is the twin's `want`: listing, stats, unitigs, keys; every survivor is in km with the same count and high count;
    returns the result"""
    res, stats = km.clip(**kw)
    y, cnt, high = res.list(1)
    assert np.array_equal(_rows(y, cnt, high), want[0]) and _stats(stats) == want[1]
    assert res.last_ms() > 0 and (res.k, res.l_pre) == (km.k, km.l_pre)
    assert gpu_lib.unitig_rows(*res.unitigs(1)) == want[2]
    vy, vcnt, vhigh, oth = res.list_vs(km)
    assert len(vcnt) == len(cnt) and np.array_equal(oth.astype(np.int64), vcnt.astype(np.int64) | vhigh.astype(np.int64) << 8)
    keys = len(cnt)
    assert int(res.hist()[1].sum()) == keys and all((1 << (res.l_pre + c)) < 2 * keys or (1 << c) < int(res.sub_sizes().max()) for c in range(2, res.cshift))
    return res


@pytest.mark.parametrize("which,form", TABLES)
def test_clip_equals_host_twin(gpu_lib, which, form):
    """on the attached table (segments converted at attach, grown from two slots per sub-table, the host's layout) and on the upload of its
    export: the result's sorted listing, the stats and the result's unitigs are the host twin's on the export; every survivor is shared
    with the input at an unchanged count and high count; the input's histogram is the same before and after"""
    c = _case(gpu_lib, which, form)
    sets = [dict(min_cnt=2, max_tip=12), dict(min_cnt=1, max_tip=12, islands=True)] if which == "fork" else [dict(min_cnt=2), dict(min_cnt=1, islands=True, max_rounds=3)]
    for kw in sets:
        want = _twin(gpu_lib, which, form, tuple(sorted(kw.items())))
        assert len(want[1]) >= (2 if which == "fork" else 1) and len(want[0]) > 500
        for km in (c.att, c.up):
            before = km.hist()
            _same(gpu_lib, km, want, **kw).close()
            after = km.hist()
            assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


@pytest.mark.parametrize("form", ["21grown", "33host"])
def test_boundary_and_mean_rule(gpu_lib, form):
    """the base fixture's tip has exactly 4 k-mers of count 2: max_tip = 4 removes it and 3 removes nothing; max_mean = 2 removes it and
    1 keeps it; max_rounds = 0 is the listing at min_cnt"""
    c = _case(gpu_lib, "fixture", form)
    f = unitig_oracle.fixture(c.k)
    tip = planes_of_strs(kmers_of(f.base.tip_read[graph_oracle.TIP_ERR + 1 - c.k:], c.k), c.k)
    assert len(tip) == 4 and (c.att.lookup(tip) & 0xff == 2).all()
    nodes = len(c.att.list(2)[1])
    for kw, goes in ((dict(max_tip=4), True), (dict(max_tip=3), False), (dict(max_tip=4, max_mean=2), True), (dict(max_tip=4, max_mean=1), False)):
        res, stats = c.att.clip(min_cnt=2, **kw)
        assert _stats(stats) == ([(1, 4, nodes - 4)] if goes else []) and ((res.lookup(tip) == -1).all() if goes else (res.lookup(tip) & 0xff == 2).all())
        assert len(res.list(1)[1]) == nodes - 4 * goes
        res.close()
    for min_cnt in (1, 2, 3):
        res, stats = c.up.clip(min_cnt=min_cnt, max_rounds=0)
        assert len(stats) == 0 and np.array_equal(_rows(*res.list(1)), _rows(*c.up.list(min_cnt))) and np.array_equal(_rows(*res.list(1)), _rows(*res.list(min_cnt)))
        res.close()


@pytest.mark.parametrize("form", ["21seg", "37grown"])
def test_two_rounds_are_needed(gpu_lib, form):
    """max_rounds = 1 leaves the forked tip's stem, 2 removes it, 8 stops by itself after 2"""
    c = _case(gpu_lib, "fork", form)
    f = clip_oracle.fixture(c.k)
    stem = planes_of_strs(kmers_of(f.stem, c.k), c.k)
    got = {}
    for r in (1, 2, 8):
        res, stats = c.att.clip(min_cnt=2, max_tip=12, max_rounds=r)
        got[r] = _stats(stats), res.lookup(stem), _rows(*res.list(1))
        res.close()
    assert len(got[1][0]) == 1 and got[1][0][0][:2] == (3, sum(clip_oracle.BRANCHES) + 4) and (got[1][1] >= 0).all()
    assert len(got[2][0]) == 2 and got[2][0][0] == got[1][0][0] and got[2][0][1][:2] == (1, clip_oracle.STEM) and (got[2][1] == -1).all()
    assert got[8][0] == got[2][0] and np.array_equal(got[8][2], got[2][2]) and len(got[1][2]) - len(got[2][2]) == clip_oracle.STEM


def test_everything_removed(gpu_lib):
    """5000 random reads of k + 2 bases, each given twice: 5000 islands of three k-mers, 10000 starts in 157 waves.  With islands all
    15000 k-mers go in one round, and the result is a usable empty table"""
    k, rng = 33, np.random.default_rng(33)
    reads = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, k + 2)) for _ in range(5000)]
    seq = np.frombuffer(b"".join(r + r for r in reads), dtype=np.uint8).copy()
    off = np.arange(0, len(seq) + 1, k + 2, dtype=np.uint64)
    g = _count(gpu_lib, k, (seq, np.full(len(seq), ord("I"), dtype=np.uint8), off), **FORMS["33host"][1])
    g.sync()
    km = gpu_lib.GpuKmers(g)
    assert int(km.hist()[1].sum()) == 15000
    kept, stats = km.clip(islands=False)
    assert len(stats) == 0 and len(kept.list(1)[1]) == 15000
    kept.close()
    res, stats = km.clip(islands=True)
    assert _stats(stats) == [(5000, 15000, 0)]
    assert int(res.hist()[1].sum()) == 0 and len(res.unitigs(1)[2]) == 0 and len(res.list(1)[1]) == 0 and int(res.graph_census(1).sum()) == 0
    host = res.to_host()
    assert host.count() == 0 and len(host.export_sorted()[1]) == 0
    again, stats = res.clip(islands=True)
    assert len(stats) == 0 and int(again.hist()[1].sum()) == 0
    for o in (host, again, res, km, g):
        o.close()


@pytest.mark.parametrize("cap", [1, 7])
def test_launch_seams(gpu_lib, monkeypatch, cap):
    """BFCG_UNITIG_CAP (read when the object is made) of 1 and 7 cuts the walks of the fixture's dead ends into many launches: the same
    result"""
    c = _case(gpu_lib, "fork", "33host")
    kw = dict(min_cnt=1, max_tip=12, islands=True)
    want = _twin(gpu_lib, "fork", "33host", tuple(sorted(kw.items())))
    monkeypatch.setenv("BFCG_UNITIG_CAP", str(cap))
    small = gpu_lib.GpuKmers(c.g)
    monkeypatch.delenv("BFCG_UNITIG_CAP")
    assert sum(r[0] for r in want[1]) > 7
    _same(gpu_lib, small, want, **kw).close()
    small.close()


def test_chaining(gpu_lib):
    """clip of a union; clip of a clip result with the same parameters removes nothing; to_host() of the result answers bfc_ch_get's
    lookups as the listing says"""
    c = _case(gpu_lib, "fork", "21grown")
    u = c.att.union(c.up)   # the same keys, every count doubled
    uh = u.to_host()
    kw = dict(min_cnt=3, max_tip=12)   # (the graph of the inputs at min_cnt 2)
    tw, tw_stats = uh.clip(**kw)
    res = _same(gpu_lib, u, (_host_rows(tw), _stats(tw_stats), gpu_lib.unitig_rows(*tw.unitigs(1))), **kw)
    assert len(tw_stats) == 2 and _stats(tw_stats)[0][:2] == (3, sum(clip_oracle.BRANCHES) + 4)
    again, stats = res.clip(**kw)
    assert len(stats) == 0 and np.array_equal(_rows(*again.list(1)), _rows(*res.list(1)))
    host = res.to_host()
    y, cnt, high = res.list(1)
    assert host.count() == len(cnt) and np.array_equal(host.occ_planes(y).astype(np.int64), cnt.astype(np.int64) | high.astype(np.int64) << 8)
    for o in (host, again, res, tw, uh, u):
        o.close()


def _raw(L, t, min_cnt=1, max_tip=10, max_mean=255, flags=0, max_rounds=2):
    """one call through the C ABI with stats and n_rounds filled with 77: (pointer, untouched)"""
    stats, n = np.full(3 * 64, 77, dtype=U), C.c_int(77)
    p = L.bfcg_kmers_clip(t, min_cnt, max_tip, max_mean, flags, max_rounds, stats.ctypes.data, C.byref(n))
    return p, n.value == 77 and bool((stats == 77).all())


def test_refusals(gpu_lib):
    """an even k, k = 39 and each parameter one outside its range are refused before any launch with a message: NULL, stats and n_rounds
    untouched, and the object still answers"""
    L = gpu_lib._lib.load()
    c = _case(gpu_lib, "fixture", "21grown")
    for k, msg in ((32, "k=32 is even"), (39, "k=39")):
        g = _count(gpu_lib, k, graph_oracle.fixture(k).reads)
        g.sync()
        km = gpu_lib.GpuKmers(g)
        with pytest.raises(gpu_lib.BfcGpuError, match=msg):
            km.clip()
        assert _raw(L, km.t) == (None, True) and msg in L.bfcg_last_error().decode()
        assert km.hist()[1].sum() > 0
        km.close()
        g.close()
    for kw, msg in ((dict(min_cnt=0), "min_cnt 0 is outside [1, 255]"), (dict(min_cnt=256), "min_cnt 256 is outside [1, 255]"), (dict(max_tip=0), "max_tip 0 is outside [1, 65535]"),
                    (dict(max_tip=65536), "max_tip 65536 is outside [1, 65535]"), (dict(max_mean=0), "max_mean 0 is outside [1, 255]"),
                    (dict(max_mean=256), "max_mean 256 is outside [1, 255]"), (dict(max_rounds=-1), "max_rounds -1 is outside [0, 64]"),
                    (dict(max_rounds=65), "max_rounds 65 is outside [0, 64]"), (dict(flags=2), "unknown flag bits 0x2")):
        assert _raw(L, c.att.t, **kw) == (None, True) and msg in L.bfcg_last_error().decode()
    with pytest.raises(gpu_lib.BfcGpuError, match="max_tip 0 is outside"):
        c.att.clip(max_tip=0)
    assert gpu_lib.unitig_rows(*c.att.unitigs(2)) == c.want[2]
    p, untouched = _raw(L, c.att.t)
    assert p and not untouched
    L.bfcg_kmers_destroy(p)


def test_kmergraph_tool(gpu_lib, tmp_path):
    """`python -m bfc_amd.kmergraph -m 2 -c 0 -u -o out.dump dump` on the forked fixture prints the oracle's clip lines, then the census and
    the unitigs of the cleaned table as the string oracle has them; out.dump restores to the oracle's key set; without -c the output is
    what it was: the ten census lines of the table as it is"""
    c = _case(gpu_lib, "fork", "21grown")
    dump, out = str(tmp_path / "f.dump"), str(tmp_path / "out.dump")
    assert c.host.dump(dump) == 0
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "bfc_amd.kmergraph", *a], capture_output=True, env=env, cwd=ROOT)
    plain, r = run("-m", "2", dump), run("-m", "2", "-c", "0", "-u", "-o", out, dump)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr.decode()

    def census(deg):
        tips = int(deg[0, 1:].sum() + deg[1:, 0].sum())
        lines = ["deg\t%d\t%s" % (o, "\t".join(str(int(v)) for v in deg[o])) for o in range(5)]
        return lines + ["nodes\t%d" % deg.sum(), "isolated\t%d" % deg[0, 0], "tips\t%d" % tips, "simple\t%d" % deg[1, 1], "branching\t%d" % (deg.sum() - deg[:2, :2].sum())]

    assert plain.stdout.decode().splitlines() == census(c.att.graph_census(2))
    surv, stats = clip_oracle.clip(unitig_oracle.dict_of_table(c.host), min_cnt=2)
    want = clip_oracle.unitigs_of(c.k, surv, 2)
    clean, _ = c.att.clip(min_cnt=2)
    lines = r.stdout.decode().splitlines()
    assert len(stats) == 2 and lines[:2] == ["clip\t%d\t%d\t%d\t%d" % ((i + 1,) + s) for i, s in enumerate(stats)]
    assert lines[2:12] == census(clean.graph_census(2)) and lines[12] == "unitigs\t%d" % len(want)
    assert lines[15:] == ["unitig\t%s\t%d\t%.2f\t%d\t%d\t%d" % (s.decode(), n, cs / n, left, right, cyc) for s, n, cs, left, right, cyc in want]
    back = gpu_lib.HostTable.restore(out)
    assert clip_oracle.survivors_of_table(back) == surv
    assert run("-a", "3", dump).returncode == 1 and run("-o", out, dump).returncode == 1   # (they belong to -c)
    back.close()
    clean.close()
