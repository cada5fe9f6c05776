"""GPU tests (-m gpu) of the bubble popping (bfcg_kmers_pop, bfc_amd/csrc/bfcg_pop.hip) through GpuKmers and the C ABI, and of
`python -m bfc_amd.kmergraph -p`.  The reference side is twofold: the host twin on the exported table (HostTable.pop_bubbles), which
tests/test_pop_host.py holds to the string oracle of tests/bubble_oracle.py, and that oracle itself on the exported table's dict.  The
inputs are the fixture of bubble_oracle.py in four forms of test_gpu_tabcmp.FORMS and the dense draws d11 and d15."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bubble_oracle
import graph_oracle
import test_dense_graph_host as H
import unitig_oracle
from test_gpu_dense_graph import _case as _dense_case
from test_gpu_kmers import _count, _rows
from test_gpu_tabcmp import FORMS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_FORMS = ["21seg", "21grown", "33host", "37grown"]
U = np.uint64


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(gpu_lib, form):
    """the bubble fixture counted on the GPU in one of test_gpu_tabcmp.py's forms: attached, exported to the host, the export uploaded
    again, and the export's dict for the string oracle -- made once, never changed"""
    c = Case()
    c.k = FORMS[form][0]
    c.reads = bubble_oracle.fixture(c.k).reads
    c.g = _count(gpu_lib, c.k, c.reads, **FORMS[form][1])
    c.g.sync()
    assert bool(c.g.table_info()["segments"]) == (form == "21seg")   # (the attach converts them)
    c.att = gpu_lib.GpuKmers(c.g)
    c.host = c.g.export_table()
    c.up = gpu_lib.GpuKmers(c.host)
    c.d = unitig_oracle.dict_of_table(c.host)
    return c


def _host_rows(t):
    """a HostTable's k-mers as sorted rows (y0, y1, count, high)"""
    slots = t.export_sorted()[1]
    return _rows(t.graph_nb(1)[0], slots & U(0xff), slots >> U(8) & U(0x3f))


def _stats(s):
    return [tuple(int(v) for v in r) for r in s]


@functools.lru_cache(maxsize=None)
def _want(gpu_lib, host, d, kw):
    """HostTable.pop_bubbles of an export: (sorted rows, stats, unitig rows), held here to the string oracle on the export's dict d:
    survivors with their values, stats, the survivors' unitigs -- made once per parameter set, never changed"""
    res, stats = host.pop_bubbles(**dict(kw))
    out = _host_rows(res), _stats(stats), gpu_lib.unitig_rows(*res.unitigs(1))
    surv, want_stats = bubble_oracle.pop(d, **dict(kw))
    assert bubble_oracle.survivors_of_table(res) == surv and out[1] == want_stats and out[2] == bubble_oracle.unitigs_of(d.k, surv)
    res.close()
    return out


def _same(gpu_lib, km, want, **kw):
    """km.pop_bubbles(**kw) is `want` (the twin's and the oracle's): listing, stats, unitigs, keys; every survivor is in km with the same
    count and high count; km's histogram is what it was; returns the result"""
    before = km.hist()
    res, stats = km.pop_bubbles(**kw)
    after = km.hist()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    y, cnt, high = res.list(1)
    assert np.array_equal(_rows(y, cnt, high), want[0]) and _stats(stats) == want[1]
    assert res.last_ms() > 0 and (res.k, res.l_pre) == (km.k, km.l_pre)
    assert gpu_lib.unitig_rows(*res.unitigs(1)) == want[2]
    vy, vcnt, vhigh, oth = res.list_vs(km)
    assert len(vcnt) == len(cnt) and np.array_equal(oth.astype(np.int64), vcnt.astype(np.int64) | vhigh.astype(np.int64) << 8)
    keys = len(cnt)
    assert int(res.hist()[1].sum()) == keys and all((1 << (res.l_pre + c)) < 2 * keys or (1 << c) < int(res.sub_sizes().max()) for c in range(2, res.cshift))
    return res


def _key(**kw):
    return tuple(sorted(kw.items()))


@pytest.mark.parametrize("form", FIXTURE_FORMS)
def test_pop_equals_host_twin_and_oracle(gpu_lib, form):
    """on the attached table (segments converted at attach, grown from two slots per sub-table, the host's layout) and on the upload of its
    export: the result's sorted listing, the stats and the result's unitigs are the host twin's on the export and the string oracle's;
    every survivor is shared with the input at an unchanged count and high count; the input's histogram is the same before and after.
    With max_diff = 2 three bubbles go in round 1 and the outer one of the nested pair in round 2"""
    c = _case(gpu_lib, form)
    sets = [dict(max_diff=2)] if c.k == 37 else [dict(max_diff=2), dict(), dict(min_cnt=3, max_arm=65535, max_diff=65535)]
    for kw in sets:
        want = _want(gpu_lib, c.host, c.d, _key(**kw))
        assert len(want[0]) > 1000 and len(want[1]) >= 1
        for km in (c.att, c.up):
            _same(gpu_lib, km, want, **kw).close()
    d = c.k // 2 + 1
    assert [r[:2] for r in _want(gpu_lib, c.host, c.d, _key(max_diff=2))[1]] == [(3, 3 * c.k - 1), (1, c.k + d)]


@pytest.mark.parametrize("name", ["d11", "d15"])
def test_dense_draws(gpu_lib, name):
    """the dense draws -- bubbles among tips, cycles and nodes of degree 3 and 4; d15 a table of 16 sub-tables -- at min_cnt 1 and 2, at
    the defaults and with longer arms that may differ by 2"""
    c = _dense_case(gpu_lib, name)
    d = H.graph(gpu_lib, name)
    popped = 0
    for kw in (dict(min_cnt=1), dict(min_cnt=2), dict(min_cnt=1, max_arm=3 * c.k, max_diff=2, max_rounds=3)):
        want = _want(gpu_lib, c.host, d, _key(**kw))
        popped += sum(r[0] for r in want[1])
        for km in (c.att, c.up):
            _same(gpu_lib, km, want, **kw).close()
    assert popped > 0


def test_every_parameter_decides(gpu_lib):
    """k = 21, grown table: max_arm k - 1 / k / 2 k, max_diff 0 / 2, max_mean 1 / 2 / 255 and max_rounds 0 / 1 / 8 each give the twin's
    result, and the results differ as the fixture says"""
    c = _case(gpu_lib, "21grown")
    k, f = c.k, bubble_oracle.fixture(c.k)
    st = {}
    for kw in (dict(max_arm=k - 1), dict(max_arm=k), dict(max_arm=2 * k), dict(max_mean=1), dict(max_mean=2), dict(max_rounds=0), dict(max_rounds=1), dict(max_rounds=8), dict(min_cnt=2)):
        want = _want(gpu_lib, c.host, c.d, _key(**kw))
        res = _same(gpu_lib, c.att, want, **kw)
        st[_key(**kw)] = [r[:2] for r in want[1]], res.lookup(graph_oracle.planes_of_strs(f.outer + f.inner + f.del_arm, k))
        res.close()
    two = [(2, 2 * k), (1, k + k // 2 + 1)]
    assert st[_key(max_arm=k - 1)][0] == st[_key(max_rounds=0)][0] == st[_key(max_mean=1)][0] == []
    assert st[_key(max_arm=k)][0] == st[_key(max_rounds=1)][0] == two[:1] and st[_key(max_arm=2 * k)][0] == st[_key(max_rounds=8)][0] == two
    n_out, n_in = len(f.outer), len(f.inner)
    gone = st[_key(max_rounds=8)][1]
    assert (gone[:n_out + n_in] == -1).all() and (gone[n_out + n_in:] >= 0).all()             # both nested arms go, the indel's stays
    kept = st[_key(max_rounds=1)][1]
    assert (kept[:n_out] >= 0).all() and (kept[n_out:n_out + n_in] == -1).all()                # one round: the inner one only


def test_chaining(gpu_lib):
    """pop_bubbles feeds clip, whose result answers unitigs, graph_census and to_host; clip feeds pop_bubbles: each step is the host
    twin's on the twin's previous step; popping a popped table again removes nothing"""
    c = _case(gpu_lib, "33host")
    pk, ck = dict(max_diff=2), dict(min_cnt=1, max_tip=12, islands=True)
    res = _same(gpu_lib, c.up, _want(gpu_lib, c.host, c.d, _key(**pk)), **pk)
    tw, _ = c.host.pop_bubbles(**pk)
    clipped, cst = res.clip(**ck)
    tw_clipped, tw_cst = tw.clip(**ck)
    assert _stats(cst) == _stats(tw_cst) and len(cst) >= 1 and np.array_equal(_rows(*clipped.list(1)), _host_rows(tw_clipped))
    assert gpu_lib.unitig_rows(*clipped.unitigs(1)) == gpu_lib.unitig_rows(*tw_clipped.unitigs(1))
    assert np.array_equal(clipped.graph_census(1), tw_clipped.graph_census(1))
    host = clipped.to_host()
    y, cnt, high = clipped.list(1)
    assert host.count() == len(cnt) and np.array_equal(host.occ_planes(y).astype(np.int64), cnt.astype(np.int64) | high.astype(np.int64) << 8)
    again, ast = res.pop_bubbles(**pk)
    assert len(ast) == 0 and np.array_equal(_rows(*again.list(1)), _rows(*res.list(1)))
    # clip first, then pop: the tips are gone, the bubbles are as they were
    first, _ = c.att.clip(**ck)
    tw_first, _ = c.host.clip(**ck)
    popped, pst = first.pop_bubbles(**pk)
    tw_popped, tw_pst = tw_first.pop_bubbles(**pk)
    assert _stats(pst) == _stats(tw_pst) and [r[:2] for r in _stats(pst)] == [(3, 3 * c.k - 1), (1, c.k + c.k // 2 + 1)]
    assert np.array_equal(_rows(*popped.list(1)), _host_rows(tw_popped))
    for o in (host, again, clipped, tw_clipped, tw, res, popped, tw_popped, first, tw_first):
        o.close()


@pytest.mark.parametrize("cap", [1, 64])
def test_launch_seams(gpu_lib, monkeypatch, cap):
    """BFCG_UNITIG_CAP (read when the object is made) of 1 and 64 cuts the walks from the fixture's open ends into many launches: the
    same result"""
    c = _case(gpu_lib, "21seg")
    kw = dict(max_diff=2)
    want = _want(gpu_lib, c.host, c.d, _key(**kw))
    monkeypatch.setenv("BFCG_UNITIG_CAP", str(cap))
    small = gpu_lib.GpuKmers(c.g)
    monkeypatch.delenv("BFCG_UNITIG_CAP")
    _same(gpu_lib, small, want, **kw).close()
    small.close()


def _raw(L, t, min_cnt=1, max_arm=42, max_diff=0, max_mean=255, max_rounds=2):
    """one call through the C ABI with stats and n_rounds filled with 77: (pointer, untouched)"""
    stats, n = np.full(3 * 64, 77, dtype=U), C.c_int(77)
    p = L.bfcg_kmers_pop(t, min_cnt, max_arm, max_diff, max_mean, max_rounds, stats.ctypes.data, C.byref(n))
    return p, n.value == 77 and bool((stats == 77).all())


def test_refusals(gpu_lib):
    """an even k, k = 39 and each parameter one outside its range are refused before any launch with a message: NULL, stats and n_rounds
    untouched, and the object still answers unitigs"""
    L = gpu_lib._lib.load()
    c = _case(gpu_lib, "21grown")
    for k, msg in ((32, "k=32 is even"), (39, "k=39")):
        g = _count(gpu_lib, k, graph_oracle.fixture(k).reads)
        g.sync()
        km = gpu_lib.GpuKmers(g)
        with pytest.raises(gpu_lib.BfcGpuError, match=msg):
            km.pop_bubbles()
        assert _raw(L, km.t) == (None, True) and msg in L.bfcg_last_error().decode()
        assert km.hist()[1].sum() > 0
        km.close()
        g.close()
    units = gpu_lib.unitig_rows(*c.host.unitigs(1))
    for kw, msg in ((dict(min_cnt=0), "min_cnt 0 is outside [1, 255]"), (dict(min_cnt=256), "min_cnt 256 is outside [1, 255]"), (dict(max_arm=0), "max_arm 0 is outside [1, 65535]"),
                    (dict(max_arm=65536), "max_arm 65536 is outside [1, 65535]"), (dict(max_diff=-1), "max_diff -1 is outside [0, 65535]"),
                    (dict(max_diff=65536), "max_diff 65536 is outside [0, 65535]"), (dict(max_mean=0), "max_mean 0 is outside [1, 255]"),
                    (dict(max_mean=256), "max_mean 256 is outside [1, 255]"), (dict(max_rounds=-1), "max_rounds -1 is outside [0, 64]"),
                    (dict(max_rounds=65), "max_rounds 65 is outside [0, 64]")):
        assert _raw(L, c.att.t, **kw) == (None, True) and msg in L.bfcg_last_error().decode()
        assert gpu_lib.unitig_rows(*c.att.unitigs(1)) == units
    stats = np.full(3 * 64, 77, dtype=U)
    assert not L.bfcg_kmers_pop(c.att.t, 1, 42, 0, 255, 2, stats.ctypes.data, None) and (stats == 77).all()
    with pytest.raises(gpu_lib.BfcGpuError, match="max_arm 0 is outside"):
        c.att.pop_bubbles(max_arm=0)
    p, untouched = _raw(L, c.att.t)
    assert p and not untouched
    L.bfcg_kmers_destroy(p)


def _census_lines(deg):
    tips = int(deg[0, 1:].sum() + deg[1:, 0].sum())
    lines = ["deg\t%d\t%s" % (o, "\t".join(str(int(v)) for v in deg[o])) for o in range(5)]
    return lines + ["nodes\t%d" % deg.sum(), "isolated\t%d" % deg[0, 0], "tips\t%d" % tips, "simple\t%d" % deg[1, 1], "branching\t%d" % (deg.sum() - deg[:2, :2].sum())]


def _unitig_lines(rows):
    total, run, n50 = sum(len(r[0]) for r in rows), 0, 0
    for v in sorted((len(r[0]) for r in rows), reverse=True):
        run += v
        if 2 * run >= total:
            n50 = v
            break
    head = ["unitigs\t%d" % len(rows), "cycles\t%d" % sum(r[5] for r in rows), "n50\t%d" % n50]
    return head + ["unitig\t%s\t%d\t%.2f\t%d\t%d\t%d" % (s.decode(), n, cs / n, left, right, cyc) for s, n, cs, left, right, cyc in rows]


def test_kmergraph_tool(gpu_lib, tmp_path):
    """`python -m bfc_amd.kmergraph -p 0 -d 2 -u -o out.dump dump` prints the twin's pop lines, then the census and the unitigs of the
    table that is left as the string oracle has them, and out.dump restores to the oracle's key set; `-c 12 -p 0 -d 2` clips, pops and
    clips again; `-m 2 -c 0 -u` prints, byte for byte, what it printed before there was a -p: the clip lines, the census, the unitig
    lines of the oracle's clipped graph; -d without -p and -i without -c are usage errors"""
    import clip_oracle
    c = _case(gpu_lib, "21grown")
    dump, out = str(tmp_path / "f.dump"), str(tmp_path / "out.dump")
    assert c.host.dump(dump) == 0
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "bfc_amd.kmergraph", *a], capture_output=True, env=env, cwd=ROOT)
    r = run("-p", "0", "-d", "2", "-u", "-o", out, dump)
    assert r.returncode == 0, r.stderr.decode()
    surv, stats = bubble_oracle.pop(c.d, max_diff=2)
    tw, tw_stats = c.host.pop_bubbles(max_diff=2)
    assert _stats(tw_stats) == stats and len(stats) == 2
    want = ["pop\t%d\t%d\t%d\t%d" % ((i + 1,) + s) for i, s in enumerate(stats)] + _census_lines(tw.graph_census(1)) + _unitig_lines(bubble_oracle.unitigs_of(c.k, surv))
    assert r.stdout.decode().splitlines() == want
    back = gpu_lib.HostTable.restore(out)
    assert bubble_oracle.survivors_of_table(back) == surv
    back.close()
    # clip, pop, clip
    r = run("-c", "12", "-i", "-p", "0", "-d", "2", dump)
    assert r.returncode == 0, r.stderr.decode()
    a, sa = c.host.clip(max_tip=12, islands=True)
    b, sb = a.pop_bubbles(max_diff=2)
    e, se = b.clip(max_tip=12, islands=True)
    lines = ["clip\t%d\t%d\t%d\t%d" % ((i + 1,) + s) for i, s in enumerate(_stats(sa))] + ["pop\t%d\t%d\t%d\t%d" % ((i + 1,) + s) for i, s in enumerate(_stats(sb))]
    lines += ["clip\t%d\t%d\t%d\t%d" % ((len(sa) + i + 1,) + s) for i, s in enumerate(_stats(se))]
    assert len(sa) >= 1 and len(sb) == 2 and r.stdout.decode().splitlines() == lines + _census_lines(e.graph_census(1))
    # what was valid before prints what it printed
    r = run("-m", "2", "-c", "0", "-u", dump)
    assert r.returncode == 0, r.stderr.decode()
    csurv, cstats = clip_oracle.clip(c.d, min_cnt=2)
    ctw, _ = c.host.clip(min_cnt=2)
    want = ["clip\t%d\t%d\t%d\t%d" % ((i + 1,) + s) for i, s in enumerate(cstats)] + _census_lines(ctw.graph_census(2)) + _unitig_lines(clip_oracle.unitigs_of(c.k, csurv, 2))
    assert len(cstats) >= 1 and r.stdout == ("\n".join(want) + "\n").encode()
    assert run("-d", "2", dump).returncode == 1 and run("-i", "-p", "0", dump).returncode == 1 and run("-a", "3", dump).returncode == 1
    for o in (tw, a, b, e, ctw):
        o.close()
