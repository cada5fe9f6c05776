"""The host twin of the bubble popping (bfcg_pop_host, bfc_amd/csrc/bfcg_pop.hip) -- the reference side of every GPU comparison in
test_gpu_pop.py -- held to the oracle of tests/bubble_oracle.py: the string oracle's unitigs with ends (3, 3) paired by the definition of
include/bfc_gpu.h and the losers deleted round by round.  The inputs are the fixture of that file at k = 11 (at k = 9 no draw of it is
free of repeated k-mers), 21, 33 and 37 and the dense draws d11, d13, d15 and d19 of tests/dense_corpus.py.  What the generator knows of
the fixture is asserted on the oracle alone first.  No GPU."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import bubble_oracle
import oracle
import test_dense_graph_host as H
import unitig_oracle
from bubble_oracle import survivors_of_table

U = np.uint64
KS = [11, 21, 33, 37]
DRAWS = ["d11", "d13", "d15", "d19"]


def param_sets(k):
    """the parameter sets every fixture table is run with"""
    return [dict(), dict(max_diff=2), dict(max_diff=65535), dict(max_arm=k - 1), dict(max_arm=k), dict(max_arm=2 * k), dict(max_mean=1), dict(max_mean=2),
            dict(max_mean=255, max_diff=2), dict(max_rounds=0), dict(max_rounds=1), dict(max_rounds=8, max_diff=2, max_arm=65535), dict(min_cnt=3), dict(min_cnt=2, max_diff=2)]


@functools.lru_cache(maxsize=None)
def _tab(gpu_lib, k):
    """the bubble fixture counted by the oracle at -b 24, dumped and restored into this library's host table -- made once, never changed"""
    c = oracle.Counter(k, 24)
    c.count(*bubble_oracle.fixture(k).reads)
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "t.hash")
        assert c.dump(fn) == 0
        t = gpu_lib.HostTable.restore(fn)
    c.close()
    assert t is not None and t.k == k
    return t


@functools.lru_cache(maxsize=None)
def _dict(gpu_lib, k):
    return unitig_oracle.dict_of_table(_tab(gpu_lib, k))


@functools.lru_cache(maxsize=None)
def _oracle(d, kw):
    """the oracle's survivors, stats and the survivors' unitigs for one set of parameters -- computed once, never changed"""
    want, stats = bubble_oracle.pop(d, **dict(kw))
    return want, stats, bubble_oracle.unitigs_of(d.k, want)


def _check(gpu_lib, t, d, **kw):
    """t.pop_bubbles(**kw) against the oracle on d: survivors with their values, stats, the result's own unitigs, its geometry"""
    want, stats, want_unitigs = _oracle(d, tuple(sorted(kw.items())))
    res, got_stats = t.pop_bubbles(**kw)
    got = survivors_of_table(res)
    assert got == want and [tuple(int(v) for v in r) for r in got_stats] == stats
    assert res.count() == len(want) and (res.k, res.l_pre) == (t.k, t.l_pre)
    assert gpu_lib.unitig_rows(*res.unitigs(1)) == want_unitigs
    sizes = res.export_sorted()[0]
    cshift = next(c for c in range(2, 40) if (1 << (t.l_pre + c)) >= 2 * len(want) and (1 << c) >= int(sizes.max()))
    assert res.L.bfc_ch_raw_cshift(C.c_void_p(res.ptr)) == cshift   # (bfc_host.h: the table's log2 slots per sub-table)
    res.close()
    return want, stats


@pytest.mark.parametrize("k", KS)
def test_fixture_on_the_oracle_alone(gpu_lib, k):
    """what bubble_oracle.fixture's docstring says of its cases, for the counts the library gave: nested takes two rounds (2 bubbles,
    then 1), the indel follows max_diff, interlocked, three-way and inverted stay"""
    st = bubble_oracle.needs_two_rounds(_dict(gpu_lib, k), bubble_oracle.fixture(k))
    d = k // 2 + 1
    assert [r[:2] for r in st] == [(2, 2 * k), (1, k + d)]


@pytest.mark.parametrize("k", KS)
def test_host_twin_equals_the_oracle(gpu_lib, k):
    """every parameter set on the fixture: the survivor set with counts and high counts, the per-round stats and the unitigs of the result
    are the oracle's; the input is not changed; max_arm, max_diff, max_mean, max_rounds and min_cnt each change the outcome"""
    t, f, d = _tab(gpu_lib, k), bubble_oracle.fixture(k), _dict(gpu_lib, k)
    before = t.export_sorted()[1].copy()
    got = [_check(gpu_lib, t, d, **kw) for kw in param_sets(k)]
    assert np.array_equal(t.export_sorted()[1], before)
    by = {tuple(sorted(kw.items())): g for kw, g in zip(param_sets(k), got)}
    st = lambda **kw: [r[:2] for r in by[tuple(sorted(kw.items()))][1]]
    surv = lambda **kw: set(by[tuple(sorted(kw.items()))][0])
    assert st() == st(max_arm=2 * k) == [(2, 2 * k), (1, k + k // 2 + 1)] and st(max_arm=k) == st(max_rounds=1) == [(2, 2 * k)]
    assert st(max_diff=2) == st(max_diff=65535) == st(max_rounds=8, max_diff=2, max_arm=65535) == [(3, 3 * k - 1), (1, k + k // 2 + 1)]
    assert st(max_arm=k - 1) == st(max_rounds=0) == st(max_mean=1) == []
    assert set(f.del_arm) <= surv() and not set(f.del_arm) & surv(max_diff=2) and set(f.never) <= surv(max_diff=65535)
    assert len(st(min_cnt=3)) == 1 and not set(f.outer) & surv(min_cnt=3)     # (the inner arm is below min_cnt: the outer bubble goes first)
    assert surv(max_mean=2) >= set(f.outer) and surv(max_mean=255, max_diff=2) == surv(max_diff=2)


@pytest.mark.parametrize("k", [21, 33, 37])
def test_tie_goes_by_the_text_of_the_first_kmer(gpu_lib, k):
    """graph_oracle's bubble has arms of equal length and equal counts: the arm that survives is the one whose emitted spelling starts with
    the smaller k-mer"""
    t, f, d = _tab(gpu_lib, k), bubble_oracle.fixture(k), _dict(gpu_lib, k)
    assert sum(bubble_oracle.counts(d, f.tie[0])) == sum(bubble_oracle.counts(d, f.tie[1]))
    first = []
    for arm in f.tie:
        rows = [u for u in unitig_oracle.unitigs(d, 1) if set(bubble_oracle.kmers_of(u[0], k)) == set(arm)]
        assert len(rows) == 1 and rows[0][3:] == (3, 3, 0)
        first.append(rows[0][0][:k])
    keep, go = (0, 1) if first[0] < first[1] else (1, 0)
    res, stats = t.pop_bubbles(max_rounds=1)
    got = survivors_of_table(res)
    assert set(f.tie[keep]) <= set(got) and not set(f.tie[go]) & set(got)
    res.close()


@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("name", DRAWS)
def test_dense_draws_equal_the_oracle(gpu_lib, name, min_cnt):
    """the dense draws, where bubbles sit among tips, cycles and nodes of degree 3 and 4: at the defaults and with arms of any length up
    to 3 k that may differ by 2"""
    t, d = H.tab(gpu_lib, name), H.graph(gpu_lib, name)
    for kw in (dict(min_cnt=min_cnt), dict(min_cnt=min_cnt, max_arm=3 * t.k, max_diff=2, max_rounds=3)):
        _check(gpu_lib, t, d, **kw)


def test_dense_draws_hold_bubbles(gpu_lib):
    """the comparison above is not empty: at min_cnt 1 the oracle pops bubbles in the draws"""
    popped = {name: sum(r[0] for r in _oracle(H.graph(gpu_lib, name), (("min_cnt", 1),))[1]) for name in DRAWS}
    assert sum(popped.values()) >= 4 and sum(1 for v in popped.values() if v) >= 2, popped


@pytest.mark.parametrize("k", [11, 21, 33])
def test_no_rounds_is_the_threshold_filter(gpu_lib, k):
    """max_rounds = 0 gives what clip(max_rounds=0) gives: the nodes at min_cnt with their values, and no stats"""
    t = _tab(gpu_lib, k)
    for min_cnt in (1, 2, 3):
        a, sa = t.pop_bubbles(min_cnt=min_cnt, max_rounds=0)
        b, sb = t.clip(min_cnt=min_cnt, max_rounds=0)
        assert len(sa) == 0 and len(sb) == 0 and survivors_of_table(a) == survivors_of_table(b) and a.count() == b.count()
        assert np.array_equal(a.export_sorted()[0], b.export_sorted()[0])
        a.close()
        b.close()


def test_nothing_left_is_an_empty_table(gpu_lib):
    """min_cnt above every count: a valid table with zero keys that still answers"""
    src = _tab(gpu_lib, 21)
    res, stats = src.pop_bubbles(min_cnt=255, max_rounds=3)
    assert res.count() == 0 and len(stats) == 0 and len(res.export_sorted()[1]) == 0 and survivors_of_table(res) == {}
    res.close()


def test_refusals(gpu_lib):
    """every refusal gives its message and NULL, leaves stats and n_rounds untouched, and the input answers afterwards"""
    L = gpu_lib._lib.load()
    ok = dict(min_cnt=1, max_arm=42, max_diff=0, max_mean=255, max_rounds=2)
    cases = [(32, {}, "k=32 is even"), (39, {}, "k=39"), (21, dict(min_cnt=0), "min_cnt 0 is outside [1, 255]"), (21, dict(min_cnt=256), "min_cnt 256 is outside [1, 255]"),
             (21, dict(max_arm=0), "max_arm 0 is outside [1, 65535]"), (21, dict(max_arm=65536), "max_arm 65536 is outside [1, 65535]"),
             (21, dict(max_diff=-1), "max_diff -1 is outside [0, 65535]"), (21, dict(max_diff=65536), "max_diff 65536 is outside [0, 65535]"),
             (21, dict(max_mean=0), "max_mean 0 is outside [1, 255]"), (21, dict(max_mean=256), "max_mean 256 is outside [1, 255]"),
             (21, dict(max_rounds=-1), "max_rounds -1 is outside [0, 64]"), (21, dict(max_rounds=65), "max_rounds 65 is outside [0, 64]")]
    from test_unitig_host import _tab as _other_tab
    for k, kw, msg in cases:
        a = dict(ok, **kw)
        t = _tab(gpu_lib, k) if k == 21 else _other_tab(gpu_lib, k)
        stats, n = np.full(3 * 64, 77, dtype=U), C.c_int(77)
        p = L.bfcg_pop_host(t.ptr, a["min_cnt"], a["max_arm"], a["max_diff"], a["max_mean"], a["max_rounds"], stats.ctypes.data, C.byref(n))
        assert not p and n.value == 77 and (stats == 77).all()
        assert msg in L.bfcg_last_error().decode()
        assert t.count() > 0 and t.hist()[1].sum() > 0
    stats = np.full(3 * 64, 77, dtype=U)
    assert not L.bfcg_pop_host(_tab(gpu_lib, 21).ptr, 1, 42, 0, 255, 2, stats.ctypes.data, None) and "bad arguments" in L.bfcg_last_error().decode()
    assert not L.bfcg_pop_host(None, 1, 42, 0, 255, 2, stats.ctypes.data, C.byref(C.c_int(0))) and (stats == 77).all()
    with pytest.raises(gpu_lib.BfcGpuError, match="k=32 is even"):
        _other_tab(gpu_lib, 32).pop_bubbles()
    with pytest.raises(gpu_lib.BfcGpuError, match="max_arm 0 is outside"):
        _tab(gpu_lib, 21).pop_bubbles(max_arm=0)
    _check(gpu_lib, _tab(gpu_lib, 21), _dict(gpu_lib, 21))   # usable afterwards
