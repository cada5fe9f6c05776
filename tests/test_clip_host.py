"""The host twin of the graph clipping (bfcg_clip_host, bfc_amd/csrc/bfcg_clip.hip) -- the reference side of every GPU comparison in
test_gpu_clip.py -- held to the oracle of tests/clip_oracle.py: the string oracle's unitigs chosen by the definition of include/bfc_gpu.h
and deleted round by round.  What the generator knows of its fixtures is asserted here.  No GPU."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import clip_oracle
import graph_oracle
import oracle
import unitig_oracle
from clip_oracle import canon, kmers_of, survivors_of_table
from test_unitig_host import _tab as _base_tab

U = np.uint64
KS = [21, 33, 37]
KS_SMALL = [21, 33]   # k = 37 has 2^24 sub-tables on the host: every pass over such a table takes a second


@functools.lru_cache(maxsize=None)
def _fork_tab(gpu_lib, k):
    """the forked-tip fixture counted by the oracle at -b 24, dumped and restored into this library's host table -- made once, never
    changed"""
    c = oracle.Counter(k, 24)
    c.count(*clip_oracle.fixture(k).reads)
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "t.hash")
        assert c.dump(fn) == 0
        t = gpu_lib.HostTable.restore(fn)
    c.close()
    assert t is not None and t.k == k
    return t


@functools.lru_cache(maxsize=None)
def _dict(gpu_lib, k, fork):
    return unitig_oracle.dict_of_table(_fork_tab(gpu_lib, k) if fork else _base_tab(gpu_lib, k))


@functools.lru_cache(maxsize=None)
def _oracle(d, kw):
    """the oracle's survivors, stats and the survivors' unitigs for one set of parameters -- computed once, never changed"""
    want, stats = clip_oracle.clip(d, **dict(kw))
    return want, stats, clip_oracle.unitigs_of(d.k, want)


def _check(gpu_lib, t, d, **kw):
    """t.clip(**kw) against the oracle on d: survivors with their values, stats, the result's own unitigs, its geometry; the survivors"""
    want, stats, want_unitigs = _oracle(d, tuple(sorted(kw.items())))
    res, got_stats = t.clip(**kw)
    got = survivors_of_table(res)
    assert got == want and [tuple(int(v) for v in r) for r in got_stats] == stats
    assert res.count() == len(want) and (res.k, res.l_pre) == (t.k, t.l_pre)
    assert gpu_lib.unitig_rows(*res.unitigs(1)) == want_unitigs
    sizes = res.export_sorted()[0]
    cshift = next(c for c in range(2, 40) if (1 << (t.l_pre + c)) >= 2 * len(want) and (1 << c) >= int(sizes.max()))
    assert res.L.bfc_ch_raw_cshift(C.c_void_p(res.ptr)) == cshift   # (bfc_host.h: the table's log2 slots per sub-table)
    res.close()
    return want, stats


@pytest.mark.parametrize("islands", [False, True])
@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_host_twin_equals_the_oracle(gpu_lib, k, min_cnt, islands):
    """on the forked-tip fixture at max_tip = 12 (above the fork's pieces, below the genome's first unitig for every k): the survivor set
    with counts and high counts, the per-round stats and the unitigs of the result are the oracle's; the input is not changed; something
    was removed, the cycle and the bubble were not"""
    t, f = _fork_tab(gpu_lib, k), clip_oracle.fixture(k)
    before = t.export_sorted()[1].copy()
    want, stats = _check(gpu_lib, t, _dict(gpu_lib, k, True), min_cnt=min_cnt, max_tip=12, islands=islands)
    assert np.array_equal(t.export_sorted()[1], before)
    assert len(stats) >= 2 and all(r[1] >= r[0] > 0 for r in stats) and stats[-1][2] == len(want)
    g = f.genome
    for kept in (kmers_of((f.base.circ + f.base.circ)[:unitig_oracle.CIRC + k - 1], k), kmers_of(g[graph_oracle.SUB - k + 1:graph_oracle.SUB + k], k),
                 kmers_of(f.base.base.variant[graph_oracle.SUB - k + 1:graph_oracle.SUB + k], k)):
        assert all(s in want for s in kept)
    assert not any(s in want for s in kmers_of(f.stem, k))
    assert (canon(f.base.base.isolated) in want) == (not islands)


@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("k", KS)
def test_two_rounds_are_needed(gpu_lib, k, min_cnt):
    """max_rounds = 1 leaves the forked tip's stem, 2 removes it, 8 stops by itself after 2 -- first on the oracle alone, then the twin"""
    t, f, d = _fork_tab(gpu_lib, k), clip_oracle.fixture(k), _dict(gpu_lib, k, True)
    st = clip_oracle.needs_two_rounds(d, f, min_cnt)
    stem = set(kmers_of(f.stem, k))
    one, s1 = _check(gpu_lib, t, d, min_cnt=min_cnt, max_tip=12, max_rounds=1)
    two, s2 = _check(gpu_lib, t, d, min_cnt=min_cnt, max_tip=12, max_rounds=2)
    more, s8 = _check(gpu_lib, t, d, min_cnt=min_cnt, max_tip=12, max_rounds=8)
    assert stem <= set(one) and not stem & set(two) and two == more
    assert (s1, s2, s8) == (st[:1], st, st)


@pytest.mark.parametrize("k", KS_SMALL)
def test_boundary_and_mean_rule(gpu_lib, k):
    """the base fixture's tip has exactly 4 k-mers of count 2: max_tip = 4 removes it and 3 removes nothing; max_mean = 2 removes it and
    1 keeps it"""
    t, f, d = _base_tab(gpu_lib, k), unitig_oracle.fixture(k), _dict(gpu_lib, k, False)
    tip = kmers_of(f.base.tip_read[graph_oracle.TIP_ERR + 1 - k:], k)
    assert len(tip) == 4 and all(d.value(s) & 0xff == 2 for s in tip)
    nodes = {s for s, v in d.d.items() if (v & 0xff) >= 2 and s <= graph_oracle.revcomp(s)}
    for kw, goes in ((dict(max_tip=4), True), (dict(max_tip=3), False), (dict(max_tip=4, max_mean=2), True), (dict(max_tip=4, max_mean=1), False)):
        want, stats = _check(gpu_lib, t, d, min_cnt=2, **kw)
        assert stats == ([(1, 4, len(nodes) - 4)] if goes else []) and set(want) == (nodes - set(tip) if goes else nodes)


@pytest.mark.parametrize("min_cnt", [1, 2, 3])
@pytest.mark.parametrize("k", KS_SMALL)
def test_no_rounds_is_the_threshold_filter(gpu_lib, k, min_cnt):
    """max_rounds = 0 gives the nodes at min_cnt with their values, and no stats"""
    t, d = _base_tab(gpu_lib, k), _dict(gpu_lib, k, False)
    want, stats = _check(gpu_lib, t, d, min_cnt=min_cnt, max_rounds=0)
    assert stats == [] and want == {s: v for s, v in d.d.items() if (v & 0xff) >= min_cnt and s <= graph_oracle.revcomp(s)}
    assert (len(want) < t.count()) == (min_cnt > 1)


@pytest.mark.parametrize("k", KS_SMALL)
def test_islands_by_stop_code(gpu_lib, k):
    """with islands at min_cnt 1: the isolated k-mer (1, 1), the A-run (6, 6), the hairpin (1, 6) and the low-count read's 4 k-mers go at
    max_tip = 4; the path of 41 k-mers into the second hairpin goes from max_tip = 41 on -- at k = 21 that is the default 2 k = 42;
    without islands all of them stay; the cycle of 200 and both arms of the bubble always survive"""
    t, f, d = _base_tab(gpu_lib, k), unitig_oracle.fixture(k), _dict(gpu_lib, k, False)
    small = [canon(f.base.isolated), canon(f.base.a_run), canon(f.hairpin[:k])] + kmers_of(f.low, k)
    path = kmers_of(f.hairpin_path[:-1], k)
    rows = {r[0]: r for r in unitig_oracle.unitigs(d, 1)}
    ends = lambda s: sorted((rows.get(s) or rows[graph_oracle.revcomp(s)])[3:5])
    assert (ends(f.base.isolated), ends(f.base.a_run), ends(f.hairpin[:k]), ends(f.low), ends(f.hairpin_path[:-1])) == ([1, 1], [6, 6], [1, 6], [1, 1], [1, 6])
    assert len(small) == 7 and len(set(path)) == 41
    stay = kmers_of((f.circ + f.circ)[:unitig_oracle.CIRC + k - 1], k) + kmers_of(f.base.genome[graph_oracle.SUB - k + 1:graph_oracle.SUB + k], k)
    stay += kmers_of(f.base.variant[graph_oracle.SUB - k + 1:graph_oracle.SUB + k], k)
    for max_tip, islands, gone_small, gone_path in ((4, True, True, False), (40, True, True, False), (41, True, True, True), (None, True, True, 2 * k >= 41),
                                                    (None, False, False, False)):
        want, stats = _check(gpu_lib, t, d, min_cnt=1, max_tip=max_tip, islands=islands)
        assert all((s in want) != gone_small for s in small) and all((s in want) != gone_path for s in path)
        assert all(s in want for s in stay)
    assert 2 * 21 == 42 and len(path) == 41


def test_nothing_left_is_an_empty_table(gpu_lib):
    """min_cnt above every count: a valid table with zero keys that still answers"""
    k = 21
    src, f = _base_tab(gpu_lib, k), unitig_oracle.fixture(k)
    y = graph_oracle.planes_of_strs([f.base.isolated], k)
    assert src.occ_planes(y)[0] > 0 and int(src.hist()[1][255]) == 0
    res, stats = src.clip(min_cnt=255, max_rounds=3)
    assert res.count() == 0 and len(stats) == 0 and len(res.export_sorted()[1]) == 0 and res.occ_planes(y)[0] == -1
    assert res.unitigs(1)[2].size == 0 and int(res.hist()[1].sum()) == 0 and survivors_of_table(res) == {}
    res.close()


def test_refusals(gpu_lib):
    """every refusal gives its message and NULL, and leaves stats and n_rounds untouched"""
    L = gpu_lib._lib.load()
    ok = dict(min_cnt=1, max_tip=10, max_mean=255, flags=0, max_rounds=2)
    cases = [(32, {}, "k=32 is even"), (39, {}, "k=39"), (21, dict(min_cnt=0), "min_cnt 0 is outside [1, 255]"), (21, dict(min_cnt=256), "min_cnt 256 is outside [1, 255]"),
             (21, dict(max_tip=0), "max_tip 0 is outside [1, 65535]"), (21, dict(max_tip=65536), "max_tip 65536 is outside [1, 65535]"),
             (21, dict(max_mean=0), "max_mean 0 is outside [1, 255]"), (21, dict(max_mean=256), "max_mean 256 is outside [1, 255]"),
             (21, dict(max_rounds=-1), "max_rounds -1 is outside [0, 64]"), (21, dict(max_rounds=65), "max_rounds 65 is outside [0, 64]"),
             (21, dict(flags=2), "unknown flag bits 0x2"), (21, dict(flags=-2), "unknown flag bits")]
    for k, kw, msg in cases:
        a = dict(ok, **kw)
        stats, n = np.full(3 * 64, 77, dtype=U), C.c_int(77)
        p = L.bfcg_clip_host(_base_tab(gpu_lib, k).ptr, a["min_cnt"], a["max_tip"], a["max_mean"], a["flags"], a["max_rounds"], stats.ctypes.data, C.byref(n))
        assert not p and n.value == 77 and (stats == 77).all()
        assert msg in L.bfcg_last_error().decode()
    with pytest.raises(gpu_lib.BfcGpuError, match="k=32 is even"):
        _base_tab(gpu_lib, 32).clip()
    with pytest.raises(gpu_lib.BfcGpuError, match="max_tip 0 is outside"):
        _base_tab(gpu_lib, 21).clip(max_tip=0)
