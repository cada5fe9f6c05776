"""GPU tests (-m gpu) of two count tables compared and merged (bfcg_kmers_joint_hist / _list_vs / _union / _export,
bfc_amd/csrc/bfcg_tabcmp.hip) through GpuKmers and the C ABI, and of `python -m bfc_amd.kmercmp`.  The oracle is numpy on
HostTable.export_sorted() of the two exported tables (tests/tabcmp_oracle.py, held to bfc_ch_union by tests/test_tabcmp_host.py); the
inputs are two pairs of subsets of g1 at -b 24, a plain one (all counts below 16) and a heavy one whose counts leave the 64 x 64 corner of
the joint spectrum and saturate in the union."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tabcmp_oracle import Join, keep_vs, pair_reads
from test_gpu_kmers import _count, _g1
from test_kmers_host import decode_slots
from test_tabcmp_host import host_union

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64

# the forms of the two tables: k, how A's counter is made (A is attached to it), how B's is (B is uploaded from its export)
FORMS = {
    "21seg": (21, dict(table_layout=0), {}),                                                      # A on region-owned segments until attach converts them
    "21grown": (21, dict(table_layout=1, l_pre=10, tab_cshift=1), dict(table_layout=1, l_pre=10, tab_cshift=11)),  # A grown from two slots per sub-table
    "32host": (32, dict(table_layout=1), {}),
    "33host": (33, dict(table_layout=1), {}),
    "37grown": (37, dict(table_layout=1, l_pre=10, tab_cshift=1), dict(l_pre=10)),                # l_pre is clamped to 24: A stays at two slots per sub-table
    "55": (55, {}, {}),
}
PAIRS = [False, True]
PAIR_IDS = ["plain", "heavy"]


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(gpu_lib, form, heavy):
    """a pair of tables on the device, their exports in L1 form and the oracle's join -- made once per (form, pair), never changed"""
    c = Case()
    c.k, kwa, kwb = FORMS[form]
    ra, rb = pair_reads(_g1(), heavy)
    c.ga = _count(gpu_lib, c.k, ra, n_batches=3, **kwa)
    c.ga.sync()
    if form == "21seg":
        assert c.ga.table_info()["segments"]
    c.a = gpu_lib.GpuKmers(c.ga)
    gb = _count(gpu_lib, c.k, rb, **kwb)
    c.tb = gb.export_table()
    gb.close()
    c.b = gpu_lib.GpuKmers(c.tb)
    ta = c.ga.export_table()
    c.ea, c.eb = ta.export_sorted(), c.tb.export_sorted()
    ta.close()
    c.j = Join(c.ea, c.eb)
    return c


@functools.lru_cache(maxsize=None)
def _a_rows(gpu_lib, form, heavy):
    """A's slots decoded on the host: sub-table, planes, high << 8 | count and B's answer for every slot of c.ea"""
    c = _case(gpu_lib, form, heavy)
    y, ch = decode_slots(gpu_lib._lib.load(), c.k, c.a.l_pre, *c.ea)
    return np.repeat(np.arange(len(c.ea[0]), dtype=np.uint64), c.ea[0]), y, ch, c.j.other_of_a()


def _rows(sub, y, ch, oth):
    """rows (sub-table, y0, y1, high << 8 | count, other) sorted inside a sub-table, sub-tables ascending"""
    r = np.empty((len(ch), 5), dtype=np.uint64)
    r[:, 0], r[:, 1:3], r[:, 3], r[:, 4] = sub, y, ch, oth.astype(np.int64) & 0xffff
    return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]


def _check_listing(gpu_lib, form, heavy, got, mask):
    """`got` = (y, cnt, high, other) of a listing equals the oracle's rows under `mask` (over A's slots).  The listing says nothing of
    sub-tables: its rows are cut into runs of the oracle's per-sub-table counts, so rows out of sub-table order do not compare equal."""
    sub, hy, hch, hoth = _a_rows(gpu_lib, form, heavy)
    y, cnt, high, oth = got
    assert len(cnt) == int(mask.sum())
    want = _rows(sub[mask], hy[mask], hch[mask], hoth[mask])
    run_sub = np.sort(sub[mask])
    assert np.array_equal(_rows(run_sub, y, cnt.astype(np.uint16) | high.astype(np.uint16) << 8, oth), want)


def _same_l1(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- joint spectrum ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heavy", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("form", ["21seg", "21grown", "33host", "37grown", "55"])
def test_joint_hist(gpu_lib, form, heavy):
    """joint_hist(a, b) equals the oracle's joint spectrum and totals; all three classes are non-empty; the heavy pair has cells with
    i >= 64 or j >= 64 (binned in HBM, not in LDS); joint_hist(b, a) is the transpose.  The grown forms join tables of different cshift,
    at k = 37 one of two slots per sub-table."""
    c = _case(gpu_lib, form, heavy)
    want, shared, only_a, only_b = c.j.joint()
    assert shared > 0 and only_a > 0 and only_b > 0
    assert (want[64:, 1:].any() and want[1:, 64:].any()) == heavy
    if form.endswith("grown"):
        assert c.a.cshift != c.b.cshift
    if form == "37grown":
        assert (c.a.l_pre, c.a.cshift) == (24, 1)
    got = c.a.joint_hist(c.b)
    assert c.a.last_ms() > 0
    assert got[1:] == (shared, only_a, only_b) and got[0][0, 0] == 0
    assert np.array_equal(got[0], want)
    back = c.b.joint_hist(c.a)
    assert back[1:] == (shared, only_b, only_a) and np.array_equal(back[0], want.T)


@pytest.mark.parametrize("form", ["21seg", "55"])
def test_joint_hist_of_a_table_with_itself(gpu_lib, form):
    """joint_hist(a, a) is diagonal and its diagonal is a.hist()"""
    c = _case(gpu_lib, form, True)
    joint, shared, only_a, only_b = c.a.joint_hist(c.a)
    assert (shared, only_a, only_b) == (len(c.ea[1]), 0, 0)
    assert np.array_equal(np.diag(joint), c.a.hist()[1]) and int(joint.sum()) == shared


# ---- listing against the other table ------------------------------------------------------------------------------------------------

# min_cnt, min_diff, other_min, other_max: private, shared, everything; B's counts in [2, 5] with -m, with -m and -d (g1 has no k-mer with a
# low-quality copy that B saw twice: this one keeps nothing), and -d on the private and on the shared k-mers
RANGES = [(0, 0, 0, 0), (0, 0, 1, 255), (0, 0, 0, 255), (3, 0, 2, 5), (2, 1, 2, 5), (0, 1, 0, 0), (0, 1, 1, 255)]
EMPTY = (2, 1, 2, 5)


@pytest.mark.parametrize("form", ["21seg", "21grown", "32host", "33host", "37grown"])
def test_list_vs(gpu_lib, form):
    """list_vs against the oracle: private, shared, everything, and a window of B's counts combined with -m / -d; other == b.lookup(y)"""
    c = _case(gpu_lib, form, False)
    slots, oth = c.ea[1], c.j.other_of_a()
    for m, d, lo, hi in RANGES:
        got = c.a.list_vs(c.b, min_cnt=m, min_diff=d, other_min=lo, other_max=hi)
        mask = keep_vs(slots, oth, m, d, lo, hi)
        assert mask.all() if (m, d, lo, hi) == (0, 0, 0, 255) else not mask.any() if (m, d, lo, hi) == EMPTY else 0 < mask.sum() < len(slots)
        _check_listing(gpu_lib, form, False, got, mask)
        if (lo, hi) == (0, 0):
            assert (got[3] == -1).all()
        if lo >= 1:
            assert (got[3] >= 0).all()
        assert np.array_equal(got[3], c.b.lookup(got[0]))
    assert c.a.last_ms() > 0


def test_list_vs_heavy_counts(gpu_lib):
    """counts and high counts above 63 in the annotation: the heavy pair, everything listed"""
    c = _case(gpu_lib, "33host", True)
    got = c.a.list_vs(c.b)
    found = got[3][got[3] >= 0]
    assert (found >> 8).max() == 63 and (found & 0xff).max() == 255 and (got[3] == -1).any()
    _check_listing(gpu_lib, "33host", True, got, np.ones(len(c.ea[1]), dtype=bool))


@pytest.mark.parametrize("form", ["21grown", "33host", "37grown"])
def test_list_vs_pieces_and_cap(gpu_lib, form):
    """sub-table ranges -- a single sub-table, the last one, an empty range -- and small pieces concatenate to the whole; a cap one
    short writes nothing and reports the need"""
    L = gpu_lib._lib.load()
    c = _case(gpu_lib, form, False)
    sub, hy, hch, hoth = _a_rows(gpu_lib, form, False)
    slots = c.ea[1]
    m, d, lo, hi = 0, 0, 1, 255
    mask = keep_vs(slots, hoth, m, d, lo, hi)
    n_sub = len(c.ea[0])
    first = int(sub[mask][0])   # a sub-table that holds a shared k-mer
    cuts = [0, first, first + 1, n_sub // 2, n_sub // 2, n_sub - 1, n_sub]
    parts = [c.a.list_vs(c.b, m, d, lo, hi, sub_lo=cuts[i], sub_hi=cuts[i + 1]) for i in range(len(cuts) - 1)]
    for i, p in enumerate(parts):
        assert len(p[1]) == int((mask & (sub >= cuts[i]) & (sub < cuts[i + 1])).sum())
    assert len(parts[1][1]) > 0 and len(parts[3][1]) == 0
    _check_listing(gpu_lib, form, False, [np.concatenate([p[j] for p in parts]) for j in range(4)], mask)
    _check_listing(gpu_lib, form, False, c.a.list_vs(c.b, m, d, lo, hi, piece=5000), mask)
    need = int(mask.sum())
    by, bch, bo = np.full((need, 2), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(need, 0xA5A5, dtype=np.uint16), np.full(need, 0x5A5A, dtype=np.int16)
    n = C.c_uint64()
    call = lambda cap: L.bfcg_kmers_list_vs(c.a.t, c.b.t, m, d, lo, hi, 0, n_sub, by.ctypes.data, bch.ctypes.data, bo.ctypes.data, cap, C.byref(n))  # noqa: E731
    assert call(need - 1) == 1 and n.value == need
    assert np.all(by == 0xA5A5A5A5A5A5A5A5) and np.all(bch == 0xA5A5) and np.all(bo == 0x5A5A)
    assert call(need) == 0 and n.value == need
    _check_listing(gpu_lib, form, False, (by, bch & 0xff, bch >> 8, bo), mask)
    assert L.bfcg_kmers_list_vs(c.a.t, c.b.t, m, d, lo, hi, 5, 5, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert L.bfcg_kmers_list_vs(c.a.t, c.b.t, m, d, lo, hi, 0, n_sub + 1, None, None, None, 0, C.byref(n)) == -1


def test_list_vs_refuses_k55(gpu_lib):
    """k = 55: list's refusal, list's message"""
    c = _case(gpu_lib, "55", False)
    with pytest.raises(gpu_lib.BfcGpuError, match="k <= 37"):
        c.a.list_vs(c.b)
    assert "k=55" in gpu_lib._lib.load().bfcg_last_error().decode()
    with pytest.raises(gpu_lib.BfcGpuError, match="k <= 37"):
        c.a.list()


# ---- union and export -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heavy", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("form", ["21seg", "21grown", "33host", "55"])
def test_union(gpu_lib, form, heavy):
    """union(a, b).to_host().export_sorted() equals bfc_ch_union's on the two exports and the numpy oracle's; the heavy pair saturates
    counts and high counts; the geometry is the documented one"""
    c = _case(gpu_lib, form, heavy)
    cs, hs = c.j.sums()
    assert ((cs > 255).any() and (hs > 63).any()) == heavy
    u = c.a.union(c.b)
    assert u.last_ms() > 0 and (u.k, u.l_pre) == (c.k, c.a.l_pre)
    both = c.ea[0].astype(np.int64) + c.eb[0]
    cshift = 2
    while 1 << (u.l_pre + cshift) < 2 * int(both.sum()) or 1 << cshift < int(both.max()):
        cshift += 1
    assert u.cshift == cshift
    hu = u.to_host()
    got = hu.export_sorted()
    assert hu.count() == len(c.j.sub) == len(got[1])
    assert _same_l1(got, c.j.union())
    ta = c.ga.export_table()
    hh = host_union(gpu_lib, ta, c.tb)
    assert _same_l1(got, hh.export_sorted())
    hh.close(); ta.close(); hu.close(); u.close()


@pytest.mark.parametrize("form", ["21seg", "33host"])
def test_union_is_a_member_of_the_family(gpu_lib, form, tmp_path):
    """the union read out like any table: hist() equals its host table's, lookup(list()) finds every k-mer with its counts (every
    probe chain walked), sub_sizes() the oracle's; a dump of to_host() restores to the same table; union(a, a) doubles, saturating"""
    c = _case(gpu_lib, form, True)
    u = c.a.union(c.b)
    hu = u.to_host()
    want = c.j.union()
    hist, hhist = u.hist(), hu.hist()
    assert hist[0] == hhist[0] and np.array_equal(hist[1], hhist[1]) and np.array_equal(hist[2], hhist[2])
    assert np.array_equal(u.sub_sizes(), want[0])
    y, cnt, high = u.list()
    assert len(cnt) == len(want[1])
    assert np.array_equal(u.lookup(y), (high.astype(np.int16) << 8) | cnt) and u.n_found == len(cnt)
    fn = str(tmp_path / "u.hash")
    assert hu.dump(fn) == 0
    back = gpu_lib.HostTable.restore(fn)
    assert _same_l1(back.export_sorted(), want) and back.count() == len(want[1])
    back.close(); hu.close(); u.close()
    for t, e in ((c.a, c.ea), (c.b, c.eb)):
        u2 = t.union(t)
        h2 = u2.to_host()
        assert _same_l1(h2.export_sorted(), Join(e, e).union())
        h2.close(); u2.close()


@pytest.mark.parametrize("form", ["21seg", "37grown", "55"])
def test_to_host_equals_the_direct_export(gpu_lib, form):
    """to_host() of an attached and of an uploaded table: the slots and the key count of the direct export"""
    c = _case(gpu_lib, form, False)
    for t, e in ((c.a, c.ea), (c.b, c.eb)):
        h = t.to_host()
        assert (h.k, h.l_pre) == (t.k, t.l_pre) and h.count() == len(e[1])
        assert _same_l1(h.export_sorted(), e)
        h.close()


def test_corrector_on_the_union(gpu_lib):
    """GpuCorrector on union.to_host() and on the host's bfc_ch_union table: the same bytes for the first 500 reads of g1"""
    c = _case(gpu_lib, "33host", False)
    seq, qual, off = _g1()
    seqs = [seq[int(off[i]):int(off[i + 1])].tobytes() for i in range(500)]
    quals = [qual[int(off[i]):int(off[i + 1])].tobytes() for i in range(500)]
    u = c.a.union(c.b)
    hu = u.to_host()
    ta = c.ga.export_table()
    hh = host_union(gpu_lib, ta, c.tb)
    outs = []
    for t in (hu, hh):
        o = gpu_lib.bfc_opt_init(); o.k = c.k
        ec = gpu_lib.GpuCorrector(t, o, max_pos=sum(len(s) + 1 for s in seqs), max_reads=len(seqs))
        outs.append(ec.correct(seqs, quals))
        ec.close()
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][2], outs[1][2]) and np.array_equal(outs[0][3], outs[1][3])
    assert outs[0][0] != seqs   # and some read was corrected
    hh.close(); ta.close(); hu.close(); u.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals(gpu_lib):
    """another k, another l_pre, NULL: every entry point returns an error and a message before any launch, and the objects work after"""
    L = gpu_lib._lib.load()
    c, c33, cg = _case(gpu_lib, "21seg", False), _case(gpu_lib, "33host", False), _case(gpu_lib, "21grown", False)
    assert c.a.l_pre != cg.b.l_pre and c.a.k == cg.b.k
    joint, n3, n = np.zeros((256, 256), dtype=np.uint64), (C.c_uint64 * 3)(), C.c_uint64()
    jp = joint.ctypes.data_as(C.POINTER(C.c_uint64))
    for other, word in ((c33.b, "differ in k"), (cg.b, "differ in l_pre"), (None, "bad arguments")):
        ot = other.t if other is not None else None
        for a_t, b_t in ((c.a.t, ot), (ot, c.a.t)):
            assert L.bfcg_kmers_joint_hist(a_t, b_t, jp, n3) == -1 and word in L.bfcg_last_error().decode()
            assert L.bfcg_kmers_list_vs(a_t, b_t, 0, 0, 0, 255, 0, 1, None, None, None, 0, C.byref(n)) == -1 and word in L.bfcg_last_error().decode()
            assert not L.bfcg_kmers_union(a_t, b_t) and word in L.bfcg_last_error().decode()
        if other is not None:
            with pytest.raises(gpu_lib.BfcGpuError, match=word):
                c.a.joint_hist(other)
            with pytest.raises(gpu_lib.BfcGpuError, match=word):
                c.a.list_vs(other)
            with pytest.raises(gpu_lib.BfcGpuError, match=word):
                c.a.union(other)
    assert L.bfcg_kmers_joint_hist(c.a.t, c.b.t, None, n3) == -1 and "bad arguments" in L.bfcg_last_error().decode()
    assert L.bfcg_kmers_list_vs(c.a.t, c.b.t, 0, 0, 0, 255, 0, 1, None, None, None, 0, None) == -1
    assert not L.bfcg_kmers_export(None, None) and "bad arguments" in L.bfcg_last_error().decode()
    assert not joint.any()
    for x in (c, c33, cg):   # everything still works
        got = x.a.joint_hist(x.b)
        assert np.array_equal(got[0], x.j.joint()[0])


# ---- the tool ---------------------------------------------------------------------------------------------------------------------------

def _tool(*args):
    return subprocess.run([sys.executable, "-m", "bfc_amd.kmercmp", *args], capture_output=True, cwd=ROOT, timeout=300)


def test_tool(gpu_lib, tmp_path):
    """python -m bfc_amd.kmercmp in a fresh process on two dumps (k = 33): summary and cell lines against the oracle, -p lines against
    list_vs, the -u dump restores to the union"""
    c = _case(gpu_lib, "33host", False)
    fa, fb, fu = str(tmp_path / "a.hash"), str(tmp_path / "b.hash"), str(tmp_path / "u.hash")
    ta = c.ga.export_table()
    assert ta.dump(fa) == 0 and c.tb.dump(fb) == 0
    ta.close()
    joint, shared, only_a, only_b = c.j.joint()
    head = ["shared\t%d" % shared, "only_a\t%d" % only_a, "only_b\t%d" % only_b, "jaccard\t%.6f" % (shared / (shared + only_a + only_b))]
    cells = ["%d\t%d\t%d" % (i, j, joint[i, j]) for i, j in zip(*joint.nonzero())]
    r = _tool("-u", fu, fa, fb)
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stdout.decode().splitlines() == head + cells and len(cells) > 20
    back = gpu_lib.HostTable.restore(fu)
    assert _same_l1(back.export_sorted(), c.j.union())
    back.close()
    r = _tool("-p", "-m", "2", fa, fb)
    assert r.returncode == 0, r.stderr[-500:]
    lines = r.stdout.splitlines()
    y, cnt, high, oth = c.a.list_vs(c.b, min_cnt=2, other_min=0, other_max=0)
    want = c.a.format_vs(y, cnt.astype(np.uint16) | high.astype(np.uint16) << 8, oth).splitlines()
    assert [ln.decode() for ln in lines[:len(head) + len(cells)]] == head + cells
    assert len(want) > 0 and sorted(lines[len(head) + len(cells):]) == sorted(want)
    assert all(ln.endswith(b"\t0\t0") and len(ln.split(b"\t")) == 5 and len(ln.split(b"\t")[0]) == 33 for ln in want)
    ys, cs, hs, os_ = c.a.list_vs(c.b, other_min=1)
    ln = c.a.format_vs(ys[:1], cs[:1].astype(np.uint16) | hs[:1].astype(np.uint16) << 8, os_[:1]).decode()
    assert ln == "%s\t%d\t%d\t%d\t%d\n" % (c.a.strings(ys[:1])[0], cs[0], hs[0], os_[0] & 0xff, os_[0] >> 8)
    assert _tool(fa).returncode == 1 and _tool("-p", "-s", fa, fb).returncode == 1
