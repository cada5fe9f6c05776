"""The numpy oracle of the two-table comparisons (tests/tabcmp_oracle.py) checked on the CPU before it judges a kernel: its saturating
union against bfc_ch_union (bfc_host.c) on the same two host tables, and the properties of the two input pairs that the GPU tests rely
on.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tabcmp_oracle import Join, pair_reads

# the plain pair on the CPU oracle (g1 at -b 24): k -> shared, only in A, only in B
PLAIN = {21: (90232, 5131, 5007), 33: (80973, 8329, 7940)}


def _host_pair(gpu_lib, g1, tmp_path, k, heavy):
    """the pair counted by the oracle, dumped and restored into this library's host tables"""
    tabs = []
    for i, (seq, qual, off) in enumerate(pair_reads(g1[1], heavy)):
        c = oracle.Counter(k, 24)
        c.count(seq, qual, off)
        fn = str(tmp_path / ("%d.hash" % i))
        assert c.dump(fn) == 0
        want = c.export()
        c.close()
        t = gpu_lib.HostTable.restore(fn)
        got = t.export_sorted()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        tabs.append(t)
    return tabs


def host_union(gpu_lib, ta, tb):
    p = gpu_lib._lib.load().bfc_ch_union((C.c_void_p * 2)(ta.ptr, tb.ptr), 2)
    return gpu_lib.HostTable(p)


@pytest.mark.parametrize("heavy", [False, True], ids=["plain", "heavy"])
@pytest.mark.parametrize("k", [21, 33])   # 2^20 sub-tables; from k = 37 on there are 2^24, and walking them takes the CPU seconds
def test_numpy_union_equals_bfc_ch_union(gpu_lib, g1, tmp_path, k, heavy):
    """export_sorted() of bfc_ch_union on the two tables equals the numpy union, sizes and slots; the union's key count is the joint
    spectrum's total.  The plain pair has the three classes the issue names; the heavy pair leaves the 64 x 64 corner and saturates."""
    ta, tb = _host_pair(gpu_lib, g1, tmp_path, k, heavy)
    j = Join(ta.export_sorted(), tb.export_sorted())
    joint, shared, only_a, only_b = j.joint()
    assert shared > 0 and only_a > 0 and only_b > 0 and joint[0, 0] == 0
    assert int(joint[1:, 1:].sum()) == shared and int(joint[1:, 0].sum()) == only_a and int(joint[0, 1:].sum()) == only_b
    if not heavy:
        assert (shared, only_a, only_b) == PLAIN[k]
        assert not joint[16:].any() and not joint[:, 16:].any()
    else:
        c, h = j.sums()
        assert joint[64:, 1:].any() and joint[1:, 64:].any()          # cells outside the corner ...
        assert ((c > 63) & (c < 255) & (j.va > 0) & (j.vb > 0)).any()  # ... some without saturating
        assert (c > 255).any() and (h > 63).any()
    u = host_union(gpu_lib, ta, tb)
    sizes, slots = u.export_sorted()
    want = j.union()
    assert u.count() == shared + only_a + only_b == len(slots)
    assert np.array_equal(sizes, want[0]) and np.array_equal(slots, want[1])
    u.close(); ta.close(); tb.close()


def test_numpy_union_of_a_table_with_itself(gpu_lib, g1, tmp_path):
    """a table against itself: a diagonal joint spectrum that is the table's own, and doubled counts, saturating"""
    ta, tb = _host_pair(gpu_lib, g1, tmp_path, 33, True)
    ea = ta.export_sorted()
    j = Join(ea, ea)
    joint, shared, only_a, only_b = j.joint()
    assert (shared, only_a, only_b) == (len(ea[1]), 0, 0) and np.array_equal(np.diag(joint), ta.hist()[1]) and joint.sum() == shared
    u = host_union(gpu_lib, ta, ta)
    sizes, slots = u.export_sorted()
    want = j.union()
    assert np.array_equal(sizes, want[0]) and np.array_equal(slots, want[1])
    cnt = (ea[1] & np.uint64(0xff)).astype(np.int64)
    assert np.array_equal((slots & np.uint64(0xff)).astype(np.int64), np.minimum(2 * cnt, 255)) and (2 * cnt > 255).any()
    u.close(); ta.close(); tb.close()
