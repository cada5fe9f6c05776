"""The host twin of the compacted graph (bfcg_unitigs_host, bfc_amd/csrc/bfcg_unitigs.hip) -- the reference side of every GPU comparison
in test_gpu_unitigs.py -- held to the oracle of tests/unitig_oracle.py: a Python dict over the exported table's strings, the link rule
and the component walk of include/bfc_gpu.h on strings.  What the generator knows of its fixture is asserted here.  No GPU."""
import ctypes as C
import functools
import os
import tempfile

import numpy as np
import pytest

import graph_oracle
import oracle
import unitig_oracle
from graph_oracle import revcomp, strs_of_planes

U = np.uint64


@functools.lru_cache(maxsize=None)
def _tab(gpu_lib, k):
    """the unitig fixture (odd k <= 37) or graph_oracle's (the k that are refused) counted by the oracle at -b 24, dumped and restored
    into this library's host table -- made once, never changed"""
    reads = unitig_oracle.fixture(k).reads if k % 2 and k <= 37 else graph_oracle.fixture(k).reads
    c = oracle.Counter(k, 24)
    c.count(*reads)
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "t.hash")
        assert c.dump(fn) == 0
        t = gpu_lib.HostTable.restore(fn)
    c.close()
    assert t is not None and t.k == k
    return t


@functools.lru_cache(maxsize=None)
def _want(gpu_lib, k, min_cnt):
    return unitig_oracle.unitigs(unitig_oracle.dict_of_table(_tab(gpu_lib, k)), min_cnt)


def _raw(L, fn, obj, min_cnt, seq_cap, n_cap, fill=77):
    """one call through the C ABI into buffers filled with `fill`: (rc, n0, n1, seq, off, n_kmers, cnt_sum, ends)"""
    seq, off = np.full(max(seq_cap, 1), fill, dtype=np.uint8), np.full(n_cap + 1, fill, dtype=U)
    nk, cs, ends = np.full(max(n_cap, 1), fill, dtype=np.uint32), np.full(max(n_cap, 1), fill, dtype=U), np.full(max(n_cap, 1), fill, dtype=np.uint8)
    n = (C.c_uint64 * 2)(fill, fill)
    rc = fn(obj, min_cnt, seq.ctypes.data, seq_cap, off.ctypes.data, nk.ctypes.data, cs.ctypes.data, ends.ctypes.data, n_cap, n)
    return rc, int(n[0]), int(n[1]), seq, off, nk, cs, ends


def untouched(r, fill=77):
    return all((a == fill).all() for a in r[3:])


@pytest.mark.parametrize("min_cnt", [1, 2])
@pytest.mark.parametrize("k", [21, 33, 37])
def test_host_twin_equals_the_oracle(gpu_lib, k, min_cnt):
    """HostTable.unitigs equals the oracle exactly after sorting; and what the generator knows holds: the circular contig is one cycle of
    200 k-mers, the old fixture's unitig is there, the hairpin is one node with ends 1 and 6, the path into the second hairpin ends with 6,
    the A-run has (6, 6), the low-count read is a unitig at min_cnt 1 only; every sequence is spelled from its smaller end; the unitigs
    partition the nodes"""
    t, f = _tab(gpu_lib, k), unitig_oracle.fixture(k)
    want = _want(gpu_lib, k, min_cnt)
    seq, off, nk, cs, ends = t.unitigs(min_cnt)
    assert off[0] == 0 and off[-1] == len(seq) and np.array_equal(np.diff(off).astype(np.int64), nk.astype(np.int64) + k - 1)
    got = gpu_lib.unitig_rows(seq, off, nk, cs, ends)
    assert got == want and len(got) > 8
    by_seq = {r[0]: r for r in got}
    either = lambda s: by_seq.get(s) or by_seq.get(revcomp(s))
    cycles = [r for r in got if r[5]]
    c = cycles[0][0]
    assert len(cycles) == 1 and cycles[0][1] == unitig_oracle.CIRC and (c[:unitig_oracle.CIRC] in f.circ + f.circ or c[:unitig_oracle.CIRC] in revcomp(f.circ + f.circ))
    assert c[unitig_oracle.CIRC:] == c[:k - 1] and cycles[0][3:5] == (0, 0)
    assert either(f.base.unitig) is not None and sorted(either(f.base.unitig)[3:5]) == [2, 3]
    assert either(f.base.a_run)[1:] == (1, either(f.base.a_run)[2], 6, 6, 0)
    assert either(f.base.isolated)[1] == 1 and either(f.base.isolated)[3:] == (1, 1, 0)
    hp = either(f.hairpin[:k])
    assert hp[1] == 1 and sorted(hp[3:5]) == [1, 6]
    hpp = either(f.hairpin_path[:-1])
    assert hpp[1] == 41 and sorted(hpp[3:5]) == [1, 6]
    assert (either(f.low) is not None) == (min_cnt == 1) and (min_cnt == 2 or either(f.low)[1:3] == (4, 4))
    assert {r[3] for r in got} | {r[4] for r in got} == {0, 1, 2, 3, 6}
    for s, n, c, left, right, cyc in got:
        assert s[:k] < revcomp(s)[:k]
    assert sum(r[1] for r in got) == int(t.graph_census(min_cnt).sum())
    kmers = sorted(min(s[i:i + k], revcomp(s[i:i + k])) for s, n, *_ in got for i in range(n))
    listed = sorted(min(s, revcomp(s)) for s in strs_of_planes(t.list_graph(min_cnt)[0], k))
    assert kmers == listed and len(set(kmers)) == len(kmers)


def test_refusals_leave_the_outputs_untouched(gpu_lib):
    """an even k, k = 39 and min_cnt 0 and 256 are refused with a message; nothing is written, n[] included"""
    L = gpu_lib._lib.load()
    for k, min_cnt, msg in ((32, 2, "k=32 is even"), (39, 2, "k=39"), (21, 0, "min_cnt 0 is outside [1, 255]"), (21, 256, "min_cnt 256 is outside [1, 255]")):
        r = _raw(L, L.bfcg_unitigs_host, _tab(gpu_lib, k).ptr, min_cnt, 1 << 16, 1 << 10)
        assert r[0] == -1 and (r[1], r[2]) == (77, 77) and untouched(r)
        assert msg in L.bfcg_last_error().decode()
    with pytest.raises(gpu_lib.BfcGpuError, match="k=32 is even"):
        _tab(gpu_lib, 32).unitigs(2)
    with pytest.raises(gpu_lib.BfcGpuError, match="k=39.*k <= 37"):
        _tab(gpu_lib, 39).unitigs(2)


@pytest.mark.parametrize("k", [21, 37])
def test_cap_protocol(gpu_lib, k):
    """caps of 0 size the call; a seq_cap one short and an n_cap one short return 1 with the right n[] and write nothing; exact caps write"""
    L, t = gpu_lib._lib.load(), _tab(gpu_lib, k)
    want = _want(gpu_lib, k, 2)
    n0, n1 = len(want), sum(len(r[0]) for r in want)
    assert L.bfcg_unitigs_host(t.ptr, 2, None, 0, None, None, None, None, 0, (C.c_uint64 * 2)()) == 1
    for seq_cap, n_cap in ((0, 0), (n1 - 1, n0), (n1, n0 - 1)):
        r = _raw(L, L.bfcg_unitigs_host, t.ptr, 2, seq_cap, n_cap)
        assert r[:3] == (1, n0, n1) and untouched(r)
    r = _raw(L, L.bfcg_unitigs_host, t.ptr, 2, n1, n0)
    assert r[:3] == (0, n0, n1) and gpu_lib.unitig_rows(*r[3:]) == want
