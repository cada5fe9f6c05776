"""Rate of the table read-out (bfcg_kmers.hip) on the c2 read set (E. coli 100x, k = 31), table resident in HBM: hist() and a full list()
from the attached context, kernels only, against the path it replaces for the spectrum -- bfcg_export_table followed by the host's
bfc_ch_hist.  Not the headline bench; numbers quoted in profiles/kmers_rate.md.

    python scripts/kmers_rate.py [k] [bf_shift] [genome size] [coverage]
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import bfc_amd  # noqa: E402
from bfc_amd import gen  # noqa: E402

COPY_TBS = 6.3  # HBM rate a streaming kernel reaches on this chip (8 TB/s peak)
arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d  # noqa: E731
k, b, G, cov = arg(1, 31), arg(2, 33), arg(3, 4_600_000), arg(4, 100)
rs = gen.ReadSet(seed=2, G=G, cov=cov)
seq, qual, off = rs.reads()
s_seq, s_qual = bfc_amd.to_stream(seq, off), bfc_amd.to_stream(qual, off)
stride, br = rs.L + 1, 786432
g = bfc_amd.GpuCounter(k, b, max_batch_pos=br * stride)
for r0 in range(0, rs.n_reads, br):
    r1 = min(rs.n_reads, r0 + br)
    g.count_host(s_seq[r0 * stride:r1 * stride], s_qual[r0 * stride:r1 * stride])
st = g.stats()
print("counted: k=%d -b%d, %d k-mers, %d distinct keys" % (k, b, st["n_kmers"], st["n_keys"]))

km = bfc_amd.GpuKmers(g)
slots = 1 << (km.l_pre + km.cshift)
print("table: 2^%d sub-tables of 2^%d slots = %.1f MiB, %.1f %% full" % (km.l_pre, km.cshift, slots * 8 / 2**20, 100.0 * st["n_keys"] / slots))


def rate(ms, passes):
    tbs = slots * 8 * passes / ms / 1e9
    return "%.3f ms, %.1f G slots/s, %.2f TB/s read = %.2f of the %.1f TB/s copy rate" % (ms, slots * passes / ms / 1e6, tbs, tbs / COPY_TBS, COPY_TBS)


hist_ms = []
for rep in range(5):
    mode, cnt, high = km.hist()
    hist_ms.append(km.last_ms())
print("hist (attached, one pass, kernel only), 5 runs: %s" % " ".join("%.3f" % v for v in hist_ms))
print("hist best: " + rate(min(hist_ms), 1) + "; mode %d, %d keys" % (mode, int(cnt.sum())))
list_ms = []
for rep in range(3):
    t0 = time.perf_counter()
    y, c, h = km.list()
    wall = time.perf_counter() - t0
    list_ms.append(km.last_ms())
print("list (all %d k-mers, count + scan + emit kernels), 3 runs: %s; wall of the last with copies %.1f ms" % (len(c), " ".join("%.3f" % v for v in list_ms), wall * 1e3))
print("list best: " + rate(min(list_ms), 2) + " (two passes over the table; %.1f MB written)" % (len(c) * 18 / 1e6))
y3, c3, h3 = km.list(min_cnt=3)
print("list -m 3: %d k-mers, %.3f ms" % (len(c3), km.last_ms()))
km.close()

# the path this replaces for the spectrum: export the whole table to the host, walk it there
t0 = time.perf_counter()
t = g.export_table()
t1 = time.perf_counter()
hmode, hcnt, hhigh = t.hist()
t2 = time.perf_counter()
assert hmode == mode and np.array_equal(hcnt, cnt) and np.array_equal(hhigh, high)
print("export + host bfc_ch_hist: %.1f ms + %.1f ms = %.1f ms (same mode and bins)" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3))
t.close()
g.close()
