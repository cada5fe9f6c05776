"""Rate of the table read-out (bfcg_kmers.hip) on the c2 read set (E. coli 100x, k = 31), table resident in HBM: hist() and a full list()
from the attached context, kernels only, against the path it replaces for the spectrum -- bfcg_export_table followed by the host's
bfc_ch_hist.  Not the headline bench; numbers quoted in profiles/kmers_rate.md.

    python scripts/kmers_rate.py [--lookup | --readstats | --compare | --graph | --unitigs | --links | --clip | --pop] [k] [bf_shift] [genome size] [coverage]

--lookup measures the other direction instead (bfcg_lookup.hip): lookup() of every listed k-mer in shuffled order, and profile() over a
prefix of the reads that built the table, each next to the host's loop over bfc_ch_kmer_occ on the same input (bfcg_kmers_occ_host,
one thread) and to the chip's rate of independent 8-byte gathers from HBM (scripts/probes/gather_probe.hip).
--readstats measures read_stats() (bfcg_readstats.hip) over a prefix of the reads of about 2^25 positions: its two kernels, the call's
wall time with its D2H, and next to them the way to the same numbers without it -- profile() and a numpy reduction per read.
--compare measures two tables against each other (bfcg_tabcmp.hip): the table of all reads and the table of the first half of the reads,
both resident; joint_hist(), a full list_vs() and union(), kernels only, against the bytes of both tables at the copy rate, and next to
them the route without them -- export both tables, bfc_ch_union on the host (one thread).
--graph measures the table read as a de Bruijn graph (bfcg_graph.hip): graph_census(), a full list_graph() and neighbors() of 2^20 listed
k-mers, kernels only.  A census is eight random 8-byte probes per node: 8 x nodes / time is put next to the chip's gather rate, and the
census next to the route without it -- export the table, bfcg_graph_census_host on the CPU (one thread).
--unitigs measures the compacted graph (bfcg_unitigs.hip): unitigs() -- the sizing call alone (listing of the path ends, counting walks,
the pass for the cycles' nodes, scans) and the call that also fills -- kernels only, next to a census of the same table and to the route
without it: export the table, bfcg_unitigs_host on the CPU (one thread).  The per-kernel split is a kernel trace of this script's run.
--links measures what the edges cost on top of the walks (bfcg_kmers_unitig_graph): unitigs() and unitig_graph(), each the call that writes,
kernels only, on the same table in the same run, and the edges by the kind of end they leave.  No host route: the twin walks for a minute.
--clip measures the graph cleaning (bfcg_clip.hip): clip() at the default parameters -- tips of at most 2 k k-mers, eight rounds at most --
and with islands, all the call's kernels, in k-mers of the input per second, beside unitigs() on the same table in the same run (the only
yardstick there is: nobody measured this before), and the unitigs of the cleaned table beside those of the input.
--pop measures the bubble popping (bfcg_pop.hip): pop_bubbles() at the default parameters -- arms of at most 2 k k-mers of equal length,
eight rounds at most -- and with max_diff 2, all the call's kernels, beside clip() at its defaults on the same table in the same run, the
unitigs before and after, and the route without it: export the table, bfcg_pop_host on the CPU (one thread).
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import bfc_amd  # noqa: E402
from bfc_amd import gen  # noqa: E402

COPY_TBS = 6.3  # HBM rate a streaming kernel reaches on this chip (8 TB/s peak)
GATHER_G = 48.8  # G random 8-byte gathers per second (profiles/round5_gather_probe.txt)
LOOKUP = "--lookup" in sys.argv
if LOOKUP:
    sys.argv.remove("--lookup")
READSTATS = "--readstats" in sys.argv
if READSTATS:
    sys.argv.remove("--readstats")
COMPARE = "--compare" in sys.argv
if COMPARE:
    sys.argv.remove("--compare")
GRAPH = "--graph" in sys.argv
if GRAPH:
    sys.argv.remove("--graph")
UNITIGS = "--unitigs" in sys.argv
if UNITIGS:
    sys.argv.remove("--unitigs")
LINKS = "--links" in sys.argv
if LINKS:
    sys.argv.remove("--links")
CLIP = "--clip" in sys.argv
if CLIP:
    sys.argv.remove("--clip")
POP = "--pop" in sys.argv
if POP:
    sys.argv.remove("--pop")
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


def lookup_rates():
    y, c, h = km.list()
    n = len(c)
    perm = np.random.default_rng(1).permutation(n)
    ys, want = np.ascontiguousarray(y[perm]), ((h.astype(np.int16) << 8) | c)[perm]
    ms, wall = [], []
    for rep in range(4):
        t0 = time.perf_counter()
        out = km.lookup(ys)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(km.last_ms())
    assert np.array_equal(out, want) and km.n_found == n
    best = min(ms)
    print("lookup (all %d listed k-mers, shuffled; %d pieces), 4 runs, kernels only (ms): %s; wall with the copies: %s"
          % (n, -(-n // (1 << 22)), " ".join("%.3f" % v for v in ms), " ".join("%.1f" % v for v in wall)))
    print("lookup best: %.3f ms = %.2f G lookups/s = %.3f of the %.1f G gathers/s ceiling" % (best, n / best / 1e6, n / best / 1e6 / GATHER_G, GATHER_G))
    # a prefix of the reads that built the table: whole reads, about 2^26 positions
    n_pos = min(len(s_seq), (1 << 26) // stride * stride)
    pms = []
    for rep in range(4):
        prof = km.profile(s_seq[:n_pos])
        pms.append(km.last_ms())
    n_k = int((prof != -2).sum())
    best_p = min(pms)
    print("profile (%d positions of the reads, %d k-mers, %d present), 4 runs, kernel only (ms): %s" % (n_pos, n_k, int((prof >= 0).sum()), " ".join("%.3f" % v for v in pms)))
    print("profile best: %.3f ms = %.2f G positions/s, %.2f G probes/s = %.3f of the gather ceiling" % (best_p, n_pos / best_p / 1e6, n_k / best_p / 1e6, n_k / best_p / 1e6 / GATHER_G))
    t = g.export_table()
    t0 = time.perf_counter()
    hout = t.occ_planes(ys)
    dt = time.perf_counter() - t0
    assert np.array_equal(hout, out)
    print("host loop over bfc_ch_kmer_occ, the same shuffled k-mers, one thread: %.1f ms = %.4f G lookups/s (the GPU kernels: %.0fx)" % (dt * 1e3, n / dt / 1e9, dt * 1e3 / best))
    # the profile's input on the host: the planes of the k-mer ending at every position of the first 2^22 (numpy, not timed), then the same loop
    m = min(n_pos, (1 << 22) // stride * stride)
    st = s_seq[:m]
    code = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = code[ch | 0x20] = i
    cd = code[st]
    ok = cd < 4
    idx = np.arange(m)
    run = idx - np.maximum.accumulate(np.where(ok, -1, idx))
    ends = run >= k
    cc = np.where(ok, cd, 0).astype(np.uint64)
    yy = np.zeros((m, 2), dtype=np.uint64)
    for l in range(k):
        yy[l:, 0] |= (cc[:m - l] & np.uint64(1)) << np.uint64(l)
        yy[l:, 1] |= (cc[:m - l] >> np.uint64(1)) << np.uint64(l)
    yq = np.ascontiguousarray(yy[ends])
    t0 = time.perf_counter()
    hp = t.occ_planes(yq)
    dt = time.perf_counter() - t0
    assert np.array_equal(hp, prof[:m][ends]) and (prof[:m][~ends] == -2).all()
    print("host loop over bfc_ch_kmer_occ, the k-mers of the first %d positions in read order (%d): %.1f ms = %.4f G lookups/s (k_profile per k-mer: %.0fx)"
          % (m, len(yq), dt * 1e3, len(yq) / dt / 1e9, (dt / len(yq)) / (best_p * 1e-3 / n_k)))
    t.close()


def reduce_numpy(prof, n, min_cov):
    """the eight words per read from a profile of n reads of equal length, in numpy"""
    v = prof.reshape(n, stride)[:, :rs.L].astype(np.int32)
    defined, present = v != -2, v >= 0
    c = np.where(present, v & 0xff, 0)
    solid = present & (c >= min_cov)
    out = np.zeros((n, 8), dtype=np.int32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = defined.sum(1), present.sum(1), solid.sum(1), c.sum(1)
    srt = np.sort(np.where(defined, c, 256), axis=1)
    nd = out[:, 0]
    pick = lambda i: np.take_along_axis(srt, np.maximum(i, 0)[:, None], 1)[:, 0]  # noqa: E731
    out[:, 4] = np.where(nd > 0, pick(np.zeros_like(nd)) | pick((nd - 1) >> 1) << 8 | pick(nd - 1) << 16, 0)
    idx = np.arange(rs.L)[None, :]
    run = idx - np.maximum.accumulate(np.where(solid, -1, idx), axis=1)   # the solid run ending at every position
    best = run.max(1)
    last = rs.L - 1 - np.argmax(run[:, ::-1], axis=1)                       # of equally long runs the last
    start = last - best + 1 - (k - 1)
    out[:, 5], out[:, 6], out[:, 7] = best, np.where(best > 0, start, -1), np.where(best > 0, start + best + k - 1, -1)
    return out


def readstats_rates(min_cov=3):
    n = min(rs.n_reads, (1 << 25) // stride)
    stream, roff = s_seq[:n * stride], np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
    ms, wall, pms, pwall, hwall = [], [], [], [], []
    for rep in range(4):
        t0 = time.perf_counter()
        got = km.read_stats(stream, roff, min_cov)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(km.last_ms())
    for rep in range(4):
        t0 = time.perf_counter()
        prof = km.profile(stream)
        t1 = time.perf_counter()
        want = reduce_numpy(prof, n, min_cov)
        t2 = time.perf_counter()
        pms.append(km.last_ms()); pwall.append((t1 - t0) * 1e3); hwall.append((t2 - t1) * 1e3)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:10]
    f = lambda v: " ".join("%.3f" % x for x in v)  # noqa: E731
    print("build %s" % bfc_amd._lib.build_id())
    print("read_stats: %d reads of %d bases, %d positions, min_cov %d; %d k-mers, %d present, %d solid; %d reads solid throughout"
          % (n, rs.L, len(stream), min_cov, got[:, 0].sum(), got[:, 1].sum(), got[:, 2].sum(), int((got[:, 5] == got[:, 0]).sum())))
    print("read_stats, k_profile + k_read_stats, 4 runs (ms): %s; wall with the H2D and the %.1f MB D2H (ms): %s" % (f(ms), n * 32 / 1e6, f(wall)))
    print("profile, k_profile alone, 4 runs (ms): %s; wall with the H2D and the %.1f MB D2H (ms): %s" % (f(pms), len(stream) * 2 / 1e6, f(pwall)))
    print("numpy reduction of the profile per read, 4 runs (ms): %s" % f(hwall))
    kp, both = min(pms), min(ms)
    print("best: k_profile %.3f ms, both kernels %.3f ms: k_read_stats %.3f ms = %.2f of k_profile, %.1f G positions/s, %.2f TB/s of profile read"
          % (kp, both, both - kp, (both - kp) / kp, len(stream) / (both - kp) / 1e6, len(stream) * 2 / (both - kp) / 1e9))
    print("best wall: read_stats %.1f ms; profile %.1f ms + numpy %.1f ms = %.1f ms (%.1fx)"
          % (min(wall), min(pwall), min(hwall), min(pwall) + min(hwall), (min(pwall) + min(hwall)) / min(wall)))


def compare_rates():
    import ctypes as C
    half = rs.n_reads // 2
    g2 = bfc_amd.GpuCounter(k, b, max_batch_pos=br * stride)
    for r0 in range(0, half, br):
        r1 = min(half, r0 + br)
        g2.count_host(s_seq[r0 * stride:r1 * stride], s_qual[r0 * stride:r1 * stride])
    kb = bfc_amd.GpuKmers(g2)
    slots_b = 1 << (kb.l_pre + kb.cshift)
    both = (slots + slots_b) * 8
    f = lambda v: " ".join("%.3f" % x for x in v)  # noqa: E731
    vs = lambda ms: "%.3f ms; both tables once (%.1f MiB) in that time = %.2f TB/s = %.2f of the %.1f TB/s copy rate" % (ms, both / 2**20, both / ms / 1e9, both / ms / 1e9 / COPY_TBS, COPY_TBS)  # noqa: E731
    print("build %s" % bfc_amd._lib.build_id())
    print("table B (first %d reads): 2^%d sub-tables of 2^%d slots = %.1f MiB, %d keys" % (half, kb.l_pre, kb.cshift, slots_b * 8 / 2**20, g2.stats()["n_keys"]))
    jms = []
    for rep in range(5):
        joint, shared, only_a, only_b = km.joint_hist(kb)
        jms.append(km.last_ms())
    print("joint_hist (two launches of k_tab_join + k_join_sum), 5 runs (ms): %s; shared %d, only A %d, only B %d; %d keys in cells outside the 64 x 64 corner, %d outside the 128 x 128 one"
          % (f(jms), shared, only_a, only_b, int(joint.sum() - joint[:64, :64].sum()), int(joint.sum() - joint[:128, :128].sum())))
    print("joint_hist best: " + vs(min(jms)))
    lms = []
    for rep in range(3):
        t0 = time.perf_counter()
        y, c, h, o = km.list_vs(kb)
        wall = time.perf_counter() - t0
        lms.append(km.last_ms())
    assert len(c) == shared + only_a and int((o >= 0).sum()) == shared
    print("list_vs (all %d k-mers of A annotated; count + scan + emit, B probed in both passes), 3 runs (ms): %s; wall of the last with copies %.1f ms" % (len(c), f(lms), wall * 1e3))
    km.list()
    print("list_vs best: " + vs(min(lms)) + "; list() of A alone: %.3f ms" % km.last_ms())
    ums = []
    for rep in range(3):
        u = km.union(kb)
        ums.append(u.last_ms())
        if rep < 2:
            u.close()
    uhist = u.hist()
    print("union (two size passes, zero-fill and two launches of k_tab_union into 2^%d x 2^%d slots = %.1f MiB), 3 runs (ms): %s" % (u.l_pre, u.cshift, 8 * 2.0**(u.l_pre + u.cshift - 20), f(ums)))
    print("union best: " + vs(min(ums)))
    t0 = time.perf_counter()
    ta, tb = g.export_table(), g2.export_table()
    t1 = time.perf_counter()
    hu = bfc_amd.HostTable(bfc_amd._lib.load().bfc_ch_union((C.c_void_p * 2)(ta.ptr, tb.ptr), 2))
    t2 = time.perf_counter()
    hh = hu.hist()
    assert hu.count() == shared + only_a + only_b == int(uhist[1].sum()) and np.array_equal(hh[1], uhist[1]) and np.array_equal(hh[2], uhist[2])
    print("export both + host bfc_ch_union: %.1f ms + %.1f ms = %.1f ms (same key count and spectrum as the device's union: %.0fx its kernels)"
          % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, (t2 - t0) * 1e3 / min(ums)))
    t0 = time.perf_counter()
    th = u.to_host()
    print("to_host() of the union: %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    for x in (th, hu, ta, tb, u, kb, g2):
        x.close()


def graph_rates(min_cnt=1):
    f = lambda v: " ".join("%.3f" % x for x in v)  # noqa: E731
    print("build %s" % bfc_amd._lib.build_id())
    cms = []
    for rep in range(5):
        deg = km.graph_census(min_cnt)
        cms.append(km.last_ms())
    nodes, best = int(deg.sum()), min(cms)
    print("graph_census (min_cnt %d; one pass, decode + eight probes per node), 5 runs (ms): %s" % (min_cnt, f(cms)))
    print("census:\n%s" % "\n".join("\t".join(str(int(v)) for v in row) for row in deg))
    print("graph_census best: %.3f ms; %d nodes, 8 probes each = %.2f G probes/s = %.3f of the %.1f G gathers/s ceiling; the table once in that time = %.2f TB/s"
          % (best, nodes, 8 * nodes / best / 1e6, 8 * nodes / best / 1e6 / GATHER_G, GATHER_G, slots * 8 / best / 1e9))
    lms = []
    for rep in range(3):
        t0 = time.perf_counter()
        y, c, h, nb = km.list_graph(min_cnt)
        wall = time.perf_counter() - t0
        lms.append(km.last_ms())
    assert len(c) == nodes
    km.list()
    print("list_graph (all %d nodes with nb; count + scan + emit, eight probes per node in both passes), 3 runs (ms): %s; wall of the last with copies %.1f ms; list() alone: %.3f ms"
          % (nodes, f(lms), wall * 1e3, km.last_ms()))
    print("list_graph best: %.3f ms = %.2f G probes/s = %.3f of the gather ceiling" % (min(lms), 16 * nodes / min(lms) / 1e6, 16 * nodes / min(lms) / 1e6 / GATHER_G))
    q = np.ascontiguousarray(y[np.random.default_rng(1).permutation(len(y))[:1 << 20]])
    nms, nwall = [], []
    for rep in range(4):
        t0 = time.perf_counter()
        nv = km.neighbors(q)
        nwall.append((time.perf_counter() - t0) * 1e3)
        nms.append(km.last_ms())
    print("neighbors (%d listed k-mers, shuffled), 4 runs, kernel only (ms): %s; wall with the copies: %s" % (len(q), f(nms), " ".join("%.1f" % v for v in nwall)))
    print("neighbors best: %.3f ms = %.2f G probes/s = %.3f of the gather ceiling" % (min(nms), 8 * len(q) / min(nms) / 1e6, 8 * len(q) / min(nms) / 1e6 / GATHER_G))
    t0 = time.perf_counter()
    t = g.export_table()
    t1 = time.perf_counter()
    hdeg = t.graph_census(min_cnt)
    t2 = time.perf_counter()
    assert np.array_equal(hdeg, deg) and np.array_equal(t.neighbors(q[:4096]), nv[:4096])
    print("export + host bfcg_graph_census_host, one thread: %.1f ms + %.1f ms = %.1f ms (the same census: %.0fx the kernel)" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, (t2 - t0) * 1e3 / best))
    t.close()


def unitig_rates(min_cnt=1):
    import ctypes as C
    f = lambda v: " ".join("%.3f" % x for x in v)  # noqa: E731
    print("build %s" % bfc_amd._lib.build_id())
    cms = []
    for rep in range(3):
        deg = km.graph_census(min_cnt)
        cms.append(km.last_ms())
    nodes = int(deg.sum())
    print("graph_census (min_cnt %d), 3 runs (ms): %s; %d nodes" % (min_cnt, f(cms), nodes))
    sms, n = [], (C.c_uint64 * 2)()
    for rep in range(3):
        assert km.L.bfcg_kmers_unitigs(km.t, min_cnt, None, 0, None, None, None, None, 0, n) == 1
        sms.append(float(km.L.bfcg_kmers_last_ms(km.t)))
    print("unitigs, the sizing call (listing of the ends, counting walks, the cycles' pass and walks, scans), 3 runs (ms): %s -> %d unitigs, %d bases" % (f(sms), n[0], n[1]))
    ums, wall = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        seq_u, off_u, nk, cs, ends = km.unitigs(min_cnt)
        wall.append((time.perf_counter() - t0) * 1e3)
        ums.append(km.last_ms())
    print("unitigs, the call that writes (the same and the fill walks), 3 runs (ms): %s; wall of sizing + writing call with the copies: %s" % (f(ums), " ".join("%.1f" % v for v in wall)))
    assert int(nk.sum()) == nodes
    lens = np.sort(np.diff(off_u).astype(np.int64))[::-1]
    n50 = int(lens[np.searchsorted(np.cumsum(lens), (int(lens.sum()) + 1) // 2)])
    print("%d unitigs over %d nodes: %d cycles, longest %d k-mers, N50 %d bases; ends with code 1 / 2 / 3 / 6: %s"
          % (len(nk), nodes, int((ends >> 6).sum()), int(nk.max()), n50, " / ".join(str(int(((ends & 7) == c).sum() + ((ends >> 3 & 7) == c).sum())) for c in (1, 2, 3, 6))))
    best = min(ums)
    print("unitigs best: %.3f ms = %.1f censuses (%.3f ms) = %.2f ns per node; fill = %.3f ms of it" % (best, best / min(cms), min(cms), best * 1e6 / nodes, best - min(sms)))
    t0 = time.perf_counter()
    t = g.export_table()
    t1 = time.perf_counter()
    print("export: %.1f ms" % ((t1 - t0) * 1e3), flush=True)
    h = t.unitigs(min_cnt)
    t2 = time.perf_counter()
    print("export + host bfcg_unitigs_host, one thread: %.1f ms + %.1f ms = %.1f ms (%.0fx the kernels, %.0fx the two calls' wall)"
          % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, (t2 - t0) * 1e3 / best, (t2 - t0) * 1e3 / min(wall)), flush=True)
    assert bfc_amd.unitig_rows(*h) == bfc_amd.unitig_rows(seq_u, off_u, nk, cs, ends)
    print("the host's sorted unitigs equal the device's")
    t.close()


def link_rates(min_cnt=1):
    f = lambda v: " ".join("%.3f" % x for x in v)  # noqa: E731
    print("build %s" % bfc_amd._lib.build_id())
    ums, gms, wall = [], [], []
    for rep in range(3):
        seq_u, off_u, nk, cs, ends = km.unitigs(min_cnt)
        ums.append(km.last_ms())
    print("unitigs (min_cnt %d), the call that writes, 3 runs (ms): %s; %d unitigs" % (min_cnt, f(ums), len(nk)))
    for rep in range(3):
        t0 = time.perf_counter()
        seq_g, off_g, nk_g, cs_g, ends_g, links = km.unitig_graph(min_cnt)
        wall.append((time.perf_counter() - t0) * 1e3)
        gms.append(km.last_ms())
    print("unitig_graph, the call that writes (the same, the end map and the edges), 3 runs (ms): %s; wall of sizing + writing call with the copies: %s"
          % (f(gms), " ".join("%.1f" % v for v in wall)))
    assert bfc_amd.unitig_rows(seq_g, off_g, nk_g, cs_g, ends_g) == bfc_amd.unitig_rows(seq_u, off_u, nk, cs, ends)
    n_out = (links >= 0).sum(axis=2)                                                            # (n, 2): the edges that leave each side
    code = np.stack([ends_g >> 3 & 7, ends_g & 7], axis=1)                                      # (n, 2): the stop code of the side they leave
    print("%d edges from %d sides; by stop code of the side 2 / 3 / 6 / cycle: %s; sides with 2 / 3 / 4 edges: %s"
          % (int(n_out.sum()), 2 * len(nk_g), " / ".join(str(int(n_out[code == c].sum())) for c in (2, 3, 6, 0)), " / ".join(str(int((n_out == v).sum())) for v in (2, 3, 4))))
    back = links[links >= 0]
    u, o, c = np.nonzero(links >= 0)
    pairs = set(zip((u * 2 + o).tolist(), back.tolist()))
    assert all(((v ^ 1), (s ^ 1)) in pairs for s, v in pairs)
    print("every edge has its mirror")
    print("unitig_graph best: %.3f ms = %.2f x unitigs (%.3f ms): the edges cost %.3f ms = %.2f ns per side" % (min(gms), min(gms) / min(ums), min(ums), min(gms) - min(ums), (min(gms) - min(ums)) * 1e6 / (2 * len(nk_g))))


def _ms3(v):
    return " ".join("%.3f" % x for x in v)


def _shape(t, min_cnt, arms=False):
    """(text, nodes, kernel ms) of unitigs() on table t; with `arms`, the text also counts the unitigs whose two ends have code 3"""
    seq_u, off_u, nk, cs, ends = t.unitigs(min_cnt)
    lens = np.sort(np.diff(off_u).astype(np.int64))[::-1]
    n50 = int(lens[np.searchsorted(np.cumsum(lens), (int(lens.sum()) + 1) // 2)]) if len(lens) else 0
    text = "%d unitigs over %d nodes, N50 %d bases" % (len(nk), int(nk.sum()), n50)
    if arms:
        text += ", %d with ends (3, 3)" % int(((ends & 63) == (3 | 3 << 3)).sum())
    return text, int(nk.sum()), t.last_ms()


def _clean3(call):
    """call() -> (table, stats), three runs: (kernel ms, wall ms, the last run's table -- the caller closes it --, its stats)"""
    ms, wall = [], []
    for rep in range(3):
        t0 = time.perf_counter()
        res, stats = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(res.last_ms())
        if rep < 2:
            res.close()
    return ms, " ".join("%.1f" % v for v in wall), res, stats


def clip_rates(min_cnt=1):
    print("build %s" % bfc_amd._lib.build_id())
    ums = []
    for rep in range(3):
        text, nodes, ms = _shape(km, min_cnt)
        ums.append(ms)
    print("unitigs (min_cnt %d), the call that writes, 3 runs (ms): %s; %s" % (min_cnt, _ms3(ums), text))
    for islands in (False, True):
        cms, wall, res, stats = _clean3(lambda: km.clip(min_cnt=min_cnt, islands=islands))
        best = min(cms)
        print("clip (min_cnt %d, max_tip %d, max_mean 255, islands %d, at most 8 rounds), all kernels, 3 runs (ms): %s; wall: %s" % (min_cnt, 2 * km.k, islands, _ms3(cms), wall))
        print("clip rounds (unitigs removed, k-mers removed, keys left): %s" % " ".join("(%d, %d, %d)" % tuple(int(v) for v in r) for r in stats))
        print("clip best: %.3f ms = %.2f G k-mers of the input per second = %.2f x unitigs (%.3f ms); result 2^%d sub-tables of 2^%d slots; %s"
              % (best, nodes / best / 1e6, best / min(ums), min(ums), res.l_pre, res.cshift, _shape(res, min_cnt)[0]))
        res.close()


def pop_rates(min_cnt=1):
    print("build %s" % bfc_amd._lib.build_id())
    text, nodes, _ = _shape(km, min_cnt, True)
    print("input (min_cnt %d): %s" % (min_cnt, text))
    cms, _, res, stats = _clean3(lambda: km.clip(min_cnt=min_cnt))
    res.close()
    print("clip (max_tip %d, max_mean 255, at most 8 rounds), all kernels, 3 runs (ms): %s; %d rounds" % (2 * km.k, _ms3(cms), len(stats)))
    for max_diff in (0, 2):
        pms, wall, res, stats = _clean3(lambda: km.pop_bubbles(min_cnt=min_cnt, max_diff=max_diff))
        best = min(pms)
        print("pop_bubbles (min_cnt %d, max_arm %d, max_diff %d, max_mean 255, at most 8 rounds), all kernels, 3 runs (ms): %s; wall: %s" % (min_cnt, 2 * km.k, max_diff, _ms3(pms), wall))
        print("pop rounds (bubbles popped, k-mers removed, keys left): %s" % " ".join("(%d, %d, %d)" % tuple(int(v) for v in r) for r in stats))
        print("pop best: %.3f ms = %.2f G k-mers of the input per second = %.2f x clip (%.3f ms); result 2^%d sub-tables of 2^%d slots; %s"
              % (best, nodes / best / 1e6, best / min(cms), min(cms), res.l_pre, res.cshift, _shape(res, min_cnt, True)[0]))
        if max_diff == 0:
            dev_stats, dev_keys = stats, len(res.list(1)[1])
        res.close()
    t0 = time.perf_counter()
    t = g.export_table()
    t1 = time.perf_counter()
    print("export: %.1f ms" % ((t1 - t0) * 1e3), flush=True)
    h, hstats = t.pop_bubbles(min_cnt=min_cnt)
    t2 = time.perf_counter()
    print("export + host bfcg_pop_host (defaults), one thread: %.1f ms + %.1f ms = %.1f ms (%.0fx the kernels)" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, (t2 - t0) * 1e3 / best))
    assert np.array_equal(hstats, dev_stats) and h.count() == dev_keys
    print("the host's rounds and keys equal the device's")
    h.close()
    t.close()


if POP:
    pop_rates()
    km.close()
    g.close()
    sys.exit(0)

if CLIP:
    clip_rates()
    km.close()
    g.close()
    sys.exit(0)

if LINKS:
    link_rates()
    km.close()
    g.close()
    sys.exit(0)

if UNITIGS:
    unitig_rates()
    km.close()
    g.close()
    sys.exit(0)

if GRAPH:
    graph_rates()
    km.close()
    g.close()
    sys.exit(0)

if COMPARE:
    compare_rates()
    km.close()
    g.close()
    sys.exit(0)

if READSTATS:
    readstats_rates()
    km.close()
    g.close()
    sys.exit(0)

if LOOKUP:
    lookup_rates()
    km.close()
    g.close()
    sys.exit(0)


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
