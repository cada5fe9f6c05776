"""Rate of error correction on the GPU (bfcg_ec_batch: coverage pass + k_ec) against the reference's correction phase on the same host.

    python scripts/ec_rate.py --set ecoli   # E. coli 30x: gen.ReadSet(2, 4_600_000, 30.0), -k31 -b30, every read
    python scripts/ec_rate.py --set c3      # c3's read set (seed 3, 248 Mbp, 30x) with c3's table (-k33 -b35), a sample of its reads
    python scripts/ec_rate.py --refine      # `bfc -R` (bfcg_ec_batch_refine): E. coli 30x's first pass (run here, on the GPU) with every
                                            # ec:Z:0 comment's max_heap set to 60, so that every read is refined, on that file's own table
    python scripts/ec_rate.py --attach      # the hand-over from counting to correcting, timed from the end of the last count batch to the end
                                            # of the first corrected batch, twice in this process on the same input: (a) export_table() +
                                            # GpuCorrector(HostTable), (b) GpuCorrector(GpuCounter), i.e. bfcg_ec_attach (one JSON line)

The table is counted on the GPU and exported to the host (bfcg_ec_create uploads it once).  GPU time is bfcg_ec_last_ms summed over
batches (HIP events around the two kernels of a batch; inputs already staged); lookups are counted on the device.  The reference:
`bfc-ref -t16 -r <dump>` on the first --ref-reads reads, timed from its `bfc_correct ... Starting...` stamp to its exit.
Prints one JSON line."""
import argparse, json, os, re, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
import bfc_amd
from bfc_amd import gen, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--set", default="ecoli", choices=["ecoli", "c3"])
ap.add_argument("--reads", type=int, default=0, help="reads to correct on the GPU (0: ecoli all, c3 4M)")
ap.add_argument("--ref-reads", type=int, default=200_000, help="reads the reference corrects (0: skip)")
ap.add_argument("--batch", type=int, default=1 << 20, help="reads per bfcg_ec_batch")
ap.add_argument("--attach", action="store_true", help="time the hand-over of the table to the corrector, exported and attached, and exit")
ap.add_argument("--refine", action="store_true", help="then refine (-R) the first pass's output, every read (prints a second JSON line)")
args = ap.parse_args()

S = {"ecoli": dict(seed=2, G=4_600_000, cov=30.0, k=31, b=30, reads=0), "c3": dict(seed=3, G=248_000_000, cov=30.0, k=33, b=35, reads=4_000_000)}[args.set]
t0 = time.time()
rs = gen.ReadSet(seed=S["seed"], G=S["G"], cov=S["cov"])
stride = rs.L + 1
n_ec = args.reads or S["reads"] or rs.n_reads
CH = 2_000_000


def count_all():
    g = bfc_amd.GpuCounter(S["k"], S["b"], max_batch_pos=CH * stride)
    for r0 in range(0, rs.n_reads, CH):
        r1 = min(rs.n_reads, r0 + CH)
        seq, qual, off = rs.reads(r0, r1)
        g.count_host(bfc_amd.to_stream(seq, off), bfc_amd.to_stream(qual, off))
    return g


if args.attach:
    B = min(args.batch, n_ec)
    seq, qual, off = rs.reads(0, B)
    s0, q0 = bfc_amd.to_stream(seq, off), bfc_amd.to_stream(qual, off)
    opt = bfc_amd.bfc_opt_init(); opt.k = S["k"]
    res = dict(set=args.set, mode="attach", k=S["k"], b=S["b"], reads_counted=rs.n_reads, first_batch_reads=B)
    outs = {}
    for how in ("export", "attach"):
        g = count_all()
        g.sync()                                                 # the end of the last count batch
        t1 = time.perf_counter()
        t = g.export_table() if how == "export" else None
        t2 = time.perf_counter()
        c = bfc_amd.GpuCorrector(t if t is not None else g, opt, max_pos=B * stride, max_reads=B)
        t3 = time.perf_counter()
        outs[how] = c.correct_stream(s0.copy(), q0.copy(), np.arange(B + 1, dtype=np.uint64) * np.uint64(stride))
        t4 = time.perf_counter()
        km = bfc_amd.GpuKmers(g)                                 # (no upload: the context holds the same table in the host's layout by now)
        res[how] = dict(hand_over_s=round(t4 - t1, 4), export_s=round(t2 - t1, 4), create_s=round(t3 - t2, 4), first_batch_s=round(t4 - t3, 4),
                        first_batch_gpu_ms=round(c.last_ms(), 2), table_bytes=8 << (km.l_pre + km.cshift), mode=c.mode,
                        host_reads=c.host_reads(), retry_reads=c.retry_reads())
        km.close(); c.close(); g.close()
        if t is not None:
            t.close()
    res["same_output"] = all(np.array_equal(a, b) for a, b in zip(outs["export"], outs["attach"]))
    print(json.dumps(res))
    sys.exit(0)

g = count_all()
t = g.export_table()
g.close()
print("[ec_rate] %s: %d reads counted, table exported (%.1fs)" % (args.set, rs.n_reads, time.time() - t0), file=sys.stderr, flush=True)

opt = bfc_amd.bfc_opt_init(); opt.k = S["k"]
B = args.batch
c = bfc_amd.GpuCorrector(t, opt, max_pos=B * stride, max_reads=B)
L = _lib.load()
ms = 0.0; lookups = 0; n_done = 0; codes = np.zeros(8, dtype=np.int64); n_changed = 0
first = []                                                       # --refine: the corrected streams and their stats
for r0 in range(0, n_ec, B):
    r1 = min(n_ec, r0 + B)
    seq, qual, off = rs.reads(r0, r1)
    s, q = bfc_amd.to_stream(seq, off), bfc_amd.to_stream(qual, off)
    o = np.arange(r1 - r0 + 1, dtype=np.uint64) * np.uint64(stride)
    aux = np.zeros(r1 - r0, dtype=np.uint32); aux2 = np.zeros(r1 - r0, dtype=np.uint32)
    rc = L.bfcg_ec_batch(c.e, s.ctypes.data, q.ctypes.data, len(s), o.ctypes.data_as(_lib.u64p), r1 - r0,
                         aux.ctypes.data_as(_lib.u32p), aux2.ctypes.data_as(_lib.u32p))
    assert rc == 0, L.bfcg_last_error()
    ms += c.last_ms(); lookups += c.last_lookups(); n_done += r1 - r0
    codes += np.bincount(aux & 7, minlength=8); n_changed += int((aux >> 18).sum())
    if args.refine:
        first.append((s, q, aux, aux2))
n_kmers = n_done * (rs.L - S["k"] + 1)
res = dict(set=args.set, mode="table", k=S["k"], b=S["b"], reads=n_done, gpu_ms=round(ms, 2), gpu_reads_per_s=round(n_done / ms * 1e3),
           ec_lookups=lookups, lookups_per_read=round((lookups + n_kmers) / n_done, 1),
           lookups_per_s=round((lookups + n_kmers) / ms * 1e3), host_fallback_reads=c.host_reads(),
           host_fallback_share=c.host_reads() / n_done, ec_codes=[int(v) for v in codes[:6]], bases_changed=n_changed)
c.close()
if args.refine:
    print(json.dumps(res), flush=True)

if args.refine:
    # the first pass above left the corrected streams in `first`; -R counts that file and refines it.  The rewrite of every comment's
    # max_heap to 60 (rf_code 1, as parse_stats sets it) is applied to the stats directly: what bfcg_ec_parse_stats would return
    t.close()
    g = bfc_amd.GpuCounter(S["k"], S["b"], max_batch_pos=CH * stride)
    for s, q, _, _ in first:
        g.count_host(s, q)
    t = g.export_table()
    g.close()
    ropt = bfc_amd.bfc_opt_init(); ropt.k = S["k"]; ropt.refine_ec = 1
    c = bfc_amd.GpuCorrector(t, ropt, max_pos=B * stride, max_reads=B)
    ms = 0.0; lookups = 0; n_done = 0; rf = np.zeros(4, dtype=np.int64); codes = np.zeros(8, dtype=np.int64)
    for s, q, a0, a20 in first:
        n = len(a0)
        ec0 = (a0 & 7) == 0
        oa = np.where(ec0, a0, a0 & 7).astype(np.uint32)
        oa2 = np.where(ec0, (a20 & ~np.uint32(0x3ff)) | np.uint32(1 << 8 | 60), np.uint32(1 << 8)).astype(np.uint32)
        o = np.arange(n + 1, dtype=np.uint64) * np.uint64(stride)
        aux = np.zeros(n, dtype=np.uint32); aux2 = np.zeros(n, dtype=np.uint32)
        rc = L.bfcg_ec_batch_refine(c.e, s.ctypes.data, q.ctypes.data, len(s), o.ctypes.data_as(_lib.u64p), n, oa.ctypes.data_as(_lib.u32p),
                                    oa2.ctypes.data_as(_lib.u32p), aux.ctypes.data_as(_lib.u32p), aux2.ctypes.data_as(_lib.u32p))
        assert rc == 0, L.bfcg_last_error()
        ms += c.last_ms(); lookups += c.last_lookups(); n_done += n
        rf += np.bincount(aux2 >> 8 & 3, minlength=4); codes += np.bincount(aux & 7, minlength=8)
    n_kmers = n_done * (rs.L - S["k"] + 1)
    res = dict(set=args.set, mode="refine", k=S["k"], b=S["b"], reads=n_done, gpu_ms=round(ms, 2), gpu_reads_per_s=round(n_done / ms * 1e3),
               ec_lookups=lookups, lookups_per_read=round((lookups + n_kmers) / n_done, 1), lookups_per_s=round((lookups + n_kmers) / ms * 1e3),
               host_fallback_reads=c.host_reads(), ec_codes=[int(v) for v in codes[:6]], rf_codes=[int(v) for v in rf])
    c.close(); t.close()
    print(json.dumps(res))
    sys.exit(0)

ref = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "bfc-ref")
if args.ref_reads and os.path.exists(ref):
    with tempfile.TemporaryDirectory() as d:
        fq, dump = os.path.join(d, "s.fq"), os.path.join(d, "t.hash")
        rs.fastq(fq, 0, args.ref_reads)
        t.dump(dump)
        t1 = time.time()
        r = subprocess.run([ref, "-t16", "-k", str(S["k"]), "-r", dump, fq], capture_output=True, timeout=560)
        wall = time.time() - t1
        err = r.stderr.decode()
        m = re.search(r"\[M::bfc_correct @([0-9.]+)\*", err)
        m_end = re.findall(r"\[M::bfc_ec_cb @([0-9.]+)\*", err)
        assert r.returncode == 0 and m and m_end, err[-1000:]
        ec_s = float(m_end[-1]) - float(m.group(1))
        res.update(ref_reads=args.ref_reads, ref_threads=16, ref_correct_s=round(ec_s, 2), ref_reads_per_s=round(args.ref_reads / ec_s),
                   ref_wall_s=round(wall, 1), speedup_vs_ref_t16=round((n_done / ms * 1e3) / (args.ref_reads / ec_s), 1))
t.close()
print(json.dumps(res))
