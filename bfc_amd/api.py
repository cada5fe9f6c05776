"""Python mirror of the reference's count-phase interface on top of the C ABI (libbfc_gpu.so).

Names follow the reference: ``bfc_opt_init`` (bfc.c:17-40), ``bfc_opt_by_size`` (bfc.c:42-53),
``bfc_count`` (count.c:127), and the query surface of ``bfc_ch_t`` / ``bfc_bf_t`` (htab.h, bbf.h).
``GpuCounter`` is the device-level interface (batches of reads already in memory).
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import BfcOpt, BfcgParams, BfcKmer, u64p, u32p, f32p

STAT_NAMES = {0: "n_kmers", 1: "n_high", 2: "n_seen", 3: "n_keys", 4: "tab_ovf", 5: "err_pool", 6: "slow_buckets", 7: "crowded_regions", 8: "tab_cshift", 9: "n_batches"}


class BfcGpuError(RuntimeError):
    pass


def bfc_opt_init():
    """Defaults of bfc.c:17-40."""
    o = BfcOpt()
    o.chunk_size = 100000000
    o.n_threads = 1
    o.q = 20
    o.k = 33
    o.l_pre = 20
    o.bf_shift = 33
    o.n_hashes = 4
    o.min_frac = 0.9
    o.min_cov = 3
    o.win_multi_ec = 10
    o.max_end_ext = 5
    o.w_ec, o.w_ec_high, o.w_absent, o.w_absent_high = 1, 7, 3, 1
    o.max_path_diff, o.max_heap = 15, 100
    return o


def bfc_opt_by_size(opt, size):
    """`-s`: bfc.c:42-53."""
    bits = math.log(size) / math.log(2)
    opt.k = int(bits + 1.0)
    if opt.k & 1 == 0:
        opt.k += 1
    opt.k = min(opt.k, 63)
    opt.bf_shift = min(int(bits + 8.0), 37)
    return opt


def to_stream(seq, off):
    """(concatenated reads, offsets) -> separator-delimited stream (one '\\n' after each read)."""
    off = np.asarray(off, dtype=np.int64)
    n = len(off) - 1
    out = np.empty(len(seq) + n, dtype=np.uint8)
    lens = np.diff(off)
    if n and np.all(lens == lens[0]):
        L = int(lens[0])
        v = out.reshape(n, L + 1)
        v[:, :L] = np.asarray(seq).reshape(n, L)
        v[:, L] = 10
    else:
        pos = off[:-1] + np.arange(n)
        mask = np.ones(len(out), dtype=bool)
        mask[off[1:] + np.arange(n)] = False
        out[mask] = seq
        out[~mask] = 10
        del pos
    return out


def _read_stats_args(seq_stream, off):
    """(stream or None, offsets u64, the result's array) of a read_stats() call"""
    s = np.ascontiguousarray(seq_stream, dtype=np.uint8) if seq_stream is not None else None
    off = np.ascontiguousarray(off, dtype=np.uint64)
    if off.ndim != 1 or len(off) < 1:
        raise BfcGpuError("read_stats needs off[n_reads + 1], the reads' stream offsets")
    return s, off, np.zeros((len(off) - 1, 8), dtype=np.int32)


def format_read_stats(out):
    """bfcg_read_stats_format's lines for an (n, 8) result, formatted in C: bytes."""
    out = np.ascontiguousarray(out, dtype=np.int32).reshape(-1, 8)
    buf = C.create_string_buffer(max(1, 110 * len(out)))
    n = _lib.load().bfcg_read_stats_format(out.ctypes.data, len(out), buf)
    return buf.raw[:n]


# ---- the table as a de Bruijn graph (bfcg_graph.hip): degree cells and their masks ------------------------------------------------------
# cell 5 * o + i: o present successors, i present predecessors, on the strand the table stores; the four classes below are symmetric in
# (o, i), so they mean the same on either strand
GRAPH_MASKS = {
    "tips": sum(1 << (5 * o + i) for o in range(5) for i in range(5) if (o == 0) != (i == 0)),
    "isolated": 1,
    "branching": sum(1 << (5 * o + i) for o in range(5) for i in range(5) if o >= 2 or i >= 2),
    "simple": 1 << 6,
    "all": (1 << 25) - 1,
}

CLIP_ISLANDS = 1  # BFCG_CLIP_ISLANDS

_POP4 = np.array([bin(i).count("1") for i in range(16)], dtype=np.int64)


def kmer_revcomp(k, y):
    """The planes of the reverse complements of y (n, 2) u64 (bfcg_kmer_revcomp; no GPU)."""
    y = np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 2)
    out, L = np.zeros_like(y), _lib.load()
    for i in range(len(y)):
        if L.bfcg_kmer_revcomp(int(k), y[i].ctypes.data_as(u64p), out[i].ctypes.data_as(u64p)) != 0:
            raise BfcGpuError("k=%d is outside [1, 63]" % k)
    return out


def nb_text(nb):
    """The neighbour bits of one k-mer as text, "successors<TAB>predecessors": the bases present on each side, '.' for none."""
    nb = int(nb)
    return "%s\t%s" % ("".join("ACGT"[c] for c in range(4) if nb >> c & 1) or ".", "".join("ACGT"[c] for c in range(4) if nb >> (4 + c) & 1) or ".")


def _graph_seeds(y, max_len):
    """(y (n, 2) u64, bases (n, max_len) u8, len_stop (n, 2) i32) of an extend() call"""
    y = np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 2)
    return y, np.zeros((len(y), max(0, int(max_len))), dtype=np.uint8), np.zeros((len(y), 2), dtype=np.int32)


def _unitigs(L, fn, obj, min_cnt):
    """(seq u8, off u64 (n + 1), n_kmers u32, cnt_sum u64, ends u8) of bfcg_kmers_unitigs / bfcg_unitigs_host on `obj`: the sizing call
    with caps of 0, then the call that writes."""
    n = (C.c_uint64 * 2)()
    rc = fn(obj, int(min_cnt), None, 0, None, None, None, None, 0, n)
    if rc < 0:
        raise BfcGpuError(L.bfcg_last_error().decode())
    seq, off = np.zeros(n[1], dtype=np.uint8), np.zeros(n[0] + 1, dtype=np.uint64)
    nk, cs, ends = np.zeros(n[0], dtype=np.uint32), np.zeros(n[0], dtype=np.uint64), np.zeros(n[0], dtype=np.uint8)
    if rc == 1 and fn(obj, int(min_cnt), seq.ctypes.data, len(seq), off.ctypes.data, nk.ctypes.data, cs.ctypes.data, ends.ctypes.data, len(nk), n) != 0:
        raise BfcGpuError(L.bfcg_last_error().decode() or "the table changed between the sizing call and the call that writes")
    return seq, off, nk, cs, ends


def _unitig_graph(L, fn, obj, min_cnt):
    """(seq, off, n_kmers, cnt_sum, ends as _unitigs gives them, links i64 (n, 2, 4)) of bfcg_kmers_unitig_graph / bfcg_unitig_graph_host
    on `obj`: the sizing call with caps of 0, then the call that writes; the edges it counted are those it wrote"""
    n = (C.c_uint64 * 3)()
    rc = fn(obj, int(min_cnt), None, 0, None, None, None, None, None, 0, n)
    if rc < 0:
        raise BfcGpuError(L.bfcg_last_error().decode())
    seq, off = np.zeros(n[1], dtype=np.uint8), np.zeros(n[0] + 1, dtype=np.uint64)
    nk, cs, ends = np.zeros(n[0], dtype=np.uint32), np.zeros(n[0], dtype=np.uint64), np.zeros(n[0], dtype=np.uint8)
    links = np.full((n[0], 2, 4), -1, dtype=np.int64)
    if rc == 1 and fn(obj, int(min_cnt), seq.ctypes.data, len(seq), off.ctypes.data, nk.ctypes.data, cs.ctypes.data, ends.ctypes.data, links.ctypes.data, len(nk), n) != 0:
        raise BfcGpuError(L.bfcg_last_error().decode() or "the table changed between the sizing call and the call that writes")
    if rc == 1 and int(n[2]) != int((links >= 0).sum()):
        raise BfcGpuError("the call counted %d links and wrote %d" % (n[2], (links >= 0).sum()))
    return seq, off, nk, cs, ends, links


def _clean(L, fn, obj, max_rounds, *rule):
    """(pointer to the new table, stats u64 (rounds, 3)) of a graph-cleaning call on `obj` -- bfcg_kmers_clip / bfcg_clip_host,
    bfcg_kmers_pop / bfcg_pop_host; `rule` = its arguments between the table and max_rounds"""
    stats, n = np.zeros((max(0, min(int(max_rounds), 64)), 3), dtype=np.uint64), C.c_int(0)
    p = fn(obj, *(int(v) for v in rule), int(max_rounds), stats.ctypes.data, C.byref(n))
    if not p:
        raise BfcGpuError(L.bfcg_last_error().decode())
    return p, stats[:n.value].copy()


def _listing(parts, *extra):
    """(y (n, 2) u64, count u8, high u8, a column of each dtype in `extra`) of the pieces that pieces(), pieces_vs() or pieces_graph() yield"""
    parts = list(parts)
    y, ch, *more = [np.concatenate([p[i] for p in parts]) if parts else np.zeros((0, 2) if i == 0 else 0, dtype=dt)
                    for i, dt in enumerate((np.uint64, np.uint16) + extra)]
    return (y, (ch & 0xff).astype(np.uint8), (ch >> 8).astype(np.uint8), *more)


def unitig_rows(seq, off, n_kmers, cnt_sum, ends):
    """The five arrays of unitigs() as a sorted list of (sequence bytes, n_kmers, cnt_sum, left stop, right stop, cycle 0 / 1)."""
    s = np.asarray(seq, dtype=np.uint8).tobytes()
    return sorted((s[int(off[i]):int(off[i + 1])], int(n_kmers[i]), int(cnt_sum[i]), int(ends[i]) & 7, int(ends[i]) >> 3 & 7, int(ends[i]) >> 6 & 1)
                  for i in range(len(n_kmers)))


def unitig_link_rows(seq, off, links):
    """The links of unitig_graph() as a sorted list of (spelling of u, o, c, spelling of v, p): an edge from oriented unitig (u, o) -- o = 1
    is the reverse complement of the emitted spelling -- by base c (A C G T = 0..3) to (v, p).  The spellings are the emitted ones."""
    s = np.asarray(seq, dtype=np.uint8).tobytes()
    name = [s[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2, 4)
    return sorted((name[u], int(o), int(c), name[int(links[u, o, c]) >> 1], int(links[u, o, c]) & 1) for u, o, c in zip(*np.nonzero(links >= 0)))


class HostTable:
    """A host-resident ``bfc_ch_t`` (opaque, htab.h:10-23)."""

    def __init__(self, ptr):
        if not ptr:
            raise BfcGpuError("NULL bfc_ch_t")
        self.L = _lib.load()
        self.ptr = ptr

    def close(self):
        if self.ptr:
            self.L.bfc_ch_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def k(self):
        return self.L.bfc_ch_get_k(self.ptr)

    @property
    def l_pre(self):
        return self.L.bfc_ch_get_lpre(self.ptr)

    def get(self, y0, y1):
        return self.L.bfc_ch_get(self.ptr, (C.c_uint64 * 2)(y0, y1))

    def kmer_occ(self, x):
        z = BfcKmer()
        for i in range(4):
            z.x[i] = int(x[i])
        return self.L.bfc_ch_kmer_occ(self.ptr, C.byref(z))

    def occ_planes(self, y):
        """bfc_ch_kmer_occ of k-mers given as listing-style planes, y (n, 2) u64, of either strand: int16 (n), -1 = absent.  The host
        twin of GpuKmers.lookup (bfcg_kmers_occ_host)."""
        y = np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 2)
        out = np.empty(len(y), dtype=np.int16)
        self.L.bfcg_kmers_occ_host(self.ptr, y.ctypes.data, len(y), out.ctypes.data)
        return out

    def read_stats(self, seq_stream, off, min_cov=3):
        """Per-read statistics of a batch stream against this table, int32 (n_reads, 8) as GpuKmers.read_stats gives them: its host
        twin (bfcg_read_stats_host)."""
        s, off, out = _read_stats_args(seq_stream, off)
        if self.L.bfcg_read_stats_host(self.ptr, s.ctypes.data, len(s), off.ctypes.data, len(off) - 1, int(min_cov), out.ctypes.data) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return out

    def neighbors(self, y):
        """The values of the eight de Bruijn neighbours of k-mers y (n, 2) u64: int16 (n, 8), columns 0-3 succ by A C G T, 4-7 pred.
        The host twin of GpuKmers.neighbors (bfcg_neighbors_host)."""
        y = np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 2)
        out = np.empty((len(y), 8), dtype=np.int16)
        if self.L.bfcg_neighbors_host(self.ptr, y.ctypes.data, len(y), out.ctypes.data) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return out

    def graph_census(self, min_cnt=1):
        """u64 (5, 5): [o, i] = the k-mers with count >= min_cnt that have o present successors and i present predecessors
        (bfcg_graph_census_host)."""
        deg = np.zeros(25, dtype=np.uint64)
        if self.L.bfcg_graph_census_host(self.ptr, int(min_cnt), deg.ctypes.data_as(u64p)) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return deg.reshape(5, 5)

    def graph_nb(self, min_cnt=1):
        """(y (n, 2) u64, nb u8 (n)) for every slot of export_sorted(), in its order: the planes and the neighbour bits (0 where the
        count is below min_cnt): bfcg_graph_nb_host."""
        n = self.L.bfcg_graph_nb_host(self.ptr, int(min_cnt), None, None)
        if n < 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        y, nb = np.zeros((n, 2), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
        if self.L.bfcg_graph_nb_host(self.ptr, int(min_cnt), y.ctypes.data, nb.ctypes.data) != n:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return y, nb

    def list_graph(self, min_cnt=1, cell_mask=GRAPH_MASKS["all"]):
        """(y, count u8, high u8, nb u8) of the k-mers with count >= min_cnt whose degree cell is in cell_mask, in export_sorted()'s
        order: the host twin of GpuKmers.list_graph, from graph_nb()."""
        if not 0 < int(cell_mask) < 1 << 25:
            raise BfcGpuError("cell_mask 0x%x names no cell or one beyond bit 24" % int(cell_mask))
        y, nb = self.graph_nb(min_cnt)
        slots = self.export_sorted()[1]
        cnt = (slots & np.uint64(0xff)).astype(np.uint8)
        cell = 5 * _POP4[nb & 15] + _POP4[nb >> 4]
        keep = (cnt >= min_cnt) & ((np.uint32(cell_mask) >> cell.astype(np.uint32)) & np.uint32(1)).astype(bool)
        return y[keep], cnt[keep], (slots >> np.uint64(8) & np.uint64(0x3f)).astype(np.uint8)[keep], nb[keep]

    def extend(self, y, min_cnt=1, max_len=300):
        """(bases u8 (n, max_len), length i32, stop i32): GpuKmers.extend's host twin (bfcg_extend_host)."""
        y, bases, ls = _graph_seeds(y, max_len)
        if self.L.bfcg_extend_host(self.ptr, y.ctypes.data, len(y), int(min_cnt), int(max_len), bases.ctypes.data, ls.ctypes.data) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return bases, ls[:, 0].copy(), ls[:, 1].copy()

    def unitigs(self, min_cnt=1):
        """(seq u8, off u64 (n + 1), n_kmers u32, cnt_sum u64, ends u8): GpuKmers.unitigs's host twin (bfcg_unitigs_host)."""
        return _unitigs(self.L, self.L.bfcg_unitigs_host, self.ptr, min_cnt)

    def unitig_graph(self, min_cnt=1):
        """(seq, off, n_kmers, cnt_sum, ends, links i64 (n, 2, 4)): GpuKmers.unitig_graph's host twin (bfcg_unitig_graph_host)."""
        return _unitig_graph(self.L, self.L.bfcg_unitig_graph_host, self.ptr, min_cnt)

    def clip(self, min_cnt=1, max_tip=None, max_mean=255, islands=False, max_rounds=8):
        """(HostTable, stats u64 (rounds, 3)): GpuKmers.clip's host twin (bfcg_clip_host)."""
        p, stats = _clean(self.L, self.L.bfcg_clip_host, self.ptr, max_rounds, min_cnt, 2 * self.k if max_tip is None else max_tip, max_mean, CLIP_ISLANDS if islands else 0)
        return HostTable(p), stats

    def pop_bubbles(self, min_cnt=1, max_arm=None, max_diff=0, max_mean=255, max_rounds=8):
        """(HostTable, stats u64 (rounds, 3)): GpuKmers.pop_bubbles's host twin (bfcg_pop_host)."""
        p, stats = _clean(self.L, self.L.bfcg_pop_host, self.ptr, max_rounds, min_cnt, 2 * self.k if max_arm is None else max_arm, max_diff, max_mean)
        return HostTable(p), stats

    def insert(self, y0, y1, is_high, forced=1):
        return self.L.bfc_ch_insert(self.ptr, (C.c_uint64 * 2)(y0, y1), int(is_high), forced)

    def count(self):
        return int(self.L.bfc_ch_count(self.ptr))

    def hist(self):
        cnt = np.zeros(256, dtype=np.uint64)
        high = np.zeros(64, dtype=np.uint64)
        mode = self.L.bfc_ch_hist(self.ptr, cnt.ctypes.data_as(u64p), high.ctypes.data_as(u64p))
        return mode, cnt, high

    def dump(self, fn):
        return self.L.bfc_ch_dump(self.ptr, fn.encode())

    def export_sorted(self):
        sizes = np.zeros(1 << self.l_pre, dtype=np.uint32)
        n = self.L.bfc_ch_export_sorted(self.ptr, sizes.ctypes.data_as(u32p), None)
        slots = np.zeros(int(n), dtype=np.uint64)
        self.L.bfc_ch_export_sorted(self.ptr, sizes.ctypes.data_as(u32p), slots.ctypes.data_as(u64p))
        return sizes, slots

    @staticmethod
    def init(k, l_pre):
        return HostTable(_lib.load().bfc_ch_init(k, l_pre))

    @staticmethod
    def from_slots(k, l_pre, cshift, slots):
        """A table whose slots the caller wrote: `slots` u64 of 2^(l_pre + cshift) entries, sub-table s in [s << cshift, (s + 1) << cshift),
        copied in as they lie and then counted.  Nothing is checked beyond the length: a key that linear probing from its home slot
        does not reach is simply not found.  cshift >= 1: nothing in the library makes a table of one slot per sub-table."""
        k, l_pre, cshift = int(k), int(l_pre), int(cshift)
        slots = np.ascontiguousarray(slots, dtype=np.uint64).reshape(-1)
        if not 1 <= k <= 63 or l_pre < 0 or cshift < 1 or l_pre + cshift > 40:
            raise BfcGpuError("from_slots: k=%d l_pre=%d cshift=%d is no table geometry (k in [1, 63], cshift >= 1)" % (k, l_pre, cshift))
        if len(slots) != 1 << (l_pre + cshift):
            raise BfcGpuError("from_slots: %d slots given, l_pre=%d and cshift=%d make %d" % (len(slots), l_pre, cshift, 1 << (l_pre + cshift)))
        L = _lib.load()
        t = HostTable(L.bfc_ch_alloc_raw(k, l_pre, cshift))
        C.memmove(L.bfc_ch_raw_slots(t.ptr), slots.ctypes.data, slots.nbytes)
        L.bfc_ch_raw_recount(t.ptr)
        return t

    def raw(self):
        """(cshift, a copy of the 2^(l_pre + cshift) slots as they lie)."""
        cshift = self.L.bfc_ch_raw_cshift(self.ptr)
        n = 1 << (self.l_pre + cshift)
        return cshift, np.ctypeslib.as_array(self.L.bfc_ch_raw_slots(self.ptr), shape=(n,)).copy()

    @staticmethod
    def restore(fn):
        p = _lib.load().bfc_ch_restore(fn.encode())
        return HostTable(p) if p else None


class HostBloom:
    """A host-resident ``bfc_bf_t`` (bbf.h:9-12)."""

    def __init__(self, ptr):
        if not ptr:
            raise BfcGpuError("NULL bfc_bf_t")
        self.L = _lib.load()
        self.ptr = ptr

    def close(self):
        if self.ptr:
            self.L.bfc_bf_destroy(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_shift(self):
        return self.ptr.contents.n_shift

    @property
    def n_hashes(self):
        return self.ptr.contents.n_hashes

    def bytes(self):
        return np.ctypeslib.as_array(self.ptr.contents.b, shape=(1 << (self.n_shift - 3),))

    def get(self, h):
        return self.L.bfc_bf_get(self.ptr, h)

    def insert(self, h):
        return self.L.bfc_bf_insert(self.ptr, h)

    @staticmethod
    def init(n_shift, n_hashes):
        p = _lib.load().bfc_bf_init(n_shift, n_hashes)
        return HostBloom(p) if p else None


def bfc_count(fn, opt):
    """count.c:127: count the k-mers of file `fn` on the GPU; returns HostTable or (filter mode) HostBloom."""
    L = _lib.load()
    p = L.bfc_count(fn.encode(), C.byref(opt))
    if opt.filter_mode:
        return HostBloom(C.cast(p, C.POINTER(_lib.BfcBf)))
    return HostTable(p)


def pack_planes(seq_stream, qual_stream, q, n_chunks=1):
    """The four bit planes of a byte-stream batch (bfcg_pack_planes; no GPU involved): uint32 array [4, bfcg_plane_words(n)].
    n_chunks > 1 packs the stream as that many word ranges one after the other (what disjoint threads would each take: tests of the seams)."""
    L = _lib.load()
    seq_stream = np.ascontiguousarray(seq_stream, dtype=np.uint8)
    qs = np.ascontiguousarray(qual_stream, dtype=np.uint8) if qual_stream is not None else None
    n = len(seq_stream)
    pw = int(L.bfcg_plane_words(n))
    planes = np.zeros((4, pw), dtype=np.uint32)
    if qs is None:
        planes[3, :] = 0xffffffff
    step = ((n + n_chunks - 1) // n_chunks + 31) // 32 * 32 if n_chunks > 1 else max(n, 32)
    for lo in range(0, n, max(step, 32)):
        L.bfcg_pack_planes(seq_stream.ctypes.data, qs.ctypes.data if qs is not None else None, lo, min(n, lo + max(step, 32)), n, q, planes.ctypes.data, pw)
    return planes


class GpuCounter:
    """Device-level counting context (bfcg_ctx_t)."""

    def __init__(self, k, bf_shift, q=20, n_hashes=4, l_pre=20, filter_mode=0, device=0, max_batch_pos=1 << 24,
                 region_shift=0, tab_cshift=0, debug_seen=False, rank=0, n_ranks=1, track_order=False, table_layout=0):
        self.L = _lib.load()
        p = BfcgParams()
        self.L.bfcg_params_default(C.byref(p))
        p.k, p.q, p.bf_shift, p.n_hashes, p.l_pre, p.filter_mode = k, q, bf_shift, n_hashes, l_pre, filter_mode
        p.device, p.max_batch_pos, p.region_shift, p.tab_cshift, p.debug_seen = device, int(max_batch_pos), region_shift, tab_cshift, int(debug_seen)
        p.rank, p.n_ranks, p.track_order, p.table_layout = rank, n_ranks, int(track_order), int(table_layout)
        self.rank, self.n_ranks = rank, n_ranks
        self.params = p
        self.bf_shift, self.k = bf_shift, k
        self.ctx = self.L.bfcg_create(C.byref(p))
        if not self.ctx:
            raise BfcGpuError("bfcg_create failed: " + self.L.bfcg_last_error().decode())

    @classmethod
    def _view(cls, ctx, params, n_ranks):
        """A GpuCounter over a context somebody else owns (a group's rank)."""
        self = cls.__new__(cls)
        self.L = _lib.load()
        self.ctx, self.params, self._borrowed = ctx, params, True
        self.rank, self.n_ranks, self.bf_shift, self.k = 0, n_ranks, params.bf_shift, params.k
        return self

    def _ck(self, rc):
        if rc != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())

    def close(self):
        if self.ctx and not getattr(self, "_borrowed", False):
            self.L.bfcg_destroy(self.ctx)
        self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._ck(self.L.bfcg_reset(self.ctx))

    def count_host(self, seq_stream, qual_stream=None):
        seq_stream = np.ascontiguousarray(seq_stream, dtype=np.uint8)
        q = np.ascontiguousarray(qual_stream, dtype=np.uint8) if qual_stream is not None else None
        self._ck(self.L.bfcg_count_batch_host(self.ctx, seq_stream.ctypes.data, q.ctypes.data if q is not None else None, len(seq_stream)))

    def count_planes(self, planes, first_pos, n_pos, has_qual=True):
        """positions [first_pos, first_pos + n_pos) of a plane set made by pack_planes (4 bits per position over PCIe instead of 16)"""
        planes = np.ascontiguousarray(planes, dtype=np.uint32)
        assert planes.ndim == 2 and planes.shape[0] == 4
        self._ck(self.L.bfcg_count_batch_planes(self.ctx, planes.ctypes.data, planes.shape[1], first_pos, n_pos, 1 if has_qual else 0))

    def count_dev(self, d_seq, d_qual, n_pos):
        self._ck(self.L.bfcg_count_batch_dev(self.ctx, d_seq, d_qual, n_pos))

    # ---- multi-GPU stages (owner computes): what bfcg_group_* drives from inside the library; exposed for tests (tests/mg_protocol.py)
    def mg_info(self):
        out = (C.c_int * 4)()
        self.L.bfcg_mg_info(self.ctx, out)
        return dict(nb1=out[0], nb_loc=out[1], rec_bytes=out[2], n_ranks=out[3])

    def batch_limit(self):
        """positions per batch (per rank: of the global batch / n_ranks) the filter's regions take at full speed"""
        return int(self.L.bfcg_batch_limit(self.ctx))

    def mg_scatter(self, d_seq, d_qual, n_pos, d_send):
        counts = np.zeros(self.mg_info()["nb1"], dtype=np.uint32)
        self._ck(self.L.bfcg_mg_scatter(self.ctx, d_seq, d_qual, n_pos, d_send, counts.ctypes.data_as(u32p)))
        return counts

    def mg_process(self, d_recv, seg_cnt):
        seg_cnt = np.ascontiguousarray(seg_cnt, dtype=np.uint32)
        self._ck(self.L.bfcg_mg_process(self.ctx, d_recv, seg_cnt.ctypes.data_as(u32p)))

    def dev_alloc(self, nbytes):
        p = self.L.bfcg_dev_alloc(self.ctx, nbytes)
        if not p:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return p

    def dev_free(self, p):
        self.L.bfcg_dev_free(self.ctx, p)

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._ck(self.L.bfcg_h2d(self.ctx, dptr, arr.ctypes.data, arr.nbytes))

    def sync(self):
        self._ck(self.L.bfcg_sync(self.ctx))

    def stats(self):
        out = np.zeros(16, dtype=np.uint64)
        self._ck(self.L.bfcg_stats(self.ctx, out.ctypes.data_as(u64p)))
        d = {STAT_NAMES[i]: int(out[i]) for i in STAT_NAMES}
        d["stream_batches"] = int(self.L.bfcg_stream_batches(self.ctx))
        d["phase_cycles"] = [int(out[i]) for i in range(10, 16)]  # BFCG_ABLATE&64: k_bloom stage/pass1/pass2/writeback/handover
        return d

    def table_info(self):
        """How the count table is held right now: region-owned segments (updated through LDS) or the host's (sub-table, key) layout."""
        out = (C.c_int * 4)()
        self.L.bfcg_table_info(self.ctx, out)
        return dict(segments=bool(out[0]), seg_shift=out[1], tab_cshift=out[2], seg_growths=out[3])

    def seg_place(self, y0, y1):
        """Where this context's geometry puts the k-mer with table hash (y0, y1): (region, identity in the region, home, block)."""
        out = (C.c_uint64 * 4)()
        self.L.bfcg_seg_place(self.ctx, int(y0), int(y1), out)
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def commit_info(self):
        """What the table's write path has done since the context was created; complete after sync()."""
        out = (C.c_uint64 * 8)()
        self.L.bfcg_commit_info(self.ctx, out)
        return dict(seg_replayed=int(out[0]), table_replayed=int(out[1]), commits=int(out[2]), max_commit_pages=int(out[3]), to_host_layout=int(out[4]))

    def progress(self, n=63):
        """(calls made, last call known complete, [distinct keys after call final, final - 1, ...]) without draining the pipeline."""
        calls, final = C.c_uint64(), C.c_uint64()
        keys = (C.c_uint64 * 63)()
        self.L.bfcg_progress(self.ctx, C.byref(calls), C.byref(final), keys, min(n, 63))
        return int(calls.value), int(final.value), [int(keys[i]) for i in range(min(n, 63, int(final.value)))]

    def partition_info(self):
        out = (C.c_uint64 * 2)()
        self.L.bfcg_partition_info(self.ctx, out)
        return dict(one_pass=bool(out[0] & 1), level2_one_pass=bool(out[0] & 2), replayed_batches=int(out[1]))

    def s1wc_launches(self):
        """Launches of k_scatter1_wc (level 1 through write-combining buffers in LDS) by this process so far."""
        return int(self.L.bfcg_s1wc_launches())

    def last_batch_ms(self):
        out = np.zeros(6, dtype=np.float32)
        self.L.bfcg_last_batch_ms(self.ctx, out.ctypes.data_as(f32p))
        return dict(hist1=float(out[0]), scatter1=float(out[1]), level2=float(out[2]), bloom=float(out[3]), commit=float(out[4]), total=float(out[5]))

    def stage_ms(self, reset=False):
        """Cumulative per-stage GPU ms over all batches since the last reset, and their number (drains the pipeline)."""
        out = (C.c_double * 6)()
        n = C.c_uint64()
        self._ck(self.L.bfcg_stage_ms(self.ctx, out, C.byref(n), int(reset)))
        return dict(hist1=out[0], scatter1=out[1], level2=out[2], bloom=out[3], commit=out[4], total=out[5]), int(n.value)

    def bloom_bytes(self, which=0):
        out = np.empty((1 << (self.bf_shift - 3)) // self.n_ranks, dtype=np.uint8)  # the slice this rank owns
        self._ck(self.L.bfcg_bloom_to_host(self.ctx, which, out.ctypes.data))
        return out

    def export_bloom(self, which=0, resident=False):
        """Host bfc_bf_t of filter `which`; resident=True also leaves a copy in HBM for a GpuTrimmer to adopt (what bfc_count does)."""
        p = (self.L.bfcg_export_bloom_resident if resident else self.L.bfcg_export_bloom)(self.ctx, which)
        if not p:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return HostBloom(p)

    def export_table(self):
        p = self.L.bfcg_export_table(self.ctx)
        if not p:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return HostTable(p)

    def hash_positions(self, seq_stream, qual_stream=None):
        seq_stream = np.ascontiguousarray(seq_stream, dtype=np.uint8)
        q = np.ascontiguousarray(qual_stream, dtype=np.uint8) if qual_stream is not None else None
        out = np.zeros((len(seq_stream), 3), dtype=np.uint64)
        self._ck(self.L.bfcg_hash_positions(self.ctx, seq_stream.ctypes.data, q.ctypes.data if q is not None else None, len(seq_stream), out.ctypes.data_as(u64p)))
        return out

    def seen_flags(self, n_pos):
        out = np.zeros(n_pos, dtype=np.uint8)
        self._ck(self.L.bfcg_seen_flags(self.ctx, out.ctypes.data, n_pos))
        return out


class GpuGroup:
    """The local ranks of a multi-GPU run, driven inside libbfc_gpu.so (bfcg_group_t): stage A, the exchange of the k-mer records over RCCL
    (or peer copies between the devices of one process) and stage B, one host thread per rank.  `devices` lists the local ranks' devices --
    all ranks of the run (one process), or one of them together with `uid` (one process per GPU).  A device may be repeated: ranks emulated
    on one GPU.  max_batch_pos = positions of ONE rank's share of a global batch."""

    def __init__(self, k, bf_shift, devices, max_batch_pos, n_ranks=None, first_rank=0, uid=None, transport=0, q=20, n_hashes=4, l_pre=20,
                 filter_mode=0, track_order=False, table_layout=0, region_shift=0, tab_cshift=0):
        self.L = _lib.load()
        p = BfcgParams()
        self.L.bfcg_params_default(C.byref(p))
        p.k, p.q, p.bf_shift, p.n_hashes, p.l_pre, p.filter_mode = k, q, bf_shift, n_hashes, l_pre, filter_mode
        p.max_batch_pos, p.region_shift, p.tab_cshift, p.track_order, p.table_layout = int(max_batch_pos), region_shift, tab_cshift, int(track_order), int(table_layout)
        self.params, self.k, self.bf_shift = p, k, bf_shift
        self.devices = list(devices)
        self.n_local = len(self.devices)
        self.n_ranks = n_ranks if n_ranks is not None else self.n_local
        dv = (C.c_int * self.n_local)(*self.devices)
        self._uid = (C.c_uint8 * 128).from_buffer_copy(bytes(uid)) if uid is not None else None
        self.g = self.L.bfcg_group_create(C.byref(p), self.n_ranks, first_rank, self.n_local, dv, self._uid, transport)
        if not self.g:
            raise BfcGpuError("bfcg_group_create failed: " + self.L.bfcg_last_error().decode())

    @staticmethod
    def unique_id():
        L = _lib.load()
        buf = (C.c_uint8 * 128)()
        if L.bfcg_group_unique_id(buf) != 0:
            raise BfcGpuError(L.bfcg_last_error().decode())
        return bytes(buf)

    def _ck(self, rc):
        if rc != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())

    def close(self):
        if self.g:
            self.L.bfcg_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = (C.c_int * 6)()
        self.L.bfcg_group_info(self.g, out)
        return dict(n_ranks=out[0], n_local=out[1], transport={1: "rccl", 2: "peer", 3: "push"}.get(out[2], out[2]), rec_bytes=out[3], nb1=out[4], first_rank=out[5],
                    slab_mode=bool(self.L.bfcg_group_slab_mode(self.g)), lazy_batches=int(self.L.bfcg_group_lazy_batches(self.g)))

    def exchange_bytes(self):
        """Bytes the local ranks put on the links since creation / reset, and the bytes of the live records among them (bfcg_group_exchange_bytes)."""
        out = (C.c_uint64 * 4)()
        self._ck(self.L.bfcg_group_exchange_bytes(self.g, out))
        return dict(links=int(out[0]), exact=int(out[1]), batches=int(out[2]), transport={1: "rccl", 2: "peer", 3: "push"}.get(int(out[3]), int(out[3])))

    def ctx(self, i):
        """Local rank i's counting context as a GpuCounter view (owned by the group)."""
        return GpuCounter._view(self.L.bfcg_group_ctx(self.g, i), self.params, self.n_ranks)

    def reset(self):
        self._ck(self.L.bfcg_group_reset(self.g))

    def sync(self):
        self._ck(self.L.bfcg_group_sync(self.g))

    def count_host(self, seq_stream, qual_stream=None):
        """One global batch from host memory; the library cuts it into the ranks' shares (every rank local)."""
        seq_stream = np.ascontiguousarray(seq_stream, dtype=np.uint8)
        q = np.ascontiguousarray(qual_stream, dtype=np.uint8) if qual_stream is not None else None
        self._ck(self.L.bfcg_group_count_batch_host(self.g, seq_stream.ctypes.data, q.ctypes.data if q is not None else None, len(seq_stream)))

    def count_dev(self, d_seq, d_qual, n_pos):
        """One global batch: lists (one entry per local rank) of device pointers on the rank's own device and stream lengths."""
        n = self.n_local
        ds = (C.c_void_p * n)(*[int(v) if v else None for v in d_seq])
        dq = (C.c_void_p * n)(*[int(v) if v else None for v in d_qual]) if d_qual is not None else None
        npos = (C.c_uint64 * n)(*[int(v) for v in n_pos])
        self._ck(self.L.bfcg_group_count_batch_dev(self.g, ds, dq, npos))

    def stats(self):
        out = np.zeros(16, dtype=np.uint64)
        self._ck(self.L.bfcg_group_stats(self.g, out.ctypes.data_as(u64p)))
        return {STAT_NAMES[i]: int(out[i]) for i in STAT_NAMES}

    def export_table(self):
        p = self.L.bfcg_group_export_table(self.g)
        if not p:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return HostTable(p)

    def export_bloom(self, which=0):
        p = self.L.bfcg_group_export_bloom(self.g, which)
        if not p:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return HostBloom(p)


class GpuTrimmer:
    """Trim pass of `bfc -1` on the GPU (bfcg_trim_*): bloom query kernel + longest streak per read."""

    def __init__(self, k, bloom, device=0, max_pos=1 << 24, max_reads=1 << 18):
        self.L = _lib.load()
        self.k = k
        self.t = self.L.bfcg_trim_create(k, bloom.ptr, device, int(max_pos), int(max_reads))
        if not self.t:
            raise BfcGpuError("bfcg_trim_create failed: " + self.L.bfcg_last_error().decode())

    def close(self):
        if self.t:
            self.L.bfcg_trim_destroy(self.t)
            self.t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def trim(self, seq_stream, off, min_frac=0.9, d_seq=None):
        """off: stream offsets (n_reads+1). Returns (start int32[n], end int32[n]); start -1 = read dropped."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        n = len(off) - 1
        start = np.empty(n, dtype=np.int32); end = np.empty(n, dtype=np.int32)
        s = np.ascontiguousarray(seq_stream, dtype=np.uint8) if seq_stream is not None else None
        rc = self.L.bfcg_trim_batch(self.t, s.ctypes.data if s is not None else None, d_seq, int(off[-1]), off.ctypes.data_as(u64p), n,
                                    C.c_float(min_frac), start.ctypes.data_as(C.POINTER(C.c_int32)), end.ctypes.data_as(C.POINTER(C.c_int32)))
        if rc != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return start, end

    def last_ms(self):
        return float(self.L.bfcg_trim_last_ms(self.t))

    @property
    def adopted(self):
        """True if the filter was found resident in HBM (left there by the count pass) instead of being uploaded."""
        return bool(self.L.bfcg_trim_adopted(self.t))


class GpuKcov:
    """bfc_ec_kcov (correct.c:96-117) for whole batches on the GPU (bfcg_kcov_*): table probe per k-mer + coverage sums.
    `table` is a HostTable (uploaded once) or a GpuCounter whose device table is used in place."""

    LCOV, HCOV, SOLID_END, HIGH_END = 0x3f, 0x3f << 6, 1 << 12, 1 << 13

    def __init__(self, table, device=0, max_pos=1 << 24):
        self.L = _lib.load()
        self._keep = table
        if isinstance(table, GpuCounter):
            self.t = self.L.bfcg_kcov_attach(table.ctx, int(max_pos))
        else:
            self.t = self.L.bfcg_kcov_create(table.ptr, device, int(max_pos))
        if not self.t:
            raise BfcGpuError("bfcg_kcov_create failed: " + self.L.bfcg_last_error().decode())

    def close(self):
        if self.t:
            self.L.bfcg_kcov_destroy(self.t)
            self.t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kcov(self, seq_stream, min_occ=3, d_seq=None, n_pos=None, fetch=True):
        """One packed u16 per stream position: lcov | hcov<<6 | solid_end<<12 | high_end<<13."""
        s = np.ascontiguousarray(seq_stream, dtype=np.uint8) if seq_stream is not None else None
        n = len(s) if s is not None else int(n_pos)
        out = np.empty(n, dtype=np.uint16) if fetch else None
        rc = self.L.bfcg_kcov_batch(self.t, s.ctypes.data if s is not None else None, d_seq, n, int(min_occ), out.ctypes.data if fetch else None)
        if rc != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return out

    def last_ms(self):
        return float(self.L.bfcg_kcov_last_ms(self.t))

    def dev_seq(self):
        return self.L.bfcg_kcov_dev_seq(self.t)


class GpuKmers:
    """The count table read out on the GPU (bfcg_kmers_*): what the reference's hash2cnt prints from a dump -- the spectrum, the sub-table
    sizes and the k-mers with their counts -- and asked by k-mer (bfcg_lookup.hip): the counts of given k-mers, the count under every
    position of a sequence.  `table` is a HostTable (uploaded once) or a GpuCounter whose device table is read in place
    (it must outlive this object and must not count meanwhile)."""

    def __init__(self, table, device=0):
        self.L = _lib.load()
        self._keep = table
        if isinstance(table, GpuCounter):
            self.t = self.L.bfcg_kmers_attach(table.ctx)
        else:
            self.t = self.L.bfcg_kmers_create(table.ptr, device)
        if not self.t:
            raise BfcGpuError("bfcg_kmers_create failed: " + self.L.bfcg_last_error().decode())
        info = (C.c_int * 3)()
        self.L.bfcg_kmers_info(self.t, info)
        self.k, self.l_pre, self.cshift = info[0], info[1], info[2]
        self._ms = 0.0
        self.n_found = 0

    def close(self):
        if self.t:
            self.L.bfcg_kmers_destroy(self.t)
            self.t = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hist(self):
        """(mode, cnt[256], high[64]) as bfc_ch_hist (htab.c:110)."""
        cnt, high = np.zeros(256, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
        mode = self.L.bfcg_kmers_hist(self.t, cnt.ctypes.data_as(u64p), high.ctypes.data_as(u64p))
        if mode < -1:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return mode, cnt, high

    def sub_sizes(self):
        sizes = np.zeros(1 << self.l_pre, dtype=np.uint32)
        if self.L.bfcg_kmers_sub_sizes(self.t, sizes.ctypes.data_as(u32p)) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return sizes

    def hist_sizes(self):
        """(mode, cnt[256], high[64], sizes) from ONE pass over the table: hist() and sub_sizes() stream it once each."""
        cnt, high, sizes = np.zeros(256, dtype=np.uint64), np.zeros(64, dtype=np.uint64), np.zeros(1 << self.l_pre, dtype=np.uint32)
        mode = self.L.bfcg_kmers_hist_sizes(self.t, cnt.ctypes.data_as(u64p), high.ctypes.data_as(u64p), sizes.ctypes.data_as(u32p))
        if mode < -1:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return mode, cnt, high, sizes

    MAX_SLOTS = 1 << 35  # of one bfcg_kmers_list call (it takes fewer than 2^36)

    def list_raw(self, min_cnt, min_diff, sub_lo, sub_hi, cap):
        """One bfcg_kmers_list call: (rc, n, y (cap, 2) u64, cnt_high u16 (cap))."""
        y, ch = np.zeros((cap, 2), dtype=np.uint64), np.zeros(cap, dtype=np.uint16)
        n = C.c_uint64()
        rc = self.L.bfcg_kmers_list(self.t, int(min_cnt), int(min_diff), int(sub_lo), int(sub_hi), y.ctypes.data, ch.ctypes.data, cap, C.byref(n))
        if rc < 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return rc, int(n.value), y, ch

    def pieces(self, min_cnt=0, min_diff=0, sub_lo=0, sub_hi=None, piece=1 << 24, sizes=None):
        """The listing in pieces of about `piece` k-mers and MAX_SLOTS slots at most (whole sub-tables, ascending), sized from `sizes`
        (what sub_sizes() or hist_sizes() returned; None: one pass to get them): yields (y (n, 2) u64, cnt_high (n) u16) per piece;
        last_ms() then is the time of the pieces' kernels so far."""
        sub_hi = (1 << self.l_pre) if sub_hi is None else sub_hi
        if self.k > 37:  # fail before any work, with the library's message
            self.list_raw(min_cnt, min_diff, sub_lo, sub_hi, 0)
        yield from self._pieces(lambda lo, hi, cap: self.list_raw(min_cnt, min_diff, lo, hi, cap), sub_lo, sub_hi, piece, sizes)

    def _pieces(self, raw, sub_lo, sub_hi, piece, sizes):
        """The walk of pieces(), pieces_vs() and pieces_graph(): raw(lo, hi, cap) is one of the *_raw calls on sub-tables [lo, hi) ->
        (rc, n, columns ...); yields the columns' first n rows per piece."""
        sub_hi = (1 << self.l_pre) if sub_hi is None else sub_hi
        ends = np.cumsum((self.sub_sizes() if sizes is None else sizes)[sub_lo:sub_hi], dtype=np.uint64)
        max_subs = max(1, self.MAX_SLOTS >> self.cshift)
        self._ms, lo, done = 0.0, sub_lo, 0
        while lo < sub_hi:
            hi = sub_lo + int(np.searchsorted(ends, done + piece, side="right"))
            hi = min(max(hi, lo + 1), lo + max_subs, sub_hi)
            cap = int(ends[hi - 1 - sub_lo]) - done
            rc, n, *cols = raw(lo, hi, cap)
            if rc != 0:
                raise BfcGpuError("sub-tables [%d, %d) hold %d k-mers, their sizes said %d: the table changed under the listing" % (lo, hi, n, cap))
            self._ms += float(self.L.bfcg_kmers_last_ms(self.t))
            yield tuple(c[:n] for c in cols)
            lo, done = hi, done + cap

    def list(self, min_cnt=0, min_diff=0, sub_lo=0, sub_hi=None, piece=1 << 24):
        """(y (n, 2) u64, count u8, high u8): the k-mers with count >= min_cnt and min(count, 63) - high >= min_diff, sub-tables ascending."""
        return _listing(self.pieces(min_cnt, min_diff, sub_lo, sub_hi, piece))

    def strings(self, y):
        """The k-mers as a list of str (bfc_kmer_2str, kmer.h:97)."""
        y = np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 2)
        ch = np.zeros(len(y), dtype=np.uint16)
        return [ln.split("\t")[0] for ln in self.format(y, ch).decode().splitlines()]

    def format(self, y, cnt_high):
        """hash2cnt's lines for a piece, formatted in C: bytes."""
        y = np.ascontiguousarray(y, dtype=np.uint64)
        cnt_high = np.ascontiguousarray(cnt_high, dtype=np.uint16)
        buf = C.create_string_buffer(max(1, len(cnt_high) * (self.k + 8)))
        n = self.L.bfcg_kmers_format(self.k, y.ctypes.data, cnt_high.ctypes.data, len(cnt_high), buf)
        return buf.raw[:n]

    def lookup(self, y):
        """The counts of given k-mers: y (n, 2) u64 as list() hands them out, on either strand (bits at and above k are ignored) ->
        int16 (n), high << 8 | count as bfc_ch_kmer_occ, -1 = the table does not hold it.  `n_found` then is the number found."""
        y = np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 2)
        out, nf = np.empty(len(y), dtype=np.int16), C.c_uint64()
        if self.L.bfcg_kmers_lookup(self.t, y.ctypes.data, len(y), out.ctypes.data, C.byref(nf)) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self.n_found = int(nf.value)
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return out

    def lookup_strings(self, strs):
        """lookup() of k-mers given as text (bfcg_kmers_parse); raises BfcGpuError naming the first entry that is not k bytes of ACGTacgt."""
        strs = list(strs)
        text = "\n".join(strs).encode()
        y, bad = np.zeros((len(strs), 2), dtype=np.uint64), C.c_uint64()
        n = self.L.bfcg_kmers_parse(self.k, text, len(text), y.ctypes.data, len(strs), C.byref(bad))
        if n != len(strs):  # a malformed entry, or one that the line grammar skips or splits
            one = (C.c_uint64 * 2)()
            i = next(i for i, v in enumerate(strs) if self.L.bfcg_kmer_from_str(self.k, v.encode(), one) != 0)
            raise BfcGpuError("entry %d is not a %d-mer of ACGT: %r" % (i, self.k, strs[i]))
        return self.lookup(y)

    def profile(self, seq_stream, d_seq=None, n_pos=None):
        """The count under every position of a batch stream (host array, or d_seq / n_pos on the device): int16 per position for the
        k-mer ENDING there -- high << 8 | count, -1 = absent from the table, -2 = no k-mer ends here."""
        s = np.ascontiguousarray(seq_stream, dtype=np.uint8) if seq_stream is not None else None
        n = len(s) if s is not None else int(n_pos)
        out = np.empty(n, dtype=np.int16)
        if self.L.bfcg_kmers_profile(self.t, s.ctypes.data if s is not None else None, None if s is not None else d_seq, n, out.ctypes.data) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return out

    def read_stats(self, seq_stream, off, min_cov=3, d_seq=None):
        """A read set screened against the table: the stream (host array, or d_seq on the device) and off[n_reads + 1], the reads'
        stream offsets as GpuTrimmer.trim takes them -> int32 (n_reads, 8): n_kmers, n_present, n_solid (count >= min_cov), the sum
        of the counts, min | median << 8 | max << 16, and the longest run of solid k-mers: its length, and the bases [start, end) it
        covers (-1, -1 if there is none).  The profile is reduced on the device: 32 bytes per read come back."""
        s, off, out = _read_stats_args(seq_stream, off)
        if self.L.bfcg_kmers_read_stats(self.t, s.ctypes.data if s is not None else None, None if s is not None else d_seq, int(off[-1]) if s is None else len(s),
                                        off.ctypes.data, len(off) - 1, int(min_cov), out.ctypes.data) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return out

    # ---- two tables (bfcg_tabcmp.hip): `other` is a GpuKmers of the same k and l_pre on the same device, of either form; self is allowed

    @classmethod
    def _adopt(cls, t, keep):
        """A GpuKmers around a bfcg_kmers_t the library made (a union, a clipped table); `keep` is what must outlive it."""
        self = cls.__new__(cls)
        self.L, self._keep, self.t = _lib.load(), keep, t
        info = (C.c_int * 3)()
        self.L.bfcg_kmers_info(self.t, info)
        self.k, self.l_pre, self.cshift = info[0], info[1], info[2]
        self._ms, self.n_found = float(self.L.bfcg_kmers_last_ms(t)), 0
        return self

    def joint_hist(self, other):
        """(joint u64 (256, 256), shared, only_self, only_other): joint[i, j] = the keys counted i times here and j times in `other`,
        0 = absent (joint[0, 0] is 0).  Every k up to 63."""
        joint, n = np.zeros((256, 256), dtype=np.uint64), (C.c_uint64 * 3)()
        if self.L.bfcg_kmers_joint_hist(self.t, other.t, joint.ctypes.data_as(u64p), n) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return joint, int(n[0]), int(n[1]), int(n[2])

    def list_vs_raw(self, other, min_cnt, min_diff, other_min, other_max, sub_lo, sub_hi, cap):
        """One bfcg_kmers_list_vs call: (rc, n, y (cap, 2) u64, cnt_high u16 (cap), other i16 (cap))."""
        y, ch, oth = np.zeros((cap, 2), dtype=np.uint64), np.zeros(cap, dtype=np.uint16), np.zeros(cap, dtype=np.int16)
        n = C.c_uint64()
        rc = self.L.bfcg_kmers_list_vs(self.t, other.t, int(min_cnt), int(min_diff), int(other_min), int(other_max), int(sub_lo), int(sub_hi),
                                       y.ctypes.data, ch.ctypes.data, oth.ctypes.data, cap, C.byref(n))
        if rc < 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return rc, int(n.value), y, ch, oth

    def pieces_vs(self, other, min_cnt=0, min_diff=0, other_min=0, other_max=255, sub_lo=0, sub_hi=None, piece=1 << 24, sizes=None):
        """pieces() against `other`: yields (y, cnt_high, other i16) per piece of whole sub-tables, each sized from this table's
        sub-table sizes (an upper bound: the filters only drop)."""
        self.list_vs_raw(other, min_cnt, min_diff, other_min, other_max, sub_lo, sub_lo, 0)  # an empty range: the library's refusals, before any work
        yield from self._pieces(lambda lo, hi, cap: self.list_vs_raw(other, min_cnt, min_diff, other_min, other_max, lo, hi, cap), sub_lo, sub_hi, piece, sizes)

    def list_vs(self, other, min_cnt=0, min_diff=0, other_min=0, other_max=255, sub_lo=0, sub_hi=None, piece=1 << 24):
        """list() with the k-mers' counts in `other`: (y (n, 2) u64, count u8, high u8, other i16).  A k-mer is kept only if its count in
        `other` (0 where absent) lies in [other_min, other_max]: (0, 0) private to this table, (1, 255) shared, (0, 255) everything;
        other[i] is what other.lookup(y[i]) answers, -1 or high << 8 | count."""
        return _listing(self.pieces_vs(other, min_cnt, min_diff, other_min, other_max, sub_lo, sub_hi, piece), np.int16)

    def format_vs(self, y, cnt_high, other):
        """The lines of a piece of list_vs, "kmer count high count_in_other high_in_other", formatted in C: bytes."""
        y, cnt_high = np.ascontiguousarray(y, dtype=np.uint64), np.ascontiguousarray(cnt_high, dtype=np.uint16)
        other = np.ascontiguousarray(other, dtype=np.int16)
        buf = C.create_string_buffer(max(1, len(cnt_high) * (self.k + 16)))
        n = self.L.bfcg_kmers_format_vs(self.k, y.ctypes.data, cnt_high.ctypes.data, other.ctypes.data, len(cnt_high), buf)
        return buf.raw[:n]

    def union(self, other):
        """A new GpuKmers that owns its table: every key of either table, the counts of a key in both added, saturating at 255 / 63
        (bfc_ch_union).  Its last_ms() is the time of the call's kernels."""
        t = self.L.bfcg_kmers_union(self.t, other.t)
        if not t:
            raise BfcGpuError("bfcg_kmers_union failed: " + self.L.bfcg_last_error().decode())
        return GpuKmers._adopt(t, None)

    def to_host(self):
        """The table as a HostTable (one copy, no order stamps): to dump, to correct with, to ask with get()."""
        p = self.L.bfcg_kmers_export(self.t, None)
        if not p:
            raise BfcGpuError("bfcg_kmers_export failed: " + self.L.bfcg_last_error().decode())
        return HostTable(p)

    # ---- the table as a de Bruijn graph (bfcg_graph.hip): include/bfc_gpu.h defines succ, pred, value, present, node and the degrees

    def neighbors(self, y):
        """The values of the eight neighbours of k-mers y (n, 2) u64, on the strand given: int16 (n, 8), columns 0-3 = succ by A C G T,
        4-7 = pred by A C G T; -1 or high << 8 | count as lookup().  Every k up to 63."""
        y = np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, 2)
        out = np.empty((len(y), 8), dtype=np.int16)
        if self.L.bfcg_kmers_neighbors(self.t, y.ctypes.data, len(y), out.ctypes.data) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return out

    def graph_census(self, min_cnt=1):
        """u64 (5, 5): [o, i] = the k-mers with count >= min_cnt that have o present successors and i present predecessors, on the strand
        the table stores (fold [o, i] with [i, o] for a strand-free view).  One streaming pass; k <= 37."""
        deg = np.zeros(25, dtype=np.uint64)
        if self.L.bfcg_kmers_graph_census(self.t, int(min_cnt), deg.ctypes.data_as(u64p)) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return deg.reshape(5, 5)

    def list_graph_raw(self, min_cnt, cell_mask, sub_lo, sub_hi, cap):
        """One bfcg_kmers_list_graph call: (rc, n, y (cap, 2) u64, cnt_high u16 (cap), nb u8 (cap))."""
        y, ch, nb = np.zeros((cap, 2), dtype=np.uint64), np.zeros(cap, dtype=np.uint16), np.zeros(cap, dtype=np.uint8)
        n = C.c_uint64()
        rc = self.L.bfcg_kmers_list_graph(self.t, int(min_cnt), int(cell_mask), int(sub_lo), int(sub_hi), y.ctypes.data, ch.ctypes.data, nb.ctypes.data, cap, C.byref(n))
        if rc < 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return rc, int(n.value), y, ch, nb

    def pieces_graph(self, min_cnt=1, cell_mask=GRAPH_MASKS["all"], sub_lo=0, sub_hi=None, piece=1 << 24, sizes=None):
        """pieces() with the graph predicate: yields (y, cnt_high, nb u8) per piece of whole sub-tables, each sized from the sub-table
        sizes (an upper bound: the predicate only drops)."""
        self.list_graph_raw(min_cnt, cell_mask, sub_lo, sub_lo, 0)  # an empty range: the library's refusals, before any work
        yield from self._pieces(lambda lo, hi, cap: self.list_graph_raw(min_cnt, cell_mask, lo, hi, cap), sub_lo, sub_hi, piece, sizes)

    def list_graph(self, min_cnt=1, cell_mask=GRAPH_MASKS["all"], sub_lo=0, sub_hi=None, piece=1 << 24):
        """(y (n, 2) u64, count u8, high u8, nb u8): the k-mers with count >= min_cnt whose degree cell 5 * o + i is a set bit of cell_mask
        (GRAPH_MASKS names some), sub-tables ascending; nb bit c: succ by base c is present, bit 4 + c: pred by base c."""
        return _listing(self.pieces_graph(min_cnt, cell_mask, sub_lo, sub_hi, piece), np.uint8)

    def extend(self, y, min_cnt=1, max_len=300):
        """The unambiguous path to the right of every seed y (n, 2) u64: (bases u8 (n, max_len) of 'A' 'C' 'G' 'T', zero beyond the
        length; length i32; stop i32: 0 max_len reached, 1 no successor, 2 several successors, 3 the successor has a second predecessor,
        4 the seed is absent, 5 back at the seed).  One lane walks one seed: for thousands of seeds of a few hundred bases.  A walk to
        the left is extend(kmer_revcomp(k, y)), read as the reverse complement."""
        y, bases, ls = _graph_seeds(y, max_len)
        if self.L.bfcg_kmers_extend(self.t, y.ctypes.data, len(y), int(min_cnt), int(max_len), bases.ctypes.data, ls.ctypes.data) != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return bases, ls[:, 0].copy(), ls[:, 1].copy()

    def unitigs(self, min_cnt=1):
        """The compacted graph, every maximal non-branching path exactly once (odd k <= 37; include/bfc_gpu.h defines link, path, cycle
        and the spelling emitted): (seq u8 of 'A' 'C' 'G' 'T', the unitigs back to back; off u64 (n + 1), unitig i = seq[off[i]:off[i + 1]];
        n_kmers u32; cnt_sum u64, the sum of its k-mers' counts; ends u8 = left stop | right stop << 3 | 64 for a cycle).  Stop codes:
        1 no next k-mer, 2 several, 3 the next one has another way in, 6 the only way on leads back into the node itself.  The order is
        unspecified (unitig_rows() sorts).  Two calls: one that sizes, one that writes; last_ms() is the second's."""
        out = _unitigs(self.L, self.L.bfcg_kmers_unitigs, self.t, min_cnt)
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return out

    def unitig_graph(self, min_cnt=1):
        """The compacted graph with its edges, out of one call (bfcg_kmers_unitig_graph; include/bfc_gpu.h defines oriented unitig and
        edge): unitigs()'s five arrays and links i64 (n, 2, 4) -- links[u, o, c] = v << 1 | p for the edge from (u, o) by base c
        (A C G T = 0..3) to (v, p), -1 where there is none; o, p = 1 mean the reverse complement of the emitted spelling; u and v index
        these arrays (the order differs from call to call: unitig_link_rows() names the ends by their spellings and sorts).  The last
        k - 1 bases of (u, o) are the first k - 1 of (v, p).  last_ms() is the writing call's, the edges' kernels included."""
        out = _unitig_graph(self.L, self.L.bfcg_kmers_unitig_graph, self.t, min_cnt)
        self._ms = float(self.L.bfcg_kmers_last_ms(self.t))
        return out

    def clip(self, min_cnt=1, max_tip=None, max_mean=255, islands=False, max_rounds=8):
        """The graph at min_cnt cleaned (odd k <= 37; include/bfc_gpu.h defines tip, island and round): (a new GpuKmers that owns its
        table, stats u64 (rounds, 3)).  A round removes every unitig of at most max_tip k-mers (None: 2 k) and a mean count of at most
        max_mean (255: any) that has one dead end and one attached end -- with `islands` also those with two dead ends -- and leaves
        the nodes that survive; rounds repeat until one removes nothing or max_rounds have run.  stats has a row per round that removed
        something: unitigs removed, k-mers removed, keys left.  max_rounds = 0 only drops the k-mers with a count below min_cnt.  This
        table is not written.  The result's last_ms() is the time of all the call's kernels."""
        p, stats = _clean(self.L, self.L.bfcg_kmers_clip, self.t, max_rounds, min_cnt, 2 * self.k if max_tip is None else max_tip, max_mean, CLIP_ISLANDS if islands else 0)
        return GpuKmers._adopt(p, None), stats

    def pop_bubbles(self, min_cnt=1, max_arm=None, max_diff=0, max_mean=255, max_rounds=8):
        """The simple bubbles of the graph at min_cnt popped (odd k <= 37; include/bfc_gpu.h defines arm, simple bubble, loser and
        round): (a new GpuKmers that owns its table, stats u64 (rounds, 3)).  A bubble is two unitigs of at most max_arm k-mers each
        (None: 2 k), their lengths at most max_diff apart, that leave one k-mer with two successors and meet in one k-mer with two
        predecessors; a round removes of each bubble the arm with the lower mean count (a tie: the one whose spelling starts with the
        larger k-mer) if that mean is at most max_mean (255: any), and leaves the nodes that survive; rounds repeat until one removes
        nothing or max_rounds have run.  stats has a row per round that removed something: bubbles popped, k-mers removed, keys left.
        max_rounds = 0 only drops the k-mers with a count below min_cnt.  This table is not written.  The result's last_ms() is the
        time of all the call's kernels."""
        p, stats = _clean(self.L, self.L.bfcg_kmers_pop, self.t, max_rounds, min_cnt, 2 * self.k if max_arm is None else max_arm, max_diff, max_mean)
        return GpuKmers._adopt(p, None), stats

    def last_ms(self):
        """GPU time of the last call's kernels: hist() / sub_sizes() / hist_sizes() / profile() one pass, list() and lookup() all their pieces,
        read_stats() its two kernels, joint_hist() its two launches, list_vs() all its pieces, neighbors() / list_graph() / extend() all their pieces, graph_census() one pass, unitigs() and unitig_graph() the call that writes; of a union() result,
        its size passes and fill; of a clip() or pop_bubbles() result, every kernel of the call."""
        return self._ms


class GpuCorrector:
    """BFC's error correction (bfc_ec1, correct.c:388-476) for whole batches of reads on the GPU (bfcg_ec_*), with the host instance of the
    same code as a twin (bfcg_ec1_host).  `table` is a HostTable (bfc_count / bfc_ch_restore); it must outlive this object.  `opt` is a
    table-mode bfc_opt_t (bfc_opt_init, k = the table's k).  Results are the reference's worker_ec: corrected bytes, aux, aux2.

    `table` may also be a GpuCounter: the corrector then attaches to the table where the counter built it (bfcg_ec_attach; nothing is
    exported, the counter must not count meanwhile, `device` is the counter's).  There is no host table then: reads the device cannot hold
    are corrected by its retry kernel (retry_reads()), and host_correct raises.

    With opt.refine_ec (`bfc -R`) every read given is refined: correct / host_correct take `ori`, the reads' earlier stats as two uint32
    arrays packed like aux / aux2 (parse_ec_stats; all zero where there were none).  Which reads to skip is the caller's choice, as in
    worker_ec (correct.c:542-546)."""

    def __init__(self, table, opt, device=0, max_pos=1 << 24, max_reads=1 << 18, gpu=True):
        self.L = _lib.load()
        self.table, self.opt = table, opt
        self.e = None
        self.attached = isinstance(table, GpuCounter)
        if self.attached:
            self.e = self.L.bfcg_ec_attach(table.ctx, C.byref(opt), int(max_pos), int(max_reads))
            if not self.e:
                raise BfcGpuError("bfcg_ec_attach failed: " + self.L.bfcg_last_error().decode())
            km = GpuKmers(table)  # the mode bfcg_ec_attach read, for callers (the counter has not counted since)
            self.mode = km.hist()[0]
            km.close()
            return
        cnt, high = np.zeros(256, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
        self.mode = int(self.L.bfc_ch_hist(table.ptr, cnt.ctypes.data_as(u64p), high.ctypes.data_as(u64p)))
        if gpu:
            self.e = self.L.bfcg_ec_create(table.ptr, C.byref(opt), device, int(max_pos), int(max_reads))
            if not self.e:
                raise BfcGpuError("bfcg_ec_create failed: " + self.L.bfcg_last_error().decode())

    def close(self):
        if self.e:
            self.L.bfcg_ec_destroy(self.e)
            self.e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ori(self, n, ori):
        if not self.opt.refine_ec:
            if ori is not None:
                raise BfcGpuError("earlier stats (ori) are for a corrector made with refine_ec")
            return None
        if ori is None:
            return np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        a, a2 = (np.ascontiguousarray(x, dtype=np.uint32) for x in ori)
        if len(a) != n or len(a2) != n:
            raise BfcGpuError("ori: two arrays of one entry per read")
        return a, a2

    def correct(self, seqs, quals=None, ori=None):
        """seqs: list of bytes (one read each); quals: list of bytes or None (FASTA); ori: (aux, aux2) earlier stats, refine_ec only.
        Returns (seqs, quals or None, aux uint32[n], aux2 uint32[n])."""
        n = len(seqs)
        ori = self._ori(n, ori)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) + 1 for s in seqs])
        s = np.frombuffer(b"".join(x + b"\n" for x in seqs), dtype=np.uint8).copy()
        q = np.frombuffer(b"".join(x + b"!" for x in quals), dtype=np.uint8).copy() if quals is not None else None
        aux, aux2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        if ori is None:
            rc = self.L.bfcg_ec_batch(self.e, s.ctypes.data, q.ctypes.data if q is not None else None, len(s), off.ctypes.data_as(u64p), n,
                                      aux.ctypes.data_as(u32p), aux2.ctypes.data_as(u32p))
        else:
            rc = self.L.bfcg_ec_batch_refine(self.e, s.ctypes.data, q.ctypes.data if q is not None else None, len(s), off.ctypes.data_as(u64p), n,
                                             ori[0].ctypes.data_as(u32p), ori[1].ctypes.data_as(u32p), aux.ctypes.data_as(u32p), aux2.ctypes.data_as(u32p))
        if rc != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        sb = s.tobytes()
        out_s = [sb[int(off[i]):int(off[i + 1]) - 1] for i in range(n)]
        out_q = None
        if q is not None:
            qb = q.tobytes()
            out_q = [qb[int(off[i]):int(off[i + 1]) - 1] for i in range(n)]
        return out_s, out_q, aux, aux2

    def correct_stream(self, s, q, off):
        """One batch already in the stream format (uint8 arrays with a separator after each read, q may be None; off: uint64[n + 1]),
        rewritten in place: (s, q, aux, aux2).  Table mode only."""
        n = len(off) - 1
        aux, aux2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        rc = self.L.bfcg_ec_batch(self.e, s.ctypes.data, q.ctypes.data if q is not None else None, len(s), off.ctypes.data_as(u64p), n,
                                  aux.ctypes.data_as(u32p), aux2.ctypes.data_as(u32p))
        if rc != 0:
            raise BfcGpuError(self.L.bfcg_last_error().decode())
        return s, q, aux, aux2

    def host_correct(self, seqs, quals=None, ori=None):
        """The same through the host instance, read by read."""
        if self.attached:
            raise BfcGpuError("host_correct: this corrector is attached to a counter's device table, there is no host table")
        n = len(seqs)
        ori = self._ori(n, ori)
        out_s, out_q = [], [] if quals is not None else None
        aux, aux2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        a, a2 = C.c_uint32(), C.c_uint32()
        for i in range(n):
            sb = C.create_string_buffer(seqs[i], len(seqs[i]) + 1)
            qb = C.create_string_buffer(quals[i], len(quals[i]) + 1) if quals is not None else None
            if ori is None:
                rc = self.L.bfcg_ec1_host(self.table.ptr, C.byref(self.opt), self.mode, sb, qb, C.byref(a), C.byref(a2))
            else:
                rc = self.L.bfcg_ec1_host_refine(self.table.ptr, C.byref(self.opt), self.mode, sb, qb, int(ori[0][i]), int(ori[1][i]), C.byref(a), C.byref(a2))
            if rc != 0:
                raise BfcGpuError(self.L.bfcg_last_error().decode())
            out_s.append(sb.raw[:len(seqs[i])])
            if qb is not None:
                out_q.append(qb.raw[:len(quals[i])])
            aux[i], aux2[i] = a.value, a2.value
        return out_s, out_q, aux, aux2

    def last_ms(self):
        return float(self.L.bfcg_ec_last_ms(self.e))

    def last_lookups(self):
        return int(self.L.bfcg_ec_last_lookups(self.e))

    def host_reads(self):
        return int(self.L.bfcg_ec_host_reads(self.e))

    def retry_reads(self):
        """Reads the retry kernel corrected since creation (an attached corrector's answer for what the first kernel leaves)."""
        return int(self.L.bfcg_ec_retry_reads(self.e))

    @property
    def adopted(self):
        """True if the table was found resident in HBM (left there by bfc_count) instead of being uploaded."""
        return bool(self.e) and bool(self.L.bfcg_ec_adopted(self.e))


def parse_ec_stats(comment):
    """worker_ec's test and parse_stats (correct.c:517-531, 542-543) on a read's comment (bytes or str), through bfcg_ec_parse_stats:
    (aux, aux2) packed as worker_ec packs them (rf_code 1, fields cut to ecstat_t's bit-field widths), or None if the comment does not
    start with "ec:Z:".  A read is skipped by `-R` if aux & 7 == 0 and aux2 & 0xff < 50."""
    if isinstance(comment, str):
        comment = comment.encode()
    a, a2 = C.c_uint32(), C.c_uint32()
    if not _lib.load().bfcg_ec_parse_stats(comment, C.byref(a), C.byref(a2)):
        return None
    return a.value, a2.value


def format_ec(names, seqs, quals, aux, aux2, opt, comments=None):
    """bfc_ec_cb's output step (correct.c:592-612) in table mode: bytes of the corrected FASTA/FASTQ.  comments[i] (bytes), where given and
    not None, is printed after the name instead of an ec:Z: tag (a read `-R` skipped: worker_ec kept its comment, aux = 0)."""
    out = []
    for i, name in enumerate(names):
        a, a2 = int(aux[i]), int(aux2[i])
        if opt.discard and a & 7:
            continue
        is_fq = quals is not None and quals[i] is not None and not opt.no_qual
        if comments is not None and comments[i] is not None:
            h = (b"@" if is_fq else b">") + name + b"\t" + comments[i]
        else:
            h = (b"@" if is_fq else b">") + name + b"\tec:Z:%d" % (a & 7)
            if a & 7 == 0:
                h += b"_%d:%d_%d_%d:%d_%d" % (a2 >> 10, a2 & 0xff, a >> 3 & 1, a >> 18 & 0x3fff, a >> 4 & 0x3fff, a2 >> 8 & 3)
        out.append(h + b"\n" + seqs[i] + b"\n")
        if is_fq:
            out.append(b"+\n" + quals[i] + b"\n")
    return b"".join(out)
