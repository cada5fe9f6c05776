"""Built inputs for the trim pass of `bfc -1` (bfcg_trim_*: run_query's kernels and k_streak): filters whose bits are chosen one by one and
reads whose runs of hits are placed by hand.  Everything here is deterministic and runs on the CPU; the expectation of every test that uses
it is the oracle's (orc_bf_get, orc_max_streak, orc_trim_decide) on the very bytes the GPU is given -- what this module calls the
`intended` answer only says what the corpus was built to contain, and test_trim_corpus_host.py holds the corpus to it.

query_case   one read of exactly k bases per chosen k-mer, so a read reports its one bloom query directly; the k-mers are chosen by how the
             walk of bbf.c:27-41 goes for them (no skipped candidate, the first skip at step 0..3, two skips, h2 adjusted) and the filter
             holds all, none, the first or all but one of their bits.
streak_case  reads for a saturated filter (every byte 0xff): the hit bit of a position is then "a k-mer ends here", and N bases place the
             runs.  The whole set stands at every bit offset 0..63 of the stream, in batches of 17, 9, 8, 7 and 1 tiles.
"""
import ctypes as C
import functools
import types

import numpy as np

import oracle

SEQ_LEN = 400_000
LONG_FROM = 380_000        # the k-mers of query_case's reads of 2k bases start here; the one-k-mer reads come from before
TILE = 4096                # positions per workgroup of the query kernels (BFCG_TILE1)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# (k, n_shift, n_hashes) of the query cases: every k and every n_hashes occur and four hashes occur at every k (k_query4 takes a word width
# from k); the 4 GiB filters, where run_query's choice changes; the k of the streak cases
SMALL = [(21, 28, 1), (21, 28, 4), (31, 28, 2), (31, 28, 4), (32, 28, 3), (32, 28, 4), (33, 28, 5), (33, 28, 4), (47, 28, 7), (47, 28, 4), (63, 28, 12), (63, 28, 4)]
BIG = [(31, 35, 3), (33, 35, 3), (31, 35, 4), (33, 35, 4)]
STREAK_KS = [5, 31, 33, 63]

# walk classes of a k-mer (bloom_addr)
NONE, SKIP0, SKIP1, SKIP2, SKIP3, MULTI, ADJ, SKIP = range(8)
CLASS_NAMES = ["none", "skip0", "skip1", "skip2", "skip3", "multi", "adj", "skip"]


def walk_classes(n_hashes):
    """the classes bloom_addr tells apart for this many hashes: k_query4's closed form (four positions) cares where the first skip is"""
    return [NONE, SKIP0, SKIP1, SKIP2, SKIP3, MULTI, ADJ] if n_hashes == 4 else [NONE, SKIP, ADJ]


def bit_states(n_hashes):
    """(name, which of the n_hashes positions are set) -- a hit needs all of them"""
    full = np.ones(n_hashes, dtype=bool)
    first = np.zeros(n_hashes, dtype=bool); first[0] = True
    out = [("all", full), ("none", ~full), ("first", first)]
    for j in range(n_hashes):
        m = full.copy(); m[j] = False
        out.append(("but%d" % j, m))
    return out


def bloom_addr(hash, n_shift, n_hashes):
    """bbf.c:27-41 in numpy: (block u64[n], positions int64[n, n_hashes], walk class int64[n]).
    The block is the hash's low n_shift - 9 bits, h1 the next nine, h2 the nine from bit n_shift on, plus one where h2 & 31 == 0; the
    positions are the first n_hashes of h1, h1 + h2, ... (mod 512) that are not below 8 (the lock byte).  h2 is no multiple of 32, so the
    walk repeats after 32 candidates at the earliest and meets at most 8 values below 8 on the way: n_hashes + 8 <= 20 candidates hold
    every position.  Class: ADJ if h2 was adjusted, else by the skipped candidates among those the walk needed -- none, one (for four
    hashes: at which step), two or more."""
    h = np.ascontiguousarray(hash, dtype=np.uint64)
    x = n_shift - 9
    blk = h & np.uint64((1 << x) - 1)
    h1 = ((h >> np.uint64(x)) & np.uint64(511)).astype(np.int64)
    h2 = ((h >> np.uint64(n_shift)) & np.uint64(511)).astype(np.int64)
    adj = (h2 & 31) == 0
    h2 = np.where(adj, (h2 + 1) & 511, h2)
    cand = (h1[:, None] + np.arange(n_hashes + 8, dtype=np.int64)[None, :] * h2[:, None]) & 511
    ok = cand >= 8
    assert (ok.sum(axis=1) >= n_hashes).all()
    order = np.argsort(~ok, axis=1, kind="stable")[:, :n_hashes]   # the candidates that count, in walk order
    pos = np.take_along_axis(cand, order, axis=1)
    n_skip = order[:, -1] + 1 - n_hashes
    first_skip = np.argmax(~ok, axis=1)
    if n_hashes == 4:
        cls = np.where(n_skip == 0, NONE, np.where(n_skip >= 2, MULTI, SKIP0 + first_skip))
    else:
        cls = np.where(n_skip == 0, NONE, SKIP)
    return blk, pos, np.where(adj, ADJ, cls).astype(np.int64)


@functools.lru_cache(maxsize=None)
def sequence():
    seq = ACGT[np.random.default_rng(20240607).integers(0, 4, SEQ_LEN)]
    seq.flags.writeable = False
    return seq


@functools.lru_cache(maxsize=None)
def hashes(k):
    """the bloom hash of every k-mer of sequence(), in order (k-mer i is bases [i, i + k)), from the oracle's trace of y0, y1"""
    seq = sequence()
    c = oracle.Counter(k, 20)
    tr = c.count(seq, None, np.array([0, len(seq)], dtype=np.uint64), trace=True)
    c.close()
    assert len(tr) == SEQ_LEN - k + 1
    y0, y1, m = tr[:, 1], tr[:, 2], np.uint64((1 << k) - 1)
    h0 = (y0 - y1) & m
    h = ((h0 ^ y1) << np.uint64(k)) | y0
    h.flags.writeable = False
    return h


def to_stream_off(reads):
    """a list of reads (bytes) -> the batch stream (a separator behind each) and off[n + 1]"""
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) + 1 for s in reads])
    return np.frombuffer(b"".join(s + b"\n" for s in reads), dtype=np.uint8), off


def window(hits, k, min_frac):
    """correct.c:478-497 and 557-567 on a read's hit bits (one per base: the k-mer ending there is in the filter): the longest run, of
    equal ones the later, kept if (run + k) / len is above the FLOAT min_frac; (start, end) in bases or (-1, -1)"""
    best = end = run = 0
    for p, h in enumerate(hits):
        run = run + 1 if h else 0
        if run and run >= best:
            best, end = run, p + 1
    if best and (best + k) / len(hits) > float(np.float32(min_frac)):
        return end - best - (k - 1), end
    return -1, -1


@functools.lru_cache(maxsize=None)
def query_case(k, n_shift, n_hashes, per_cell=40):
    """per_cell k-mers for every (walk class, bit state), each as a read of its k bases, cell after cell.  Behind every read stand as many
    empty reads as make the next query's stream position one more (mod 4) than this one's: a cell's queries then take every member of
    their group of four lanes, and any 64 reads in a row every bit of a result word.  Then 50 reads of 2k bases whose k + 1 k-mers are
    hits in alternating runs (each miss has exactly one bit clear), so that windows come out of real bit tests.
    Returns: reads, stream, off; blk / bit: the filter bits to set; want[n, 2]: the intended (start, end) at any min_frac <= 0.5;
    cell[n]: index into cells = [(class, state name)], -1 for the other reads; kmer[n]: the read's k-mer in hashes(k), -1 for the others."""
    seq, hs = sequence(), hashes(k)
    blk, pos, cls = bloom_addr(hs, n_shift, n_hashes)
    states = bit_states(n_hashes)
    reads, want, cell, kmer, cells, sb, sp = [], [], [], [], [], [], []

    def put(i, mask):
        sb.append(np.repeat(blk[i], int(mask.sum()))); sp.append(pos[i][mask])

    gap = (-k) % 4
    for c in walk_classes(n_hashes):
        idx = np.flatnonzero(cls[:LONG_FROM - k] == c)
        assert len(idx) >= per_cell * len(states), (k, n_shift, n_hashes, CLASS_NAMES[c], len(idx))
        for s, (name, mask) in enumerate(states):
            cells.append((c, name))
            for i in idx[s::len(states)][:per_cell]:   # a class's k-mers are dealt to its states in turn
                put(i, mask)
                reads.append(seq[i:i + k].tobytes()); want.append((0, k) if mask.all() else (-1, -1)); cell.append(len(cells) - 1); kmer.append(int(i))
                reads += [b""] * gap; want += [(-1, -1)] * gap; cell += [-1] * gap; kmer += [-1] * gap
    rng = np.random.default_rng(1000 * k + n_hashes)
    for t in range(50):
        i0 = LONG_FROM + t * (2 * k + 10)
        if t < 35:
            hit = ((np.arange(k + 1) // (1 + t % 7)) & 1) == (t & 1)
        else:
            hit = rng.random(k + 1) < 0.6
        for j in range(k + 1):
            m = np.ones(n_hashes, dtype=bool)
            m[j % n_hashes] = bool(hit[j])
            put(i0 + j, m)
        reads.append(seq[i0:i0 + 2 * k].tobytes()); cell.append(-1); kmer.append(-1)
        want.append(window(np.concatenate([np.zeros(k - 1, dtype=bool), hit]), k, 0.5))
    stream, off = to_stream_off(reads)
    out = types.SimpleNamespace(k=k, n_shift=n_shift, n_hashes=n_hashes, reads=reads, stream=stream, off=off, blk=np.concatenate(sb),
                                bit=np.concatenate(sp), want=np.array(want, dtype=np.int32), cell=np.array(cell), kmer=np.array(kmer), cells=cells)
    for a in (out.stream, out.off, out.blk, out.bit, out.want, out.cell, out.kmer):
        a.flags.writeable = False
    return out


def set_bits(view, blk, bit):
    """set bit `bit` of 64-byte block `blk` in a filter's bytes"""
    np.bitwise_or.at(view, blk.astype(np.int64) * 64 + (bit >> 3), (1 << (bit & 7)).astype(np.uint8))


# ---- streaks ----------------------------------------------------------------------------------------------------------------------------

RUNS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
STREAK_TILES = (17, 9, 8, 7)
MIN_FRACS = (0.5, 0.9, 1.0)


def keep_len(k):
    """length of the keep-rule reads: 100 bases; 200 for k = 63, where streak + k = 50 has no streak"""
    return 100 if k < 50 else 200


@functools.lru_cache(maxsize=None)
def streak_case(k):
    """The set (names in `names`, the index of a named read in `tags`):
      run<r>        N, a run of r hits, N                          -> window (1, r + k)
      twin, twin64  two runs of 30 (64) hits, N between            -> the later one
      first / middle / last   runs of 100, 3 and 5 hits, the longest there (100 + k is above half the read for every k: kept at 0.5)
      tail          NN and a run of 40 hits that ends on the read's last base
      len0, len1, lenk-1, lenk, lenk+1, allN, lower, mixed, three empty reads
      keep_eq / keep_above   L = keep_len(k) bases, streak + k = L / 2 and L / 2 + 1: at min_frac 0.5 dropped (0.5 > 0.5 is false), kept
      keep_09       streak + k = 0.9 L: kept at min_frac 0.9, a float (0.9f < 0.9)
      full / notfull   L clean bases ((L + 1) / L > 1: kept at 1.0); L - 1 bases and an N (L / L: dropped)
      long          (the first copy only) 20 001 bases: runs of 9000 and 10 100 hits (above half the read: kept at 0.5), 130 N between them, a short run behind
    Batches: copy s of the set stands behind a pad read sized so that the copy starts at bit offset s of a result word; copies fill a batch
    of 17, 9, 8, 7 tiles in turn until every s in 0..63 has stood somewhere, and a read of N fills the batch up to 37 positions below its
    last tile's end; the batch of one tile holds a pad (bit offset 17) and as much of the set as fits.  Longest first.
    A batch: stream, off, tiles, src[n, 2] = (s, index in the set) or (-1, -1) for pads and fillers."""
    rng = np.random.default_rng(77 + k)
    bases = lambda n: ACGT[rng.integers(0, 4, n)].tobytes()  # noqa: E731
    seg = lambda r: bases(r + k - 1)  # noqa: E731  (r k-mers, so r hits under a saturated filter)
    runs = lambda rs: b"N".join(seg(r) for r in rs)  # noqa: E731
    L = keep_len(k)
    fill = lambda s: s + b"N" * (L - len(s))  # noqa: E731
    named = [("run%d" % r, b"N" + seg(r) + b"N") for r in RUNS]
    named += [("twin", runs([30, 30])), ("twin64", runs([64, 64])), ("first", runs([100, 3, 5])), ("middle", runs([3, 100, 5])), ("last", runs([3, 5, 100])),
              ("tail", b"NN" + seg(40)), ("len0", b""), ("len1", bases(1)), ("lenk-1", bases(k - 1)), ("lenk", bases(k)), ("lenk+1", bases(k + 1)),
              ("allN", b"N" * 70), ("lower", seg(60).lower()), ("mixed", bytes(c | 0x20 if i % 3 else c for i, c in enumerate(seg(60)))),
              ("empty_a", b""), ("empty_b", b""), ("empty_c", b""),
              ("keep_eq", fill(seg(L // 2 - k))), ("keep_above", fill(seg(L // 2 + 1 - k))), ("keep_09", fill(seg(9 * L // 10 - k))),
              ("full", bases(L)), ("notfull", bases(L - 1) + b"N")]
    head = seg(9000) + b"N" * 130 + seg(10100) + b"N"
    long_read = head + bases(20001 - len(head))
    names = [n for n, _ in named] + ["long"]
    tags = {n: i for i, n in enumerate(names)}
    size = sum(len(s) + 1 for _, s in named)
    batches, covered, s = [], set(), 0

    def close(reads, src, tiles):
        stream, off = to_stream_off(reads)
        assert (len(stream) + TILE - 1) // TILE == tiles and any(a >= 0 for a, _ in src), (k, tiles, len(stream))
        b = types.SimpleNamespace(stream=stream, off=off, tiles=tiles, src=np.array(src, dtype=np.int64))
        for a in (b.stream, b.off, b.src):
            a.flags.writeable = False
        batches.append(b)

    while len(covered) < 64:
        for tiles in STREAK_TILES:
            reads, src, n_pos, cap = [], [], 0, tiles * TILE
            while True:
                pad = (s - n_pos - 1) % 64
                with_long = s == 0 and not covered
                need = pad + 1 + size + (len(long_read) + 1 if with_long else 0)
                if n_pos + need > cap:
                    break
                reads.append(bases(pad)); src.append((-1, -1))
                reads += [r for _, r in named]; src += [(s, i) for i in range(len(named))]
                if with_long:
                    reads.append(long_read); src.append((s, tags["long"]))
                n_pos += need
                covered.add(s); s = (s + 1) % 64
            if n_pos + 1 <= cap - 37:
                reads.append(b"N" * (cap - 37 - n_pos - 1)); src.append((-1, -1))
            close(reads, src, tiles)
    reads, src, n_pos = [bases(16)], [(-1, -1)], 17
    for i, (_, r) in enumerate(named):
        if n_pos + len(r) + 1 > TILE:
            break
        reads.append(r); src.append((17, i)); n_pos += len(r) + 1
    close(reads, src, 1)
    batches.sort(key=lambda b: -len(b.stream))
    return types.SimpleNamespace(k=k, names=names, tags=tags, batches=batches, keep_len=L)


# ---- the oracle on a filter's bytes -------------------------------------------------------------------------------------------------

def bf_ptr(bf):
    """a filter as the oracle's functions take it: an orc_bf_t * as it is, a HostBloom through its bfc_bf_t (the same three fields, bbf.h:9-12)"""
    return C.cast(bf.ptr, C.c_void_p) if hasattr(bf, "ptr") else bf


class OrcFilter:
    """an orc_bf_t with its bytes writable in place"""

    def __init__(self, n_shift, n_hashes):
        self.L = oracle.lib()
        self.ptr = C.c_void_p(self.L.orc_bf_new(n_shift, n_hashes))
        self.n_shift, self.n_hashes = n_shift, n_hashes

    def bytes(self):
        return np.ctypeslib.as_array(C.cast(self.L.orc_bf_bits(self.ptr), oracle.u8p), shape=(1 << (self.n_shift - 3),))

    def close(self):
        if self.ptr:
            self.L.orc_bf_free(self.ptr)
            self.ptr = None


def orc_gets(bf, hs):
    """orc_bf_get of each hash: the number of its bits that are set"""
    L, p = oracle.lib(), bf_ptr(bf)
    return np.array([L.orc_bf_get(p, int(h)) for h in hs], dtype=np.int64)


def orc_windows(bf, k, stream, off, min_fracs):
    """per min_frac the (start, end)[n, 2] of orc_max_streak + orc_trim_decide on every read of a stream; (-1, -1) = dropped"""
    L, p = oracle.lib(), bf_ptr(bf)
    stream = np.ascontiguousarray(stream)
    n = len(off) - 1
    out = [np.full((n, 2), -1, dtype=np.int32) for _ in min_fracs]
    a, e = C.c_int(), C.c_int()
    for r in range(n):
        ln = int(off[r + 1]) - int(off[r]) - 1
        if ln <= 0:
            continue
        mx = L.orc_max_streak(k, p, stream.ctypes.data + int(off[r]), ln)
        for o, mf in zip(out, min_fracs):
            if L.orc_trim_decide(mx, k, ln, C.c_float(mf), C.byref(a), C.byref(e)):
                o[r] = a.value, e.value
    return out


def unstream(stream, off):
    """(concatenated reads, off[n + 1]) without separators, as oracle.ref_trim takes them"""
    n = len(off) - 1
    keep = np.ones(len(stream), dtype=bool)
    keep[np.asarray(off[1:], dtype=np.int64) - 1] = False
    return np.ascontiguousarray(stream[keep]), (np.asarray(off, dtype=np.int64) - np.arange(n + 1)).astype(np.uint64)
