"""Reads whose k-mers land where the test says, for the count table's write path (test_commit_corpus_host.py, test_gpu_commit.py).  No GPU.

The write path -- k_commit_seg with its three ways through a block, seg_upsert / seg_park / k_seg_rehash / k_seg_replay, k_seg_to_table, and in
the host's layout agg_add / k_commit / k_commit_stream / table_upsert / k_table_rehash / k_table_replay, with the hand-over log in front -- is
otherwise fed reads of a random genome: the segments grow at 62 % load, so a full segment, a probe of every slot or a chain round a block's end
is there by accident.  Here a k-mer is chosen by where it lands:

  segments     (bloom region, block of the segment, home slot): the region is a bit field of Y0, the home a multiplicative hash of the k-mer's
               identity inside its region (seg_id, seg_home in kmer_dev.h) -- candidates are drawn with the region's bits set and kept by home
  host layout  (sub-table, home slot): bit fields of the hash (ch_subkey)

A candidate hash (Y0, Y1) becomes a k-mer by undoing the two sums and the two mixes (planes_of_hash, the restatement of bfcg_kdec.h's
hash_to_kmer for every k) and is kept if the oracle hashes that k-mer back to (Y0, Y1): the decode inverts the hash of the strand the forward
hash chose, so about half of the candidates fail.  A placed k-mer travels as a read of exactly k bases -- one k-mer per read, nothing else in
the table -- and a case says how often it comes in which call and how many of those reads are of high quality.  A k-mer is in the table from
its second occurrence on (the first only sets its bits in the filter): keys_after() is that rule, and the host test holds it to the oracle
counted prefix by prefix.  The expected filter, statistics and table of every case are the oracle's (expected()).

The geometry bfcg_create derives (R, F, F1 / F2, seg_lo / seg_hi) is restated in geometry(); test_gpu_commit.py holds every placed k-mer to
bfcg_seg_place, the library's own functions on the host, before it counts.  A class that cannot be filled raises CorpusError.

Geometries, the smallest at which each mechanism exists:
  ONE     -b16, k = 21: one bloom region; tab_cshift = 1 / 3 / 7 gives segments of 2^4 / 2^6 / 2^10 slots.  A call of up to 3117 positions is
          one batch there (the cold limit of one region); longer calls are cut at read ends, which the saturation cases use
  WINDOWS -b22, region_shift = 4: 512 regions of segments of 2^4 slots, level 2 in one pass (BFCG_ONEPASS_MIN_TILES = 0), so a batch takes a
          page of the hand-over log; a region's share of a batch stays far below its slab (208 records)
  CAS     -b24, region_shift = 4: 2048 regions, so that a call of 1.44 M positions stays one batch
  HOST    table_layout = 1; k = 21 at l_pre 4 and 8, k = 33 and 47 at the l_pre htab.c clamps them to (16 and 24)
"""
import collections
import ctypes as C
import functools

import numpy as np

import oracle
from packed_corpus import CorpusError

U = np.uint64
GOLD = U(0x9E3779B97F4A7C15)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
ONE_BATCH = 3117          # positions of a call that geometry ONE still takes as one batch into a cold filter (split_rule)
HIGH, LOW = 73, 33        # quality bytes: 40 and 0 against the threshold of 20

Geometry = collections.namedtuple("Geometry", "k bf_shift R F F1 F2 seg_lo seg_hi")
Geom = collections.namedtuple("Geom", "k bf_shift l_pre kw env max_batch_pos")
Key = collections.namedtuple("Key", "Y y row region id home sub skey")   # Y hash, y planes, row = the k bases; home = seg_home (26 bits); (sub, skey) = ch_subkey
Item = collections.namedtuple("Item", "key n high")                      # n reads of the k-mer in a call, `high` of them of high quality


def _mask(n):
    return (1 << n) - 1


# ---- the geometry of a context and the placement of a hash, restated ---------------------------------------------------------------------

def geometry(k, bf_shift, region_shift=0):
    """bfcg_create's R, F, F1, F2 and the segment identity's implied bit field [seg_lo, seg_hi) of Y0 (no BFCG_R / BFCG_F1 set)"""
    R = region_shift if region_shift > 0 else 8
    R = max(4, min(R, 10))
    R = min(R, bf_shift - 9)
    while bf_shift - 9 - R > 20 and R < 10:
        R += 1
    F = bf_shift - 9 - R
    if F <= 8:
        F1, F2 = F, 0
    else:
        F2 = min((F + 1) // 2, 10)
        F1 = F - F2
    lo = min(R, k)
    hi = max(lo, min(k, bf_shift - 9))
    return Geometry(k, bf_shift, R, F, F1, F2, lo, hi)


def fine_id(g, y0, y1):
    """the bloom region of hashes (u64 arrays): block id >> R, the block id being the low bf_shift - 9 bits of (h0 ^ h1) << k | y0"""
    m = U(_mask(g.k))
    h0 = (y0 - y1) & m
    h = ((h0 ^ y1) << U(g.k)) | y0
    return (h & U(_mask(g.bf_shift - 9))) >> U(g.R)


def seg_id(g, y0, y1):
    """kmer_dev.h seg_id: (y0, y1) without the bits of y0 that the region implies"""
    low = y0 & U(_mask(g.seg_lo))
    up = y0 >> U(g.seg_hi) if g.seg_hi < g.k else U(0) * y0
    return low | up << U(g.seg_lo) | y1 << U(g.k - (g.seg_hi - g.seg_lo))


def seg_unpack(g, region, sid):
    """kmer_dev.h seg_unpack on python ints: (y0, y1) of an identity in a region"""
    nimp = g.seg_hi - g.seg_lo
    kb = g.k - nimp
    kept = sid & _mask(kb)
    y0 = (kept & _mask(g.seg_lo)) | (region & _mask(nimp)) << g.seg_lo | ((kept >> g.seg_lo) << g.seg_hi if g.seg_hi < g.k else 0)
    return y0, sid >> kb


def seg_home(sid):
    with np.errstate(over="ignore"):
        return (np.asarray(sid, dtype=U) * GOLD) >> U(38)


def slot_of(home, blk_shift, seg_shift):
    """(block, home slot inside the block) of a 26-bit home in segments of 2^seg_shift slots made of blocks of 2^blk_shift"""
    b = min(blk_shift, seg_shift)
    return (int(home) >> b) & _mask(seg_shift - b), int(home) & _mask(b)


# ---- from a hash back to its k-mer ------------------------------------------------------------------------------------------------------------

def _unxs(v, s):
    x, t = v, v >> s
    while t:
        x ^= t
        t >>= s
    return x


def _unmix(v, k):
    """the inverse of kmer.h:30-40 modulo 2^k: four odd multipliers, three v ^= v >> s"""
    M = 1 << k
    v = v * pow((1 << 31) + 1, -1, M) % M
    v = _unxs(v, 28)
    v = v * pow(21, -1, M) % M
    v = _unxs(v, 14)
    v = v * pow(265, -1, M) % M
    v = _unxs(v, 24)
    return (v + 1) * pow((1 << 21) - 1, -1, M) % M


def planes_of_hash(k, Y0, Y1):
    """the planes (a, b) of the k-mer whose hash is (Y0, Y1) on the strand the hash was taken from (bfcg_kdec.h hash_to_kmer, any k)"""
    m = _mask(k)
    h0 = (Y0 - Y1) & m
    b = _unmix(Y1, k) ^ h0
    return (_unmix(h0, k) - b) & m, b


def row_of_planes(k, a, b):
    """the k bases, 5' to 3', as ASCII"""
    return ACGT[[((b >> l & 1) << 1) | (a >> l & 1) for l in range(k - 1, -1, -1)]]


@functools.lru_cache(maxsize=None)
def _tracer(k):
    return oracle.Counter(k, 20)


def forward(k, rows):
    """(n, 2) u64: the oracle's hash (y0, y1) of every row (n, k) of bases"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, k)
    tr = _tracer(k).count(rows.reshape(-1), None, np.arange(len(rows) + 1, dtype=U) * U(k), trace=True)
    if len(tr) != len(rows):
        raise CorpusError("a row is not one k-mer")
    return tr[:, 1:3].copy()


class Picker:
    """draws k-mers of a geometry by where they land, each once"""

    def __init__(self, geom, seed):
        self.geom, self.k, self.l_pre = geom, geom.k, oracle.lib().orc_ch_clamp_lpre(geom.k, geom.l_pre)
        self.g = geometry(geom.k, geom.bf_shift, geom.kw.get("region_shift", 0))
        self.rng, self.used, self.stats = np.random.default_rng(seed), set(), collections.Counter()

    def _accept(self, cands, want):
        """the Keys of up to `want` of the candidate hashes [(Y0, Y1)]: unused, and hashed back to by their k-mer"""
        cands = [Y for Y in dict.fromkeys(cands) if Y not in self.used]
        if not cands or want <= 0:
            return []
        ys = [planes_of_hash(self.k, *Y) for Y in cands]
        rows = np.array([row_of_planes(self.k, a, b) for a, b in ys], dtype=np.uint8)
        got = forward(self.k, rows)
        out = []
        for Y, y, row, G in zip(cands, ys, rows, got):
            self.stats["tried"] += 1
            if (int(G[0]), int(G[1])) != Y or len(out) == want:
                continue
            self.stats["kept"] += 1
            self.used.add(Y)
            key = C.c_uint64()
            sub = oracle.lib().orc_ch_subkey(self.k, self.l_pre, (C.c_uint64 * 2)(*Y), C.byref(key))
            a0, a1 = np.array([Y[0]], dtype=U), np.array([Y[1]], dtype=U)
            sid = int(seg_id(self.g, a0, a1)[0])
            out.append(Key(Y, y, row.tobytes(), int(fine_id(self.g, a0, a1)[0]), sid, int(seg_home(sid)), int(sub), key.value >> 14))
        return out

    def _draw(self, n, region):
        k, g = self.k, self.g
        y0 = self.rng.integers(0, 1 << k, n, dtype=np.uint64)
        y1 = self.rng.integers(0, 1 << k, n, dtype=np.uint64)
        nb = g.bf_shift - 9
        if nb > g.R:
            if k < nb:
                raise CorpusError("the region is not a bit field of Y0 at k=%d, -b%d" % (k, g.bf_shift))
            y0 = (y0 & ~U(_mask(nb) ^ _mask(g.R))) | U(region << g.R)
        elif region:
            raise CorpusError("this geometry has one region")
        return y0, y1

    def seg(self, region, n, pred=None, what=""):
        """n Keys of bloom region `region` whose 26-bit home satisfies pred (an array predicate)"""
        out = []
        for _ in range(200):
            y0, y1 = self._draw(1 << 14, region)
            at = np.arange(len(y0)) if pred is None else np.flatnonzero(pred(seg_home(seg_id(self.g, y0, y1))))
            at = at[:4 * (n - len(out)) + 8]
            out += self._accept([(int(y0[i]), int(y1[i])) for i in at], n - len(out))
            if len(out) == n:
                for key in out:
                    if key.region != region or (pred is not None and not pred(np.array([key.home], dtype=U))[0]):
                        raise CorpusError("a key of %s is not where it was asked for" % what)
                return out
        raise CorpusError("no %d k-mers of region %d for %s (%d found)" % (n, region, what, len(out)))

    def at(self, region, blk_shift, seg_shift, block, slot, n, what=""):
        """n Keys of (region, block, home slot) in segments of 2^seg_shift slots made of blocks of 2^blk_shift; block / slot None = any"""
        b = min(blk_shift, seg_shift)

        def pred(home):
            ok = np.ones(len(home), dtype=bool)
            if slot is not None:
                ok &= (home & U(_mask(b))) == U(slot)
            if block is not None:
                ok &= ((home >> U(b)) & U(_mask(seg_shift - b))) == U(block)
            return ok
        return self.seg(region, n, pred, what)

    def host(self, sub, home, cshift, n, what=""):
        """n Keys of sub-table `sub` (None: any) of the host's layout whose home slot at `cshift` is `home` (None: any)"""
        k, lp, out = self.k, self.l_pre, []
        t = 2 * k - lp if k <= 32 else k - lp
        if k <= 32 and t < k:
            raise CorpusError("the sub-table reaches into Y1 at k=%d l_pre=%d" % (k, lp))
        if k > 32 and (k if t + k < 50 else 50 - t) < cshift:
            raise CorpusError("the home slot is not Y1's low bits at k=%d l_pre=%d cshift=%d" % (k, lp, cshift))
        for _ in range(200):
            y0, y1 = self._draw(8 * n + 16, 0)
            cands = []
            for a, b in zip(y0.tolist(), y1.tolist()):
                if sub is not None:
                    a = (a & _mask(t - k)) | sub << (t - k) if k <= 32 else (a & _mask(t)) | sub << t
                if home is not None:
                    b = (b & ~_mask(cshift)) | home
                cands.append((a, b))
            out += self._accept(cands, n - len(out))
            if len(out) == n:
                for key in out:
                    if (sub is not None and key.sub != sub) or (home is not None and key.skey & _mask(cshift) != home):
                        raise CorpusError("a key of %s is not where it was asked for" % what)
                return out
        raise CorpusError("no %d k-mers of sub-table %r, home %r for %s" % (n, sub, home, what))

    def same_y0(self, n, what=""):
        """n Keys that share Y0 and differ in Y1 (k > 32: agg_add tells them apart by Y1 alone)"""
        Y0 = int(self._draw(1, 0)[0][0])
        out = []
        for _ in range(200):
            out += self._accept([(Y0, int(v)) for v in self._draw(4 * n + 8, 0)[1]], n - len(out))
            if len(out) == n:
                return out
        raise CorpusError("no %d k-mers with one Y0 for %s" % (n, what))


# ---- a case: calls of (k-mer, occurrences, high-quality ones) -------------------------------------------------------------------------------

class Case:
    """name, geom (Geom), calls [[Item]], roles {name: [Key]} (what it was built to contain), want (what the context must report after the
    whole: keys of GpuCounter.commit_info / table_info / partition_info, or (key, 'min') pairs), absent [Key] (never counted),
    checks ({call: the same, when drained behind that call}), sync_after (calls, from 1, behind which the test drains: where the case needs its parked k-mers replayed before it goes on)"""

    def __init__(self, name, geom, seed):
        self.name, self.geom, self.seed = name, geom, seed
        self.calls, self.roles, self.want, self.absent, self.sync_after = [], collections.OrderedDict(), {}, [], set()
        self.checks = {}   # {call: what the context must report when drained behind it}
        self.blk_shift = int(geom.env.get("BFCG_SEG_BLOCK", 12))
        self.seg_shift = geom.kw.get("tab_cshift", 0) + 3   # after a reset (segments; tab_cshift > 0 in every geometry here)
        self.P = Picker(geom, seed)

    def role(self, name, keys):
        self.roles.setdefault(name, []).extend(keys)
        return keys

    def call(self, *groups, sync=False):
        """one call: groups of (keys, occurrences, high-quality ones)"""
        items = [Item(key, n, min(high, n)) for keys, n, high in groups for key in keys if n > 0]
        self.calls.append(items)
        if sync:
            self.sync_after.add(len(self.calls))

    def keys(self):
        return list(dict.fromkeys(it.key for items in self.calls for it in items))

    def reads(self, i):
        """(item index, high-quality flag) of every read of call i (from 0), in the order of the stream"""
        items = self.calls[i]
        n = np.array([it.n for it in items], dtype=np.int64)
        idx = np.repeat(np.arange(len(items)), n)
        first = np.repeat(np.cumsum(n) - n, n)
        high = (np.arange(len(idx)) - first) < np.repeat(np.array([it.high for it in items], dtype=np.int64), n)
        order = np.random.default_rng(1000 * self.seed + i).permutation(len(idx))
        return idx[order], high[order]

    def stream(self, i):
        """(seq u8, qual u8, off u64) of call i (from 0): every read exactly k bases, the reads of the call's k-mers shuffled"""
        items, k = self.calls[i], self.geom.k
        rows = np.array([np.frombuffer(it.key.row, dtype=np.uint8) for it in items], dtype=np.uint8).reshape(-1, k)
        idx, high = self.reads(i)
        seq = rows[idx].reshape(-1)
        qual = np.where(high[:, None], np.uint8(HIGH), np.uint8(LOW)) * np.ones((1, k), dtype=np.uint8)
        return seq, qual.reshape(-1).astype(np.uint8), np.arange(len(idx) + 1, dtype=U) * U(k)

    def positions(self, i):
        return sum(it.n for it in self.calls[i]) * (self.geom.k + 1)

    def keys_after(self):
        """distinct keys after every call: a k-mer is in the table from its second occurrence on.  shared_bits (the cases of k-mers with one
        Y0 at k = 33 and 47): the filter's block and bit positions are bits of Y0 there (bbf.c:27-41 on a hash whose low k bits are Y0), so
        such k-mers share them -- only the very first read of the group finds clear bits, and a k-mer is in the table once any read of it
        is not that one: taken from the order of the reads"""
        out = []
        if not getattr(self, "shared_bits", False):
            seen = collections.Counter()
            for items in self.calls:
                for it in items:
                    seen[it.key.Y] += it.n
                out.append(sum(1 for v in seen.values() if v >= 2))
            return out
        bits, table = set(), set()
        for i, items in enumerate(self.calls):
            for j in self.reads(i)[0].tolist():
                Y = items[j].key.Y
                if Y[0] in bits:
                    table.add(Y)
                bits.add(Y[0])
            out.append(len(table))
        return out

    def totals(self):
        """{hash: (occurrences, high-quality ones)} over all calls"""
        t = collections.defaultdict(lambda: [0, 0])
        for items in self.calls:
            for it in items:
                t[it.key.Y][0] += it.n
                t[it.key.Y][1] += it.high
        return t


def count_case(case, counter_factory=None):
    """the case through oracle.Counter call by call: (keys after every call, the Counter)"""
    g = case.geom
    oc = (counter_factory or oracle.Counter)(g.k, g.bf_shift, l_pre=g.l_pre)
    after = []
    for i in range(len(case.calls)):
        oc.count(*case.stream(i))
        after.append(oc.table_count())
    return after, oc


@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's answer for a case, computed once: keys after every call, statistics, the filter's bytes, the table in L1 form"""
    c = case(name)
    after, oc = count_case(c)
    out = dict(keys_after=after, stats=oc.stats(), bloom=oc.bloom_bytes(), table=oc.export())
    out["get"] = {key.Y: int(oc.table_get(*key.Y)) for key in c.keys() + c.absent}   # high << 8 | count, -1 = absent
    for a in (out["bloom"],) + tuple(out["table"]):
        a.setflags(write=False)
    oc.close()
    return out


# ---- the geometries ---------------------------------------------------------------------------------------------------------------------------

def ONE(cshift, **env):
    return Geom(21, 16, 20, dict(tab_cshift=cshift), {k: str(v) for k, v in env.items()}, 1 << 18)


def WINDOWS(K):
    return Geom(21, 22, 20, dict(tab_cshift=1, region_shift=4), dict(BFCG_ONEPASS_MIN_TILES="0", BFCG_COMMIT_K=str(K)), 1 << 16)


def CAS():
    return Geom(21, 24, 20, dict(tab_cshift=4, region_shift=4), {}, 1 << 21)


def HOST(k, l_pre, cshift, bf_shift=16, max_batch_pos=1 << 16):
    return Geom(k, bf_shift, l_pre, dict(tab_cshift=cshift, table_layout=1), {}, max_batch_pos)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------

CASES = collections.OrderedDict()


def _case(name):
    def deco(fn):
        CASES[name] = fn
        return fn
    return deco


def _one_home(name, home, extra, n_calls, seed):
    """2^4 + extra keys of one home slot of the one 2^4-slot segment: extra = -1, 0 (exactly full: no park), +1 (one key finds no slot after a
    probe of all 16: each of its occurrences behind the first is parked once).  n_calls = 1: every key 4 times in one call; 2: the first
    occurrences in a call of their own (it creates nothing), then 3 more; 3: first, then 3 more (the creating call), then 2 hits -- drained
    behind the creating call, so that what it parked is replayed before the hits arrive"""
    c = Case(name, ONE(1), seed)
    keys = c.role("home%d" % home, c.P.at(0, 12, 4, 0, home, 16 + extra, name))
    m = 3   # occurrences behind the first in the creating call
    if n_calls == 1:
        c.call((keys, 1 + m, 2))
    else:
        c.call((keys, 1, 1))
        c.call((keys, m, 1), sync=True)
        if n_calls == 3:
            c.call((keys, 2, 2))
    c.absent = c.P.at(0, 12, 4, 0, home, 1, name + " absent")
    c.want = dict(seg_replayed=m if extra > 0 else 0, table_replayed=0, to_host_layout=0, segments=True, seg_growths=("min", 1))
    c.full_homes = [home] if extra >= 0 else []
    return c


for _home, _tag in ((6, "even"), (9, "odd"), (15, "last")):
    for _extra, _etag in ((-1, "less"), (0, "full"), (1, "more")):
        for _n in (1, 2, 3):
            _nm = "home_%s_%s_%dcalls" % (_tag, _etag, _n)
            CASES[_nm] = functools.partial(_one_home, _nm, _home, _extra, _n, 100 + 16 * _home + 4 * (_extra + 1) + _n)


def _interleaved(name, homes, seed):
    """chains of two / three homes that fill the 2^4-slot segment exactly, created in one batch, hit in the next"""
    c = Case(name, ONE(1), seed)
    share = [16 // len(homes) + (1 if i < 16 % len(homes) else 0) for i in range(len(homes))]
    keys = []
    for h, n in zip(homes, share):
        keys += c.role("home%d" % h, c.P.at(0, 12, 4, 0, h, n, name))
    c.call((keys, 1, 0))
    c.call((keys, 2, 1), sync=True)
    c.call((keys, 3, 3))
    c.absent = [c.P.at(0, 12, 4, 0, h, 1, name + " absent")[0] for h in homes]
    c.want = dict(seg_replayed=0, table_replayed=0, to_host_layout=0, segments=True)
    c.full_homes = list(homes)
    return c


CASES["interleaved_2"] = functools.partial(_interleaved, "interleaved_2", (15, 4), 301)
CASES["interleaved_3"] = functools.partial(_interleaved, "interleaved_3", (15, 0, 1), 302)


@_case("pair_read")
def _pair_read():
    """the 16-byte read of an even slot and its neighbour: two keys of an even home (the second's first free slot is the `nxt` of the pair
    read; from the next batch on it is a hit in `nxt`), two of an odd home, and two new keys of one even home with 64 occurrences each behind
    the first in ONE batch, so that lanes read a zero that another lane has filled meanwhile"""
    c = Case("pair_read", ONE(1), 310)
    even = c.role("even", c.P.at(0, 12, 4, 0, 2, 2, "pair even"))
    odd = c.role("odd", c.P.at(0, 12, 4, 0, 7, 2, "pair odd"))
    hot = c.role("hot", c.P.at(0, 12, 4, 0, 10, 2, "pair hot"))
    c.call((even + odd, 2, 1))
    c.call((even + odd, 2, 1), (hot, 65, 33))
    c.call((even + odd + hot, 2, 0))
    if c.positions(1) > ONE_BATCH:
        raise CorpusError("the hot keys' call is more than one batch")
    c.want = dict(seg_replayed=0, to_host_layout=0, segments=True)
    c.full_homes = []
    return c


SAT_SEEN = (2, 3, 254, 255, 256, 257, 300)     # occurrences behind the first: the count the table must show, saturating at 255


def _sat_highs(seen):
    return sorted(set(h for h in (0, 1, 62, 63, 64, seen) if h <= seen))


def _saturation(name, split, seed):
    """keys whose count in the table is 2, 3, 254, 255, 256, 257 and 300 inserts, with 0, 1, 62, 63, 64 and all of them of high quality, in
    segments of 2^10 slots.  split = False: each in one call (which the library cuts into batches of a region's worth, so the count arrives
    by the slot's creating entry, the counter pair of that batch and those of later batches); split = True: the first occurrence, the
    creating one, then the rest in two calls and a last call that comes on keys already at 255 / 63"""
    c = Case(name, ONE(7), seed)
    plan = [(s, h) for s in SAT_SEEN for h in _sat_highs(s)]
    keys = c.P.seg(0, len(plan), None, name)
    for key, (s, h) in zip(keys, plan):
        c.role("seen%d_high%d" % (s, h), [key])
    if not split:
        for key, (s, h) in zip(keys, plan):
            c.call(([key], s + 1, h))
    else:
        c.call((keys, 1, 0))
        c.call(*[([key], 1, min(h, 1)) for key, (s, h) in zip(keys, plan)], sync=True)
        c.call(*[([key], (s - 1) // 2, min(max(h - 1, 0), (s - 1) // 2)) for key, (s, h) in zip(keys, plan)])
        c.call(*[([key], s - 1 - (s - 1) // 2, max(h - 1 - (s - 1) // 2, 0)) for key, (s, h) in zip(keys, plan)])
        c.call((keys, 2, 0))
    c.want = dict(seg_replayed=0, to_host_layout=0, segments=True)
    c.full_homes = []
    return c


CASES["saturation_whole"] = functools.partial(_saturation, "saturation_whole", False, 320)
CASES["saturation_split"] = functools.partial(_saturation, "saturation_split", True, 321)


@_case("park_then_saturate")
def _park_then_saturate():
    """17 keys of one home, 7 occurrences each behind the first in one batch: the key without a slot is parked 7 times and its count arrives
    by the replay; then 300 more of every key, all of high quality"""
    c = Case("park_then_saturate", ONE(1), 330)
    keys = c.role("home5", c.P.at(0, 12, 4, 0, 5, 17, "park"))
    c.call((keys, 8, 4), sync=True)
    if c.positions(0) > ONE_BATCH:
        raise CorpusError("the parking call is more than one batch")
    c.call((keys[::4], 300, 300), (keys[1::4], 247, 55))
    c.want = dict(seg_replayed=7, table_replayed=0, to_host_layout=0, segments=True)
    c.full_homes = []
    return c


@_case("way_in_place")
def _way_in_place():
    """fewer entries than slots / 16 into a segment of 2^10 slots: the block is updated in HBM, not staged -- 30 creating entries and one
    key twice among them"""
    c = Case("way_in_place", ONE(7), 340)
    keys = c.role("few", c.P.seg(0, 30, None, "in place"))
    twice = c.role("twice", c.P.seg(0, 1, None, "in place twice"))
    c.call((keys + twice, 1, 1))
    c.call((keys, 1, 0), (twice, 2, 2), sync=True)
    c.call((keys[:10], 1, 1), (twice, 3, 0))
    c.entries = [0, 32, 13]
    c.want = dict(seg_replayed=0, to_host_layout=0, segments=True, seg_shift=10)
    c.full_homes = []
    return c


@_case("way_in_place_full_block")
def _way_in_place_full_block():
    """seg_upsert's own probe loop on a full block: segments of 2^10 slots in blocks of 2^5 (BFCG_SEG_BLOCK = 5), one block filled by 32 keys
    of one home in one batch while the segment is a thirty-second full.  Then every key once more in a call of its own -- ONE entry, fewer
    than slots / 16, so the block is updated in place -- one of which sits 31 slots from its home; last a 33rd key of that home: parked
    after a probe of all 32 slots, the segment doubled, the k-mer replayed"""
    c = Case("way_in_place_full_block", ONE(7, BFCG_SEG_BLOCK=5), 341)
    keys = c.role("home20", c.P.at(0, 5, 10, 7, 20, 32, "full block"))
    late = c.role("late", c.P.at(0, 5, 10, 7, 20, 1, "full block late"))
    c.call((keys + late, 1, 0))
    c.call((keys, 1, 1), sync=True)
    for key in keys:
        c.call(([key], 1, 1))
    # (drained and looked at before the 33rd key comes: a hit that is wrongly parked doubles the segment and is replayed just as that key is,
    # and the sums after the whole would be the same)
    c.sync_after.add(len(c.calls))
    c.checks[len(c.calls)] = dict(seg_replayed=0, seg_growths=0, seg_shift=10)
    c.call((late, 1, 1))
    c.absent = c.P.at(0, 5, 10, 7, 20, 1, "full block absent")
    c.want = dict(seg_replayed=1, to_host_layout=0, segments=True, seg_shift=11, seg_growths=1)
    c.full_homes = []
    return c


@_case("way_cas")
def _way_cas():
    """one k-mer 65 600 times in a call beside 40 ordinary keys of its region: 65 536 entries and more switch the counter pairs off, the
    block is staged and updated by compare-and-swap.  The region's share overflows its slab: the batch is replayed through the two-pass
    partition and handed over at its records' offsets"""
    c = Case("way_cas", CAS(), 350)
    region = 1234
    hot = c.role("hot", c.P.seg(region, 1, None, "cas hot"))
    plain = c.role("plain", c.P.seg(region, 40, None, "cas plain"))
    c.call((hot, 65600, 70), (plain, 3, 1))
    c.call((hot + plain, 1, 1))
    c.want = dict(seg_replayed=0, to_host_layout=0, segments=True, replayed_batches=("min", 1))
    c.full_homes = []
    return c


@_case("block_full_low_load")
def _block_full_low_load():
    """segments of 2^6 slots in blocks of 2^3 (BFCG_SEG_BLOCK = 3): nine keys of block 2 of a segment that is otherwise empty -- one is
    parked although the segment is a seventh full (seg_target_shift's "one full segment under a low overall load") -- four of which move to
    block 2 + 8 when the segment doubles.  The parked k-mer is replayed into its block of the grown segment"""
    c = Case("block_full_low_load", ONE(3, BFCG_SEG_BLOCK=3), 360)
    stay = c.role("stay", c.P.seg(0, 5, lambda h: ((h >> U(3)) & U(15)) == U(2), "block stays"))
    move = c.role("move", c.P.seg(0, 4, lambda h: ((h >> U(3)) & U(15)) == U(10), "block moves"))
    c.call((stay + move, 2, 1), sync=True)
    c.call((stay + move, 1, 1))
    c.absent = c.P.seg(0, 1, lambda h: ((h >> U(3)) & U(7)) == U(2), "block absent")
    c.want = dict(seg_replayed=1, to_host_layout=0, segments=True, seg_shift=7, seg_growths=1)
    c.full_homes = []
    return c


@_case("block_three_growths")
def _block_three_growths():
    """three growths in a row, each forced by a ninth key of one block of 2^3 slots at the size the segment then has (2^6, 2^7, 2^8)"""
    c = Case("block_three_growths", ONE(3, BFCG_SEG_BLOCK=3), 361)
    for stage, (bits, blk) in enumerate(((3, 5), (4, 3), (5, 17))):
        keys = c.role("stage%d" % stage, c.P.seg(0, 9, lambda h, bits=bits, blk=blk: ((h >> U(3)) & U(_mask(bits))) == U(blk), "growth %d" % stage))
        c.call((keys, 2, stage), sync=True)
    c.call((c.keys(), 1, 1))
    c.want = dict(seg_replayed=3, to_host_layout=0, segments=True, seg_shift=9, seg_growths=3)
    c.full_homes = []
    return c


W_REGIONS = (0, 255, 511)


def _windows(name, K, tail, seed, drain=True):
    """512 regions, hand-over windows of up to K pages.  Per region of (first, middle, last): 16 keys that fill its segment exactly
    (`fill`), 3 keys that come when it is full (`late`: their page creates nothing, all its entries are parked), and in the regions beside
    them keys that are first seen in one page and again in every later one (`spread`); a key of region 300 that saturates over the windows
    (`sat`).  Calls: 1 first occurrences only (a page that creates nothing, a window of its own: the first commit), 2 creates fill and
    spread, 3 hits, 4 the late keys' first occurrences, 5 their second (all parked) -- the test drains behind it, so the replay's keys are
    the parking call's --, 6 .. 9 go on.  tail = True: the parking call is the last one and nothing is drained before the end.
    drain = False: call 5 parks and the run goes on undrained, as bfc_count runs.  The context learns of the parked k-mers when it finalises the
    batch that carried the commit -- one call later -- and drains then, with the next call's batch (whose third occurrences of the late
    keys park as well) already in flight: the replay's keys go to the call drained at, and the calls between (`short_calls`: 5 for windows
    of one page; 5 and 6 for windows of four, where call 6 carries the commit of pages 3 .. 6 and call 7 is drained at) stay short by them"""
    c = Case(name, WINDOWS(K), seed)
    fill, late, spread = [], [], []
    for r in W_REGIONS:
        fill += c.role("fill%d" % r, c.P.seg(r, 16, None, "fill"))
        late += c.role("late%d" % r, c.P.seg(r, 3, None, "late"))
    for r in (1, 256, 510):
        spread += c.role("spread%d" % r, c.P.seg(r, 4, None, "spread"))
    sat = c.role("sat", c.P.seg(300, 1, None, "sat"))
    more = c.role("more", c.P.seg(77, 5, None, "more"))
    c.call((fill + spread, 1, 1), (sat, 1, 0))
    c.call((fill + spread, 1, 0), (sat, 100, 30))
    c.call((fill[::2] + spread, 1, 1), (sat, 100, 30))
    c.call((late, 1, 1), (spread, 1, 0))
    if tail:
        c.call((spread, 1, 0), (sat, 100, 10), (more, 1, 1))
        c.call((spread + more, 1, 0))
        c.call((fill, 2, 1), (spread, 1, 1))
        c.call((late, 1, 0), (spread, 1, 1))
    else:
        c.call((late, 1, 0), (spread, 1, 1), sync=drain)
        c.call((late + spread, 1, 1), (sat, 100, 10), (more, 1, 1))
        c.call((spread + more, 1, 0))
        c.call((fill, 2, 1), (spread, 1, 1))
        c.call((spread + more, 1, 1))
    c.parking_call = len(c.calls) if tail else 5
    c.want = dict(seg_replayed=9 if drain else 18, to_host_layout=0, segments=True, seg_shift=5, max_commit_pages=K, replayed_batches=0, level2_one_pass=True)
    c.short_calls, c.short_by = (set() if drain else {5} if K == 1 else {5, 6}), len(late)
    c.full_homes = []
    return c


for _K in (1, 4):
    CASES["windows_nodrain_K%d" % _K] = functools.partial(_windows, "windows_nodrain_K%d" % _K, _K, False, 440 + _K, False)
for _K in (1, 2, 4):
    CASES["windows_K%d" % _K] = functools.partial(_windows, "windows_K%d" % _K, _K, False, 400 + _K)
for _K in (2, 4):
    CASES["windows_tail_K%d" % _K] = functools.partial(_windows, "windows_tail_K%d" % _K, _K, True, 410 + _K)


@_case("leave_segments")
def _leave_segments():
    """BFCG_SEG_BLOCK = 4, BFCG_SEG_TOTAL = 5: a segment may have 2^4 or 2^5 slots.  17 keys of one home in one batch park one k-mer 3 times and
    ask for 2^6 slots: the segments leave for the host's layout with k-mers still parked (seg_to_legacy, then k_table_replay); two more
    calls are counted there"""
    c = Case("leave_segments", ONE(1, BFCG_SEG_BLOCK=4, BFCG_SEG_TOTAL=5), 500)
    keys = c.role("home3", c.P.at(0, 4, 4, 0, 3, 17, "leave"))
    other = c.role("other", c.P.seg(0, 6, None, "leave other"))
    c.call((keys, 4, 2), sync=True)
    c.call((keys[:9], 2, 2), (other, 2, 0))
    c.call((keys[5:] + other, 1, 1))
    c.want = dict(seg_replayed=0, table_replayed=3, to_host_layout=1, segments=False)
    c.full_homes = []
    return c


@_case("after_reset")
def _after_reset():
    """what the same context counts in segments again after bfcg_reset: a chain of 12 keys of one home that wraps round the segment's end"""
    c = Case("after_reset", ONE(1, BFCG_SEG_BLOCK=4, BFCG_SEG_TOTAL=5), 501)
    keys = c.role("home12", c.P.at(0, 4, 4, 0, 12, 12, "after reset"))
    c.call((keys, 3, 1), sync=True)
    c.call((keys, 1, 1))
    c.want = dict(segments=True, seg_shift=4)   # (12 keys in 16 slots: below 85 %, and 2^6 slots are not allowed: the segments run fuller)
    c.full_homes = []
    c.absent = c.P.at(0, 4, 4, 0, 12, 1, "after reset absent")
    return c


def _host_chain(name, k, l_pre, cshift, park, seed):
    """the host's layout from the start: a sub-table filled exactly by keys of its last slot (the chain wraps), one filled by keys of an odd
    home, and with `park` one that gets a key more than it has slots (parked, the table rehashed, the k-mer replayed) -- first, middle and
    last sub-table; all created in one batch.  The two occurrences of the parked k-mer in that batch reach the table as ONE aggregated update
    (agg_add), so one entry is parked and replayed"""
    c = Case(name, HOST(k, l_pre, cshift), seed)
    n_sub, R = 1 << c.P.l_pre, 1 << cshift
    wrap = c.role("wrap", c.P.host(0, R - 1, cshift, R, "host wrap"))
    odd = c.role("odd", c.P.host(n_sub // 2, 1, cshift, R, "host odd"))
    over = c.role("over", c.P.host(n_sub - 1, 0, cshift, R + 1, "host over")) if park else []
    keys = wrap + odd + over
    c.call((keys, 1, 0))
    c.call((keys, 2, 1), sync=True)
    c.call((keys, 1, 1))
    c.absent = c.P.host(0, R - 1, cshift, 1, "host absent") + c.P.host(n_sub // 2, 1, cshift, 1, "host absent")
    c.want = dict(seg_replayed=0, table_replayed=1 if park else 0, to_host_layout=0, segments=False, tab_cshift=cshift + (1 if park else 0))
    c.full_homes = []
    return c


for _k, _lp, _cs in ((21, 4, 1), (21, 8, 3), (33, 16, 3), (47, 24, 1)):
    for _park in (False, True):
        _nm = "host_chain_k%d_l%d_c%d_%s" % (_k, _lp, _cs, "park" if _park else "full")
        CASES[_nm] = functools.partial(_host_chain, _nm, _k, _lp, _cs, _park, 600 + _k + _lp + _cs + int(_park))


AGG_SEEN = (254, 255, 256, 300, 65539, 70000)   # 65 536 + 3: a hand-over that wrapped at 16 bits instead of capping would leave a count of 3


@_case("host_aggregated")
def _host_aggregated():
    """counts that reach the table as ONE aggregated update of 254, 255, 256, 300, 65 539 and 70 000 (k_bloom's hand-over caps at 0xffff): every key's
    occurrences in one batch of a filter large enough to take the call whole"""
    c = Case("host_aggregated", HOST(21, 8, 3, bf_shift=28, max_batch_pos=1 << 22), 700)
    keys = c.P.host(None, None, 3, len(AGG_SEEN), "aggregated")
    for key, s in zip(keys, AGG_SEEN):
        c.role("seen%d" % s, [key])
    c.call(*[([key], s + 1, s // 2) for key, s in zip(keys, AGG_SEEN)])
    c.call((keys, 1, 1))
    c.want = dict(segments=False, to_host_layout=0)
    c.full_homes = []
    return c


def _host_same_y0(name, k, seed):
    """k > 32: agg_add finds a k-mer by Y0 and tells k-mers that share it apart by Y1.  Two k-mers with one Y0 in one batch; three of which
    one comes once, one 300 times and one not at all in the first call.  One Y0 is one sub-table (ch_subkey takes it from Y0's high bits)"""
    c = Case(name, HOST(k, 20, 3 if k == 33 else 1), seed)
    two = c.role("two", c.P.same_y0(2, name))
    three = c.role("three", c.P.same_y0(3, name))
    c.call((two, 3, 1), (three[:1], 1, 1), (three[1:2], 300, 7))
    c.call((two[:1], 2, 2), (three, 2, 1), sync=k == 47)
    c.call((three[2:], 3, 3), (two, 1, 0))
    c.shared_bits = True
    # (k = 47: the three share a sub-table of 2 slots, so the third is parked -- one aggregated update -- and replayed into the table rehashed)
    c.want = dict(segments=False, to_host_layout=0, table_replayed=1 if k == 47 else 0, tab_cshift=2 if k == 47 else 3)
    c.full_homes = []
    return c


CASES["host_same_y0_k33"] = functools.partial(_host_same_y0, "host_same_y0_k33", 33, 710)
CASES["host_same_y0_k47"] = functools.partial(_host_same_y0, "host_same_y0_k47", 47, 711)


@functools.lru_cache(maxsize=None)
def case(name):
    """the case of that name -- made once, never changed"""
    c = CASES[name]()
    if c.name != name:
        raise CorpusError("case %s calls itself %s" % (name, c.name))
    return c


def crowded_reads(seed=720, length=700):
    """(seq, qual, off): one read of `length` random bases three times over -- more than ag_cap = 256 distinct seen k-mers in the one region
    of geometry ONE in one batch (not placed: the aggregation table overflows whatever they are)"""
    rng = np.random.default_rng(seed)
    read = ACGT[rng.integers(0, 4, length)]
    seq = np.concatenate([read, read, read])
    return seq, np.full(len(seq), HIGH, dtype=np.uint8), np.arange(4, dtype=U) * U(length)
