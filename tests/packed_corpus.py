"""Count tables whose slots the test writes (test_packed_host.py, test_gpu_packed.py).  No GPU.

Every read-out of the count table probes it the same way: from the home slot (key & cmask) of the region sub << cshift, linearly, until the
key, an empty slot, or a whole region.  The tables the other tests read are at most 4/7 full, so a full region or a chain that wraps
round a region's end is there only by accident.  Here the layout is the test's choice, through HostTable.from_slots:

  chain_case(k, l_pre, cshift)   tables laid out slot by slot, with the expected answer of every query (below)
  relaid(table, cshift)          the slots of a HostTable placed at another cshift
  filled(table)                  the table at the smallest cshift its largest sub-table fits, three of its regions filled up exactly
  full_result(table, how)        an input whose clip / pop_bubbles / union result has one region exactly full
  sweep_case(l_pre, cshift)      random slots, a full and an empty region: for the passes that stream and do not probe

A key is chosen by (sub-table, key), so its home slot is known.  Its k-mer comes from bfcg_kmer_decode_host; the candidate is kept only if
the oracle's forward hash (oracle.orc_kmer_hash + orc_ch_subkey) gives the same (sub-table, key) back: the decode inverts the hash of the
strand the forward hash chose, so about half of the candidates fail.  Every table of chain_case records its own count (Table.stats).  The tables of chain_case at k = 33 and 37 have
fewer sub-tables than bfc_ch_init would give them (it clamps l_pre to 2 k - 50 there); ch_subkey then folds Y0 into Y1 (its second key
formula with sh < k) and the key is no longer decodable.  Such a key is drawn as a hash (Y0, Y1) and its k-mer decoded at the lossless
geometry; a listing of such a table decodes to bits that are not the k-mer, which the tests hold to the host's instance of the same decode.

chain_case: VARIANTS tables per case.  A region is one sub-table's, so a table has one first and one last region: over the variants every
region class below stands once in the first and once in the last sub-table and, in every variant, in a middle one.
  b  a full region whose keys all share one home h != 0: the key displaced by d for every d in 0 .. 2^cshift - 1, the chain wrapped
  c  a full region whose chains of three homes (the last slot, 0, 1) interleave
  d  a chain that starts in the region's last slot and goes on at slot 0, an empty slot behind it
  e  a region with one key, at home (slot 0 in the first sub-table, the last slot in the last one)
  f  an empty region
  r  (the other sub-tables) two keys at their homes, or nothing
Class a, a key at home, is every key with a displacement of 0.  Absent queries: one per home of every full region (the probe walks the
whole region); one that ends at the empty slot behind the wrap of d; one into the empty region; near misses of present keys -- another
bit at or above 32 of the key, the same key in another sub-table, another key of the same home.  Counts 1, 2, 255 and high counts 0, 63
in turn.  Every present k-mer is asked on both strands.  A class that cannot be filled raises CorpusError."""
import collections
import ctypes as C
import functools

import numpy as np

import oracle
from graph_oracle import revcomp, strs_of_planes
from test_kmers_host import _forward

U = np.uint64
KS = (21, 33, 37)
GEOMS = ((4, 2), (4, 3), (8, 5))
CLASSES = "bcdef"
VARIANTS = len(CLASSES)
COUNTS, HIGHS = (1, 2, 255), (0, 63)

Key = collections.namedtuple("Key", "sub key y Y")                  # key = slot >> 14; y = planes (a, b); Y = hash (Y0, Y1)
Placed = collections.namedtuple("Placed", "sub pos key value y disp cls")
Query = collections.namedtuple("Query", "y want cls sub")


class CorpusError(AssertionError):
    pass


def _lib():
    from bfc_amd import _lib
    return _lib.load()


def _mask(n):
    return (1 << n) - 1


def subkey(k, l_pre, Y0, Y1):
    """ch_subkey (kmer_dev.h, htab.c:45-58) without the slot's low bits: (sub-table, key)"""
    if k <= 32:
        t = 2 * k - l_pre
        z = Y0 << k | Y1
        return z >> t, z & _mask(t)
    t = k - l_pre
    sh = k if t + k < 50 else 50 - t
    return Y0 >> t, ((Y0 & _mask(t)) << sh) ^ Y1


def kmer_of_hash(k, Y0, Y1):
    """the planes (a, b) that bfcg_kmer_decode_host gives for the hash (Y0, Y1), at the geometry where the key is lossless"""
    lc = oracle.lib().orc_ch_clamp_lpre(k, 0)
    sub, key = subkey(k, lc, Y0, Y1)
    out = (C.c_uint64 * 2)()
    if _lib().bfcg_kmer_decode_host(k, lc, sub, key << 14 | 1, out) != 0:
        raise CorpusError("k=%d is not decodable" % k)
    return int(out[0]), int(out[1])


def accept(k, l_pre, Y0, Y1, stats=None):
    """the planes of the k-mer with hash (Y0, Y1), or None where the oracle's forward hash of that k-mer is another one; `stats`, a
    Counter, is told of the candidate ("tried") and of its being kept"""
    stats = collections.Counter() if stats is None else stats
    a, b = kmer_of_hash(k, Y0, Y1)
    stats["tried"] += 1
    Y = _forward(k, [((b >> l & 1) << 1) | (a >> l & 1) for l in range(k - 1, -1, -1)])
    if Y != (Y0, Y1):
        return None
    key = C.c_uint64()
    sub = oracle.lib().orc_ch_subkey(k, l_pre, (C.c_uint64 * 2)(*Y), C.byref(key))
    if (sub, key.value >> 14) != subkey(k, l_pre, Y0, Y1):
        raise CorpusError("the oracle's ch_subkey and this file's differ at k=%d l_pre=%d" % (k, l_pre))
    stats["kept"] += 1
    return a, b


class Picker:
    """draws keys of a given sub-table and home slot, each once"""

    def __init__(self, k, l_pre, cshift, seed):
        self.k, self.l_pre, self.cshift = k, l_pre, cshift
        self.rng, self.used, self.stats = np.random.default_rng(seed), set(), collections.Counter()
        self.t = 2 * k - l_pre if k <= 32 else k - l_pre
        if k > 32 and (k if self.t + k < 50 else 50 - self.t) < cshift:
            raise CorpusError("the home slot is not Y1's low bits at k=%d l_pre=%d cshift=%d" % (k, l_pre, cshift))

    def _bits(self, n):
        return int(self.rng.integers(0, 1 << 62)) & _mask(n)

    def _hash(self, sub, home):
        k, cm = self.k, _mask(self.cshift)
        if k <= 32:
            z = sub << self.t | (self._bits(self.t) & ~cm) | home
            return z >> k, z & _mask(k)
        return sub << self.t | self._bits(self.t), (self._bits(k) & ~cm) | home   # (the fold leaves the key's low bits Y1's)

    def take(self, Y0, Y1):
        """the Key of a hash if nothing holds it yet and its k-mer hashes back to it, else None"""
        sub, key = subkey(self.k, self.l_pre, Y0, Y1)
        if (sub, key) in self.used:
            return None
        y = accept(self.k, self.l_pre, Y0, Y1, self.stats)
        if y is None:
            return None
        self.used.add((sub, key))
        return Key(sub, key, y, (Y0, Y1))

    def key(self, sub, home, what=""):
        for _ in range(200):
            got = self.take(*self._hash(sub, home))
            if got is not None:
                assert got.sub == sub and got.key & _mask(self.cshift) == home
                return got
        raise CorpusError("no key of sub-table %d with home %d after 200 candidates (%s)" % (sub, home, what))

    # ---- near misses of a held key: hashes that differ from it in one respect
    def miss_high(self, held):
        """the same sub-table and low 32 key bits, another bit at or above 32"""
        k, (Y0, Y1) = self.k, held.Y
        if k <= 32:
            z = Y0 << k | Y1
            cands = [((z ^ 1 << j) >> k, (z ^ 1 << j) & _mask(k)) for j in range(32, self.t)]
        else:
            sh = k if self.t + k < 50 else 50 - self.t
            cands = [(Y0, Y1 ^ 1 << j) for j in range(32, k)] + [(Y0 ^ 1 << i, Y1) for i in range(self.t) if sh + i >= 32]
        for c in cands:
            sub, key = subkey(k, self.l_pre, *c)
            if sub == held.sub and key & _mask(32) == held.key & _mask(32) and key != held.key:
                got = self.take(*c)
                if got is not None:
                    return got
        return None

    def miss_sub(self, held, subs):
        """the same key in another sub-table"""
        k, (Y0, Y1) = self.k, held.Y
        for s in subs:
            if s == held.sub:
                continue
            if k <= 32:
                z = s << self.t | ((Y0 << k | Y1) & _mask(self.t))
                c = z >> k, z & _mask(k)
            else:
                c = s << self.t | (Y0 & _mask(self.t)), Y1
            assert subkey(k, self.l_pre, *c) == (s, held.key)
            got = self.take(*c)
            if got is not None:
                return got
        return None


class Table:
    """one laid-out table: slots u64 (2^(l_pre + cshift)), placed (list of Placed), queries (list of Query), roles {sub-table: class},
    stats {"tried", "kept"}: the candidates its builder decoded and those whose forward hash came back"""

    def host(self, gpu_lib):
        return gpu_lib.HostTable.from_slots(self.k, self.l_pre, self.cshift, self.slots)

    def arrays(self):
        """(y (n, 2) u64, want i16 (n)) of the queries"""
        return np.array([q.y for q in self.queries], dtype=U).reshape(-1, 2), np.array([q.want for q in self.queries], dtype=np.int16)

    def l1(self):
        """(sizes u32, slots u64) as export_sorted() must give them: the chosen slots by (sub-table, value)"""
        vals = sorted((p.sub, p.key << 14 | p.value) for p in self.placed)
        sizes = np.bincount([s for s, v in vals], minlength=1 << self.l_pre).astype(np.uint32)
        return sizes, np.array([v for s, v in vals], dtype=U)


def _layout(cls, sub, n_sub, R):
    """the class's plan for a region of R slots: ([(position, home)], [(home, class of an absent query)])"""
    if cls == "b":
        h = 1 + sub % (R - 1)
        return [((h + d) % R, h) for d in range(R)], [(hh, "full-home") for hh in range(R)]
    if cls == "c":
        return [(p, (R - 1, 0, 1)[p % 3]) for p in range(R)], [(hh, "full-home") for hh in range(R)]
    if cls == "d":
        m = 2 if R == 4 else 3
        chain = [((R - 1 + i) % R, R - 1) for i in range(m)]
        return chain + ([(R // 2, R // 2)] if R >= 8 else []), [(R - 1, "wrap-empty")]
    if cls == "e":
        h = 0 if sub == 0 else R - 1 if sub == n_sub - 1 else R // 2
        return [(h, h)], [(h, "miss-key"), ((h + 1) % R, "next-empty")]
    if cls == "f":
        return [], [(sub % R, "empty-region")]
    if cls == "r":
        return ([] if sub % 4 == 3 else [(sub % R, sub % R), ((sub + R // 2) % R, (sub + R // 2) % R)]), []
    raise CorpusError(cls)


def roles_of(v, n_sub):
    """{sub-table: class} of variant v: class v in the first sub-table, class v + 2 in the last, all five in the middle"""
    roles = {s: "r" for s in range(n_sub)}
    for j, c in enumerate(CLASSES):
        roles[n_sub // 2 - 2 + j] = c
    roles[0], roles[n_sub - 1] = CLASSES[v], CLASSES[(v + 2) % VARIANTS]
    return roles


@functools.lru_cache(maxsize=None)
def chain_case(k, l_pre, cshift):
    """the VARIANTS tables of a case, as a tuple of Table -- made once, never changed"""
    from bfc_amd import api
    n_sub, R, out = 1 << l_pre, 1 << cshift, []
    for v in range(VARIANTS):
        P = Picker(k, l_pre, cshift, seed=1000 * k + 100 * l_pre + 10 * cshift + v)
        t = Table()
        t.k, t.l_pre, t.cshift, t.variant, t.roles = k, l_pre, cshift, v, roles_of(v, n_sub)
        t.slots, t.placed, keys, absent = np.zeros(n_sub << cshift, dtype=U), [], [], []
        for sub in range(n_sub):
            plan, ask = _layout(t.roles[sub], sub, n_sub, R)
            for pos, home in plan:
                key = P.key(sub, home, "class %s" % t.roles[sub])
                i = len(t.placed)
                value = HIGHS[i % 2] << 8 | COUNTS[i % 3]
                if t.slots[(sub << cshift) + pos]:
                    raise CorpusError("two keys planned for one slot")
                t.slots[(sub << cshift) + pos] = key.key << 14 | value
                t.placed.append(Placed(sub, pos, key.key, value, key.y, (pos - home) % R, t.roles[sub]))
                keys.append(key)
            absent += [(P.key(sub, home, "absent, %s" % c), c) for home, c in ask]
        # near misses: of the first held keys that allow one of each kind (three of a kind at most)
        for kind in ("miss-high", "miss-sub", "miss-key"):
            n = 0
            for p, h in zip(t.placed, keys):
                got = (P.miss_high(h) if kind == "miss-high" else P.miss_sub(h, [n_sub - 1, 0, n_sub // 2, 1]) if kind == "miss-sub"
                       else P.key(p.sub, p.key & _mask(cshift), "miss-key"))
                if got is not None:
                    absent.append((got, kind))
                    n += 1
                if n == 3:
                    break
            if n == 0:
                raise CorpusError("no near miss of kind %s at k=%d l_pre=%d cshift=%d" % (kind, k, l_pre, cshift))
        t.queries = [Query(p.y, p.value, p.cls, p.sub) for p in t.placed]
        rc = api.kmer_revcomp(k, np.array([p.y for p in t.placed], dtype=U))
        t.queries += [Query((int(r[0]), int(r[1])), p.value, p.cls + "/rc", p.sub) for p, r in zip(t.placed, rc)]
        t.queries += [Query(key.y, -1, c, key.sub) for key, c in absent]
        rc = api.kmer_revcomp(k, np.array([key.y for key, c in absent], dtype=U))
        t.queries += [Query((int(r[0]), int(r[1])), -1, c + "/rc", key.sub) for (key, c), r in zip(absent, rc)]
        t.stats = dict(P.stats)
        if result_cshift(l_pre, len(t.placed), 1 << cshift) != cshift:
            raise CorpusError("a copy of this table would not keep cshift %d: %d keys" % (cshift, len(t.placed)))
        t.slots.setflags(write=False)
        out.append(t)
    return tuple(out)


def inventory(t):
    """what a Table holds, from its own records: {class: set of sub-tables} of the regions, the displacements of class b per sub-table,
    the classes of the absent queries, the full regions with a wrapped chain"""
    R = 1 << t.cshift
    inv = {"regions": collections.defaultdict(set), "b_disp": collections.defaultdict(set), "absent": collections.Counter(), "at_home": set(), "wrapped_full": set()}
    for s, c in t.roles.items():
        inv["regions"][c].add(s)
    for p in t.placed:
        if p.cls == "b":
            inv["b_disp"][p.sub].add(p.disp)
        if p.disp == 0:
            inv["at_home"].add(p.sub)
        if p.pos - p.disp < 0:   # its home lies behind it: the chain went round the region's end
            if (t.slots[p.sub << t.cshift:(p.sub + 1) << t.cshift] != 0).all():
                inv["wrapped_full"].add(p.sub)
    for q in t.queries:
        if q.want == -1 and not q.cls.endswith("/rc"):
            inv["absent"][q.cls] += 1
    assert R == len(t.slots) >> t.l_pre
    return inv


# ---- placing slots: the second table of the two-table reads, relaid(), filled(), the inputs of full_result() ---------------------------

def place(l_pre, cshift, subs, vals):
    """slots u64 (2^(l_pre + cshift)) with every value of vals put into its sub-table's region by linear probing from its home slot, in the
    order given; CorpusError if a region overflows"""
    cm, slots = _mask(cshift), np.zeros(1 << (l_pre + cshift), dtype=U)
    for s, v in zip(subs, vals):
        s, v = int(s), int(v)
        base, pos = s << cshift, (v >> 14) & cm
        for _ in range(cm + 1):
            if not slots[base + pos]:
                slots[base + pos] = v
                break
            pos = (pos + 1) & cm
        else:
            raise CorpusError("sub-table %d does not fit 2^%d slots" % (s, cshift))
    return slots


def occupied(t):
    """(sub-table, slot value) of every occupied slot of a HostTable, in slot order"""
    cshift, slots = t.raw()
    at = np.flatnonzero(slots)
    return at >> cshift, slots[at]


def relaid(gpu_lib, t, cshift):
    """a new HostTable: t's slots at another cshift"""
    subs, vals = occupied(t)
    return gpu_lib.HostTable.from_slots(t.k, t.l_pre, cshift, place(t.l_pre, cshift, subs, vals))


def _strings(t):
    """(sub-table, stored string) of every key of a HostTable, in export_sorted()'s order"""
    sizes = t.export_sorted()[0]
    return np.repeat(np.arange(len(sizes)), sizes), strs_of_planes(t.graph_nb(1)[0], t.k)


def fillers(t, sub, n, have, seed, isolated=False):
    """n slot values (count 1) of sub-table `sub` of HostTable t: random keys, decoded and forward-checked, whose k-mer `have` (a set of
    strings, both strands; extended here) does not hold; with `isolated`, none of whose eight neighbours `have` holds either"""
    k, l_pre = t.k, t.l_pre
    if k > 32:
        raise CorpusError("fillers are drawn for k <= 32")
    bits, rng, out = 2 * k - l_pre, np.random.default_rng(seed), []
    for _ in range(200 * n + 200):
        if len(out) == n:
            return out
        key = int(rng.integers(0, 1 << 62)) & _mask(bits)
        z = sub << bits | key
        y = accept(k, l_pre, z >> k, z & _mask(k))
        if y is None:
            continue
        s = strs_of_planes(np.array([y], dtype=U), k)[0]
        r = revcomp(s)
        if s in have or r in have:
            continue
        if isolated and any(x[1:] + bytes([c]) in have or bytes([c]) + x[:-1] in have for x in (s, r) for c in b"ACGT"):
            continue
        if isolated and (s[1:] == s[:-1] or any(s[1:] + bytes([c]) == r or bytes([c]) + s[:-1] == r for c in b"ACGT")):
            continue   # (its own neighbour)
        have.update((s, r))
        out.append(key << 14 | 1)
    raise CorpusError("sub-table %d of k=%d l_pre=%d has no %d %sfillers" % (sub, k, l_pre, n, "isolated " if isolated else ""))


def filled(gpu_lib, t, seed=0):
    """(a new HostTable, its cshift, the three sub-tables made exactly full): t at the smallest cshift its largest sub-table fits, with
    filler nodes of count 1 added to the largest sub-table, the first and the last one (the middle one where these coincide)"""
    sizes = t.export_sorted()[0].astype(np.int64)
    n_sub, big = len(sizes), int(sizes.argmax())
    cshift = max(1, int(sizes.max() - 1).bit_length())
    targets = []
    for s in (big, 0, n_sub - 1, n_sub // 2, n_sub // 2 + 1):
        if s not in targets and len(targets) < 3:
            targets.append(s)
    subs, vals = occupied(t)
    have = set()
    for s in _strings(t)[1]:
        have.update((s, revcomp(s)))
    add_s, add_v = [], []
    for s in targets:
        new = fillers(t, s, (1 << cshift) - int(sizes[s]), have, seed + s)
        add_s += [s] * len(new)
        add_v += new
    out = gpu_lib.HostTable.from_slots(t.k, t.l_pre, cshift, place(t.l_pre, cshift, np.concatenate([subs, np.array(add_s, dtype=np.int64)]),
                                                                   np.concatenate([vals, np.array(add_v, dtype=U)])))
    return out, cshift, targets


def result_cshift(l_pre, keys, most):
    """the library's geometry rule for a result table (clip_cshift in bfcg_gclean.h, bfcg_kmers_union, and bfc_ch_union where no region
    overflows earlier): the smallest cshift >= 2 whose table is at most half full and whose regions take the largest sub-table"""
    return next(c for c in range(2, 40) if (1 << (l_pre + c)) >= 2 * keys and (1 << c) >= most)


def result_geometry(l_pre, sizes):
    """(c, sub-table): the fullest sub-table s and the smallest c >= 2 such that, with sizes[s] raised to 2^c, the library's rule for a
    result -- the smallest cshift >= 2 with 2^(l_pre + cshift) >= 2 keys and 2^cshift >= the largest sub-table -- gives c (it cannot
    give less: the raised sub-table does not fit 2^(c - 1))"""
    sizes = np.asarray(sizes, dtype=np.int64)
    s = int(sizes.argmax())
    for c in range(2, 30):
        keys = int(sizes.sum() - sizes[s]) + (1 << c)
        if int(sizes.max()) <= 1 << c and 2 * keys <= 1 << (l_pre + c):
            return c, s
    raise CorpusError("no result geometry")


def full_result(gpu_lib, t, how, survivors):
    """The input of a call whose result has a full region.  how = "clip" / "pop": (HostTable, c, sub-table) -- t with isolated filler nodes
    added to one sub-table so that its survivors (`survivors`: the canonical strings the oracle keeps of t) number exactly 2^c and the
    result's geometry rule gives c.  An isolated node survives clip without islands and any pop_bubbles, and changes no other node's fate.
    how = "union": (A, B, c, sub-table) -- A is t, B holds fillers of that sub-table and every third key of A's others, so that the
    union's sub-table has 2^c keys and both geometry rules (bfc_ch_union's and the GPU's, which sums the inputs' sizes) give c."""
    subs, strs = _strings(t)
    n_sub = 1 << t.l_pre
    have = set()
    for s in strs:
        have.update((s, revcomp(s)))
    o_subs, o_vals = occupied(t)
    native = t.raw()[0]
    if how in ("clip", "pop"):
        alive = np.array([min(s, revcomp(s)) in survivors for s in strs], dtype=bool)
        sizes = np.bincount(subs[alive], minlength=n_sub)
        c, sub = result_geometry(t.l_pre, sizes)
        new = fillers(t, sub, (1 << c) - int(sizes[sub]), have, 77, isolated=True)
        all_s, all_v = np.concatenate([o_subs, np.full(len(new), sub, dtype=np.int64)]), np.concatenate([o_vals, np.array(new, dtype=U)])
        need = max(native, int(np.bincount(all_s, minlength=n_sub).max() - 1).bit_length())
        return gpu_lib.HostTable.from_slots(t.k, t.l_pre, need, place(t.l_pre, need, all_s, all_v)), c, sub
    if how != "union":
        raise CorpusError(how)
    a_sizes = np.bincount(o_subs, minlength=n_sub)
    share = np.zeros(len(o_subs), dtype=bool)
    share[::3] = True
    for c in range(2, 30):
        sub = int(a_sizes.argmax())
        share_c = share & (o_subs != sub)
        both = a_sizes + np.bincount(o_subs[share_c], minlength=n_sub)
        n_new = (1 << c) - int(a_sizes[sub])
        keys = int(a_sizes.sum()) + int(share_c.sum()) + n_new
        if n_new >= 1 and int(np.delete(both, sub).max()) <= 1 << c and 2 * keys <= 1 << (t.l_pre + c):
            break
    else:
        raise CorpusError("no union geometry")
    new = fillers(t, sub, n_new, have, 78)
    b_s = np.concatenate([o_subs[share_c], np.full(n_new, sub, dtype=np.int64)])
    b_v = np.concatenate([(o_vals[share_c] & ~U(0x3fff)) | U(63 << 8 | 200), np.array(new, dtype=U)])   # (shared keys: the sums saturate for counts >= 55)
    need = max(2, int(np.bincount(b_s, minlength=n_sub).max() - 1).bit_length())
    return t, gpu_lib.HostTable.from_slots(t.k, t.l_pre, need, place(t.l_pre, need, b_s, b_v)), c, sub


def absent_of_region(t, sub, cshift, n, seed):
    """planes (m, 2) u64 of absent k-mers of sub-table `sub` of HostTable t, one per home slot for min(n, 2^cshift) homes spread over the
    region at `cshift`"""
    have = set()
    for s in _strings(t)[1]:
        have.update((s, revcomp(s)))
    R, k, bits, rng, out = 1 << cshift, t.k, 2 * t.k - t.l_pre, np.random.default_rng(seed), []
    for home in sorted(set(int(h) for h in np.linspace(0, R - 1, min(n, R)))):
        for _ in range(200):
            key = (int(rng.integers(0, 1 << 62)) & _mask(bits) & ~_mask(cshift)) | home
            z = sub << bits | key
            y = accept(k, t.l_pre, z >> k, z & _mask(k))
            if y is not None and strs_of_planes(np.array([y], dtype=U), k)[0] not in have:
                out.append(y)
                break
        else:
            raise CorpusError("no absent k-mer of sub-table %d, home %d" % (sub, home))
    return np.array(out, dtype=U).reshape(-1, 2)


# ---- random slots for the passes that stream -------------------------------------------------------------------------------------------

SWEEP_K = 21


@functools.lru_cache(maxsize=None)
def sweep_case(l_pre, cshift):
    """slots u64 (2^(l_pre + cshift)), read-only: keys of k = 21 that differ inside a sub-table, counts mostly 1, 2, 3 and 255; an all-full
    and an all-empty region (the two regions of l_pre 1), the others filled at random to a share that differs by region"""
    rng = np.random.default_rng(100 * l_pre + cshift)
    n_sub, R, bits = 1 << l_pre, 1 << cshift, 2 * SWEEP_K - l_pre
    slots = np.zeros((n_sub, R), dtype=U)
    full, empty = (0, 1) if n_sub == 2 else (1, 2)
    for s in range(n_sub):
        if s == empty:
            continue
        keys = np.unique(rng.integers(0, 1 << bits, 2 * R, dtype=np.uint64))
        rng.shuffle(keys)
        keys = keys[:R]
        assert len(keys) == R
        cnt = rng.choice(np.array([1, 2, 3, 255, 17, 64], dtype=np.uint64), R, p=[0.4, 0.3, 0.1, 0.1, 0.05, 0.05])
        high = np.minimum(rng.choice(np.array([0, 1, 63], dtype=np.uint64), R), np.minimum(cnt, U(63)))
        on = np.ones(R, dtype=bool) if s == full else rng.random(R) < rng.random()
        slots[s] = np.where(on, keys << U(14) | high << U(8) | cnt, U(0))
    slots = slots.reshape(-1)
    slots.setflags(write=False)
    return slots


# ---- the second table of the two-table reads ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def second_table(k, l_pre, cshift, variant):
    """(cshift + 2, slots u64, read-only) of the table B that chain_case's table A is compared and merged with: every other key of A at
    count 3 / high 1 (shared: a walk of B finds them in A behind their chains), and keys A does not hold -- one per home of A's full
    regions, so that looking them up in A walks a whole region, and two in every other sub-table"""
    a = chain_case(k, l_pre, cshift)[variant]
    P = Picker(k, l_pre, cshift, seed=7 + 1000 * k + 100 * l_pre + 10 * cshift + variant)
    P.used = {(p.sub, p.key) for p in a.placed}
    subs, vals = [p.sub for p in a.placed[::2]], [p.key << 14 | 1 << 8 | 3 for p in a.placed[::2]]
    for s in range(1 << l_pre):
        homes = range(1 << cshift) if a.roles[s] in "bc" else (0, (1 << cshift) - 1)
        for i, h in enumerate(homes):
            subs.append(s)
            vals.append(P.key(s, h, "second table").key << 14 | HIGHS[i % 2] << 8 | COUNTS[i % 3])
    slots = place(l_pre, cshift + 2, subs, vals)
    slots.setflags(write=False)
    return cshift + 2, slots


def l1_of_slots(slots, cshift):
    """(sizes u32, slots u64) in export_sorted()'s form of a slot array: the occupied slots by (sub-table, value)"""
    at = np.flatnonzero(slots)
    sub, v = at >> cshift, np.asarray(slots)[at]
    order = np.lexsort((v, sub))
    return np.bincount(sub, minlength=len(slots) >> cshift).astype(np.uint32), v[order]
