"""The oracle of the two-table tests (test_tabcmp_host.py, test_gpu_tabcmp.py) and their inputs.  No GPU, no library: numpy on two tables in
L1 form, (sizes, slots) as HostTable.export_sorted() gives them.  A key is (sub-table, slot >> 14), its value slot & 0x3fff; inside a
sub-table export_sorted() orders by slot, i.e. by key, so everything here comes out in that order too."""
import numpy as np

U = np.uint64


def pair_reads(reads, heavy):
    """The two read sets of a pair from (seq, qual, off): A the first two thirds of the reads, B the last two thirds.  heavy: reads 0-49
    appended 40 times to each (shared counts above 63, sums below 255) and reads 50-99 appended 150 times (sums and high sums saturate)."""
    seq, qual, off = reads
    n = len(off) - 1

    def take(idx):
        idx = np.asarray(idx, dtype=np.int64)
        lens = (off[idx + 1] - off[idx]).astype(np.int64)
        o = np.zeros(len(idx) + 1, dtype=np.uint64)
        o[1:] = np.cumsum(lens)
        pos = np.repeat(off[idx].astype(np.int64) - o[:-1].astype(np.int64), lens) + np.arange(int(o[-1]))
        return np.ascontiguousarray(seq[pos]), np.ascontiguousarray(qual[pos]), o

    extra = np.concatenate([np.tile(np.arange(50), 40), np.tile(np.arange(50, 100), 150)]) if heavy else np.zeros(0, dtype=np.int64)
    a = np.concatenate([np.arange(0, 2 * n // 3), extra])
    b = np.concatenate([np.arange(n - 2 * n // 3, n), extra])
    return take(a), take(b)


def split(sizes, slots):
    """(sub-table, key, value) of every slot"""
    sub = np.repeat(np.arange(len(sizes), dtype=np.uint64), sizes)
    return sub, slots >> U(14), (slots & U(0x3fff)).astype(np.uint16)


class Join:
    """The distinct keys of two tables in (sub-table, key) order: sub, key, va, vb (a value of 0 = the table does not hold the key: a
    held key has count >= 1), and ia / ib, the row of every slot of A / B."""

    def __init__(self, ta, tb):
        sa, ka, va = split(*ta)
        sb, kb, vb = split(*tb)
        sub, key = np.concatenate([sa, sb]), np.concatenate([ka, kb])
        order = np.lexsort((key, sub))
        s, k = sub[order], key[order]
        new = np.ones(len(s), dtype=bool)
        new[1:] = (s[1:] != s[:-1]) | (k[1:] != k[:-1])
        ids = np.empty(len(s), dtype=np.int64)
        ids[order] = np.cumsum(new) - 1
        self.n_sub = len(ta[0])
        self.sub, self.key = s[new], k[new]
        self.ia, self.ib = ids[:len(sa)], ids[len(sa):]
        self.va, self.vb = np.zeros(len(self.sub), dtype=np.uint16), np.zeros(len(self.sub), dtype=np.uint16)
        self.va[self.ia], self.vb[self.ib] = va, vb
        assert (va > 0).all() and (vb > 0).all() and len(np.unique(self.ia)) == len(sa) and len(np.unique(self.ib)) == len(sb)

    def joint(self):
        """(joint (256, 256) u64, shared, only_a, only_b)"""
        j = np.zeros((256, 256), dtype=np.uint64)
        np.add.at(j, ((self.va & 0xff).astype(np.int64), (self.vb & 0xff).astype(np.int64)), 1)
        ina, inb = self.va > 0, self.vb > 0
        return j, int((ina & inb).sum()), int((ina & ~inb).sum()), int((~ina & inb).sum())

    def sums(self):
        """the unsaturated count and high sums of every key"""
        return ((self.va & 0xff).astype(np.int64) + (self.vb & 0xff), (self.va >> 8).astype(np.int64) + (self.vb >> 8))

    def union(self):
        """the saturating union in L1 form"""
        c, h = self.sums()
        slots = self.key << U(14) | np.minimum(h, 63).astype(np.uint64) << U(8) | np.minimum(c, 255).astype(np.uint64)
        return np.bincount(self.sub.astype(np.int64), minlength=self.n_sub).astype(np.uint32), slots

    def other_of_a(self):
        """for every slot of A what a lookup in B answers: -1, or high << 8 | count"""
        v = self.vb[self.ia].astype(np.int16)
        return np.where(v == 0, np.int16(-1), v)


def keep(slots, min_cnt, min_diff):
    """hash2cnt's -m / -d on the slots' fields"""
    cnt, high = (slots & U(0xff)).astype(np.int64), (slots >> U(8) & U(0x3f)).astype(np.int64)
    return (cnt >= min_cnt) & (np.minimum(cnt, 63) - high >= min_diff)


def keep_vs(slots, other, min_cnt, min_diff, other_min, other_max):
    oc = np.where(other < 0, 0, other.astype(np.int64) & 0xff)
    return keep(slots, min_cnt, min_diff) & (oc >= other_min) & (oc <= other_max)
