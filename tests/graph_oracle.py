"""The fixture and the oracle of the de Bruijn graph tests (test_graph_host.py, test_gpu_graph.py).  No GPU.

The fixture is a constructed read set in which every class of node is there by design:
  - a random 600-base genome G, as reads of 150 bases every 50;
  - a copy of it with one substitution at SUB (a bubble: the k-mer ending at SUB - 1 has two successors, the one starting at SUB + 1 two
    predecessors);
  - G[0:150] with an error 3 bases from its end, at TIP_ERR (a tip of four k-mers, hanging off the k-mer that ends at TIP_ERR - 1);
  - one read of exactly k random bases (an isolated k-mer);
  - a run of k + 5 A's (one k-mer that is its own successor);
  - for even k, a read that is one reverse-palindromic k-mer.
Every read is given three times, so that its k-mers reach the table with a count of 2 at least.

The oracle (DictGraph) is a third route that never touches the library's hash: a dict from the strings of both strands of every k-mer of
an exported table to high << 8 | count, neighbours by slicing strings.  It is the value of the definitions for odd k only: for even k
the reference's strand rule leaves k-mers undecided and a lookup then depends on the strand given."""
import numpy as np

G_LEN, READ_LEN, STEP, SUB, TIP_ERR = 600, 150, 50, 300, 146
SEED_AT = 160    # a mid-genome seed: G[SEED_AT : SEED_AT + k], between the tip's branch and the bubble for every k <= 63
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s.translate(COMP)[::-1]


def unitig_bounds(k):
    """[lo, hi) of G: the unitig around the seed -- from the k-mer after the tip's branch node (a walk to the left stops before stepping on
    a node with a second successor) to the k-mer ending just left of the bubble (it has two successors)"""
    return TIP_ERR + 1 - k, SUB


class Fixture:
    pass


def fixture(k):
    """the reads as (seq, qual, off), and what the generator knows: genome, its variant, the isolated k-mer, the tip read"""
    rng = np.random.default_rng(7000 + k)
    f = Fixture()
    f.k = k
    f.genome = bytes(b"ACGT"[c] for c in rng.integers(0, 4, G_LEN))
    other = b"ACGT"[(b"ACGT".index(f.genome[SUB]) + 1 + int(rng.integers(0, 3))) % 4]
    f.variant = f.genome[:SUB] + bytes([other]) + f.genome[SUB + 1:]
    err = b"ACGT"[(b"ACGT".index(f.genome[TIP_ERR]) + 1 + int(rng.integers(0, 3))) % 4]
    f.tip_read = f.genome[:TIP_ERR] + bytes([err]) + f.genome[TIP_ERR + 1:READ_LEN]
    f.isolated = bytes(b"ACGT"[c] for c in rng.integers(0, 4, k))
    f.a_run = b"A" * k
    reads = [g[s:s + READ_LEN] for g in (f.genome, f.variant) for s in range(0, G_LEN - READ_LEN + 1, STEP)]
    reads += [f.tip_read, f.isolated, b"A" * (k + 5)]
    f.palindrome = None
    if k % 2 == 0:
        half = bytes(b"ACGT"[c] for c in rng.integers(0, 4, k // 2))
        f.palindrome = half + revcomp(half)
        reads.append(f.palindrome)
    reads = [r for r in reads for _ in range(3)]
    f.seq = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    f.qual = np.full(len(f.seq), ord("I"), dtype=np.uint8)
    f.off = np.zeros(len(reads) + 1, dtype=np.uint64)
    f.off[1:] = np.cumsum([len(r) for r in reads])
    f.reads = (f.seq, f.qual, f.off)
    f.seed = f.genome[SEED_AT:SEED_AT + k]
    f.left_of_bubble = f.genome[SUB - k - 5:SUB - 5]      # five steps before the k-mer with two successors
    f.in_branch = f.genome[SUB - 3:SUB - 3 + k]           # holds the variable base: walks to the merge
    lo, hi = unitig_bounds(k)
    f.unitig = f.genome[lo:hi]
    return f


def planes_of_strs(strs, k):
    """k-mers as text -> listing-style planes (n, 2) u64"""
    y = np.zeros((len(strs), 2), dtype=np.uint64)
    for i, s in enumerate(strs):
        a = b = 0
        for l in range(k):
            c = b"ACGT".index(s[k - 1 - l])
            a |= (c & 1) << l
            b |= (c >> 1) << l
        y[i] = a, b
    return y


def strs_of_planes(y, k):
    y = np.asarray(y, dtype=np.uint64).reshape(-1, 2)
    return [bytes(b"ACGT"[(int(b) >> l & 1) << 1 | (int(a) >> l & 1)] for l in range(k - 1, -1, -1)) for a, b in y]


class DictGraph:
    """value / neighbours / census / extension from a dict over both strands' strings (odd k)"""

    def __init__(self, k, strs, cnt_high):
        assert k % 2 == 1
        self.k, self.d = k, {}
        for s, v in zip(strs, cnt_high):
            self.d[s] = self.d[revcomp(s)] = int(v)

    def value(self, s):
        return self.d.get(s, -1)

    def neighbors(self, s):
        return [self.value(s[1:] + bytes([c])) for c in b"ACGT"] + [self.value(bytes([c]) + s[:-1]) for c in b"ACGT"]

    def nb(self, s, min_cnt):
        return sum(1 << j for j, v in enumerate(self.neighbors(s)) if v >= 0 and (v & 0xff) >= min_cnt)

    def extend(self, s, min_cnt, max_len):
        """(path, stop) by the rule of include/bfc_gpu.h"""
        seed, out = s, b""
        v = self.value(s)
        if v < 0 or (v & 0xff) < min_cnt:
            return out, 4
        while True:
            if len(out) == max_len:
                return out, 0
            o = self.nb(s, min_cnt) & 15
            if o == 0:
                return out, 1
            if o & (o - 1):
                return out, 2
            c = b"ACGT"[o.bit_length() - 1]
            nxt = s[1:] + bytes([c])
            i = self.nb(nxt, min_cnt) >> 4
            if i & (i - 1):
                return out, 3
            if nxt == seed:
                return out, 5
            out += bytes([c])
            s = nxt


def census_of_nb(nb):
    """the 5 x 5 census of an array of neighbour bits"""
    nb = np.asarray(nb, dtype=np.uint8)
    pop = np.array([bin(i).count("1") for i in range(16)], dtype=np.int64)
    deg = np.zeros((5, 5), dtype=np.uint64)
    np.add.at(deg, (pop[nb & 15], pop[nb >> 4]), 1)
    return deg


def cells_of_nb(nb):
    """the degree cell 5 * o + i of every entry of an array of neighbour bits"""
    nb = np.asarray(nb, dtype=np.uint8)
    pop = np.array([bin(i).count("1") for i in range(16)], dtype=np.int64)
    return 5 * pop[nb & 15] + pop[nb >> 4]


def in_mask(nb, cell_mask):
    """which entries of an array of neighbour bits have their degree cell set in cell_mask (list_graph's predicate)"""
    return ((int(cell_mask) >> cells_of_nb(nb)) & 1).astype(bool)


def paths(bases, length):
    """the rows of extend()'s bases as bytes, each checked to be zero beyond its length"""
    out = []
    for row, n in zip(bases, length):
        assert not row[n:].any()
        out.append(row[:n].tobytes())
    return out
