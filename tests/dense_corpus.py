"""The draws of the dense-graph tests (test_dense_graph_host.py, test_gpu_dense_graph.py).  No GPU, no library calls.

At k >= 21 a random genome is an almost linear graph.  At k = 8..19 a few kilobases with 2 % errors are not: nodes of degree 3 and 4,
tips and islands of every length that hang off the same branch node and cascade over several clipping rounds, hairpins, palindromic
k-mers at even k -- none of it constructed.  A draw is, from one seed:
  - a random genome of G bases, read at 12x in reads of 60 bases, half of them reverse-complemented, 2 % of the bases substituted;
  - circular contigs of 2 (AC), 3 (ACG), 7, 64, 65 and 130 bases (the last four random), each as reads of k + 20 bases every 5 bases
    round the circle, every read given three times; no read holds both a contig and the genome;
  - a low-count read: k + 3 random bases given TWICE, so that its four k-mers reach the table with a count of 1 (the counter keeps a
    k-mer from its second occurrence on): a unitig at min_cnt 1, absent at 2, as in unitig_oracle.
  - a low-count circular contig of 33 bases: one lap of 33 + k - 1 bases given twice -- a cycle at min_cnt 1 that is absent at 2, so
    that a unitigs(1) call finds more cycle nodes than a unitigs(2) call.
Quality 'I' throughout.  Every draw is counted at -b 20 with its own l_pre, down to 16 sub-tables.

What a draw must contain -- cycles of 2, 64 and 65 nodes, degrees 3 and 4, three clipping rounds, palindromes -- is asserted on the
string oracle by test_dense_graph_host.py; the seeds below were chosen there until every condition held."""
import collections
import functools

import numpy as np

from graph_oracle import revcomp

B = 20                                  # -b of every draw
READ_LEN, COV, ERR = 60, 12, 0.02
CIRC_LENS = (2, 3, 7, 64, 65, 130)
CIRC_STEP, CIRC_OVER, COPIES = 5, 20, 3
LOW_CIRC = 33

#        name: (k, l_pre, G, seed)
DRAWS = {
    "d9": (9, 8, 3000, 0),
    "d11": (11, 12, 4000, 3),
    "d13": (13, 16, 6000, 76),      # (a node of degree 4 at k = 13 takes about one seed in thirty)
    "d15": (15, 4, 8000, 3),
    "d19": (19, 20, 8000, 1),
    "e8": (8, 8, 2000, 0),
    "e12": (12, 12, 4000, 36),      # (five palindromes among 7000 12-mers: about one seed in sixty)
}
ODD = [n for n, d in DRAWS.items() if d[0] % 2]
EVEN = [n for n, d in DRAWS.items() if d[0] % 2 == 0]

Draw = collections.namedtuple("Draw", "k l_pre reads planted")


class Planted:
    """what the generator knows: the genome, the circular contigs by length, the low-count read and circle"""


def _rand(rng, n):
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, n))


def generate(k, G, seed):
    """(reads as a list of bytes, Planted)"""
    rng = np.random.default_rng(seed)
    p = Planted()
    p.genome = _rand(rng, G)
    reads = []
    for _ in range(COV * G // READ_LEN):
        at = int(rng.integers(0, G - READ_LEN + 1))
        r = bytearray(p.genome[at:at + READ_LEN])
        for i in np.flatnonzero(rng.random(READ_LEN) < ERR):
            r[i] = b"ACGT"[(b"ACGT".index(r[i]) + 1 + int(rng.integers(0, 3))) % 4]
        r = bytes(r)
        reads.append(revcomp(r) if rng.integers(0, 2) else r)
    p.circ = {}
    for n in CIRC_LENS:
        c = p.circ[n] = {2: b"AC", 3: b"ACG"}.get(n) or _rand(rng, n)
        lap = c * ((k + CIRC_OVER) // n + 2)
        reads += [lap[s:s + k + CIRC_OVER] for s in range(0, n, CIRC_STEP) for _ in range(COPIES)]
    p.low = _rand(rng, k + 3)
    p.low_circ = _rand(rng, LOW_CIRC)
    low_lap = (p.low_circ * 2)[:LOW_CIRC + k - 1]
    reads += [p.low, p.low, low_lap, low_lap]
    return reads, p


@functools.lru_cache(maxsize=None)
def draw(name):
    """Draw(k, l_pre, reads = (seq, qual, off), planted) -- made once, never changed"""
    k, l_pre, G, seed = DRAWS[name]
    reads, planted = generate(k, G, seed)
    seq = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    qual = np.full(len(seq), ord("I"), dtype=np.uint8)
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    for a in (seq, qual, off):
        a.setflags(write=False)
    planted.reads = reads
    return Draw(k, l_pre, (seq, qual, off), planted)


def cycle_nodes(circ, k):
    """the k-mers round a circular contig, as spelled"""
    lap = circ * (k // len(circ) + 2)
    return [lap[s:s + k] for s in range(len(circ))]
