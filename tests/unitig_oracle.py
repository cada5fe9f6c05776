"""The fixture and the oracle of the unitig tests (test_unitig_host.py, test_gpu_unitigs.py).  No GPU.

The fixture is graph_oracle.fixture(k)'s reads -- genome, bubble, tip, isolated k-mer, A-run -- plus, for odd k:
  - a circular contig: a random sequence of CIRC bases, doubled and cut into reads of 100 every 25 (a cycle of CIRC k-mers);
  - a hairpin: a read u + P + comp(u) of k + 1 bases, u one base and P a reverse palindrome of k - 1 bases that no other read shares.  Its
    two k-mers u P and P comp(u) are reverse complements of each other: one node, whose only successor on that side is itself reversed
    (stop code 6) and which has nothing on the other side (stop code 1);
  - a path that ends in a hairpin node: a second hairpin with its own P, preceded by 40 random bases (a unitig of 41 k-mers, ends 1 and 6);
  - a low-count read: k + 3 random bases given TWICE, so that its four k-mers reach the table with a count of 1 (the counter keeps a k-mer
    from its second occurrence on, so a read given once would leave nothing): a unitig at min_cnt 1, absent at 2.
Every other read is given three times, as in graph_oracle.

The oracle is DictGraph (graph_oracle.py: a dict over both strands' strings of an exported table, neighbours by slicing) plus the link rule
and the component walk of include/bfc_gpu.h, on strings.  It never touches the library's hash."""
import numpy as np

import graph_oracle
from graph_oracle import DictGraph, revcomp, strs_of_planes

CIRC = 200


class Fixture:
    pass


def _rand(rng, n):
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, n))


def _hairpin(rng, k):
    half = _rand(rng, (k - 1) // 2)
    u = _rand(rng, 1)
    return u + half + revcomp(half) + u.translate(graph_oracle.COMP)


def fixture(k):
    """the reads as (seq, qual, off), and what the generator knows"""
    assert k % 2 == 1
    base = graph_oracle.fixture(k)
    rng = np.random.default_rng(9000 + k)
    f = Fixture()
    f.k, f.base = k, base
    reads = [base.seq[int(base.off[i]):int(base.off[i + 1])].tobytes() for i in range(len(base.off) - 1)]
    f.circ = _rand(rng, CIRC)
    f.hairpin = _hairpin(rng, k)
    f.hairpin_path = _rand(rng, 40) + _hairpin(rng, k)
    f.low = _rand(rng, k + 3)
    more = [(f.circ + f.circ)[s:s + 100] for s in range(0, 2 * CIRC - 100 + 1, 25)] + [f.hairpin, f.hairpin_path]
    reads += [r for r in more for _ in range(3)] + [f.low, f.low]
    f.seq = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    f.qual = np.full(len(f.seq), ord("I"), dtype=np.uint8)
    f.off = np.zeros(len(reads) + 1, dtype=np.uint64)
    f.off[1:] = np.cumsum([len(r) for r in reads])
    f.reads = (f.seq, f.qual, f.off)
    return f


def dict_of_table(t):
    """DictGraph of a HostTable (odd k <= 37), from the decoded slots of its export"""
    y, nb = t.graph_nb(1)
    ch = (t.export_sorted()[1] & np.uint64(0x3fff)).astype(np.uint16)
    return DictGraph(t.k, strs_of_planes(y, t.k), ch)


def link(d, s, min_cnt):
    """(y, 0) if link(s) = y, else (None, stop code): the rules of include/bfc_gpu.h in their order"""
    o = d.nb(s, min_cnt) & 15
    if o == 0:
        return None, 1
    if o & (o - 1):
        return None, 2
    y = s[1:] + bytes([b"ACGT"[o.bit_length() - 1]])
    i = d.nb(y, min_cnt) >> 4
    if i & (i - 1):
        return None, 3
    if y == s or y == revcomp(s):
        return None, 6
    return y, 0


def _cnt(d, s):
    return d.value(s) & 0xff


def unitigs(d, min_cnt):
    """the sorted list of (seq, n_kmers, cnt_sum, left stop, right stop, cycle) of the graph at min_cnt"""
    nodes = sorted(set(min(s, revcomp(s)) for s, v in d.d.items() if (v & 0xff) >= min_cnt))
    seen, out = set(), []
    for x in nodes:
        if x in seen:
            continue
        # to the left end: to the right from rc(x), until a side is open or the walk is back
        cur, cyc = revcomp(x), False
        while True:
            y, code = link(d, cur, min_cnt)
            if y is None:
                break
            if y == revcomp(x):
                cyc = True
                break
            cur = y
        if cyc:
            lap = [x]
            while True:
                y, code = link(d, lap[-1], min_cnt)
                assert code == 0
                if y == x:
                    break
                lap.append(y)
            s = min(lap + [revcomp(v) for v in lap])
            path, left, right = [s], 0, 0
            while len(path) < len(lap):
                path.append(link(d, path[-1], min_cnt)[0])
            assert link(d, path[-1], min_cnt)[0] == s
        else:
            s = revcomp(cur)
            path, left = [s], code
            while True:
                y, right = link(d, path[-1], min_cnt)
                if y is None:
                    break
                path.append(y)
            other = revcomp(path[-1])
            assert other != s
            if other < s:
                path, left, right = [revcomp(v) for v in reversed(path)], right, left
        for v in path:
            c = min(v, revcomp(v))
            assert c not in seen
            seen.add(c)
        out.append((path[0] + b"".join(v[-1:] for v in path[1:]), len(path), sum(_cnt(d, v) for v in path), left, right, int(cyc)))
    return sorted(out)
