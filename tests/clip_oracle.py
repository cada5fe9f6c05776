"""The fixture and the oracle of the clipping tests (test_clip_host.py, test_gpu_clip.py).  No GPU.

The fixture is unitig_oracle.fixture(k)'s reads -- genome, bubble, a tip of four k-mers, isolated k-mer, A-run, cycle, two hairpins, a
low-count read -- plus a FORKED TIP, every read of it given three times:
  - G[0:100] + e + X: the genome's first hundred bases, a wrong base e and 12 random bases X;
  - a read that shares that one up to 5 bases into X, then differs in one base and goes on with 3 more random bases.
The k-mers that hold e hang off the genome as a STEM of six (those ending at e and at X[0..4]), which forks into two BRANCHES of seven and
of four k-mers.  The stem is attached at both ends: to the genome on one side, to the fork on the other.  A first round can clip only the
two branches; the stem becomes a tip by that and goes in the second round, after which the genome's first unitig runs through the place.
needs_two_rounds() asserts exactly that on the oracle below.

The oracle takes the dict of an exported table (unitig_oracle.dict_of_table), calls unitig_oracle.unitigs, chooses by the definition of
include/bfc_gpu.h -- a path of at most max_tip k-mers whose counts sum to at most max_mean times their number, one end DEAD (stop code 1
or 6) and the other ATTACHED (2 or 3) for a tip, both DEAD for an island --, deletes both strands' strings and repeats.  It never touches
the library's hash."""
import numpy as np

import graph_oracle
import unitig_oracle
from graph_oracle import DictGraph, revcomp

FORK_AT, SHARED, X_LEN, TAIL = 100, 5, 12, 3
STEM, BRANCHES = SHARED + 1, (X_LEN - SHARED, 1 + TAIL)
DEAD = (1, 6)


class Fixture:
    pass


def fixture(k):
    """the reads as (seq, qual, off), and what the generator knows"""
    base = unitig_oracle.fixture(k)
    rng = np.random.default_rng(11000 + k)
    f = Fixture()
    f.k, f.base, f.genome = k, base, base.base.genome
    other = lambda c: b"ACGT"[(b"ACGT".index(c) + 1 + int(rng.integers(0, 3))) % 4]
    x = unitig_oracle._rand(rng, X_LEN)
    head = f.genome[:FORK_AT] + bytes([other(f.genome[FORK_AT])])
    f.fork_a = head + x
    f.fork_b = head + x[:SHARED] + bytes([other(x[SHARED])]) + unitig_oracle._rand(rng, TAIL)
    f.stem = f.fork_a[FORK_AT + 1 - k:FORK_AT + 1 + SHARED]          # its six k-mers, as one sequence
    reads = [base.seq[int(base.off[i]):int(base.off[i + 1])].tobytes() for i in range(len(base.off) - 1)]
    reads += [r for r in (f.fork_a, f.fork_b) for _ in range(3)]
    f.seq = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    f.qual = np.full(len(f.seq), ord("I"), dtype=np.uint8)
    f.off = np.zeros(len(reads) + 1, dtype=np.uint64)
    f.off[1:] = np.cumsum([len(r) for r in reads])
    f.reads = (f.seq, f.qual, f.off)
    return f


def canon(s):
    return min(s, revcomp(s))


def kmers_of(seq, k):
    """the canonical k-mers of a sequence"""
    return [canon(seq[i:i + k]) for i in range(len(seq) - k + 1)]


def _graph(k, d):
    g = DictGraph.__new__(DictGraph)
    g.k, g.d = k, d
    return g


def clippable(u, max_tip, max_mean, islands):
    """is the unitig u = (seq, n_kmers, cnt_sum, left, right, cycle) removed by a round"""
    seq, n, cs, left, right, cyc = u
    if cyc or n > max_tip or cs > max_mean * n:
        return False
    dead = (left in DEAD) + (right in DEAD)
    return dead == 1 or (dead == 2 and islands)


def clip(d, min_cnt=1, max_tip=None, max_mean=255, islands=False, max_rounds=8):
    """({canonical string: high << 8 | count} of the survivors, [(unitigs removed, k-mers removed, keys left)] per round that removed
    something) of DictGraph d clipped by the definition of include/bfc_gpu.h; d is not changed"""
    k = d.k
    max_tip = 2 * k if max_tip is None else max_tip
    g = _graph(k, {s: v for s, v in d.d.items() if (v & 0xff) >= min_cnt})
    stats = []
    for _ in range(max_rounds):
        gone = [u for u in unitig_oracle.unitigs(g, min_cnt) if clippable(u, max_tip, max_mean, islands)]
        if not gone:
            break
        for seq, n, *_ in gone:
            for i in range(n):
                s = seq[i:i + k]
                del g.d[s], g.d[revcomp(s)]
        stats.append((len(gone), sum(u[1] for u in gone), len(g.d) // 2))
    return {s: v for s, v in g.d.items() if s <= revcomp(s)}, stats


def survivors_of_table(t):
    """{canonical string: high << 8 | count} of a HostTable"""
    return {s: v for s, v in unitig_oracle.dict_of_table(t).d.items() if s <= revcomp(s)}


def unitigs_of(k, surv, min_cnt=1):
    """the oracle's unitigs of a survivor dict"""
    d = dict(surv)
    d.update({revcomp(s): v for s, v in surv.items()})
    return unitig_oracle.unitigs(_graph(k, d), min_cnt)


def needs_two_rounds(d, f, min_cnt, max_tip=12):
    """On the oracle: one round clips the two branches (and the old fixture's tip) and leaves the stem whole, the second takes the stem and
    nothing else, a third finds nothing; before it the genome's first unitig ends at the fork, afterwards it runs to the bubble."""
    k = f.k
    assert max(BRANCHES) <= max_tip and STEM <= max_tip < min(FORK_AT, graph_oracle.TIP_ERR) + 1 - k
    stem = set(kmers_of(f.stem, k))
    assert len(stem) == STEM and all(s in d.d for s in stem)
    one, st1 = clip(d, min_cnt, max_tip, max_rounds=1)
    two, st2 = clip(d, min_cnt, max_tip, max_rounds=2)
    more, st8 = clip(d, min_cnt, max_tip, max_rounds=8)
    assert len(st1) == 1 and st1[0][:2] == (3, sum(BRANCHES) + 4) and stem <= set(one)
    assert st2 == st8 and two == more and len(st2) == 2 and st2[0] == st1[0] and st2[1][:2] == (1, STEM) and set(one) - set(two) == stem
    first = f.genome[:graph_oracle.SUB]
    has = lambda surv, seq: any(u[0] in (seq, revcomp(seq)) for u in unitigs_of(k, surv, min_cnt))
    assert not has(one, first) and has(two, first)
    return st2
