"""The fixture and the oracle of the bubble-popping tests (test_pop_host.py, test_gpu_pop.py).  No GPU.

The fixture is, for odd k, graph_oracle.fixture(k)'s reads -- whose genome and variant, three times each, are a bubble of two arms with
equal counts: the TIE case -- plus a second random genome H of 850 bases in two reads of 450 that overlap by 50, A = H[0:450] and
B = H[400:850], each given five times, and whole-read variants of them (every read at least twice: the counter keeps a k-mer from its
second occurrence on):
  - NESTED, with d = k // 2 + 1: A with substitutions at X and X + d, four times, and A with one substitution at X + d // 2, three times.
    Every k-mer over X + d // 2 lies over X or X + d as well (d < k), so the inner bubble -- k k-mers a side -- lies inside the reference
    side of the outer one, whose other arm has k + d k-mers.  Round 1 pops the inner bubble, round 2 the outer one;
  - INTERLOCKED: A with a substitution at Z and, as another read, A with one at Z + k // 2, three times each.  The arm of either is beside
    a reference path that the other cuts: never popped;
  - INDEL: B without its bases Y and Y + 1, three times: arms of k + 1 and k - 1 k-mers, popped only with max_diff >= 2;
  - THREE-WAY: B with one substitution at W and B with another one at W, three and four times: three branches, never popped;
  - INVERTED: the read P + M + revcomp(P) with |P| = 3 k and M = "A" + k + 3 random bases + "C", three times.  The 2 k + 4 k-mers that
    hold a base of M are one unitig with code 3 on both ends whose sibling under the entry is itself read backwards: never popped.
No k-mer over a site of one case lies over a site of another, over the reads' overlap or at a read's end (asserted for k <= 37), so the
cases do not interact.  The draw is repeated with the next seed until no k-mer of H, its variants and the inverted read occurs twice, on either strand, or in
graph_oracle's reads; needs_two_rounds() asserts what is said above on the oracle below, for the counts the library gave.

The oracle takes the dict of an exported table (unitig_oracle.dict_of_table), calls unitig_oracle.unitigs per round, takes the unitigs
with ends (3, 3), finds entry, exit and sibling by slicing strings, applies the definition of include/bfc_gpu.h -- two successors of the
entry, two predecessors of the exit, the sibling not the arm read backwards, the sibling's unitig an arm with the same exit, both at most
max_arm k-mers and at most max_diff apart, the loser the arm with the lower mean count or, on a tie, the one whose emitted spelling starts
with the larger k-mer, removed if its mean is at most max_mean -- and deletes both strands' strings.  It never touches the library's
hash."""
import functools

import numpy as np

import graph_oracle
import unitig_oracle
from clip_oracle import _graph, canon, kmers_of, survivors_of_table, unitigs_of  # noqa: F401 (the tests take them from here)
from graph_oracle import revcomp

H_LEN, READ, OVERLAP = 850, 450, 50
X, Z, Y, W = 120, 300, 560, 720        # nested and interlocked in A, indel and three-way in B (positions in H)
N_REF, N_HAP1, N_HAP2, N_DEL = 5, 4, 3, 3


class Fixture:
    pass


def _sub(rng, seq, at, avoid=()):
    """seq with another base at `at`, none of `avoid`"""
    while True:
        c = b"ACGT"[(b"ACGT".index(seq[at]) + 1 + int(rng.integers(0, 3))) % 4]
        if c not in avoid:
            return seq[:at] + bytes([c]) + seq[at + 1:], c


def _draw(k, seed, taken):
    rng = np.random.default_rng(seed)
    f = Fixture()
    f.k, f.d = k, k // 2 + 1
    h = unitig_oracle._rand(rng, H_LEN)
    f.h, f.a, f.b = h, h[:READ], h[READ - OVERLAP:]
    f.hap1 = _sub(rng, _sub(rng, f.a, X)[0], X + f.d)[0]
    f.hap2 = _sub(rng, f.a, X + f.d // 2)[0]
    f.inter = [_sub(rng, f.a, Z)[0], _sub(rng, f.a, Z + k // 2)[0]]
    y = Y - (READ - OVERLAP)
    f.deleted = f.b[:y] + f.b[y + 2:]
    w = W - (READ - OVERLAP)
    three1, c1 = _sub(rng, f.b, w)
    f.three = [three1, _sub(rng, f.b, w, avoid=(c1,))[0]]
    p = unitig_oracle._rand(rng, 3 * k)
    f.inv_mid = b"A" + unitig_oracle._rand(rng, k + 3) + b"C"
    f.inverted = p + f.inv_mid + revcomp(p)
    f.inv_unitig = f.inverted[2 * k + 1:5 * k + 4]      # the last k - 1 bases of P, M, the first k - 1 of revcomp(P): 2 k + 4 k-mers
    # every k-mer of the construction once: H, the variants' own k-mers, the inverted read's first half and middle
    own = kmers_of(h, k)
    for ref, var in [(f.a, f.hap1), (f.a, f.hap2), (f.a, f.inter[0]), (f.a, f.inter[1]), (f.b, f.deleted), (f.b, f.three[0]), (f.b, f.three[1])]:
        have = set(kmers_of(ref, k))
        own += [s for s in kmers_of(var, k) if s not in have]
    own += kmers_of((p + f.inv_mid + revcomp(p)[:k - 1]), k)
    f.clean = len(set(own)) == len(own) and not taken & set(own) and h[Y + 2] != h[Y] and h[Y - 1] != h[Y + 1]
    f.more = [f.a] * N_REF + [f.b] * N_REF + [f.hap1] * N_HAP1 + [f.hap2] * N_HAP2 + f.inter * 3 + [f.deleted] * N_DEL + [f.three[0]] * 3 + [f.three[1]] * 4 + [f.inverted] * 3
    return f


@functools.lru_cache(maxsize=None)
def fixture(k):
    """the reads as (seq, qual, off), and what the generator knows"""
    assert k % 2 == 1 and k < X and X + k // 2 + 1 + 2 * k < Z and Z + k // 2 + k < READ - OVERLAP and READ + k < Y and Y + 2 + 2 * k < W and W + k < H_LEN
    base = graph_oracle.fixture(k)
    reads = [base.seq[int(base.off[i]):int(base.off[i + 1])].tobytes() for i in range(len(base.off) - 1)]
    taken = set(s for r in reads for s in kmers_of(r, k))
    for seed in range(13000 + 1000 * k, 13000 + 1000 * k + 1000):
        f = _draw(k, seed, taken)
        if f.clean:
            break
    assert f.clean, "no clean draw of the bubble fixture for k=%d" % k
    f.base, f.seed = base, seed
    reads += f.more
    f.seq = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    f.qual = np.full(len(f.seq), ord("I"), dtype=np.uint8)
    f.off = np.zeros(len(reads) + 1, dtype=np.uint64)
    f.off[1:] = np.cumsum([len(r) for r in reads])
    f.reads = (f.seq, f.qual, f.off)
    # the arms as the generator knows them, as lists of canonical k-mers
    own = lambda ref, var: [s for s in kmers_of(var, k) if s not in set(kmers_of(ref, k))]
    sub = graph_oracle.SUB
    f.tie = [kmers_of(g[sub - k + 1:sub + k], k) for g in (base.genome, base.variant)]
    f.inner, f.outer = own(f.a, f.hap2), own(f.a, f.hap1)
    f.inner_ref, f.outer_ref = kmers_of(f.a[X + f.d // 2 - k + 1:X + f.d // 2 + k], k), kmers_of(f.a[X - k + 1:X + f.d + k], k)
    f.del_arm, f.del_ref = own(f.b, f.deleted), own(f.deleted, f.b)
    f.never = own(f.a, f.inter[0]) + own(f.a, f.inter[1]) + own(f.b, f.three[0]) + own(f.b, f.three[1]) + kmers_of(f.inv_unitig, k)
    f.never += kmers_of(f.a[Z - k + 1:Z + k // 2 + k], k) + kmers_of(f.b[W - (READ - OVERLAP) - k + 1:W - (READ - OVERLAP) + k], k)
    return f


def _arms(g, min_cnt):
    """{oriented first k-mer: (unitig index, first, last, n_kmers, cnt_sum, entry, exit, emitted first k-mer)} of the unitigs with ends
    (3, 3), each under both of its orientations; entry and exit are asserted to be unique"""
    k, out = g.k, {}
    for i, (seq, n, cs, left, right, cyc) in enumerate(unitig_oracle.unitigs(g, min_cnt)):
        if cyc or (left, right) != (3, 3):
            continue
        s, e = seq[:k], seq[-k:]
        pred = [bytes([c]) + s[:-1] for c in b"ACGT" if bytes([c]) + s[:-1] in g.d]
        succ = [e[1:] + bytes([c]) for c in b"ACGT" if e[1:] + bytes([c]) in g.d]
        assert len(pred) == 1 and len(succ) == 1
        p, q = pred[0], succ[0]
        out[s] = (i, s, e, n, cs, p, q, s)
        out[revcomp(e)] = (i, revcomp(e), revcomp(s), n, cs, revcomp(q), revcomp(p), s)
    return out


def _losers(g, min_cnt, max_arm, max_diff, max_mean):
    """the arms a round removes, as lists of their oriented k-mers"""
    k, arms, gone = g.k, _arms(g, min_cnt), []
    for key, (i, s, e, n, cs, p, q, first) in arms.items():
        if key != first:
            continue                                        # every arm once, in its emitted orientation
        succ = [p[1:] + bytes([c]) for c in b"ACGT" if p[1:] + bytes([c]) in g.d]
        pred = [bytes([c]) + q[:-1] for c in b"ACGT" if bytes([c]) + q[:-1] in g.d]
        assert s in succ and e in pred
        if len(succ) != 2 or len(pred) != 2:
            continue
        sib = succ[0] if succ[1] == s else succ[1]
        if sib == revcomp(e) or sib not in arms:
            continue
        j, s2, e2, n2, cs2, p2, q2, first2 = arms[sib]
        assert j != i and p2 == p
        if q2 != q:
            continue
        assert sorted(pred) == sorted([e, e2])
        if n > max_arm or n2 > max_arm or abs(n - n2) > max_diff:
            continue
        loses = cs * n2 < cs2 * n or (cs * n2 == cs2 * n and first > first2)
        if loses and cs <= max_mean * n:
            gone.append(_walk(g, s, n, min_cnt))
    return gone


def _walk(g, s, n, min_cnt):
    path = [s]
    while len(path) < n:
        path.append(unitig_oracle.link(g, path[-1], min_cnt)[0])
    return path


def pop(d, min_cnt=1, max_arm=None, max_diff=0, max_mean=255, max_rounds=8):
    """({canonical string: high << 8 | count} of the survivors, [(bubbles popped, k-mers removed, keys left)] per round that removed
    something) of DictGraph d with its simple bubbles popped by the definition of include/bfc_gpu.h; d is not changed"""
    k = d.k
    max_arm = 2 * k if max_arm is None else max_arm
    g = _graph(k, {s: v for s, v in d.d.items() if (v & 0xff) >= min_cnt})
    stats = []
    for _ in range(max_rounds):
        gone = _losers(g, min_cnt, max_arm, max_diff, max_mean)
        if not gone:
            break
        nodes = [canon(s) for path in gone for s in path]
        assert len(set(nodes)) == len(nodes)             # removed arms are disjoint
        for s in nodes:
            del g.d[s], g.d[revcomp(s)]
        stats.append((len(gone), len(nodes), len(g.d) // 2))
    return {s: v for s, v in g.d.items() if s <= revcomp(s)}, stats


def counts(d, arm):
    """the counts d holds for a list of k-mers"""
    return [d.value(s) & 0xff for s in arm]


def needs_two_rounds(d, f, min_cnt=1):
    """On the oracle alone, for the counts d holds: round 1 at the defaults pops one arm of graph_oracle's bubble and the inner bubble
    (k k-mers each) and leaves the outer arm, round 2 pops the outer arm (k + d k-mers), a third finds nothing; the indel follows
    max_diff; interlocked, three-way and inverted stay whatever max_arm and max_diff are.  Returns the defaults' stats.  (Whether
    graph_oracle's bubble is a tie for these counts is counts()'s to say: at k = 11 the counter's filter adds one to a count here and
    there)"""
    k = f.k
    cnt = lambda arm: counts(d, arm)
    assert all(len(a) == k and all(s in d.d for s in a) for a in f.tie + [f.inner, f.inner_ref])
    assert (len(f.outer), len(f.del_arm), len(f.del_ref)) == (k + f.d, k - 1, k + 1)
    assert max(cnt(f.inner)) < min(cnt(f.inner_ref)) and max(cnt(f.outer)) < min(cnt(f.outer_ref)) and max(cnt(f.del_arm)) < min(cnt(f.del_ref))
    rows = {u[0]: u for u in unitig_oracle.unitigs(d, min_cnt)}
    inv = rows.get(f.inv_unitig)
    assert inv is not None and inv[1:] == (2 * k + 4, sum(cnt(kmers_of(f.inv_unitig, k))), 3, 3, 0)
    one, st1 = pop(d, min_cnt, max_rounds=1)
    two, st2 = pop(d, min_cnt, max_rounds=2)
    more, st8 = pop(d, min_cnt, max_rounds=8)
    tie_gone = [a for a in f.tie if not set(a) & set(one)]
    assert len(tie_gone) == 1 and all(set(a) <= set(one) or a in tie_gone for a in f.tie)
    assert len(st1) == 1 and st1[0][:2] == (2, 2 * k) and not set(f.inner) & set(one) and set(f.outer) <= set(one)
    assert st2 == st8 and two == more and len(st2) == 2 and st2[0] == st1[0] and st2[1][:2] == (1, k + f.d) and set(one) - set(two) == set(f.outer)
    assert set(f.del_arm) <= set(more) and set(f.del_arm) <= set(pop(d, min_cnt, max_diff=1)[0])
    wide, st_wide = pop(d, min_cnt, max_diff=2)
    assert not set(f.del_arm) & set(wide) and set(f.del_ref) <= set(wide) and [r[:2] for r in st_wide] == [(3, 3 * k - 1), (1, k + f.d)]
    all_in, st_all = pop(d, min_cnt, max_arm=65535, max_diff=65535)
    assert set(f.never) <= set(all_in) and all_in == wide and st_all == st_wide
    return st2
