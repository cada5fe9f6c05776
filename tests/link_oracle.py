"""The oracle of the linked unitigs (test_links_host.py, test_gpu_links.py): the edges between the oriented unitigs of
unitig_oracle.unitigs, found on strings with a dict -- it never touches the library's hash --, and a reader of the GFA 1 files that
`python -m bfc_amd.kmergraph -g` writes.  No GPU.

links() asserts, on the oracle alone, what include/bfc_gpu.h states of the edges: every present successor of an oriented unitig's last
k-mer is the first k-mer of exactly one oriented unitig; what each kind of end produces; the mirror rule; the overlap of k - 1 bases; and
    edges = sum over the nodes of (out-degree + in-degree) - 2 x sum over the unitigs of (n_kmers - 1),
every node's every neighbour being either the next node inside its unitig or beyond an end of it."""
from graph_oracle import DictGraph, revcomp


def oriented(seq, o):
    return revcomp(seq) if o else seq


def links(d, rows, min_cnt):
    """the sorted list of (spelling of u, o, c, spelling of v, p) over `rows`, the unitigs of DictGraph d at min_cnt as
    unitig_oracle.unitigs gives them"""
    k = d.k
    head = {}
    for u, r in enumerate(rows):
        for o in (0, 1):
            first = oriented(r[0], o)[:k]
            assert first not in head, "two oriented unitigs start with %r" % first
            head[first] = (u, o)
    out, pairs = [], set()
    for u, (seq, nk, cs, left, right, cyc) in enumerate(rows):
        for o in (0, 1):
            s = oriented(seq, o)
            x, code = s[-k:], (left if o else right)
            found = []
            for c in range(4):
                y = x[1:] + b"ACGT"[c:c + 1]
                v = d.value(y)
                if v >= 0 and (v & 0xff) >= min_cnt:
                    assert y in head, "the successor %r of an end starts no oriented unitig" % y
                    found.append((c, y) + head[y])
            # what each kind of end produces
            if cyc:
                assert code == 0 and [(c, t) for c, y, *t in found] == [(b"ACGT".index(s[k - 1]), [u, o])]
            elif code == 1:
                assert found == []
            elif code == 2:
                assert 2 <= len(found) <= 4
            elif code == 3:
                assert len(found) == 1
            else:
                assert code == 6 and len(found) == 1
                c, y, v, p = found[0]
                assert y in (x, revcomp(x)) and (v, p) == ((u, o) if y == x else (u, 1 - o))
            for c, y, v, p in found:
                t = oriented(rows[v][0], p)
                assert s[-(k - 1):] == t[:k - 1] and t[:k] == y
                out.append((seq, o, c, rows[v][0], p))
                assert (u, o, v, p) not in pairs   # (two bases from one end cannot lead to one k-mer)
                pairs.add((u, o, v, p))
    for u, o, v, p in pairs:   # the mirror; the hairpin's edge is its own and is there once
        assert (v, 1 - p, u, 1 - o) in pairs
    degrees = sum(bin(d.nb(s, min_cnt)).count("1") for s, v in d.d.items() if s <= revcomp(s) and (v & 0xff) >= min_cnt)
    assert len(out) == degrees - 2 * sum(r[1] - 1 for r in rows)
    return sorted(out)


def kmer_edges(d, min_cnt):
    """({the nodes as their smaller strands}, {(x, y): y a present successor of the present oriented k-mer x}) of a DictGraph at min_cnt"""
    nodes, edges = set(), set()
    for x, v in d.d.items():
        if (v & 0xff) < min_cnt:
            continue
        nodes.add(min(x, revcomp(x)))
        for c in b"ACGT":
            y = x[1:] + bytes([c])
            w = d.value(y)
            if w >= 0 and (w & 0xff) >= min_cnt:
                edges.add((x, y))
    return nodes, edges


def dict_of_reads(k, reads, min_cnt=1):
    """a DictGraph straight from reads, without the library: every k-mer with the number of times it occurs (255 at most)"""
    cnt = {}
    for r in reads:
        for i in range(len(r) - k + 1):
            c = min(r[i:i + k], revcomp(r[i:i + k]))
            cnt[c] = min(cnt.get(c, 0) + 1, 255)
    keep = sorted(s for s, v in cnt.items() if v >= min_cnt)
    return DictGraph(k, keep, [cnt[s] for s in keep])


def read_gfa(text, k):
    """A GFA 1 file of kmergraph -g parsed back, every line checked for its form: (segments {id: (seq, KC, km text)}, links
    [(id, o, id, p)], the k-mers of the S lines as smaller strands, the k-mer edges (x, y) -- those inside the segments, on both strands,
    and one per L line, from the last k-mer of the oriented source to the first of the oriented target, which must overlap in k - 1)"""
    lines = text.split(b"\n")
    assert lines[0] == b"H\tVN:Z:1.0" and lines[-1] == b""
    segs, ls, nodes, edges = {}, [], [], set()
    for ln in lines[1:-1]:
        f = ln.split(b"\t")
        if f[0] == b"S":
            assert len(f) == 6 and not ls, ln   # (every segment before the first link)
            sid, seq = int(f[1]), f[2]
            assert sid == len(segs) + 1 and set(seq) <= set(b"ACGT") and len(seq) >= k
            assert f[3] == b"LN:i:%d" % len(seq) and f[4].startswith(b"KC:i:") and f[5].startswith(b"km:f:")
            kc, n = int(f[4][5:]), len(seq) - k + 1
            assert f[5][5:] == b"%.2f" % (kc / n)
            segs[sid] = (seq, kc, f[5][5:])
            for s in (seq, revcomp(seq)):
                edges |= {(s[i:i + k], s[i + 1:i + 1 + k]) for i in range(n - 1)}
            nodes += [min(seq[i:i + k], revcomp(seq[i:i + k])) for i in range(n)]
        else:
            assert f[0] == b"L" and len(f) == 6 and f[2] in (b"+", b"-") and f[4] in (b"+", b"-") and f[5] == b"%dM" % (k - 1), ln
            u, o, v, p = int(f[1]), int(f[2] == b"-"), int(f[3]), int(f[4] == b"-")
            s, t = oriented(segs[u][0], o), oriented(segs[v][0], p)
            assert s[-(k - 1):] == t[:k - 1]
            ls.append((u, o, v, p))
            edges.add((s[-k:], t[:k]))
    assert len(set(nodes)) == len(nodes) and len(set(ls)) == len(ls) and ls == sorted(ls)
    assert [s[0] for s in segs.values()] == sorted(s[0] for s in segs.values())
    return segs, ls, set(nodes), edges
