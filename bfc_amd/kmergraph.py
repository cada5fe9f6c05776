"""A `bfc -d` dump read as a de Bruijn graph on the GPU: how many k-mers are dead ends, how many branch, and what lies around a k-mer.

    python -m bfc_amd.kmergraph [-m INT] [-c INT [-i]] [-p INT [-d INT]] [-a INT] [-r INT] [-o FILE] [-t|-b] [-u] [-g FILE] [-x FILE] [-l INT] table.dump

The dump is restored with bfc_ch_restore and uploaded.  A k-mer is PRESENT if the table holds it with count >= INT (-m, default 1); a NODE
is a k-mer of the table with such a count, on the strand the table stores (the one hash2cnt prints); its out-degree o is the number of
bases whose successor is present, its in-degree i that of the predecessors (include/bfc_gpu.h states all of it).  The reference has no
such tool, so the output format is this project's.  Standard output, in this order:

    clip<TAB>round<TAB>unitigs<TAB>kmers<TAB>keys_left
                          under -c INT, first: the graph is cleaned on the GPU (bfcg_kmers_clip; odd k <= 37) and EVERY line below then
                          describes the cleaned table.  A round removes the tips -- unitigs of at most INT k-mers (0: 2 k) with one dead
                          end and one end attached to a branch -- whose mean count is at most -a INT (default 255: any), with -i also the
                          islands (both ends dead); it leaves the k-mers with a count of at least -m that survive.  Rounds repeat until
                          one removes nothing or -r INT (default 8) have run.  One line per round that removed something, rounds from 1:
                          the unitigs and k-mers it removed and the keys it left.  -o FILE writes the cleaned table as a dump
    pop<TAB>round<TAB>bubbles<TAB>kmers<TAB>keys_left
                          under -p INT, after the clip lines: the simple bubbles of the graph are popped on the GPU (bfcg_kmers_pop; odd
                          k <= 37) and every line below describes the table that is left.  A bubble is two unitigs of at most INT k-mers
                          each (0: 2 k), their lengths at most -d INT apart (default 0), between one k-mer with two successors and one
                          with two predecessors; a round removes of each the arm with the lower mean count if that mean is at most -a
                          INT.  Rounds and -r, -o as for -c.  One line per round that removed something: the bubbles it popped, the
                          k-mers it removed, the keys it left.  With -c and -p the tips are clipped first, then the bubbles popped, then
                          the tips clipped once more with the same parameters (popping makes no tip, but the chain is closed): that
                          second clipping's lines follow the pop lines, its rounds numbered on from the first's
    deg<TAB>o<TAB>n0<TAB>n1<TAB>n2<TAB>n3<TAB>n4
                          five lines, o = 0..4: the nodes with out-degree o and in-degree 0..4 (bfcg_kmers_graph_census; k <= 37).  A
                          node stored as its reverse complement has the two degrees swapped; the five lines below count classes that are
                          symmetric in (o, i): cell (o, i) is folded with (i, o), so they mean the same on either strand
    nodes<TAB>N           all of them
    isolated<TAB>N        o = 0 and i = 0
    tips<TAB>N            exactly one of o, i is 0 (dead ends; a tip that also branches is counted under both)
    simple<TAB>N          o = 1 and i = 1
    branching<TAB>N       o >= 2 or i >= 2
    kmer<TAB>count<TAB>high<TAB>successors<TAB>predecessors
                          under -t / -b: the tips / the branching k-mers (bfcg_kmers_list_graph), sub-table by sub-table, with the bases
                          whose successor / predecessor is present ('.' for none)
    seed<TAB>unitig<TAB>left_len<TAB>left_stop<TAB>right_len<TAB>right_stop
                          under -x FILE (one k-mer per line, '>' lines and empty lines skipped; every k up to 63): the unambiguous
                          sequence around each k-mer, walked both ways for at most INT bases (-l, default 10000) by bfcg_kmers_extend --
                          to the left as the same walk on the reverse complement.  Stop codes: 0 the limit, 1 no next k-mer, 2 several,
                          3 the next one has another way in, 4 the seed is absent, 5 back at the seed
    unitigs<TAB>N, cycles<TAB>N, n50<TAB>N
                          under -u (odd k <= 37), after the census lines: the compacted graph (bfcg_kmers_unitigs) -- its unitigs, how many
                          of them are cycles, and the N50 of their lengths in bases; then one line per unitig, sorted by sequence:
    unitig<TAB>seq<TAB>n_kmers<TAB>mean_count<TAB>left_stop<TAB>right_stop<TAB>circular
                          mean_count with two decimals; the stop codes of the two ends are 1, 2, 3 as above and 6, the only way on
                          leads back into the node itself (its own k-mer or its reverse complement); a cycle has 0 0 1 and repeats its
                          first k - 1 bases at the end
    links<TAB>N
                          under -g FILE (odd k <= 37), after the n50 line -- the three lines unitigs, cycles, n50 are printed under -g
                          also without -u, the unitig lines only under -u: the edges of the compacted graph (bfcg_kmers_unitig_graph,
                          the unitigs and their edges out of one call), which FILE then holds as GFA 1:
                              H<TAB>VN:Z:1.0
                              S<TAB>id<TAB>seq<TAB>LN:i:bases<TAB>KC:i:cnt_sum<TAB>km:f:mean_count
                              L<TAB>id<TAB>+|-<TAB>id<TAB>+|-<TAB>(k-1)M
                          The segments are named 1..n in the order of the unitig lines (sorted by sequence); a cycle's segment keeps
                          its k + n - 1 bases.  One L line per edge, sorted by (id, strand, id, strand), + before -: from the last
                          k-mer of the first segment read on that strand to the first k-mer of the second, which overlap in k - 1
                          bases.  Every edge is there with its mirror (a - b + for a + b -), a hairpin's, which is its own, once; a
                          cycle links to itself on both strands.  With -c / -p the file describes the cleaned table.  A FILE that
                          cannot be written is an error, exit status 1
"""
import ctypes as C
import getopt
import sys

import numpy as np

USAGE = """Usage: kmergraph [options] <table.dump>
Options:
  -m INT   a k-mer is present with occ >= INT [1]
  -c INT   clip tips of at most INT k-mers first (0: 2k); all output describes the cleaned table (odd k <= 37)
  -p INT   pop simple bubbles with arms of at most INT k-mers (0: 2k), after -c; all output describes the table left (odd k <= 37)
  -d INT   the arms of a bubble differ by at most INT k-mers [0] (with -p)
  -a INT   clip / pop only unitigs whose mean count is at most INT [255]
  -i       clip islands too (with -c)
  -r INT   at most INT rounds of clipping, of popping [8]
  -o FILE  write the cleaned table as a dump (with -c or -p)
  -t       list the tips
  -b       list the branching k-mers
  -u       list the unitigs of the compacted graph (odd k <= 37)
  -g FILE  write the compacted graph with its edges as GFA 1 (odd k <= 37)
  -x FILE  extend the k-mers of FILE both ways and print the unitig around each
  -l INT   at most INT bases each way [10000]
"""

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _atoi(s):
    try:
        return int(s)
    except ValueError:
        return 0


def summary(deg):
    """(nodes, isolated, tips, simple, branching) of a (5, 5) census"""
    from .api import GRAPH_MASKS
    flat = [int(v) for v in np.asarray(deg).reshape(25)]
    pick = lambda name: sum(v for b, v in enumerate(flat) if GRAPH_MASKS[name] >> b & 1)
    return sum(flat), pick("isolated"), pick("tips"), pick("simple"), pick("branching")


def _extend_file(api, km, fn, min_cnt, max_len, out):
    text = open(fn, "rb").read()
    y, bad = np.zeros((text.count(b"\n") + 1, 2), dtype=np.uint64), C.c_uint64()
    n = km.L.bfcg_kmers_parse(km.k, text, len(text), y.ctypes.data, len(y), C.byref(bad))
    if bad.value:
        sys.stderr.write("ERROR: line %d of %s is not a %d-mer of ACGT\n" % (bad.value, fn, km.k))
        return 1
    y = y[:n]
    rb, rl, rs = km.extend(y, min_cnt, max_len)
    lb, ll, ls = km.extend(api.kmer_revcomp(km.k, y), min_cnt, max_len)
    for i, seed in enumerate(km.strings(y)):
        left = lb[i, :ll[i]].tobytes().translate(_COMP)[::-1]
        out.write(b"%s\t%s\t%d\t%d\t%d\t%d\n" % (seed.encode(), left + seed.encode() + rb[i, :rl[i]].tobytes(), ll[i], ls[i], rl[i], rs[i]))
    return 0


def n50(lengths):
    """the length L such that unitigs of at least L bases hold half of all bases"""
    total, run = sum(lengths), 0
    for v in sorted(lengths, reverse=True):
        run += v
        if 2 * run >= total:
            return v
    return 0


def gfa(k, seq, off, n_kmers, cnt_sum, links):
    """(the GFA 1 text, the number of L lines) of unitig_graph()'s arrays: segments 1..n in unitig_rows()'s order"""
    s = np.asarray(seq, dtype=np.uint8).tobytes()
    name = [s[int(off[u]):int(off[u + 1])] for u in range(len(n_kmers))]
    sid = [0] * len(name)
    for rank, u in enumerate(sorted(range(len(name)), key=name.__getitem__)):
        sid[u] = rank + 1
    segs = sorted((sid[u], name[u], int(cnt_sum[u]), int(cnt_sum[u]) / int(n_kmers[u])) for u in range(len(name)))
    links = np.asarray(links, dtype=np.int64).reshape(-1, 2, 4)
    edges = sorted((sid[u], int(o), sid[int(links[u, o, c]) >> 1], int(links[u, o, c]) & 1) for u, o, c in zip(*np.nonzero(links >= 0)))
    text = b"H\tVN:Z:1.0\n" + b"".join(b"S\t%d\t%s\tLN:i:%d\tKC:i:%d\tkm:f:%.2f\n" % (i, q, len(q), cs, mean) for i, q, cs, mean in segs)
    return text + b"".join(b"L\t%d\t%s\t%d\t%s\t%dM\n" % (u, b"+-"[o:o + 1], v, b"+-"[p:p + 1], k - 1) for u, o, v, p in edges), len(edges)


def _unitig_lines(rows, out, n_links=None, listed=True):
    out.write(b"unitigs\t%d\ncycles\t%d\nn50\t%d\n" % (len(rows), sum(r[5] for r in rows), n50([len(r[0]) for r in rows])))
    if n_links is not None:
        out.write(b"links\t%d\n" % n_links)
    if listed:
        out.write(b"".join(b"unitig\t%s\t%d\t%.2f\t%d\t%d\t%d\n" % (s, nk, cs / nk, left, right, cyc) for s, nk, cs, left, right, cyc in rows))


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    try:
        opts, args = getopt.getopt(argv, "tbuim:x:l:c:a:r:o:p:d:g:")
    except getopt.GetoptError:
        opts, args = [], []
    o = dict(opts)
    modes = [f for f in ("-t", "-b") if f in o]
    cleans = "-c" in o or "-p" in o
    if len(args) != 1 or len(modes) > 1 or (not cleans and any(f in o for f in ("-a", "-r", "-o"))) or ("-i" in o and "-c" not in o) or ("-d" in o and "-p" not in o):
        sys.stderr.write(USAGE)
        return 1
    from . import api
    t = api.HostTable.restore(args[0])
    if t is None:
        return 1
    min_cnt, max_len = _atoi(o.get("-m", "1")), _atoi(o.get("-l", "10000"))
    out = sys.stdout.buffer
    km = api.GpuKmers(t)
    rc = 0
    try:
        if cleans:   # (refused, like -u, before any output)
            max_mean, max_rounds, clipped = _atoi(o.get("-a", "255")), _atoi(o.get("-r", "8")), 0
            steps = ["clip", "pop", "clip"] if "-c" in o and "-p" in o else ["clip"] if "-c" in o else ["pop"]
            for step in steps:
                if step == "clip":
                    clean, stats = km.clip(min_cnt, _atoi(o["-c"]) or None, max_mean, "-i" in o, max_rounds)
                else:
                    clean, stats = km.pop_bubbles(min_cnt, _atoi(o["-p"]) or None, _atoi(o.get("-d", "0")), max_mean, max_rounds)
                km.close()
                km = clean
                first = clipped if step == "clip" else 0
                out.write(b"".join(b"%s\t%d\t%d\t%d\t%d\n" % (step.encode(), first + i + 1, r[0], r[1], r[2]) for i, r in enumerate(stats)))
                clipped += len(stats) if step == "clip" else 0
            if "-o" in o:
                h = km.to_host()
                failed = h.dump(o["-o"]) != 0
                h.close()
                if failed:
                    raise api.BfcGpuError("cannot write %s" % o["-o"])
        rows = n_links = None
        if "-g" in o:   # (the unitigs and their edges out of one call: a second call need not number the unitigs alike)
            g = km.unitig_graph(min_cnt)
            rows = api.unitig_rows(*g[:5])
            text, n_links = gfa(t.k, g[0], g[1], g[2], g[3], g[5])
            try:
                with open(o["-g"], "wb") as fh:
                    fh.write(text)
            except OSError:
                raise api.BfcGpuError("cannot write %s" % o["-g"])
        elif "-u" in o:
            rows = api.unitig_rows(*km.unitigs(min_cnt))   # (an even k or k > 37 is refused here, before any output)
        if t.k <= 37 or "-x" not in o:   # (k > 37 with -x alone: the walks need no decode)
            deg = km.graph_census(min_cnt)
            out.write("".join("deg\t%d\t%s\n" % (i, "\t".join(str(int(v)) for v in deg[i])) for i in range(5)).encode())
            out.write(b"nodes\t%d\nisolated\t%d\ntips\t%d\nsimple\t%d\nbranching\t%d\n" % summary(deg))
        if rows is not None:
            _unitig_lines(rows, out, n_links, "-u" in o)
        if modes:
            mask = api.GRAPH_MASKS["tips" if modes[0] == "-t" else "branching"]
            for y, ch, nb in km.pieces_graph(min_cnt, mask):
                lines = km.format(y, ch).split(b"\n")[:-1]
                out.write(b"".join(ln + b"\t" + api.nb_text(v).encode() + b"\n" for ln, v in zip(lines, nb)))
        if "-x" in o:
            rc = _extend_file(api, km, o["-x"], min_cnt, max_len, out)
    except api.BfcGpuError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        rc = 1
    out.flush()
    km.close()
    t.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
