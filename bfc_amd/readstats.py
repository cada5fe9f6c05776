"""A read set screened against the count table of a `bfc -d` dump on the GPU: per-read k-mer statistics and the longest solid window.

    python -m bfc_amd.readstats [-c INT] [-f FLOAT] [-t] dump.hash [reads|-]

Every FASTA / FASTQ record is answered with one line: its name, a tab, and
"n_kmers n_present n_solid sum min median max streak start end" (tab-separated): the k-mers the record has, how many of them the table
holds, how many it holds at least -c times (solid), the sum, minimum, lower median and maximum of their counts (0 for an absent k-mer),
and the longest run of consecutive solid k-mers -- its length and the bases [start, end) it covers, -1 -1 if there is none; of equally
long runs the last.  With -t the records themselves are written back instead, cut to that window, qualities too, under the rule of
`bfc -1` (correct.c:557): a record is kept if it has a solid k-mer and (streak + k) / length > -f, and dropped otherwise.  That is
`bfc -1` asked of the exact table instead of the Bloom filter: no false positives, and a real coverage threshold.
The dump is restored with bfc_ch_restore and uploaded once; the kernels of bfcg_lookup.hip and bfcg_readstats.hip work on a piece of
the input at a time, 32 bytes per record come back, and the lines are formatted in C.  Any k up to 63 works.  A record of 2^24 bases
or more ends the run with exit status 1.
"""
import getopt
import sys

import numpy as np

from ._fastx import records

USAGE = """Usage: readstats [options] <dump.hash> [reads|-]
Options:
  -c INT     a k-mer is solid if its count is at least INT [3]
  -f FLOAT   with -t: keep a record if (streak + k) / length > FLOAT [0.9]
  -t         write the records back, trimmed to their longest solid window
"""
PIECE = 32 << 20   # positions of sequence per piece


def keep(stats, k, l_seq, min_frac):
    """The window [start, end) of a record with the words `stats` and l_seq bases under correct.c:557, or None if it is dropped.
    min_frac is compared as the float the reference keeps it in (bfc.h:21)."""
    streak = int(stats[5])
    if streak > 0 and (streak + k) / l_seq > float(np.float32(min_frac)):
        return int(stats[6]), int(stats[7])
    return None


def _piece(km, recs, min_cov, min_frac, trim, out):
    from . import api
    if not recs:
        return
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    np.cumsum([len(s) + 1 for _, s, _ in recs], out=off[1:])
    stream = np.frombuffer(b"".join(s + b"\n" for _, s, _ in recs), dtype=np.uint8)
    st = km.read_stats(stream, off, min_cov)
    if not trim:
        lines = api.format_read_stats(st).split(b"\n")
        out.write(b"".join(name + b"\t" + ln + b"\n" for (name, _, _), ln in zip(recs, lines)))
        return
    for (name, s, q), w in zip(recs, st):
        win = keep(w, km.k, len(s), min_frac)
        if win is None:
            continue
        a, e = win
        if q is None:
            out.write(b">" + name + b"\n" + s[a:e] + b"\n")
        else:
            out.write(b"@" + name + b"\n" + s[a:e] + b"\n+\n" + q[a:e] + b"\n")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    try:
        opts, args = getopt.getopt(argv, "c:f:t")
        o = dict(opts)
        min_cov, min_frac = int(o.get("-c", "3")), float(o.get("-f", "0.9"))
    except (getopt.GetoptError, ValueError):
        args = []
    if not args or len(args) > 2:
        sys.stderr.write(USAGE)
        return 1
    from . import api
    tab = api.HostTable.restore(args[0])
    if tab is None:
        return 1
    fn = args[1] if len(args) > 1 else "-"
    f = sys.stdin.buffer if fn == "-" else open(fn, "rb")
    out = sys.stdout.buffer
    km = api.GpuKmers(tab)
    rc = 0
    try:
        recs, n = [], 0
        for rec in records(f):
            recs.append(rec)
            n += len(rec[1]) + 1
            if n >= PIECE:
                _piece(km, recs, min_cov, min_frac, "-t" in o, out)
                recs, n = [], 0
        _piece(km, recs, min_cov, min_frac, "-t" in o, out)
    except api.BfcGpuError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        rc = 1
    out.flush()
    km.close()
    tab.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
