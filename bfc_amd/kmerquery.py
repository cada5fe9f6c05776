"""The count table of a `bfc -d` dump asked by k-mer on the GPU: what was counted for these k-mers, or under this sequence?

    python -m bfc_amd.kmerquery [-p] dump.hash [queries|-]

Without -p the queries are one k-mer per line (the first field up to a tab or space; '>' lines and empty lines are skipped) on either
strand, and every k-mer is answered with hash2cnt's line, "%s\\t%d\\t%d\\n": the k-mer as given, its count and its high-quality count,
0 and 0 for a k-mer the table does not hold.  A line that is not k bases of ACGT ends the run with exit status 1 and its number.
With -p the queries are FASTA / FASTQ records and every record is answered with ">name" and one line of space-separated counts, one per
base, for the k-mer ENDING there: '.' where none ends (the first k - 1 bases, a window with an N), 0 for an absent k-mer.
The dump is restored with bfc_ch_restore and uploaded once; the kernels of bfcg_lookup.hip probe it, a piece of the input at a time, and
the lines are formatted in C.  Any k up to 63 works: a lookup needs the forward hash only.
"""
import ctypes as C
import getopt
import sys

import numpy as np

from ._fastx import records

USAGE = """Usage: kmerquery [options] <dump.hash> [queries|-]
Options:
  -p       queries are FASTA/FASTQ: print the count under every base of each record
"""
PIECE = 32 << 20   # bytes of query text, or positions of sequence, per piece


def _lookup_lines(km, f, out):
    line0 = 0
    while True:
        lines = f.readlines(PIECE)
        if not lines:
            return 0
        text = b"".join(lines)
        y, bad = np.empty((len(lines), 2), dtype=np.uint64), C.c_uint64()
        n = km.L.bfcg_kmers_parse(km.k, text, len(text), y.ctypes.data, len(lines), C.byref(bad))
        if bad.value:
            sys.stderr.write("ERROR: line %d is not a %d-mer of ACGT\n" % (line0 + bad.value, km.k))
            return 1
        occ = km.lookup(y[:n])
        buf = C.create_string_buffer(len(text) + 8 * n + 16)
        m = km.L.bfcg_lookup_format(text, len(text), occ.ctypes.data, n, buf)
        out.write(buf.raw[:m])
        line0 += len(lines)


def _profile_piece(km, recs, out):
    if not recs:
        return
    stream = np.frombuffer(b"".join(s + b"\n" for _, s in recs), dtype=np.uint8)
    occ = km.profile(stream)
    buf = C.create_string_buffer(4 * max(len(s) for _, s in recs) + 2)
    p = 0
    for name, s in recs:
        out.write(b">" + name + b"\n")
        m = km.L.bfcg_profile_format(occ[p:p + len(s)].ctypes.data, len(s), buf)
        out.write(buf.raw[:m])
        p += len(s) + 1


def _profile_records(km, f, out):
    recs, n = [], 0
    for name, seq, _ in records(f):
        recs.append((name, seq))
        n += len(seq) + 1
        if n >= PIECE:
            _profile_piece(km, recs, out)
            recs, n = [], 0
    _profile_piece(km, recs, out)
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    try:
        opts, args = getopt.getopt(argv, "p")
    except getopt.GetoptError:
        opts, args = [], []
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
    rc = (_profile_records if ("-p", "") in opts else _lookup_lines)(km, f, out)
    out.flush()
    km.close()
    tab.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
