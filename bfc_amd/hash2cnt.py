"""The reference's hash2cnt on the GPU: k-mers with their counts, sub-table sizes and the spectrum of a `bfc -d` dump.

    python -m bfc_amd.hash2cnt [-s] [-h] [-m INT] [-d INT] dump.hash

Flags and line formats are hash2cnt.c's: "%s\\t%d\\t%d\\n" per k-mer (k-mer, count, high-quality count), "%d\\n" per sub-table under -s,
the 256 histogram lines under -h.  The dump is restored with bfc_ch_restore and uploaded once; the kernels of bfcg_kmers.hip read it out
and the lines are formatted in C, a piece of the table at a time.  K-mers come out sub-table by sub-table as in the reference, in
another order inside a sub-table (the reference's is its hash buckets').  A listing needs k <= 37 (hash2cnt.c:37); -s and -h work for any k.
"""
import ctypes as C
import getopt
import sys

USAGE = """Usage: hash2cnt [options] <dump.hash>
Options:
  -s       only show # elements in each sub- hash table
  -h       only show k-mer histogram
  -m INT   occ >= INT [0]
  -d INT   occ - occHigh >= INT [0]
"""


def _atoi(s):
    try:
        return int(s)
    except ValueError:
        return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    try:
        opts, args = getopt.getopt(argv, "shm:d:")
    except getopt.GetoptError:
        opts, args = [], []
    o = dict(opts)
    sub_only, hist_only = "-s" in o, "-h" in o
    min_cnt, min_diff = _atoi(o.get("-m", "0")), _atoi(o.get("-d", "0"))
    if not args:
        sys.stderr.write(USAGE)
        return 1
    from . import api
    tab = api.HostTable.restore(args[0])
    if tab is None:
        return 1
    listing = not sub_only and not hist_only
    if listing and tab.k > 37:
        sys.stderr.write("ERROR: hash2cnt does not work for k>37\n")
        return 1
    out = sys.stdout.buffer
    km = api.GpuKmers(tab)
    if sub_only or hist_only:  # both come from one pass over the table
        _, cnt, high, sizes = km.hist_sizes()
    if sub_only:
        buf = C.create_string_buffer(11 * len(sizes))
        n = km.L.bfcg_kmers_format_sizes(sizes.ctypes.data, len(sizes), buf)
        out.write(buf.raw[:n])
    if listing:
        for y, ch in km.pieces(min_cnt, min_diff):
            out.write(km.format(y, ch))
    if hist_only:
        out.write("".join("%d\t%d\n" % (i, cnt[i]) if i >= 64 else "%d\t%d\t%d\n" % (i, cnt[i], high[i]) for i in range(256)).encode())
    out.flush()
    km.close()
    tab.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
