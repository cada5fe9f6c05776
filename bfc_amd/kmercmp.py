"""Two `bfc -d` dumps compared on the GPU: which k-mers two samples share, which are private to one, and their union.

    python -m bfc_amd.kmercmp [-m INT] [-d INT] [-p|-s|-a] [-u OUT] A.dump B.dump

Both dumps are restored with bfc_ch_restore and uploaded; they must have the same k and the same number of sub-tables.  The reference has
no such tool, so the output format is this project's.  Standard output, in this order:

    shared<TAB>N          keys in both tables                       (always these four lines)
    only_a<TAB>N          keys in A alone
    only_b<TAB>N          keys in B alone
    jaccard<TAB>F         shared / (shared + only_a + only_b), six decimals; 0.000000 for two empty tables
    i<TAB>j<TAB>n         every non-zero cell of the joint spectrum, rows ascending: n keys counted i times in A and j times in B,
                          0 = absent from that table (bfcg_kmers_joint_hist; any k)
    kmer<TAB>count<TAB>high<TAB>count_in_B<TAB>high_in_B
                          under -p / -s / -a: A's k-mers that are private to A / shared with B / all of them (bfcg_kmers_list_vs; k <= 37
                          as for hash2cnt), sub-table by sub-table; an absent k-mer has 0 0 in B.  -m INT and -d INT filter on A's
                          counts as hash2cnt does: count >= INT, min(count, 63) - high >= INT.  Lines are formatted in C.

With -u OUT the union of both tables (counts of shared k-mers added, saturating at 255 / 63) is built on the GPU (bfcg_kmers_union) and
written with bfc_ch_dump: a dump `bfc -r` and every tool here reads.
"""
import getopt
import sys

USAGE = """Usage: kmercmp [options] <A.dump> <B.dump>
Options:
  -p       list the k-mers private to A
  -s       list the k-mers A shares with B
  -a       list all k-mers of A, with their counts in B
  -m INT   listed k-mers: occ >= INT [0]
  -d INT   listed k-mers: occ - occHigh >= INT [0]
  -u FILE  write the union of both tables as a dump
"""


def _atoi(s):
    try:
        return int(s)
    except ValueError:
        return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    try:
        opts, args = getopt.getopt(argv, "psam:d:u:")
    except getopt.GetoptError:
        opts, args = [], []
    o = dict(opts)
    modes = [f for f in ("-p", "-s", "-a") if f in o]
    if len(args) != 2 or len(modes) > 1:
        sys.stderr.write(USAGE)
        return 1
    from . import api
    ta, tb = api.HostTable.restore(args[0]), api.HostTable.restore(args[1])
    if ta is None or tb is None:
        return 1
    if modes and ta.k > 37:
        sys.stderr.write("ERROR: k-mers cannot be listed for k>37\n")
        return 1
    out = sys.stdout.buffer
    a, b = api.GpuKmers(ta), api.GpuKmers(tb)
    try:
        joint, shared, only_a, only_b = a.joint_hist(b)
    except api.BfcGpuError as e:
        sys.stderr.write("ERROR: %s\n" % e)
        return 1
    total = shared + only_a + only_b
    out.write(b"shared\t%d\nonly_a\t%d\nonly_b\t%d\njaccard\t%.6f\n" % (shared, only_a, only_b, shared / total if total else 0.0))
    out.write("".join("%d\t%d\t%d\n" % (i, j, joint[i, j]) for i, j in zip(*joint.nonzero())).encode())
    if modes:
        lo, hi = {"-p": (0, 0), "-s": (1, 255), "-a": (0, 255)}[modes[0]]
        for y, ch, oth in a.pieces_vs(b, _atoi(o.get("-m", "0")), _atoi(o.get("-d", "0")), lo, hi):
            out.write(a.format_vs(y, ch, oth))
    out.flush()
    rc = 0
    if "-u" in o:
        u = a.union(b)
        tu = u.to_host()
        rc = 0 if tu.dump(o["-u"]) == 0 else 1
        tu.close()
        u.close()
    a.close()
    b.close()
    ta.close()
    tb.close()
    return rc


if __name__ == "__main__":
    sys.exit(main())
