#!/usr/bin/env python3
"""Regenerates tests/golden/ec_paths_goldens.json from THE REFERENCE ITSELF (oracle/_ref/bfc-ref and oracle/_ref/libbfcref_ec.so, built by
oracle/Makefile where the reference's sources are present):

    make -C oracle && python tests/golden/make_ec_paths_goldens.py

For every k of tests/ec_corpus.py and for FASTQ and FASTA: the reference's bfc_correct (correct.c:620) on the corpus of that k with the
table `bfc-ref -t1 -E -k K -b22 -d` counted on the counting file.  Recorded: the md5 of its stdout, the reads per ec_code as its ec:Z:
tags give them, and the reads with ec_code 0 whose tag has the brute flag set (the tag of any other code carries no fields).  The file
holds numbers and digests only; the inputs are defined by the seeded generators of tests/ec_corpus.py."""
import hashlib
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
import ec_corpus as EC  # noqa: E402
import oracle  # noqa: E402
from test_ec_host import ref_correct, ref_dump  # noqa: E402

TAG = re.compile(rb"^[@>]\S+\tec:Z:(\d)(?:_\d+:\d+_(\d)_)?", re.M)


def tags(out, fastq):
    """(reads per ec_code, reads of ec_code 0 with the brute flag) from the headers of a corrected file"""
    lines = out.split(b"\n")
    hist, brute0 = [0] * 8, 0
    for h in lines[0:len(lines) - 1:4 if fastq else 2]:
        m = TAG.match(h)
        hist[int(m.group(1))] += 1
        brute0 += m.group(2) == b"1"
    return hist, brute0


def main():
    assert oracle.have_ref(), "build oracle/_ref first (make -C oracle)"
    _, genome, reads, quals = EC.count_set()
    gold = {}
    with tempfile.TemporaryDirectory() as d:
        cnt = os.path.join(d, "count.fq")
        EC.write_reads(cnt, reads, quals)
        for k in EC.KS:
            dump = os.path.join(d, "k%d.hash" % k)
            ref_dump(cnt, k, dump)
            seqs, qs = EC.corpus(genome, k)
            for fmt in ("fq", "fa"):
                fn = os.path.join(d, "corpus_k%d.%s" % (k, fmt))
                EC.write_reads(fn, seqs, qs if fmt == "fq" else None)
                out = ref_correct(dump, fn, {"k": k})
                hist, brute0 = tags(out, fmt == "fq")
                assert sum(hist) == len(seqs)
                gold["k%d_%s" % (k, fmt)] = dict(k=k, format=fmt, n_reads=len(seqs), stdout_md5=hashlib.md5(out).hexdigest(), ec_code_hist=hist,
                                                 brute_code0=brute0)
                print(gold["k%d_%s" % (k, fmt)], file=sys.stderr)
    json.dump(gold, open(os.path.join(HERE, "ec_paths_goldens.json"), "w"), indent=1)
    print("wrote ec_paths_goldens.json (%d entries)" % len(gold))


if __name__ == "__main__":
    main()
