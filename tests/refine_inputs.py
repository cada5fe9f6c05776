"""Inputs of the `bfc -R` tests (tests/test_ec_refine_host.py, tests/test_gpu_ec_refine.py): seeded rewrites of a first-pass output, a
reader that keeps comments as the reference's bseq_read does, and the refinement pipeline (worker_ec + bfc_ec_cb, correct.c:533-612)
restated in Python over the library's corrector, for files of reads.  The recipes are the record behind tests/golden/ec_refine_goldens.json:
a golden is the md5 of `bfc -R -k31 -b26 -t1` (the reference) on the file a recipe makes from g1's first pass."""
import re

import numpy as np

RE_EC0 = re.compile(rb"^ec:Z:0_(\d+):(\d+)_(\d+)_(\d+):(\d+)_(\d+)$")


def read_records(data):
    """FASTQ / FASTA records as kseq reads them (kseq.h:185-224) and bseq_read keeps them (bseq.c:64, keep_comment): names, comments (a
    header without one gets the last comment seen, None before the first), sequences, qualities (None for FASTA).  One line per field."""
    lines = data.split(b"\n")
    names, comments, seqs, quals = [], [], [], []
    cmt, i = None, 0
    while i < len(lines) and lines[i]:
        h = lines[i]
        fq = h[:1] == b"@"
        m = re.match(rb"^[@>](\S*)(?:[ \t](.*))?$", h)
        if m.group(2) is not None:
            cmt = m.group(2)
        names.append(m.group(1)); comments.append(cmt); seqs.append(lines[i + 1])
        quals.append(lines[i + 3] if fq else None)
        i += 4 if fq else 2
    return names, comments, seqs, quals


def write_records(names, comments, seqs, quals):
    out = []
    for i, n in enumerate(names):
        h = (b"@" if quals[i] is not None else b">") + n + (b"\t" + comments[i] if comments[i] is not None else b"")
        out.append(h + b"\n" + seqs[i] + b"\n" + (b"+\n" + quals[i] + b"\n" if quals[i] is not None else b""))
    return b"".join(out)


def _ec0(c, n_absent=None, max_heap=None):
    m = RE_EC0.match(c)
    f = list(m.groups())
    if n_absent is not None:
        f[0] = b"%d" % n_absent
    if max_heap is not None:
        f[1] = b"%d" % max_heap
    return b"ec:Z:0_%s:%s_%s_%s:%s_%s" % tuple(f)


def recipe_b(data, seed=21):
    """every ec:Z:0 comment: max_heap 60 (so every read is refined), n_absent from {0, 1, as it was, 2^22 - 1}: both rf 2 and rf 3"""
    rng = np.random.default_rng(seed)
    names, comments, seqs, quals = read_records(data)
    out = []
    for c in comments:
        if c is not None and RE_EC0.match(c):
            v = int(rng.integers(0, 4))
            c = _ec0(c, n_absent=[0, 1, None, 4194303][v], max_heap=60)
        out.append(c)
    return write_records(names, out, seqs, quals)


def recipe_c(data, seed=22):
    """a mixture: headers without a comment (the last one stays in kseq's buffer), other comments, ec:Z:3, ec_code 8 / 9, max_heap 300 /
    306 / 60, n_absent changed, '#' qualities (a C read from the quality string) in the reads.  Every rewritten ec:Z:0 comment keeps all
    its fields, so the reference's parser never reads past the NUL."""
    rng = np.random.default_rng(seed)
    names, comments, seqs, quals = read_records(data)
    out, qs = [], []
    for i, c in enumerate(comments):
        u = rng.random()
        if i == 0 or c is None or not RE_EC0.match(c):
            pass
        elif u < 0.10:
            c = None                                            # no comment: the previous record's stays
        elif u < 0.15:
            c = b"foo bar baz"
        elif u < 0.20:
            c = b"ec:Z:3"
        elif u < 0.25:
            c = b"ec:Z:%d%s" % (8 + int(rng.integers(0, 2)), c[6:])   # 8 -> 0 (all fields parsed), 9 -> 1
        elif u < 0.35:
            c = _ec0(c, max_heap=int(rng.choice([300, 306, 60, 49, 50])))
        elif u < 0.55:
            c = _ec0(c, n_absent=int(rng.integers(0, 3)), max_heap=int(rng.choice([55, 255, 1000])))
        q = quals[i]
        if q is not None and rng.random() < 0.2:
            q = bytearray(q)
            for j in rng.integers(0, len(q), int(rng.integers(1, 4))):
                q[j] = ord("#")
            q = bytes(q)
        out.append(c); qs.append(q)
    return write_records(names, out, seqs, qs)


def recipe_fasta(data):
    names, comments, seqs, _ = read_records(data)
    return write_records(names, comments, seqs, [None] * len(names))


def rewrite_all_refined(data):
    """(b) without the n_absent draw, for large files: every ec:Z:0 comment's max_heap becomes 60 (bytes only, no record parsing)"""
    return re.sub(rb"(\tec:Z:0_\d+:)\d+(_)", rb"\g<1>60\2", data)


def refine(corrector, names, comments, seqs, quals, opt, gpu=False):
    """`-R` over a file's records with the library's corrector (GpuCorrector made with refine_ec): worker_ec's skip and ori_st in stream
    order (`-t1`), the reads to refine corrected as one batch (device or host instance), the output of bfc_ec_cb.  Returns (bytes, aux2
    of the refined reads)."""
    from bfc_amd import format_ec, parse_ec_stats
    n = len(names)
    ori = (0, 0)
    idx, oa, oa2, kept = [], [], [], [None] * n
    for i in range(n):
        st = parse_ec_stats(comments[i]) if comments[i] is not None else None
        if st is not None:
            ori = st
            if st[0] & 7 == 0 and st[1] & 0xff < 50:
                kept[i] = comments[i]
                continue
        idx.append(i); oa.append(ori[0]); oa2.append(ori[1])
    fq = quals[0] is not None if n else True
    sub_q = [quals[i] for i in idx] if fq else None
    run = corrector.correct if gpu else corrector.host_correct
    s, q, a, a2 = run([seqs[i] for i in idx], sub_q, ori=(np.array(oa, dtype=np.uint32), np.array(oa2, dtype=np.uint32)))
    S, Q = list(seqs), list(quals) if fq else None
    A, A2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    for j, i in enumerate(idx):
        S[i] = s[j]
        if fq:
            Q[i] = q[j]
        A[i], A2[i] = a[j], a2[j]
    return format_ec(names, S, Q, A, A2, opt, comments=kept), a2
