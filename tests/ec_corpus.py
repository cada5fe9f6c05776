"""The reads of the error-correction tests (tests/test_ec_host.py on the host instance, tests/test_gpu_ec_paths.py on the device): one
genome, one counting file, and per k one corpus that takes every exit of bfc_ec1 (correct.c:388-476) that a read can take.

What the corpus must reach (conditions(), asserted by every test that uses corpus(); always computed from the host instance's aux, never
from a device's): for every k in KS, as FASTQ and as FASTA, at least one read of each ec_code in {0, 2, 3, 4, 5}, and at least one read
that took the brute path (bfc_ec_greedy_k) and still ended with ec_code 0.

  0  corrected (or clean)                                      edge_reads
  2  CODE_MANY_N: more than 5 % of the bases are not ACGT      edge_reads
  3  CODE_NO_SOLID: no solid k-mer and the brute path found none  edge_reads
  4  CODE_UNCORR_N: the search's heap ran empty                exit_reads: the genome's last bases + N + random bases (and its mirror);
                                                               no k-mer of the table continues the genome's last one
  5  CODE_MANY_FAIL: more than 2n steps without a choice       exit_reads: a genome stretch followed by random bases (a chimera)

ec_code 1 (CODE_MISC) is unreachable: it is bfc_ec1's initial value, bfc_ec1dir leaves its loop without a path only through its -2 and
-3 exits (codes 4 and 5), and every other way out of bfc_ec1 overwrites the code (2, 3 or 0)."""
import numpy as np

KS = (21, 31, 33, 47, 55, 63)
CODES = (0, 2, 3, 4, 5)


def write_reads(fn, seqs, quals=None):
    with open(fn, "wb") as f:
        for i, s in enumerate(seqs):
            if quals is None:
                f.write(b">r%d\n%s\n" % (i, s))
            else:
                f.write(b"@r%d c%d\n%s\n+\n%s\n" % (i, i, s, quals[i]))


def _genome(rng, G):
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, G))


def count_file(rng, genome, n, L=120, err=0.004):
    """reads from both strands at high coverage: the table the corrections are checked with"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    out = []
    for _ in range(n):
        p = int(rng.integers(0, len(genome) - L))
        s = bytearray(genome[p:p + L])
        for j in np.nonzero(rng.random(L) < err)[0]:
            s[j] = b"ACGT"[int(rng.integers(0, 4))]
        s = bytes(s)
        out.append(s.translate(comp)[::-1] if rng.random() < 0.5 else s)
    return out


def count_set(seed=11, G=4000, n=1500):
    """the genome and the counting file's reads and qualities (1500 reads of 120 bases); the generator is returned as it stands after them"""
    rng = np.random.default_rng(seed)
    genome = _genome(rng, G)
    reads = count_file(rng, genome, n)
    quals = [bytes(rng.integers(40, 74, len(s)).astype(np.uint8)) for s in reads]
    return rng, genome, reads, quals


def edge_reads(rng, genome, k):
    """clean and erroneous reads, reads shorter than k, N-rich reads, N runs inside solid stretches, reads with no solid k-mer (errors
    every k/2 bases: the brute path), lower case and IUPAC codes, random reads.  These end with ec_code 0, 2 or 3 (see the module's text;
    exit_reads has the rest)"""
    G = len(genome)
    reads = []

    def pick(L):
        p = int(rng.integers(0, G - L))
        return bytearray(genome[p:p + L])
    for _ in range(60):                                         # sequencing errors, 0-6 per read, some close together
        s = pick(int(rng.integers(k + 5, 250)))
        for _ in range(int(rng.integers(0, 7))):
            s[int(rng.integers(0, len(s)))] = b"ACGT"[int(rng.integers(0, 4))]
        reads.append(s)
    for _ in range(10):
        reads.append(pick(int(rng.integers(1, k))))             # shorter than k
    for _ in range(10):                                         # N-rich
        s = pick(150)
        for j in rng.integers(0, 150, 12):
            s[j] = ord("N")
        reads.append(s)
    for _ in range(15):                                         # one N or a short N run inside
        s = pick(200)
        j = int(rng.integers(k, 200 - k))
        s[j:j + int(rng.integers(1, 4))] = b"N" * 3
        reads.append(s[:200])
    for _ in range(20):                                         # no solid k-mer: an error every k/2 bases
        s = pick(int(rng.integers(k + 2, 2 * k + 10)))
        for j in range(int(rng.integers(0, k // 2)), len(s), max(2, k // 2)):
            s[j] = b"ACGT"[(b"ACGT".index(s[j]) + 1) % 4]
        reads.append(s)
    for _ in range(10):                                         # lower case, IUPAC codes
        s = pick(180)
        s[int(rng.integers(0, 180))] = b"RYKMSWBDHVN"[int(rng.integers(0, 11))]
        if rng.random() < 0.5:
            s = bytearray(bytes(s).lower())
        else:
            s[10:60] = bytes(s[10:60]).lower()
        reads.append(s)
    for _ in range(5):
        reads.append(bytearray(b"ACGT"[c] for c in rng.integers(0, 4, 150)))
    return [bytes(s) for s in reads]


def exit_reads(rng, genome, k):
    """the exits edge_reads does not take.  Nine chimeras (a genome head of k + 10, 100 or 200 bases, then 30, 100 or 250 random bases:
    CODE_MANY_FAIL where the tail is long enough), nine reads `the genome's last bases + N + random` and their nine mirrors `random + N +
    the genome's first bases` (CODE_UNCORR_N: the heap runs empty at the N, since the table holds no continuation of the genome's last
    k-mer), and reads that mix the cases: a chimera with an error inside its head, a lower-case chimera, reads whose only island lies
    within k bases of the genome's end or start."""
    G = len(genome)
    heads, tails = (k + 10, 100, 200), (30, 100, 250)

    def rnd(L):
        return bytes(b"ACGT"[c] for c in rng.integers(0, 4, L))

    def pick(L):
        p = int(rng.integers(0, G - L))
        return genome[p:p + L]
    reads = []
    for h in heads:
        for t in tails:
            reads.append(pick(h) + rnd(t))
    for h in heads:
        for t in tails:
            reads.append(genome[G - h:] + b"N" + rnd(t))
    for h in heads:
        for t in tails:
            reads.append(rnd(t) + b"N" + genome[:h])
    s = bytearray(pick(200) + rnd(250))                         # a chimera with an error inside its head
    s[100] = b"ACGT"[(b"ACGT".index(s[100]) + 1) % 4]
    reads.append(bytes(s))
    reads.append((pick(100) + rnd(250)).lower())                # a lower-case chimera
    reads.append(rnd(250) + pick(100))                          # the head at the other end
    # the only island within k of the genome's end, and of its start: 21 k-mers that stop 20 bases short of it (the counting file's reads
    # start anywhere but in the last 120 bases, so the outermost k-mers are not solid: the reads above whose head is the genome's last k + 10
    # bases end with CODE_NO_SOLID for that reason)
    reads.append(rnd(60) + genome[G - k - 40:G - 20])
    reads.append(genome[20:k + 40] + rnd(60))
    reads.append(genome[G - k - 40:G - 20] + b"N" + rnd(20))
    return reads


def corpus(genome, k):
    """edge_reads + exit_reads for this k with a quality string each (bytes 33 .. 73), seeded by k alone"""
    rng = np.random.default_rng(300 + k)
    seqs = edge_reads(rng, genome, k) + exit_reads(rng, genome, k)
    quals = [bytes(rng.integers(33, 74, len(s)).astype(np.uint8)) for s in seqs]
    return seqs, quals


def histogram(aux):
    """(reads per ec_code 0 .. 7, reads that took the brute path) of a batch's aux words"""
    aux = np.asarray(aux, dtype=np.uint32)
    return [int(c) for c in np.bincount(aux & 7, minlength=8)], int((aux >> 3 & 1).sum())


def conditions(aux):
    """what the corpus must reach, on the aux words of the expected side (the host instance or the reference)"""
    aux = np.asarray(aux, dtype=np.uint32)
    hist, brute = histogram(aux)
    for code in CODES:
        assert hist[code] > 0, "no read of the corpus ends with ec_code %d: %s" % (code, hist)
    assert hist[1] == 0 and hist[6] == 0 and hist[7] == 0, hist
    assert ((aux >> 3 & 1 == 1) & (aux & 7 == 0)).any(), "no read took the brute path to ec_code 0 (%d brute reads)" % brute
