"""FASTA / FASTQ records for the command-line tools (kmerquery -p, readstats)."""


def records(f):
    """(name, sequence, quality) of every FASTA / FASTQ record of a binary file (kseq's grammar: multi-line sequences, '+' starts as
    many quality bytes); quality is None for a FASTA record"""
    name, seq, qual, n_qual = None, [], None, -1   # n_qual >= 0: inside a quality string, bytes still missing
    for line in f:
        line = line.rstrip(b"\r\n")
        if n_qual > 0:
            n_qual -= len(line)
            qual.append(line)
            continue
        if line[:1] in (b">", b"@"):
            if name is not None:
                yield name, b"".join(seq), None if qual is None else b"".join(qual)
            name, seq, qual, n_qual = (line[1:].split() or [b""])[0], [], None, -1
        elif line[:1] == b"+" and name is not None and n_qual < 0:
            n_qual, qual = sum(len(s) for s in seq), []
        elif name is not None and n_qual < 0:
            seq.append(line)
    if name is not None:
        yield name, b"".join(seq), None if qual is None else b"".join(qual)
