"""Deterministic driver for profiles/mg_rank_batch.md: every path of a rank's batch in bfcg_mg.hip that one GPU can run, in ONE process.

    python scripts/mg_rank_batch_paths.py                       # prints one line of hashes per part
    rocprofv3 --kernel-trace -d DIR -o NAME --output-format csv -- python scripts/mg_rank_batch_paths.py
    BFC_GPU_LIB=/path/to/another/libbfc_gpu.so ...              # the same with another build of the library

Parts: two clean global batches through a 2-rank group on device 0 with the lazy protocol, with BFCG_MG_LAZY=0 (sized slabs) and with
BFCG_MG_SLABS=0 (two passes); one 4-rank group with transport 2 (peer copies).  The hashes: the exact statistics, the filter, the table."""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bfc_amd  # noqa: E402
from bfc_amd import gen  # noqa: E402

L, PER, K, B = 150, 60_000, 33, 30


def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def reads():
    rng = np.random.default_rng(20240)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = rng.choice(acgt, 30_000_000 + L)
    seq = genome[(rng.integers(0, 30_000_000, 2 * PER)[:, None] + np.arange(L)[None, :])].astype(np.uint8).reshape(-1)
    seq[rng.integers(0, len(seq), 300)] = ord("N")
    qual = rng.integers(33, 74, len(seq)).astype(np.uint8)
    return seq, qual


def part(name, seq, qual, n_ranks, env, transport=0):
    for k in ("BFCG_MG_LAZY", "BFCG_MG_SLABS"):
        os.environ.pop(k, None)
    os.environ.update(env)
    grp = bfc_amd.GpuGroup(K, B, [0] * n_ranks, max_batch_pos=PER * (L + 1) // n_ranks + 4096, transport=transport)
    for t in range(2):
        a, e = t * PER * L, (t + 1) * PER * L
        grp.count_host(gen.to_stream(seq[a:e], L, 10), gen.to_stream(qual[a:e], L, 33))
    grp.sync()
    info, st = grp.info(), grp.stats()
    bf = grp.export_bloom(0)
    tab = grp.export_table()
    sizes, slots = tab.export_sorted()
    print("%s: transport=%s slab_mode=%d lazy_batches=%d stats=%s crowded_regions=%s filter=%s table=%s" % (
        name, info["transport"], info["slab_mode"], info["lazy_batches"], h(np.array([st[x] for x in ("n_kmers", "n_high", "n_seen", "n_keys")], dtype=np.uint64)),
        st.get("crowded_regions"), h(bf.bytes()), h(sizes) + h(slots)), flush=True)
    bf.close(); tab.close(); grp.close()


def main():
    seq, qual = reads()
    part("lazy", seq, qual, 2, {})
    part("sized slabs", seq, qual, 2, {"BFCG_MG_LAZY": "0"})
    part("two passes", seq, qual, 2, {"BFCG_MG_SLABS": "0"})
    part("4 ranks, peer copies", seq, qual, 4, {}, transport=2)


if __name__ == "__main__":
    main()
