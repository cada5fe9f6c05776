"""bfc_amd -- MI355X-native k-mer counting for BFC (count.c + bbf.c + htab.c of lh3/bfc r181).

The product is ``libbfc_gpu.so`` (C ABI: include/bfc_gpu.h); this package is its thin Python
mirror of the reference's count-phase interface.  Nothing here computes k-mers on the CPU.
"""
from .api import (GRAPH_MASKS, BfcGpuError, GpuCorrector, GpuCounter, GpuGroup, GpuKcov, GpuKmers, GpuTrimmer, HostBloom, HostTable, bfc_count, bfc_opt_by_size, bfc_opt_init, format_ec, format_read_stats, kmer_revcomp, nb_text, pack_planes, parse_ec_stats, to_stream, unitig_link_rows, unitig_rows)  # noqa: F401
from ._lib import BfcOpt  # noqa: F401
