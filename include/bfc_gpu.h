/* bfc_gpu.h -- C ABI of libbfc_gpu.so: MI355X-native k-mer counting for BFC.
 *
 * PART 1 is the drop-in boundary: exactly the symbols the reference's count.o + bbf.o + htab.o
 * export, with the reference's argument meaning and error behaviour, so that an unmodified
 * correct.c / bfc.c link against this library instead.  Each declaration cites
 * the reference interface it replaces (paths relative to lh3/bfc r181).
 *
 * PART 2 is the device-level interface underneath (context, batches already resident in HBM,
 * export), used by bench.py, the parity tests and multi-GPU orchestration.
 *
 * Plain C, plain pointers and sizes.  All counting work runs in HIP kernels on gfx950; there is
 * no CPU fallback: without a usable GPU every entry point that has to count fails loudly
 * ("[E::bfcg] ..." on stderr, then abort() for the reference-shaped entry points that have no
 * error channel, or a negative return code for the bfcg_* ones).
 */
#ifndef BFC_GPU_H
#define BFC_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ============================================================ PART 1: reference-shaped API */

/* k-mer as four k-bit planes -- replaces kmer.h:6-8 */
typedef struct { uint64_t x[4]; } bfc_kmer_t;

/* blocked bloom filter -- replaces bbf.h:9-12.  The layout is public: correct.c:490 reads
 * bf->n_hashes directly.  `b` is host memory (2^(n_shift-3) bytes, 64-byte aligned). */
#define BFC_BLK_SHIFT 9
#define BFC_BLK_MASK  ((1 << BFC_BLK_SHIFT) - 1)
typedef struct { int n_shift, n_hashes; uint8_t *b; } bfc_bf_t;

bfc_bf_t *bfc_bf_init(int n_shift, int n_hashes);      /* bbf.h:14, bbf.c:5   NULL if n_shift outside [9,55] */
void      bfc_bf_destroy(bfc_bf_t *b);                 /* bbf.h:15, bbf.c:19 */
int       bfc_bf_insert(bfc_bf_t *b, uint64_t hash);   /* bbf.h:16, bbf.c:25  returns # of bits already set */
int       bfc_bf_get(const bfc_bf_t *b, uint64_t hash);/* bbf.h:17, bbf.c:47  thread-safe, read-only */

/* k-mer count table -- replaces htab.h:10-23 (opaque) */
#define BFC_CH_KEYBITS 50
#define BFC_CH_MAXPRE  24
struct bfc_ch_s;
typedef struct bfc_ch_s bfc_ch_t;

bfc_ch_t *bfc_ch_init(int k, int l_pre);                                               /* htab.c:19  */
void      bfc_ch_destroy(bfc_ch_t *ch);                                                /* htab.c:36  */
int       bfc_ch_insert(bfc_ch_t *ch, const uint64_t x[2], int is_high, int forced);   /* htab.c:60  0, or -1 if !forced and busy */
int       bfc_ch_get(const bfc_ch_t *ch, const uint64_t x[2]);                         /* htab.c:84  -1 | high<<8|count; thread-safe */
uint64_t  bfc_ch_count(const bfc_ch_t *ch);                                            /* htab.c:101 */
int       bfc_ch_hist(const bfc_ch_t *ch, uint64_t cnt[256], uint64_t high[64]);       /* htab.c:110 returns the mode (i>=3) or -1 */
int       bfc_ch_dump(const bfc_ch_t *ch, const char *fn);                             /* htab.c:129 0 | -1 */
bfc_ch_t *bfc_ch_restore(const char *fn);                                              /* htab.c:151 NULL on failure */
int       bfc_ch_get_k(const bfc_ch_t *ch);                                            /* htab.c:178 */
int       bfc_ch_kmer_occ(const bfc_ch_t *ch, const bfc_kmer_t *z);                    /* htab.c:94  */

/* options -- replaces bfc.h:15-33; field order and types are the ABI */
typedef struct {
	int chunk_size;
	int n_threads, no_mt_io;
	int q, k;
	int filter_mode, refine_ec, no_qual;
	float min_frac;
	int l_pre, bf_shift, n_hashes;
	int discard;
	int max_end_ext;
	int win_multi_ec;
	int min_cov;
	int w_ec, w_ec_high, w_absent, w_absent_high;
	int max_path_diff, max_heap;
} bfc_opt_t;

/* the count phase -- replaces bfc.h:39 / count.c:127.  Returns a bfc_ch_t* (table mode) or the
 * bfc_bf_t* holding k-mers seen at least twice (opt->filter_mode); the caller frees it with
 * bfc_ch_destroy / bfc_bf_destroy (bfc.c:146,149).  fn may be "-" (stdin) or gzip'd. */
void *bfc_count(const char *fn, const bfc_opt_t *opt);

/* the second phase's entry point -- bfc.h:40 / correct.c:620.  Provided ONLY for the trim pass of `bfc -1`
 * (opt->filter_mode, ptr = the bfc_bf_t* bfc_count returned): bloom queries (bbf.c:47-63), longest streak
 * (correct.c:478-497) and the keep/trim rule (correct.c:557-569) run on the GPU, output as correct.c:595-611.
 * With filter_mode off it forwards to bfc_correct_cpu(), i.e. the reference's correct.c compiled with
 * -Dbfc_correct=bfc_correct_cpu.  Error correction (table mode, with or without refine_ec, i.e. `-R`) runs on the GPU
 * (bfcg_ec_*, PART 2) when BFC_GPU_EC=1 is set or bfc_correct_cpu is not linked; otherwise it is bfc_correct_cpu's. */
void bfc_correct(const char *fn, const bfc_opt_t *opt, const void *ptr);

/* ============================================================ PART 2: device-level API */

typedef struct bfcg_ctx bfcg_ctx_t;

typedef struct {
	int k, q, bf_shift, n_hashes, l_pre, filter_mode;  /* as bfc_opt_t */
	int device;                 /* HIP device ordinal */
	uint64_t max_batch_pos;     /* capacity: positions (bases + separators) per batch, < 2^32 */
	int region_shift;           /* log2 bloom blocks per LDS region; 0 = default */
	int tab_cshift;             /* initial log2 slots per sub-table; 0 = default */
	int debug_seen;             /* allocate the per-position seen-flag buffer (tests) */
	int track_order;            /* keep per-key first-insert / per-sub-table last-call stamps: bfc_ch_dump becomes byte-identical to `bfc -t1 -d` */
	int rank, n_ranks;          /* multi-GPU, owner computes: this process is rank of n_ranks (0/0 or 0/1: single GPU) */
	int table_layout;           /* 0: region-owned table segments updated through LDS wherever the geometry allows (2k minus the bits a bloom region
	                             * implies <= 50), converted to the host's layout at export; 1: the host's (sub-table, key) layout from the start */
} bfcg_params_t;

void bfcg_params_default(bfcg_params_t *p);
/* NULL on failure (message on stderr); never falls back to the CPU */
bfcg_ctx_t *bfcg_create(const bfcg_params_t *p);
void bfcg_destroy(bfcg_ctx_t *c);
const char *bfcg_last_error(void);
/* "src:<sha256/16 of the library's sources> git:<HEAD when it was built>": ties a travelling libbfc_gpu.so to the sources it claims
 * (bfc_amd/build.py::source_hash recomputes the first part from the tree; __graft_entry__.smoke() and bench.py compare). */
const char *bfcg_build_id(void);
/* HIP devices this process sees (0 if none, or if the runtime cannot start): callers that spread a run over several GPUs (bfc_count with
 * BFC_GPU_DEVICES, bench.py --gpus N) check their device list against it and fail loudly rather than run on fewer */
int bfcg_device_count(void);
/* clear both bloom filters and the table */
int bfcg_reset(bfcg_ctx_t *c);

/* A batch is a byte stream: reads concatenated, each followed by ONE separator byte (any byte
 * that is not ACGTacgt, e.g. '\n'); `qual` is the aligned Phred+33 stream or NULL (FASTA:
 * every base counts as high quality, count.c:85).  Batches must be submitted in file order.
 * _dev: the streams are already resident in HBM.  _host: pageable/pinned host memory, copied
 * asynchronously.  Both return 0 or a negative error. */
int bfcg_count_batch_dev(bfcg_ctx_t *c, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_pos);
int bfcg_count_batch_host(bfcg_ctx_t *c, const uint8_t *h_seq, const uint8_t *h_qual, uint64_t n_pos);
/* The same batch as FOUR BIT PLANES (bit i of a plane = stream position i, 32 positions per word): all that count.c:72-89 reads of a position
 * is its base code (seq_nt6_table minus one: A C G T = 0 1 2 3, bseq.c:9-26, count.c:82), whether it is a base at all (count.c:83,88) and
 * whether `qual - 33 >= q` (count.c:85, a signed char) -- 4 bits instead of the 16 that cross PCIe with bfcg_count_batch_host, whose rate is
 * the link's (17 G k-mers/s at 45 GB/s).  Plane p starts at planes + p * plane_words: [0] low code bit, [1] high code bit, [2] not ACGTacgt
 * (separators included; positions beyond the batch's end in the last word too), [3] quality - 33 >= q.
 *   bfcg_plane_words(n)     words per plane for n positions
 *   bfcg_pack_planes        positions [lo, hi) of a byte-stream batch into its planes; lo a multiple of 32 (threads pack disjoint word ranges),
 *                           hi a multiple of 32 or the batch's end n_pos; qual NULL: no quality plane is written
 *   bfcg_count_batch_planes counts positions [first_pos, first_pos + n_pos) of the plane set; has_qual = 0: the records carry no qualities
 *                           (every base is high quality, count.c:85) and plane [3] is not read.  Same results as the byte streams, bit for bit. */
uint64_t bfcg_plane_words(uint64_t n_pos);
void bfcg_pack_planes(const uint8_t *seq, const uint8_t *qual, uint64_t lo, uint64_t hi, uint64_t n_pos, int q, uint32_t *planes, uint64_t plane_words);
int bfcg_count_batch_planes(bfcg_ctx_t *c, const uint32_t *h_planes, uint64_t plane_words, uint64_t first_pos, uint64_t n_pos, int has_qual);
int bfcg_sync(bfcg_ctx_t *c);

/* Multi-GPU (one process per GPU; SURVEY 8e partitioning B, "owner computes"): rank r owns 1/n_ranks of the bloom
 * regions and every k-mer that falls into them.  Per global batch every rank calls bfcg_mg_scatter on ITS contiguous
 * share of the batch (rank-major file order): records are written to d_send grouped by level-1 bucket and
 * counts[2^F1] (host) receives the bucket sizes; bucket b belongs to rank b / nb_loc.  The caller exchanges records
 * (all-to-all over RCCL) so that d_recv holds, source-major, the records of the owned buckets, and calls
 * bfcg_mg_process with seg_cnt[source][owned bucket].  info: {2^F1, owned buckets nb_loc, bytes per record, n_ranks}. */
int bfcg_mg_info(bfcg_ctx_t *c, int out[4]);
/* Positions per batch the filter's regions take at full speed (a region holds about list-capacity k-mers with clear bits in LDS; beyond
 * that it takes an exact but far slower path).  bfcg_count_batch_* cut larger batches themselves.  With several ranks the GLOBAL batch
 * (all ranks' shares together) should stay below n_ranks times this: size the filter, or the shares, accordingly -- bench.py keeps
 * 2^33 bits of filter per rank. */
uint64_t bfcg_batch_limit(bfcg_ctx_t *c);
int bfcg_mg_scatter(bfcg_ctx_t *c, const uint8_t *d_seq, const uint8_t *d_qual, uint64_t n_pos, void *d_send, uint32_t *counts);
int bfcg_mg_process(bfcg_ctx_t *c, const void *d_recv, const uint32_t *seg_cnt);
/* stage B may partition what it received in one pass (region slabs; an overflow is found one call later and that stage B replayed from d_recv)
 * only if the caller keeps every d_recv unchanged until the call after the next has returned -- bfcg_group_* alternates its receive buffers and
 * turns this on; callers of bfcg_mg_process that reuse one buffer leave it off (the default) */
void bfcg_mg_allow_onepass(bfcg_ctx_t *c, int on);

enum { BFCG_ST_KMERS = 0, BFCG_ST_HIGH, BFCG_ST_SEEN, BFCG_ST_KEYS, BFCG_ST_TAB_OVF, BFCG_ST_ERR_POOL, BFCG_ST_SLOW_BUCKETS, BFCG_ST_CROWDED,
       BFCG_ST_TAB_CSHIFT = 8, BFCG_ST_BATCHES, BFCG_ST_N = 16 };

/* Multi-GPU in C.  A GROUP drives the local ranks of an owner-computes run of n_ranks GPUs from inside the library -- stage A, the
 * exchange of the k-mer records (grouped ncclSend / ncclRecv over RCCL, or direct peer copies between the devices of one process) and
 * stage B, one host thread per local rank, no Python and no torch in the data path.  Either every rank is local (one process, n_ranks
 * devices: what bfc_count does with BFC_GPU_DEVICES=0,1,...; a device may be named several times to emulate ranks on one GPU), or
 * exactly one is (one process per GPU, as torch.distributed.run launches bench.py): then `uid` is the run's RCCL unique id, made by
 * bfcg_group_unique_id on one process and handed to the others out of band.  `prm` as for bfcg_create (device / rank / n_ranks are set
 * per rank; max_batch_pos = positions of ONE RANK's share of a global batch).  transport: 0 auto, 1 RCCL, 2 peer copies.
 * A global batch is the ranks' shares in rank order (rank-major file order): results are those of `bfc -t1` on that order.
 * Stage A of a rank is ONE pass since round 4 (K1 once): its records land in 8 slabs per level-1 bucket, a destination's buckets are one
 * contiguous range of slabs and travel as they are, the rank's own share is written straight into its receive buffer; input that overflows
 * a slab (few, often repeated k-mers) sends that batch and the rest of the run through the two-pass stage A with exact bucket sizes.
 * reference: count.c:106 (kt_for over reads), count.c:143 (kt_pipeline) -- the fan-out lives inside bfc_count. */
typedef struct bfcg_group bfcg_group_t;
#define BFCG_UID_BYTES 128
int bfcg_group_unique_id(uint8_t uid[BFCG_UID_BYTES]);
bfcg_group_t *bfcg_group_create(const bfcg_params_t *prm, int n_ranks, int first_rank, int n_local, const int *devices, const uint8_t *uid, int transport);
void bfcg_group_destroy(bfcg_group_t *g);
int bfcg_group_info(bfcg_group_t *g, int out[6]);     /* n_ranks, n_local, transport in use (1 RCCL, 2 peer copies, 3 peer copies with the PUSH kernel for exact sizes), bytes per record, 2^F1, first rank */
/* out[0] bytes the local ranks put on the links since creation / the last reset (blocks and messages as sent), out[1] the bytes of the live records
 * among them (what an exact exchange moves; transport 3 moves exactly these + the rows), out[2] global batches, out[3] transport.  Drains the exchange. */
int bfcg_group_exchange_bytes(bfcg_group_t *g, uint64_t out[4]);
bfcg_ctx_t *bfcg_group_ctx(bfcg_group_t *g, int i);  /* local rank i's context (statistics, exports of its slice); owned by the group */
int bfcg_group_slab_mode(bfcg_group_t *g);           /* 1: stage A runs in one pass into slabs; 0: two passes (never possible, switched off, or a slab overflowed in this run) */
uint64_t bfcg_group_lazy_batches(bfcg_group_t *g);   /* global batches since creation whose exchange and stage B were enqueued before the host saw any size (slab mode; in-process and multi-process groups alike -- the processes agree on it through the set-up's all-gather, bit 1 of its first word) */
int bfcg_group_reset(bfcg_group_t *g);
/* one global batch: local rank i contributes the stream d_seq[i] / d_qual[i] (on ITS device) of n_pos[i] positions (0 = nothing) */
int bfcg_group_count_batch_dev(bfcg_group_t *g, const uint8_t *const *d_seq, const uint8_t *const *d_qual, const uint64_t *n_pos);
/* one global batch from host memory, cut by the library into n_ranks contiguous shares at read boundaries (all ranks local) */
int bfcg_group_count_batch_host(bfcg_group_t *g, const uint8_t *h_seq, const uint8_t *h_qual, uint64_t n_pos);
/* Drains every local rank.  COLLECTIVE when the ranks live in several processes: it ends with a one-word all-gather of the ranks' status, so
 * every process of the run must call it (also one that has met an error -- it then reports -1 everywhere), or its peers block in that
 * all-gather.  The same holds for bfcg_group_count_batch_*: every process submits every global batch (an empty share is fine). */
int bfcg_group_sync(bfcg_group_t *g);
int bfcg_group_stats(bfcg_group_t *g, uint64_t out[BFCG_ST_N]);   /* sums over the local ranks */
/* progress without draining (as bfcg_progress, below): *batches = global batches submitted, *final = the last one complete on every local rank,
 * keys_of[j], j < n: distinct keys (local ranks summed) after global batch *final - j; returns the number of valid entries */
int bfcg_group_progress(bfcg_group_t *g, uint64_t *batches, uint64_t *final, uint64_t *keys_of, int n);
bfc_ch_t *bfcg_group_export_table(bfcg_group_t *g);              /* all ranks local: THE table (union of the ranks' disjoint tables) */
bfc_bf_t *bfcg_group_export_bloom(bfcg_group_t *g, int which);   /* all ranks local: THE filter (the ranks' slices in rank order) */
/* the same, and every local device keeps a full copy of the filter in HBM (all-gathered from the slices by peer copies) for the sharded
 * trim pass of `bfc -1` to adopt (bfcg_trim_create on that device), until bfc_bf_destroy */
bfc_bf_t *bfcg_group_export_bloom_resident(bfcg_group_t *g, int which);

/* device memory helpers so that callers (bench.py) can stage inputs without another runtime */
void *bfcg_dev_alloc(bfcg_ctx_t *c, uint64_t bytes);
void  bfcg_dev_free(bfcg_ctx_t *c, void *p);
int   bfcg_h2d(bfcg_ctx_t *c, void *dst, const void *src, uint64_t bytes);
int   bfcg_d2h(bfcg_ctx_t *c, void *dst, const void *src, uint64_t bytes);
void *bfcg_host_alloc(uint64_t bytes);   /* pinned host memory */
void  bfcg_host_free(void *p);

int bfcg_stats(bfcg_ctx_t *c, uint64_t out[BFCG_ST_N]);   /* drains the pipeline first */
/* progress without draining: *calls = bfcg_count_batch_* calls since the last reset, *final = the last of them whose batches are all
 * complete, keys_of[i] (i < n) = distinct keys in the table after call *final - i: the table's counters are copied out right behind every
 * batch's table stage (count.c:113 prints the count after every chunk; bfc_count prints it from here).  Exact as long as no k-mer is
 * parked (a full segment or sub-table).  The keys that the replay of parked k-mers creates are counted at the call the context drains at:
 * a call whose k-mers parked and the calls up to that one lack them, the calls from that one on are exact again. */
int bfcg_progress(bfcg_ctx_t *c, uint64_t *calls, uint64_t *final, uint64_t *keys_of, int n);
/* how the count table is held right now: out[0] 1 = region-owned segments, 0 = the host's layout; out[1] log2 slots per segment;
 * out[2] log2 slots per sub-table; out[3] segment growths so far */
int bfcg_table_info(bfcg_ctx_t *c, int out[4]);
/* where the context's geometry puts the k-mer with table hash (y0, y1), computed on the host by the functions the kernels use: out[0] its
 * bloom region, out[1] its identity inside the region, out[2] the 26-bit home of that identity (the home slot is its low bits), out[3] the
 * block of a segment of the current size that holds it (0 in the host's layout).  Read-only; for tests that place k-mers. */
int bfcg_seg_place(bfcg_ctx_t *c, uint64_t y0, uint64_t y1, uint64_t out[4]);
/* the same functions without a context (no GPU needed): out[0] the identity of (y0, y1) inside its region for the implied bit field [lo, hi) of
 * y0, out[1] its home, out[2], out[3] the hash rebuilt from (region, identity); -1 for a geometry that cannot be */
int bfcg_seg_id_host(int k, int lo, int hi, uint64_t region, uint64_t y0, uint64_t y1, uint64_t out[4]);
/* what the table's write path has done since the context was created (a reset clears nothing): out[0] parked k-mers replayed into segments,
 * out[1] parked k-mers replayed into the host's layout, out[2] commits of the hand-over log, out[3] pages of the largest of them,
 * out[4] conversions of the segments to the host's layout, out[5..7] zero.  Complete once the pipeline is drained (bfcg_sync). */
int bfcg_commit_info(bfcg_ctx_t *c, uint64_t out[8]);
/* how the k-mers are partitioned: out[0] bit 0 = the one-pass level-1 partition (the k-mer hash is computed once per batch, no histogram pass) is in
 * use, bit 1 = level 2 runs in one pass too (a slab per bloom region, no k_hist2); out[1] batches that had to be replayed through the two-pass
 * partition so far (input with few, often repeated k-mers overflows a one-pass slab) */
int bfcg_partition_info(bfcg_ctx_t *c, uint64_t out[2]);
/* launches of k_scatter1_wc (level 1 of the one-pass partition through write-combining buffers in LDS: bfcg_scatter1wc.hip) by this process so far */
uint64_t bfcg_s1wc_launches(void);
/* batches handled without aggregation (k-mers that hardly repeat inside a batch: seen k-mers are streamed to the table kernel) */
uint64_t bfcg_stream_batches(bfcg_ctx_t *c);

/* per-stage GPU time of the last batch, HIP events on the context's stream (ms):
 * [0] hist1+scans [1] scatter1 [2] hist2+scan2+scatter2 [3] bloom regions [4] table commit [5] total */
int bfcg_last_batch_ms(bfcg_ctx_t *c, float out[6]);
/* the same, summed over every batch finalised since the last reset != 0 call; drains the pipeline first */
int bfcg_stage_ms(bfcg_ctx_t *c, double out[6], uint64_t *n_batches, int reset);

/* results */
int bfcg_bloom_to_host(bfcg_ctx_t *c, int which /*0: bf, 1: bf_high*/, uint8_t *dst);   /* 2^(bf_shift-3) / n_ranks bytes: the owned slice */
bfc_bf_t *bfcg_export_bloom(bfcg_ctx_t *c, int which);   /* host bfc_bf_t (caller: bfc_bf_destroy) */
/* the same, and a copy of the filter stays in HBM behind the returned object until bfc_bf_destroy / a host bfc_bf_insert on it:
 * bfcg_trim_create on the same device adopts that copy instead of uploading 2^(n_shift-3) bytes (`bfc -1`: count.c:153 -> correct.c:556) */
bfc_bf_t *bfcg_export_bloom_resident(bfcg_ctx_t *c, int which);
void bfcg_resident_drop(const void *bf);                   /* drop the HBM copy behind a host filter, if there is one */
bfc_ch_t *bfcg_export_table(bfcg_ctx_t *c);              /* host bfc_ch_t (caller: bfc_ch_destroy) */
/* the same, and a copy of the table stays in HBM behind the returned object until bfc_ch_destroy / a host bfc_ch_insert on it: the first
 * bfcg_kcov_create / bfcg_ec_create on the same device adopts that copy instead of uploading 8 << (l_pre + cshift) bytes (bfc_count ->
 * bfc_correct); a second one uploads.  Without room for the copy the host table alone is returned.  bfcg_resident_drop drops it too. */
bfc_ch_t *bfcg_export_table_resident(bfcg_ctx_t *c);

/* Ingest only, no GPU: parses `fn` (FASTA/FASTQ, plain or gzip) into the batches bfc_count would submit -- kseq's grammar
 * (kseq.h:185-224) and bseq_read's batch boundary (bseq.c:52-76) -- and digests them: out[0] batches, [1] reads, [2] stream positions,
 * [3]/[4] FNV-1a of all sequence / quality streams, [5] FNV-1a of the per-batch read counts, [6] batches parsed by the multi-threaded
 * fast path (uncompressed strict 4-line FASTQ; n_threads = 0 forces the serial parser).  Used to test that both parsers agree. */
int bfc_ingest_digest(const char *fn, uint64_t chunk_size, uint64_t cap, int n_threads, uint64_t out[7]);
/* the same batches as bit planes: direct = 1 written by the FASTQ fast path straight from the mapped file, 0 packed from the byte streams (they
 * must agree word for word: tests/test_ingest.py).  out[0] batches, out[1] positions, out[2..5] FNV-1a of planes 0..3, out[6] batches packed directly */
int bfc_ingest_planes_digest(const char *fn, uint64_t chunk_size, uint64_t cap, int n_threads, int q, int direct, uint64_t out[7]);
/* gzip input (bseq.c:33-50 reads it through one gzread stream): bfc_count inflates a regular .gz file with n_threads threads -- guessed
 * block starts, 16-bit symbols with markers for the unknown 32 KiB window, pieces chained only where one started exactly where its
 * predecessor stopped, CRC-32 / ISIZE of every member checked (bfc_pgz.h); anything it cannot decode goes through gzread.  This runs that
 * inflate alone over `fn` in windows of `window` bytes with compressed chunks of `chunk` bytes: out[0] text bytes, [1] their CRC-32,
 * [2] pieces taken as guessed, [3] pieces decoded again from the chain position, [4] rounds.  0 / -1 not a mappable gzip file / -2 damaged. */
int bfc_pgz_digest(const char *fn, int n_threads, uint64_t chunk, uint64_t window, uint64_t out[5]);

/* Union of the per-GPU tables of an owner-computes run (disjoint key sets: the union is the reference's table); order stamps travel
 * along, so that bfc_ch_dump of the union is byte-identical to `bfc -t1 -d` across GPUs too.  NULL if k / l_pre differ. */
bfc_ch_t *bfc_ch_union(const bfc_ch_t *const *tabs, int n);

/* L1 form of a host table: sizes[2^l_pre]; slots (may be NULL) = per sub-table sorted */
int      bfc_ch_get_lpre(const bfc_ch_t *ch);
uint64_t bfc_ch_export_sorted(const bfc_ch_t *ch, uint32_t *sizes, uint64_t *slots);

/* Trim pass of `bfc -1` (BASELINE config c5: bloom query-only kernel): replaces, for a whole batch of reads, the per-read
 * max_streak (correct.c:478-497: one bfc_bf_get per k-mer, bbf.c:47-63) and the keep/trim rule (correct.c:557-569).
 * `bf` is the filter bfc_count returned in filter mode; it is uploaded once.  The stream is the batch format of PART 2
 * (one separator byte after each read); off[n_reads+1] are the reads' stream offsets.  start[r] = -1: read dropped;
 * otherwise keep bases [start[r], end[r]) -- exactly correct.c's memmove window. */
typedef struct bfcg_trim bfcg_trim_t;
bfcg_trim_t *bfcg_trim_create(int k, const bfc_bf_t *bf, int device, uint64_t max_pos, uint64_t max_reads);
void bfcg_trim_destroy(bfcg_trim_t *t);
int bfcg_trim_batch(bfcg_trim_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos, const uint64_t *h_off, uint64_t n_reads,
                    float min_frac, int32_t *start, int32_t *end);
float bfcg_trim_last_ms(bfcg_trim_t *t);   /* GPU time of the last batch's query + streak kernels (HIP events) */
int bfcg_trim_adopted(bfcg_trim_t *t);     /* 1 if the filter was found resident in HBM (no upload) */
void *bfcg_trim_dev_seq(bfcg_trim_t *t);   /* the context's device staging buffer (max_pos bytes) */

/* k-mer coverage of the corrector: replaces, for a whole batch of reads, bfc_ec_kcov (correct.c:96-117) as
 * bfc_ec1 first calls it on the unmodified read (correct.c:403) -- one bfc_ch_kmer_occ (htab.c:94-99) per k-mer.  The table
 * is uploaded once from the host bfc_ch_t that bfc_count / bfc_ch_restore returned (bfcg_kcov_create), or borrowed in place
 * from a counting context (bfcg_kcov_attach: no export).  Output: one u16 per stream position, packed like ecbase_t's
 * bit-fields (correct.c:17): lcov (bits 0-5) | hcov (6-11) | solid_end (12) | high_end (13); 0 for separators.
 * min_occ is opt->min_cov (bfc.h:20, correct.c:403). */
typedef struct bfcg_kcov bfcg_kcov_t;
bfcg_kcov_t *bfcg_kcov_create(const bfc_ch_t *ch, int device, uint64_t max_pos);
bfcg_kcov_t *bfcg_kcov_attach(bfcg_ctx_t *ctx, uint64_t max_pos);
void bfcg_kcov_destroy(bfcg_kcov_t *t);
int bfcg_kcov_batch(bfcg_kcov_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos, int min_occ, uint16_t *out);
float bfcg_kcov_last_ms(bfcg_kcov_t *t);   /* GPU time of the last batch's two kernels (HIP events) */
void *bfcg_kcov_dev_seq(bfcg_kcov_t *t);   /* device staging buffer for the stream (max_pos bytes) */
void *bfcg_kcov_dev_out(bfcg_kcov_t *t);   /* device result of the last batch (max_pos u16) */

/* BFC's error correction (bfc_ec1, correct.c:388-476) for whole batches of reads (bfcg_ec.hip): the k-mer coverage pass above, then one
 * read per lane of a persistent grid (bfcg_ec1.h: the per-read search, shared with the host).  Output is byte-identical to the reference's
 * worker_ec / bfc_ec_cb in table mode (opt->filter_mode off) for any other option, refine_ec included.  The table is uploaded once from
 * the host bfc_ch_t, which must outlive the object: reads the device cannot hold (heap or stack full, longer than its bound) are corrected
 * after the batch by the host instance, bfcg_ec1_host, on that table.  BFCG_EC_HEAP / BFCG_EC_STACK / BFCG_EC_LMAX set the device's heap
 * and stack entries and read length per lane (results do not depend on them).
 *   bfcg_ec_batch: the stream and off[] as bfcg_trim_batch (off[n_reads] = n_pos); qual NULL: no quality strings.  seq / qual are
 *   rewritten in place as bfc_ec1 does (reads with ec_code != 0 untouched); aux / aux2 as worker_ec packs them (correct.c:552-553).
 *   bfcg_ec1_host: one NUL-terminated read on the host; mode = bfc_ch_hist(ch, ...).
 * Refinement (`bfc -R`, opt->refine_ec set at bfcg_ec_create; bfcg_ec_batch then refuses the corrector): bases are read from the quality
 * string where bfc wrote them there (bfc_seq_conv's b_from_q, correct.c:31; quality bytes <= 33 decode to N), and every read carries
 * the stats of its earlier correction, ori_aux / ori_aux2, packed as aux / aux2 (worker_ec's ori_st, correct.c:542-546; all zero for a
 * read that had none).  Each read given is corrected -- skipping the reads whose stats say so (ec_code 0, max_heap < 50) is the caller's
 * job, as worker_ec returns before bfc_ec1.  aux2's rf_code (bits 8-9) is 3 for a corrected read, 2 where the earlier stats stand
 * (correct.c:438-442: the read untouched, aux / aux2 = ori with rf_code 2), 1 where ec_code != 0.
 *   bfcg_ec_batch_refine: bfcg_ec_batch with ori_aux[n_reads] / ori_aux2[n_reads].
 *   bfcg_ec1_host_refine: bfcg_ec1_host with one read's earlier stats (bfcg_ec1_host refuses refine_ec).
 *   bfcg_ec_parse_stats: worker_ec's test and parse_stats (correct.c:517-531, 542-543) on a read's comment: returns 1 and the stats
 *   packed as above (rf_code 1, every field cut to ecstat_t's width as its bit-fields do: max_heap 300 is 44) if it starts with "ec:Z:",
 *   else 0 (aux / aux2 untouched).  It never reads past the comment's NUL: fields missing at its end are 0, where the reference reads on.
 * A corrector on a counting context's table, with no host table (bfcg_ec_attach): bfcg_kcov_attach's contract -- a table-mode context, which
 * is drained and whose segments are converted to the host's layout; it must outlive the corrector and must not count meanwhile.  opt->k
 * must be the context's k, opt->filter_mode is refused (both before anything is drained), refine_ec is honoured as above.  Nothing is
 * exported: the mode is bfc_ch_hist's, from one pass over the table on the device at attach, and the reads the device cannot hold are
 * corrected by a second kernel over the list of those reads whose capacities grow 4x per round until none is left (bfcg_ec_retry_reads
 * counts them; bfcg_ec_host_reads stays 0; bfcg_ec_last_ms / _last_lookups include those launches).  If the device cannot allocate what
 * a read needs the batch fails with an error that names the read, and seq / qual are as they were given. */
typedef struct bfcg_ec bfcg_ec_t;
bfcg_ec_t *bfcg_ec_create(const bfc_ch_t *ch, const bfc_opt_t *opt, int device, uint64_t max_pos, uint64_t max_reads);
bfcg_ec_t *bfcg_ec_attach(bfcg_ctx_t *ctx, const bfc_opt_t *opt, uint64_t max_pos, uint64_t max_reads);
int   bfcg_ec_batch(bfcg_ec_t *e, uint8_t *seq, uint8_t *qual, uint64_t n_pos, const uint64_t *off, uint64_t n_reads, uint32_t *aux, uint32_t *aux2);
void  bfcg_ec_destroy(bfcg_ec_t *e);
float bfcg_ec_last_ms(bfcg_ec_t *e);          /* GPU time of the last batch: coverage + correction kernels (HIP events) */
uint64_t bfcg_ec_host_reads(bfcg_ec_t *e);    /* reads the host fallback corrected, since creation */
uint64_t bfcg_ec_last_lookups(bfcg_ec_t *e);  /* table lookups of the last batch's correction kernel (the coverage pass adds one per k-mer) */
uint64_t bfcg_ec_retry_reads(bfcg_ec_t *e);   /* reads the retry kernel corrected, since creation (0 on a corrector made by bfcg_ec_create) */
int   bfcg_ec_adopted(bfcg_ec_t *e);          /* 1 if the table was found resident in HBM (bfcg_export_table_resident: no upload) */
int   bfcg_ec1_host(const bfc_ch_t *ch, const bfc_opt_t *opt, int mode, char *seq, char *qual, uint32_t *aux, uint32_t *aux2);
int   bfcg_ec_batch_refine(bfcg_ec_t *e, uint8_t *seq, uint8_t *qual, uint64_t n_pos, const uint64_t *off, uint64_t n_reads,
                           const uint32_t *ori_aux, const uint32_t *ori_aux2, uint32_t *aux, uint32_t *aux2);
int   bfcg_ec1_host_refine(const bfc_ch_t *ch, const bfc_opt_t *opt, int mode, char *seq, char *qual, uint32_t ori_aux, uint32_t ori_aux2,
                           uint32_t *aux, uint32_t *aux2);
int   bfcg_ec_parse_stats(const char *comment, uint32_t *aux, uint32_t *aux2);

/* The count table read out where it lies in HBM (bfcg_kmers.hip): what the reference's hash2cnt (hash2cnt.c) prints from a dump.  The table
 * is uploaded once from a host bfc_ch_t (bfcg_kmers_create) or borrowed in place from a table-mode counting context (bfcg_kmers_attach,
 * with bfcg_kcov_attach's contract: the context is drained, nothing is exported, it must outlive the object and must not count meanwhile).
 *   bfcg_kmers_info       out[0] k, out[1] l_pre (2^l_pre sub-tables), out[2] log2 slots per sub-table
 *   bfcg_kmers_hist       bfc_ch_hist (htab.c:110) in one streaming pass: returns the mode (largest bin with i >= 3, -1 if none), -2 on error
 *   bfcg_kmers_sub_sizes  sizes[2^l_pre]: the keys of every sub-table (hash2cnt -s)
 *   bfcg_kmers_hist_sizes both from ONE pass (each of the two calls above streams the whole table and drops the other half of what the
 *                         kernel computed: nothing is cached, because an attached table may change between calls); cnt / high together,
 *                         or sizes, may be NULL; returns as bfcg_kmers_hist (-1 also when no histogram was asked for)
 *   bfcg_kmers_list       the k-mers of sub-tables [sub_lo, sub_hi) with count >= min_cnt and min(count, 63) - high >= min_diff (hash2cnt's
 *                         -m / -d): y[2 i], y[2 i + 1] = the two bit planes of k-mer i (bit l = the base l from the 3' end, low / high code
 *                         bit, of the strand the hash chose), cnt_high[i] = high << 8 | count.  Sub-tables ascending, unordered inside one.
 *                         0: *n k-mers written; 1: cap too small, nothing written, *n = the number needed; -1: error -- k > 37, whose
 *                         keys do not hold the whole hash (hash2cnt.c:37; sizes and histogram work for every k)
 *   bfcg_kmers_last_ms    GPU time of the last call's kernels (HIP events)
 *   bfcg_kmer_decode_host one slot of sub-table `sub` decoded on the host by the same code (bfcg_kdec.h), checked against the forward
 *                         hash; -1 for k > 37
 *   bfcg_kmer_2str        the planes as text (k + 1 bytes), kmer.h:97
 *   bfcg_kmers_format / _format_sizes   hash2cnt's lines "%s\t%d\t%d\n" (at most k + 8 bytes each) / "%d\n" (at most 11): bytes written
 * The other direction (bfcg_lookup.hip): the table asked by k-mer, on either form of the object, for every k up to 63 (a lookup needs the
 * forward hash only).  A k-mer is given as a listing hands it out, y[2 i], y[2 i + 1], on either strand; bits at and above k are ignored.
 *   bfcg_kmers_lookup     out[i] = bfc_ch_kmer_occ (htab.c:94) of k-mer i: high << 8 | count, -1 if the table does not hold it; *n_found
 *                         (may be NULL) = the k-mers found.  y / out are host memory; n above the object's staging capacity (2^22 k-mers,
 *                         or BFCG_LOOKUP_CAP in the environment when the object is made) is cut into pieces inside the call, and
 *                         bfcg_kmers_last_ms then is the time of all its kernels.  For even k the reference's strand rule (kmer.h:81)
 *                         does not always choose the same strand from both sides: a k-mer and its reverse complement may then differ
 *   bfcg_kmers_profile    the stream is the batch format of PART 2, exactly one of h_seq / d_seq as in bfcg_kcov_batch; out[p] (host) for
 *                         the k-mer ENDING at position p: its bfc_ch_kmer_occ value, -1 if absent, -2 where no k-mer ends (separators,
 *                         the first k - 1 bases of a read, a window holding a byte that is not ACGTacgt)
 * A read set screened against the table (bfcg_readstats.hip): the profile reduced per read on the device, 32 bytes per read of output
 * instead of 2 bytes per base.
 *   bfcg_kmers_read_stats the stream and off[n_reads + 1] as bfcg_trim_batch / bfcg_ec_batch take them (exactly one of h_seq / d_seq;
 *                         read r is positions [off[r], off[r + 1] - 1), the last byte of its span the separator; off[n_reads] = n_pos);
 *                         out (host) gets eight int32 per read.  With v the profile's value at a position and c = v & 0xff if v >= 0,
 *                         else 0, a position is DEFINED if v != -2 and SOLID if v >= 0 and c >= min_cov:
 *                           0 n_kmers    defined positions          1 n_present  positions with v >= 0       2 n_solid
 *                           3 the sum of c over the defined positions (a 32-bit word: int32_t holds its bits)
 *                           4 min | median << 8 | max << 16 of c over the defined positions, the median the element (n_kmers - 1) >> 1
 *                             of the sorted values (the lower median); 0 if n_kmers = 0
 *                           5 streak     the k-mers of the longest run of consecutive solid positions (anything else ends a run), of
 *                                        equally long runs the LAST, as max_streak keeps it (correct.c:494)
 *                           6 start, 7 end   that run's bases [start, end) counted from the read's first: its first k-mer ends at
 *                                        position start + k - 1, end = start + streak + k - 1; both -1 if streak = 0
 *                         This is `bfc -1`'s question (correct.c:478-497) asked of the exact table with a coverage threshold.  Refused
 *                         before anything is launched, out untouched, the message naming the read: min_cov outside [1, 255], offsets
 *                         that do not ascend, off[n_reads] != n_pos, a read of 2^24 or more positions (word 3 stays inside 32 bits).
 *                         n_reads = 0 or n_pos = 0: 0, nothing written.  On either form of the object, for every k up to 63;
 *                         bfcg_kmers_last_ms covers both kernels.  One wavefront walks one read: made for reads of 50 to 300 bases; a
 *                         megabase contig comes out right, at the pace of one wave.
 * Two tables compared and merged (bfcg_tabcmp.hip).  a and b are two objects of either form, in any mix, of equal k and l_pre on one
 * device (cshift may differ; a == b is allowed).  Anything else -- NULL, another k, another l_pre, another device -- is refused before
 * any launch with a message, and the objects stay usable.  Equal k and l_pre mean equal sub-table index and key, so nothing is hashed or
 * decoded and every k up to 63 works, except where planes are handed out.
 *   bfcg_kmers_joint_hist joint[i * 256 + j] = the keys with count i in a and j in b, 0 = absent (joint[0] is 0);
 *                         n = { shared, only in a, only in b }.  0, or -1 on error; bfcg_kmers_last_ms(a) is the time of its two launches
 *   bfcg_kmers_list_vs    bfcg_kmers_list on a -- the same order, planes, cap / *n protocol, return codes and refusal of k > 37 -- with a
 *                         slot kept only if its count in b (0 where b does not hold the key) lies in [other_min, other_max]: [0, 0] lists
 *                         what is private to a, [1, 255] what is shared, [0, 255] everything.  other[i] = what bfcg_kmers_lookup would
 *                         answer for k-mer i in b: -1, or high << 8 | count
 *   bfcg_kmers_union      a new object that owns its table: a's k and l_pre, every key of either input, counts and high counts of a key in
 *                         both added and saturated at 255 and 63 (bfc_ch_union, htab.c:74-79).  Its cshift is the smallest value >= 2
 *                         with 2^(l_pre + cshift) >= 2 (keys_a + keys_b) and 2^cshift >= the largest size_a[s] + size_b[s], taken from one
 *                         size pass over each input: no region can overflow, nothing is retried.  The order inside a sub-table is
 *                         unspecified.  NULL on error; bfcg_kmers_last_ms(result) covers the size passes and the fill
 *   bfcg_kmers_export     a host bfc_ch_t from any bfcg_kmers_t (one copy, no order stamps; *n_keys, which may be NULL, = its keys): to be
 *                         dumped, handed to bfcg_ec_create, asked with bfc_ch_get; the caller destroys it.  NULL on error
 *   bfcg_kmers_format_vs  a piece of bfcg_kmers_list_vs as lines "%s\t%d\t%d\t%d\t%d\n": k-mer, count, high, count in b, high in b (0 0 for
 *                         an absent one); at most k + 16 bytes each
 * The table read as a de Bruijn graph (bfcg_graph.hip), on either form of the object.  With m = 2^k - 1 and a base c in 0..3 (A C G T):
 *   succ(x, c)  both planes shifted left by one and masked with m, bit 0 of the low plane c & 1, of the high plane c >> 1: the base at
 *               the 5' end falls out, c is the new base at the 3' end
 *   pred(x, c)  both planes shifted right by one, bit k - 1 of the low plane c & 1, of the high plane c >> 1
 * The VALUE of a k-mer is what bfcg_kmers_lookup answers for it on the strand as constructed: -1, or high << 8 | count (for even k the
 * caveat stated there holds for neighbours as for any other k-mer: nothing is special-cased).  A k-mer is PRESENT at min_cnt if its
 * value is >= 0 and value & 0xff >= min_cnt.  A NODE is a slot of the table with count >= min_cnt, on the strand the decode yields (the
 * one a listing prints); its out-degree o is the number of c with succ(x, c) present, its in-degree i that of pred(x, c).  Both refer
 * to the stored strand: a node stored as its reverse complement has the two swapped, and a caller who wants a strand-free view folds
 * cell (o, i) with (i, o).  Every call sets bfcg_kmers_last_ms; every refusal below happens before any launch, leaves the outputs
 * untouched and the object usable, and puts a message in bfcg_last_error.  min_cnt outside [1, 255] is refused wherever it is taken.
 *   bfcg_kmers_neighbors  y as for bfcg_kmers_lookup, every k up to 63; out (host) int16_t[8 n]: out[8 i + c] = the value of
 *                         succ(x_i, c), out[8 i + 4 + c] = that of pred(x_i, c).  16 bytes in and 16 bytes out per k-mer: the eight
 *                         neighbours are built in registers.  n above the lookup's staging capacity is cut inside the call
 *   bfcg_kmers_graph_census  one streaming pass: deg[5 o + i] = the nodes with out-degree o and in-degree i.  k > 37 is refused with the
 *                         listing's message (a node has to be decoded)
 *   bfcg_kmers_list_graph bfcg_kmers_list -- the same order, planes, cap / *n protocol, return codes and refusal of k > 37 -- of the nodes
 *                         whose cell is named by cell_mask (bit 5 o + i; 0, or a bit at or above 2^25, is refused), with nb[j] per
 *                         k-mer: bit c set if succ by c is present, bit 4 + c if pred by c is.  Tips are the cells where exactly one
 *                         of o, i is 0, isolated k-mers cell (0, 0), branching ones o >= 2 or i >= 2, simple ones cell (1, 1)
 *   bfcg_kmers_extend     the unambiguous path to the right of each of n seeds, every k up to 63: bases (host) uint8_t[n * max_len]
 *                         gets 'A' 'C' 'G' 'T', zero beyond a seed's length; len_stop int32_t[2 n] the length and the stop code.  The
 *                         rule, in order: a seed that is not present stops with code 4 and length 0; else repeat: the length equals
 *                         max_len: code 0; o = the present successors of the current k-mer: o = 0 code 1, o >= 2 code 2; nxt = the one
 *                         present successor: two or more present predecessors, counted on nxt as constructed: code 3; nxt equals the
 *                         seed's planes: code 5; else its base is appended and the walk goes on from nxt.  max_len outside [1, 65535]
 *                         is refused; n * max_len above the staging room (16 bytes per k-mer of the lookup's capacity, one path at
 *                         least) is cut inside the call.  One lane walks one seed with sequential probes, as the corrector's kernel
 *                         walks a read: made for thousands of seeds and paths of a few hundred bases, not for one long contig.  A walk
 *                         to the left is the same call on the reverse complement
 *   bfcg_kmer_revcomp     the planes of the reverse complement (no GPU); -1 for k outside [1, 63]
 * The compacted graph (bfcg_unitigs.hip): every maximal non-branching path of the graph exactly once, on either form of the object.
 * Only ODD k <= 37 is served.  For even k the reference's strand rule (kmer.h:81) leaves some k-mers undecided, a k-mer and its reverse
 * complement can be two keys and there is no strand-free graph to compact; for k > 37 a node cannot be decoded.  Both are refused before
 * any launch with a message, as is min_cnt outside [1, 255]; a refusal leaves every output untouched and the object usable.
 *   NODES       for odd k, x and rc(x) (its reverse complement) have one slot and one value.  A node is a slot with count >= min_cnt.  It
 *               has two oriented k-mers, x and rc(x), and two sides: its right side is where succ(x, .) leaves, its left side is the
 *               right side of rc(x)
 *   link(x)     for an oriented k-mer x, with o = the present successors of x, the rules in this order:
 *                 1. o is empty: no link, stop code 1
 *                 2. o has more than one: no link, stop code 2
 *                 3. y is the single one; two or more predecessors of y are present, counted on y as constructed: no link, stop code 3
 *                 4. y == x or y == rc(x) -- the only way on leads back into the node itself: no link, stop code 6
 *                 5. otherwise link(x) = y
 *               Codes 1 to 3 are bfcg_kmers_extend's; 6 is new (extend keeps its own rule: it walks through a hairpin and reports a
 *               seed's self-loop as 5).  A side without a link is OPEN and carries its stop code
 *   UNITIGS     for odd k, link(x) = y holds exactly when link(rc(y)) = rc(x): every side has at most one partner, and the components are
 *               simple paths and simple cycles of nodes.  Each component is one unitig, of n k-mers and k + n - 1 bases
 *   a path      starts at the oriented k-mer s whose left side is open (link(rc(s)) is none); each link adds one base, up to the oriented
 *               k-mer e whose right side is open.  Read from the other end it is the reverse complement, from rc(e) to rc(s).  The
 *               spelling emitted is the one whose first k-mer is smaller as text (A < C < G < T, compared from the 5' end): s against
 *               rc(e), which cannot be equal for odd k.  A node with both sides open is a unitig of one k-mer, spelled on the smaller of
 *               its two strands
 *   a cycle     has every side linked.  It is spelled from its smallest oriented k-mer over both strands, once round: k + n - 1 bases,
 *               the last k - 1 of which are the first k - 1 of the next lap
 *               So: an isolated k-mer is one unitig of k bases with ends (1, 1); the k-mer of a run of A's, whose only successor is
 *               itself, is one unitig "AAA...A" with ends (6, 6); a node whose only successor on one side is its own reverse
 *               complement (a hairpin, u P comp(u) with P a reverse palindrome of k - 1 bases) has code 6 on that side, and a path
 *               that runs into it ends there with 6; a cycle has ends 0 and the cycle bit
 *   bfcg_kmers_unitigs    seq (host) gets 'A' 'C' 'G' 'T', the unitigs back to back, unitig i at [off[i], off[i + 1]); off has n[0] + 1
 *                         entries; n_kmers[i] and cnt_sum[i] = its k-mers and the sum of their counts; ends[i] = the stop code of the
 *                         emitted spelling's left side | that of its right side << 3 | 64 for a cycle (whose codes are 0).  n[0] = the
 *                         unitigs, n[1] = the bases.  The cap protocol is the listing's -- 0: written; 1: seq_cap < n[1] or n_cap <
 *                         n[0], nothing is written, n[] holds what is needed (a first call with caps of 0 sizes the second); -1: refused,
 *                         or an error.  The order of the unitigs is unspecified (it is that of the table's slots: paths by the slot of
 *                         the end that emits, then cycles); the SET does not depend on the table's layout, so an attached table and the
 *                         upload of its export give the same.  bfcg_kmers_last_ms covers all its kernels.
 *                         How: a listing pass (bfcg_kmers_list's two kernels, the predicate = a node with an open side; both link rules
 *                         are evaluated per node, up to 16 probes) yields the path ends; one lane per end and open side walks to the far
 *                         end, counts, decides which end emits and marks every node it passes in a bitmap of one bit per slot; the
 *                         nodes left unmarked are the cycles' and are collected by one streaming pass; one lane per such node walks its
 *                         cycle and gives up at the first oriented k-mer smaller than its own smaller strand, so only the cycle's
 *                         smallest completes the lap; a scan of the winners' lengths; a fill walk that writes the bases.  A walk kernel
 *                         takes at most 2^22 starts a launch (BFCG_UNITIG_CAP in the environment when the object is made).  Device
 *                         memory: one bit per slot, 56 bytes per side of a path end and per cycle node, and the output itself.  A walk is one
 *                         lane's sequential probes: expected work is near-linear on ordinary sequence (a cycle node gives up after about
 *                         ln n steps on average), but one unitig of millions of k-mers -- a path, or a cycle's leader on its lap -- runs
 *                         at the pace of one lane, the caveat bfcg_kmers_read_stats makes for a megabase contig
 * The unitigs linked (bfcg_unitigs.hip): the compacted graph with its edges, out of one call -- the order of the unitigs is unspecified
 * and the cycles are placed by an atomic counter, so a second call need not number them alike.  The domain is that of bfcg_kmers_unitigs
 * -- odd k <= 37, min_cnt in [1, 255], l_pre + cshift <= 31 --, and nodes, link(x), unitigs, stop codes and the spelling emitted are
 * exactly those defined above.
 *   ORIENTED UNITIG  (u, 0) is unitig u as emitted, (u, 1) its reverse complement.  Its first and last oriented k-mers are the first
 *               and last k bases of that spelling; for a cycle the spelling is the emitted k + n - 1 bases, so its last k-mer is the
 *               lap's last node
 *   EDGE        (u, o) -> (v, p) by base c exists when succ(x, c) is present at min_cnt, x being the last oriented k-mer of (u, o);
 *               (v, p) is the oriented unitig whose first oriented k-mer succ(x, c) is.  That is well defined: the left side of
 *               succ(x, c) is always open, by the symmetry of link stated under UNITIGS (if x has several successors, each of them
 *               has code 3 or 2 to its left; if the single one has several predecessors, it has code 2 to its left; under code 6 it is
 *               x or rc(x), whose side this is).  The last k - 1 bases of (u, o) are the first k - 1 of (v, p)
 *   PER END     a side with code 1 has no edge, with code 2 two to four, with code 3 exactly one; with code 6 exactly one, whose target
 *               is u itself -- (u, o) for a self-loop such as the A-run, (u, 1 - o) for a hairpin; a cycle has exactly one per side, to
 *               (u, o) itself, by the base at position k - 1 of that spelling
 *   MIRROR      if (u, o) -> (v, p) is an edge, so is (v, 1 - p) -> (u, 1 - o).  Both appear; an edge that is its own mirror (the
 *               hairpin's) appears once
 *   bfcg_kmers_unitig_graph  the first five outputs, the cap protocol (0 / 1 / -1), the refusals and their messages are
 *                         bfcg_kmers_unitigs's.  links has 8 entries per unitig: links[8 u + 4 o + c] = v << 1 | p for the edge from
 *                         (u, o) by base c (A C G T = 0..3), -1 if there is none; u and v index this call's own outputs.  links ==
 *                         NULL with n_cap > 0 is refused like the other buffers.  n[2] = the entries >= 0, set only on return 0 (the
 *                         sizing call leaves it alone: the edges are found after the fill); on return 1 or -1 links is untouched.
 *                         The set {(spelling of u, o, c, spelling of v, p)} does not depend on the table's layout.  The input is never
 *                         written.  bfcg_kmers_last_ms covers every kernel of the call.
 *                         How: bfcg_kmers_unitigs's passes, whose fill walk also leaves the planes of each unitig's first and last
 *                         k-mer (32 bytes per unitig) and enters the table slots of a path's two end nodes into an end map -- open
 *                         addressing with linear probing over 64-bit words slot << 32 | u, inserted by a compare-and-swap on an empty
 *                         word, the smallest power of two >= 4 x the paths, so never more than half full (BFCG_LINK_MAP_MIN=1 in the
 *                         environment when the object is made: the smallest power of two above 2 x the paths, for tests); cycles enter
 *                         nothing, no edge leads into one from outside.  Then one lane per (unitig, side), at most BFCG_UNITIG_CAP a
 *                         launch: the four successors of the side's last k-mer probed at once, and per present one its slot, the
 *                         map's unitig for it, and p = 0 if it is that unitig's first k-mer, 1 if the reverse complement of its last.
 *                         A miss, or a successor that is neither, fails the call: the table changed under the call.  Device memory
 *                         on top of bfcg_kmers_unitigs's: the map, and 96 bytes per unitig
 * The graph cleaned (bfcg_clip.hip): tips and islands clipped into a new table, on either form of the object.  The domain is that of
 * bfcg_kmers_unitigs -- odd k <= 37, min_cnt in [1, 255] --, and nodes, link(x), unitigs and stop codes are exactly those defined above.
 *   DEAD, ATTACHED  stop codes 1 and 6 are DEAD (nothing lies beyond but the node itself), 2 and 3 are ATTACHED
 *   CLIPPABLE   a unitig of the graph at min_cnt is clippable at (max_tip, max_mean) if it is a path, not a cycle; n_kmers <= max_tip;
 *               and cnt_sum <= max_mean * n_kmers (integer arithmetic; max_mean = 255 switches this rule off)
 *   TIP, ISLAND a clippable unitig is a tip if one end is DEAD and the other ATTACHED, an island if both ends are DEAD.  A unitig with
 *               both ends ATTACHED is never touched: bubbles stay
 *   a ROUND     decides on its input graph only and removes all k-mers of all tips at once; with BFCG_CLIP_ISLANDS in flags those of the
 *               islands too.  Unitigs are node-disjoint, so the result does not depend on any order.  Its output is a table of the
 *               surviving NODES: slots with count < min_cnt are dropped as well; key, count and high count of a survivor are unchanged.
 *               Rounds repeat on the previous round's output until one removes nothing or max_rounds rounds have run.  max_rounds = 0
 *               gives the table of the nodes at min_cnt and nothing else: a threshold filter
 *   bfcg_kmers_clip       a new object that owns its table, as bfcg_kmers_union's does (its keys are known): the input's k and l_pre; its
 *                         cshift follows the union's rule applied to the survivors, the smallest value >= 2 with 2^(l_pre + cshift) >=
 *                         2 * keys and 2^cshift >= the largest per-sub-table survivor count; the order inside a sub-table is
 *                         unspecified.  An empty result (every node removed) is a valid table with zero keys.  The input is never
 *                         written: an attached input stays attached and unchanged.  *n_rounds = the rounds that ran and removed
 *                         something; stats (may be NULL, else room for 3 * max_rounds words) gets three words per such round: unitigs
 *                         removed, k-mers removed, keys left.  Refused before any launch with a message, the outputs untouched and the
 *                         object usable: even k and k > 37 (the unitigs' messages), min_cnt outside [1, 255], max_tip outside
 *                         [1, 65535], max_mean outside [1, 255], max_rounds outside [0, 64], unknown flag bits.  NULL on refusal or
 *                         error; bfcg_kmers_last_ms(result) covers every kernel of the call.
 *                         How, per round: the unitigs' listing pass yields the nodes with an open side; one lane per DEAD side walks
 *                         away from the dead end for at most max_tip k-mers, summing counts -- a lane that has not met an open side by
 *                         then stops, so no lane walks further than max_tip steps whatever the graph holds (the one-lane-per-long-unitig
 *                         caveat of bfcg_kmers_unitigs does not apply); of an island's two lanes the one the unitigs' spelling rule picks
 *                         goes on; a lane that removes walks the same steps again and sets one bit per slot in a bitmap; one streaming
 *                         pass counts the survivors per sub-table, a second upserts them into the new table.  Intermediate tables are
 *                         freed as soon as the next one stands.  Device memory: one bit per slot, the listing, and the tables of two rounds
 * Simple bubbles popped (bfcg_pop.hip): of two parallel unitigs between one k-mer and another -- a substitution error seen twice, a
 * heterozygous SNP, a short indel -- the weaker one is removed into a new table, on either form of the object.  The domain is
 * bfcg_kmers_clip's -- odd k <= 37, min_cnt in [1, 255] --, and nodes, link(x), unitigs, stop codes and the spelling emitted are exactly
 * those defined above.
 *   ARM         a unitig of the graph at min_cnt that is a path, not a cycle, with stop code 3 on both ends.  Oriented from its first
 *               oriented k-mer s to its last e: s has exactly one present predecessor p, its ENTRY, and e exactly one present successor
 *               q, its EXIT (both follow from code 3).  Read from the other end the entry is rc(q) and the exit rc(p)
 *   SIMPLE BUBBLE  an arm U and a second unitig V such that: p has exactly two present successors, s and s'; q has exactly two present
 *               predecessors; s' != rc(e), so the sibling is not U read backwards (the inverted case q == rc(p)); V, oriented to
 *               start at s', is an arm whose exit is the same oriented k-mer q; n_kmers(U) <= max_arm and n_kmers(V) <= max_arm;
 *               |n_kmers(U) - n_kmers(V)| <= max_diff.  V is unique given U, the relation is symmetric, and U and V share no node
 *   LOSER       the arm with the lower mean count: cnt_sum(U) * n_kmers(V) < cnt_sum(V) * n_kmers(U), in 64-bit integers; on a tie the
 *               arm whose emitted spelling's first k-mer is larger as text.  The loser is removed only if cnt_sum <= max_mean *
 *               n_kmers (max_mean = 255 switches this rule off); if it fails that, neither arm goes
 *   a ROUND     as bfcg_kmers_clip's: it decides on its input graph only and removes the losers of all simple bubbles at once.  Arms of
 *               different bubbles are node-disjoint, so the result does not depend on any order.  Its output is the table of the
 *               surviving nodes at min_cnt; key, count and high count of a survivor are unchanged.  Rounds repeat on the previous
 *               round's output until one removes nothing or max_rounds rounds have run.  max_rounds = 0 is the threshold filter,
 *               identical to bfcg_kmers_clip's
 *   not touched, deliberately: a site with three or more branches; two variants closer than k that come from different reads (their
 *               arms interlock: beside each lies a path that the other cuts, not an arm); an arm beside a direct edge p -> q (the edge
 *               is no unitig); the inverted case.  A bubble nested inside another's arm is popped in one round and the outer one in the
 *               next, once the arm it sat in is one unitig
 *   bfcg_kmers_pop        a new object that owns its table, word for word as bfcg_kmers_clip's: the input's k and l_pre, cshift by the
 *                         union's rule on the survivors, the order inside a sub-table unspecified; an empty result is a valid table;
 *                         the input is never written, and an attached input stays attached and unchanged.  *n_rounds = the rounds
 *                         that ran and removed something; stats (may be NULL, else room for 3 * max_rounds words) gets three words per
 *                         such round: bubbles popped, k-mers removed, keys left.  Refused before any launch with a message, the outputs
 *                         untouched and the object usable: even k and k > 37 (the unitigs' messages), min_cnt outside [1, 255],
 *                         max_arm outside [1, 65535], max_diff outside [0, 65535], max_mean outside [1, 255], max_rounds outside
 *                         [0, 64], NULL t or n_rounds.  NULL on refusal or error; bfcg_kmers_last_ms(result) covers every kernel of
 *                         the call.
 *                         How, per round: the unitigs' listing pass yields the nodes with an open side; one lane per side with code 3
 *                         walks its arm for at most max_arm k-mers, summing counts, and goes on only if the far side has code 3 too
 *                         and its own end is the one that emits, so one lane per arm continues; it checks the entry's two successors
 *                         and the exit's two predecessors, walks the sibling's unitig for at most max_arm k-mers to the same exit,
 *                         applies max_diff, the loser rule and max_mean, and if its own arm is to go walks it again and sets one bit
 *                         per slot.  A lane decides its own arm only, so no two lanes mark the same node, and no lane takes more than
 *                         3 * max_arm steps whatever the graph holds.  The marks become the new table by bfcg_kmers_clip's two
 *                         streaming passes (one piece of code for both).  Device memory as for bfcg_kmers_clip
 * Their host twins and the text forms use no GPU:
 *   bfcg_clip_host        bfcg_kmers_clip -- result, stats, refusals -- by the same rule (one piece of code for both) on
 *                         bfcg_kmer_occ_host, over bfc_ch_export_sorted's slots, into a table made at the same cshift rule
 *   bfcg_pop_host         bfcg_kmers_pop -- result, stats, refusals -- by the same rule (one piece of code for both) on
 *                         bfcg_kmer_occ_host, over bfc_ch_export_sorted's slots: every side with code 3 decides on its arm, the removed
 *                         nodes go into a set, and the call fails if the k-mers removed are not the set's size
 *   bfcg_kmer_from_str    the inverse of bfcg_kmer_2str; -1 unless s has exactly k bytes of ACGTacgt
 *   bfcg_kmer_occ_host    bfc_ch_kmer_occ on listing-style planes of either strand (the four planes of bfc_kmer_t built from the two)
 *   bfcg_kmers_occ_host   the same for n k-mers
 *   bfcg_kmers_parse      one k-mer per line (its first field, up to tab / space / CR), '>' lines and empty lines skipped: returns the
 *                         k-mers written to y (at most cap); *bad_line = the 1-based number of the first malformed line, 0 if none
 *   bfcg_lookup_format    the answers to the first n k-mer lines of the same text, "%s\t%d\t%d\n": the k-mer as given, count, high
 *                         (0 0 for an absent one); at most the line's length + 8 bytes each
 *   bfcg_profile_format   n positions of a profile as one line, space-separated counts, '.' for -2, 0 for -1 (at most 4 n + 1 bytes)
 *   bfcg_read_stats_host  bfcg_kmers_read_stats's eight words per read from bfc_ch_kmer_occ on the k-mers rolled from the stream's bytes;
 *                         the same refusals
 *   bfcg_read_stats_format one line per read, "%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n": n_kmers n_present n_solid sum min median max
 *                         streak start end (at most 110 bytes each)
 *   bfcg_neighbors_host   bfcg_kmers_neighbors from eight bfcg_kmer_occ_host per k-mer
 *   bfcg_graph_census_host  bfcg_kmers_graph_census over bfc_ch_export_sorted's slots, decoded by bfcg_kmer_decode_host's code
 *   bfcg_graph_nb_host    the listing's twin, per exported slot: y[2 i], y[2 i + 1] (may be NULL) = the planes of slot i of
 *                         bfc_ch_export_sorted, nb[i] (may be NULL) = its neighbour bits as bfcg_kmers_list_graph gives them, 0 for a slot
 *                         with count < min_cnt; returns the number of slots (with both NULL nothing else), -1 refused (k > 37, min_cnt)
 *   bfcg_extend_host      bfcg_kmers_extend by the same rule (one piece of code for both) on bfcg_kmer_occ_host
 *   bfcg_unitigs_host     bfcg_kmers_unitigs -- outputs, cap protocol, refusals -- by the same link rule (one piece of code for both) on
 *                         bfcg_kmer_occ_host, over bfc_ch_export_sorted's slots: every node walks, no bitmap
 *   bfcg_unitig_graph_host  bfcg_kmers_unitig_graph -- outputs, cap protocol, refusals -- on bfcg_unitigs_host's unitigs: a hash map from
 *                         the first oriented k-mer of every oriented unitig to (u, o), asked for each present successor of every
 *                         oriented unitig's last k-mer; cycles go the same way, there is no end map and no slot.  Everything is made before
 *                         anything is copied out: a return of -1 has written nothing, n[] included */
typedef struct bfcg_kmers bfcg_kmers_t;
bfcg_kmers_t *bfcg_kmers_create(const bfc_ch_t *ch, int device);
bfcg_kmers_t *bfcg_kmers_attach(bfcg_ctx_t *ctx);
void  bfcg_kmers_destroy(bfcg_kmers_t *t);
int   bfcg_kmers_info(bfcg_kmers_t *t, int out[3]);
int   bfcg_kmers_hist(bfcg_kmers_t *t, uint64_t cnt[256], uint64_t high[64]);
int   bfcg_kmers_sub_sizes(bfcg_kmers_t *t, uint32_t *sizes);
int   bfcg_kmers_hist_sizes(bfcg_kmers_t *t, uint64_t cnt[256], uint64_t high[64], uint32_t *sizes);
int   bfcg_kmers_list(bfcg_kmers_t *t, int min_cnt, int min_diff, uint32_t sub_lo, uint32_t sub_hi, uint64_t *y, uint16_t *cnt_high, uint64_t cap, uint64_t *n);
float bfcg_kmers_last_ms(bfcg_kmers_t *t);
int   bfcg_kmer_decode_host(int k, int l_pre, uint32_t sub, uint64_t slot, uint64_t y[2]);
void  bfcg_kmer_2str(int k, const uint64_t y[2], char *buf);
uint64_t bfcg_kmers_format(int k, const uint64_t *y, const uint16_t *cnt_high, uint64_t n, char *buf);
uint64_t bfcg_kmers_format_sizes(const uint32_t *sizes, uint64_t n, char *buf);
int   bfcg_kmers_lookup(bfcg_kmers_t *t, const uint64_t *y, uint64_t n, int16_t *out, uint64_t *n_found);
int   bfcg_kmers_profile(bfcg_kmers_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos, int16_t *out);
int   bfcg_kmer_from_str(int k, const char *s, uint64_t y[2]);
int   bfcg_kmer_occ_host(const bfc_ch_t *ch, const uint64_t y[2]);
void  bfcg_kmers_occ_host(const bfc_ch_t *ch, const uint64_t *y, uint64_t n, int16_t *out);
uint64_t bfcg_kmers_parse(int k, const char *text, uint64_t len, uint64_t *y, uint64_t cap, uint64_t *bad_line);
uint64_t bfcg_lookup_format(const char *text, uint64_t len, const int16_t *occ, uint64_t n, char *buf);
uint64_t bfcg_profile_format(const int16_t *occ, uint64_t n, char *buf);
int   bfcg_kmers_read_stats(bfcg_kmers_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos, const uint64_t *h_off, uint64_t n_reads,
                            int min_cov, int32_t *out);
int   bfcg_read_stats_host(const bfc_ch_t *ch, const uint8_t *seq, uint64_t n_pos, const uint64_t *off, uint64_t n_reads, int min_cov, int32_t *out);
uint64_t bfcg_read_stats_format(const int32_t *out, uint64_t n_reads, char *buf);
int   bfcg_kmers_joint_hist(bfcg_kmers_t *a, bfcg_kmers_t *b, uint64_t joint[256 * 256], uint64_t n[3]);
int   bfcg_kmers_list_vs(bfcg_kmers_t *a, bfcg_kmers_t *b, int min_cnt, int min_diff, int other_min, int other_max,
                         uint32_t sub_lo, uint32_t sub_hi, uint64_t *y, uint16_t *cnt_high, int16_t *other, uint64_t cap, uint64_t *n);
bfcg_kmers_t *bfcg_kmers_union(bfcg_kmers_t *a, bfcg_kmers_t *b);
bfc_ch_t     *bfcg_kmers_export(bfcg_kmers_t *t, uint64_t *n_keys);
uint64_t bfcg_kmers_format_vs(int k, const uint64_t *y, const uint16_t *cnt_high, const int16_t *other, uint64_t n, char *buf);
int   bfcg_kmers_neighbors(bfcg_kmers_t *t, const uint64_t *y, uint64_t n, int16_t *out);
int   bfcg_kmers_graph_census(bfcg_kmers_t *t, int min_cnt, uint64_t deg[25]);
int   bfcg_kmers_list_graph(bfcg_kmers_t *t, int min_cnt, uint32_t cell_mask, uint32_t sub_lo, uint32_t sub_hi, uint64_t *y, uint16_t *cnt_high, uint8_t *nb,
                            uint64_t cap, uint64_t *n);
int   bfcg_kmers_extend(bfcg_kmers_t *t, const uint64_t *y, uint64_t n, int min_cnt, int max_len, uint8_t *bases, int32_t *len_stop);
int   bfcg_kmer_revcomp(int k, const uint64_t y_in[2], uint64_t y_out[2]);
int   bfcg_neighbors_host(const bfc_ch_t *ch, const uint64_t *y, uint64_t n, int16_t *out);
int   bfcg_graph_census_host(const bfc_ch_t *ch, int min_cnt, uint64_t deg[25]);
int64_t bfcg_graph_nb_host(const bfc_ch_t *ch, int min_cnt, uint64_t *y, uint8_t *nb);
int   bfcg_extend_host(const bfc_ch_t *ch, const uint64_t *y, uint64_t n, int min_cnt, int max_len, uint8_t *bases, int32_t *len_stop);
int   bfcg_kmers_unitigs(bfcg_kmers_t *t, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                         uint64_t n_cap, uint64_t n[2]);
int   bfcg_unitigs_host(const bfc_ch_t *ch, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                        uint64_t n_cap, uint64_t n[2]);
int   bfcg_kmers_unitig_graph(bfcg_kmers_t *t, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                              int64_t *links, uint64_t n_cap, uint64_t n[3]);
int   bfcg_unitig_graph_host(const bfc_ch_t *ch, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                             int64_t *links, uint64_t n_cap, uint64_t n[3]);
enum { BFCG_CLIP_ISLANDS = 1 };
bfcg_kmers_t *bfcg_kmers_clip(bfcg_kmers_t *t, int min_cnt, int max_tip, int max_mean, int flags, int max_rounds,
                              uint64_t *stats /* 3 per round: unitigs removed, k-mers removed, keys left */, int *n_rounds);
bfc_ch_t     *bfcg_clip_host(const bfc_ch_t *ch, int min_cnt, int max_tip, int max_mean, int flags, int max_rounds, uint64_t *stats, int *n_rounds);
bfcg_kmers_t *bfcg_kmers_pop(bfcg_kmers_t *t, int min_cnt, int max_arm, int max_diff, int max_mean, int max_rounds,
                             uint64_t *stats /* 3 per round: bubbles popped, k-mers removed, keys left */, int *n_rounds);
bfc_ch_t     *bfcg_pop_host(const bfc_ch_t *ch, int min_cnt, int max_arm, int max_diff, int max_mean, int max_rounds, uint64_t *stats, int *n_rounds);

/* unit-test hooks: K1 only.  out = 3 u64 per position: y0, y1, flags (bit0 k-mer ends here, bit1 high) */
int bfcg_hash_positions(bfcg_ctx_t *c, const uint8_t *h_seq, const uint8_t *h_qual, uint64_t n_pos, uint64_t *out);
/* per-position seen flags of the last batch (debug_seen): 0 none, 1 not seen, 2 seen */
int bfcg_seen_flags(bfcg_ctx_t *c, uint8_t *dst, uint64_t n_pos);

#ifdef __cplusplus
}
#endif
#endif
