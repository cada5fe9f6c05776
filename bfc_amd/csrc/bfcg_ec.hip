// bfcg_ec.hip -- BFC's error correction (bfc_ec1, correct.c:388-476) for whole batches of reads on gfx950, and its host instance.
//
// A batch: the k-mer coverage of every position first (k_occ / k_cov behind a bfcg_kcov_t, which also holds the uploaded table), then
// k_ec: a persistent grid in which every lane corrects one read at a time with bfcg_ec1.h and takes the next read from a global
// counter when it is done, so a slow read holds up only its own lane.  The search's heap (hcap entries) and stack (scap entries) and
// the two directions' results (lmax bytes each) live in a per-lane slice of a global workspace.  A read that would overflow either
// array, or is longer than lmax, is left untouched with aux2 = BFCG_EC_FALLBACK and corrected after the batch by the host instance of
// the same code (bfcg_ec1_host): the results do not depend on hcap / scap / lmax (BFCG_EC_HEAP / BFCG_EC_STACK / BFCG_EC_LMAX).
//
// Refinement (`bfc -R`: a corrector made with opt->refine_ec, bfcg_ec_batch_refine) runs the RF instances of the same code.  Its bases
// may come from the quality string (bfcg_ec1.h), so the coverage pass gets a decoded copy of the stream (k_decode writes it into the
// bfcg_kcov_t's input buffer) and k_ec<true> corrects the original bytes in a buffer of their own: a read it leaves alone comes back as
// it was.
//
// A corrector attached to a counting context (bfcg_ec_attach) reads the context's table where it lies and has no host table, so the host
// instance cannot take the reads k_ec left: they go to k_ec_retry, the same per-read code on a list of read indices, with capacities
// that grow 4x per round as host_ec1's do -- a quarter of the lanes, each with four times the slice of the same workspace -- until no
// read is left (ec_retry).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "kmer_dev.h"
#include "bfcg_ec1.h"

using namespace ec1k;

static Opt ec_opt(const bfc_opt_t *opt, int mode)
{
	Opt o;
	o.k = opt->k; o.q = opt->q; o.max_end_ext = opt->max_end_ext; o.win_multi_ec = opt->win_multi_ec; o.min_cov = opt->min_cov;
	o.w_ec = opt->w_ec; o.w_ec_high = opt->w_ec_high; o.w_absent = opt->w_absent; o.w_absent_high = opt->w_absent_high;
	o.max_path_diff = opt->max_path_diff; o.max_heap = opt->max_heap; o.mode = mode;
	return o;
}

// ------------------------------------------------------------------------------------------------ host instance

struct HostLookup {
	const bfc_ch_t *ch;
	int operator()(uint64_t y0, uint64_t y1) const { const uint64_t y[2] = {y0, y1}; return bfc_ch_get(ch, y); }
};

// one read of n bases; the heap and stack grow until the read fits.  ori: the read's earlier stats (RF only)
template <bool RF>
static void host_ec1(const bfc_ch_t *ch, const Opt &o, uint8_t *seq, uint8_t *qual, int n, Result ori, uint32_t *aux, uint32_t *aux2)
{
	const HostLookup lk = {ch};
	uint16_t *cov = (uint16_t *)malloc((size_t)(n > 0 ? n : 1) * 2);
	uint8_t *ecb = (uint8_t *)malloc((size_t)(n > 0 ? n : 1) * 2);
	kcov<RF>(o, seq, qual, n, lk, cov);
	Result res;
	for (int hcap = 64, scap = 4 * n + 256;; hcap *= 4, scap *= 4) {
		Work w;
		w.hcap = hcap; w.scap = scap;
		w.heap = (Heap1 *)malloc(sizeof(Heap1) * (size_t)hcap); w.stack = (Stack1 *)malloc(sizeof(Stack1) * (size_t)scap);
		if (!w.heap || !w.stack) { fprintf(stderr, "[E::bfcg_ec1_host] out of memory\n"); abort(); }
		const int rc = ec1<RF>(o, seq, qual, cov, n, lk, w, ecb, ecb + n, &res, ori);
		free(w.heap); free(w.stack);
		if (rc == EC_OK) break;
	}
	free(cov); free(ecb);
	*aux = res.aux; *aux2 = res.aux2;
}

extern "C" int bfcg_ec1_host(const bfc_ch_t *ch, const bfc_opt_t *opt, int mode, char *seq, char *qual, uint32_t *aux, uint32_t *aux2)
{
	if (!ch || !opt || !seq || opt->k != bfc_ch_get_k(ch)) return bfcg::fail("bad arguments to bfcg_ec1_host");
	if (opt->refine_ec) return bfcg::fail("bfcg_ec1_host: refine_ec is set (bfcg_ec1_host_refine corrects with a read's earlier stats)");
	const Opt o = ec_opt(opt, mode);
	host_ec1<false>(ch, o, (uint8_t *)seq, (uint8_t *)qual, (int)strlen(seq), Result(), aux, aux2);
	return 0;
}

extern "C" int bfcg_ec1_host_refine(const bfc_ch_t *ch, const bfc_opt_t *opt, int mode, char *seq, char *qual, uint32_t ori_aux, uint32_t ori_aux2,
                                    uint32_t *aux, uint32_t *aux2)
{
	if (!ch || !opt || !seq || opt->k != bfc_ch_get_k(ch)) return bfcg::fail("bad arguments to bfcg_ec1_host_refine");
	const Opt o = ec_opt(opt, mode);
	Result ori; ori.aux = ori_aux; ori.aux2 = ori_aux2;
	host_ec1<true>(ch, o, (uint8_t *)seq, (uint8_t *)qual, (int)strlen(seq), ori, aux, aux2);
	return 0;
}

// ------------------------------------------------------------------------------------------------ device

struct DevLookup {
	int k, l_pre, cshift;
	const unsigned long long *tab;
	unsigned *n;                                               // lookups by this lane
	__device__ int operator()(uint64_t y0, uint64_t y1) const { ++*n; return bfcg::ch_get_dev(k, l_pre, cshift, tab, y0, y1); }
};

enum { EC_BT = 256 };

// ctr[0]: next read; ctr[1]: table lookups; ctr[2]: reads left to the host.  ori_aux / ori_aux2: the reads' earlier stats (RF only)
template <bool RF>
__global__ __launch_bounds__(EC_BT) void k_ec(Opt o, int l_pre, int cshift, const unsigned long long *__restrict__ tab, uint8_t *seq, uint8_t *qual,
                                              const uint16_t *__restrict__ cov, const uint64_t *__restrict__ off, uint64_t n_reads,
                                              uint32_t *__restrict__ aux, uint32_t *__restrict__ aux2, Heap1 *heap_ws, Stack1 *stack_ws, uint8_t *ec_ws,
                                              int hcap, int scap, int lmax, unsigned long long *ctr,
                                              const uint32_t *__restrict__ ori_aux, const uint32_t *__restrict__ ori_aux2)
{
	const uint64_t lane = (uint64_t)blockIdx.x * EC_BT + threadIdx.x;
	unsigned n_look = 0, n_host = 0;
	const DevLookup lk = {o.k, l_pre, cshift, tab, &n_look};
	Work w;
	w.heap = heap_ws + lane * (uint64_t)hcap; w.stack = stack_ws + lane * (uint64_t)scap; w.hcap = hcap; w.scap = scap;
	uint8_t *ec0 = ec_ws + lane * 2 * (uint64_t)lmax, *ec1b = ec0 + lmax;
	for (;;) {
		const uint64_t r = atomicAdd(&ctr[0], 1ULL);
		if (r >= n_reads) break;
		const uint64_t a = off[r];
		const int n = (int)(off[r + 1] - a - 1);
		Result res, ori;
		if (RF) { ori.aux = ori_aux[r]; ori.aux2 = ori_aux2[r]; }
		if (n > lmax || ec1<RF>(o, seq + a, qual ? qual + a : nullptr, cov + a, n, lk, w, ec0, ec1b, &res, ori) != EC_OK) {
			res.aux = 0; res.aux2 = BFCG_EC_FALLBACK; ++n_host;
		}
		aux[r] = res.aux; aux2[r] = res.aux2;
	}
	atomicAdd(&ctr[1], (unsigned long long)n_look);
	if (n_host) atomicAdd(&ctr[2], (unsigned long long)n_host);
}

// The reads k_ec left (aux2 = BFCG_EC_FALLBACK), by index: list[0 .. n_list).  n_lanes lanes (any number: the grid's last workgroup may be
// partly idle) with hcap / scap / lmax of this round.  ctr[0]: next list entry; ctr[1]: table lookups; ctr[2]: reads that still do not fit
// (they keep aux2 = BFCG_EC_FALLBACK and their bytes).  The coverage is the batch's, which k_ec read too.
template <bool RF>
__global__ __launch_bounds__(EC_BT) void k_ec_retry(Opt o, int l_pre, int cshift, const unsigned long long *__restrict__ tab, uint8_t *seq, uint8_t *qual,
                                                    const uint16_t *__restrict__ cov, const uint64_t *__restrict__ off, const uint64_t *__restrict__ list,
                                                    uint64_t n_list, uint32_t *__restrict__ aux, uint32_t *__restrict__ aux2, Heap1 *heap_ws, Stack1 *stack_ws,
                                                    uint8_t *ec_ws, int hcap, int scap, int lmax, uint64_t n_lanes, unsigned long long *ctr,
                                                    const uint32_t *__restrict__ ori_aux, const uint32_t *__restrict__ ori_aux2)
{
	const uint64_t lane = (uint64_t)blockIdx.x * EC_BT + threadIdx.x;
	if (lane >= n_lanes) return;
	unsigned n_look = 0, n_left = 0;
	const DevLookup lk = {o.k, l_pre, cshift, tab, &n_look};
	Work w;
	w.heap = heap_ws + lane * (uint64_t)hcap; w.stack = stack_ws + lane * (uint64_t)scap; w.hcap = hcap; w.scap = scap;
	uint8_t *ec0 = ec_ws + lane * 2 * (uint64_t)lmax, *ec1b = ec0 + lmax;
	for (;;) {
		const uint64_t i = atomicAdd(&ctr[0], 1ULL);
		if (i >= n_list) break;
		const uint64_t r = list[i], a = off[r];
		const int n = (int)(off[r + 1] - a - 1);
		Result res, ori;
		if (RF) { ori.aux = ori_aux[r]; ori.aux2 = ori_aux2[r]; }
		if (n > lmax || ec1<RF>(o, seq + a, qual ? qual + a : nullptr, cov + a, n, lk, w, ec0, ec1b, &res, ori) != EC_OK) { ++n_left; continue; }
		aux[r] = res.aux; aux2[r] = res.aux2;
	}
	atomicAdd(&ctr[1], (unsigned long long)n_look);
	if (n_left) atomicAdd(&ctr[2], (unsigned long long)n_left);
}

// the bases refinement reads (base_at<true>) as sequence bytes, for the coverage pass: one wavefront per read, separators copied as they are
enum { DEC_BT = 256, DEC_W = 64 };
__global__ __launch_bounds__(DEC_BT) void k_decode(const uint8_t *__restrict__ seq, const uint8_t *__restrict__ qual, const uint64_t *__restrict__ off,
                                                   uint64_t n_reads, uint8_t *__restrict__ out)
{
	const uint64_t r = (uint64_t)blockIdx.x * (DEC_BT / DEC_W) + threadIdx.x / DEC_W;
	if (r >= n_reads) return;
	const uint64_t a = off[r], e = off[r + 1] - 1;                // [a, e): the read's bases; e: its separator
	for (uint64_t p = a + threadIdx.x % DEC_W; p <= e; p += DEC_W)
		out[p] = p == e ? seq[p] : (uint8_t)"ACGTN"[base_at<true>(seq + a, qual ? qual + a : nullptr, (int)(p - a))];
}

struct bfcg_ec {
	bfcg_kcov_t *kc;
	const bfc_ch_t *ch;                                        // NULL: attached to a counting context's table (no host instance: ec_retry)
	Opt o;
	bfcg::KParams P;
	const unsigned long long *tab;
	int device, hcap, scap, lmax;
	uint64_t lanes, max_pos, max_reads, ec_bytes;              // ec_bytes: d_ec's size (ec_retry grows it for reads longer than lmax)
	hipStream_t st;
	hipEvent_t e0, e1;
	uint8_t *d_qual, *d_ec;
	uint64_t *d_off;
	uint32_t *d_aux, *d_aux2;
	int refine;
	uint8_t *d_oseq;                                           // refinement: the original bytes k_ec<true> rewrites
	uint32_t *d_oaux, *d_oaux2;                                // refinement: the reads' earlier stats
	Heap1 *d_heap;
	Stack1 *d_stack;
	unsigned long long *d_ctr;
	float last_ms;
	uint64_t host_reads, last_lookups, last_host, retry_reads;
	uint64_t *d_list, list_cap;                                // ec_retry: the listed reads
};

static int env_int(const char *name, int dflt, int lo, int hi)
{
	const char *s = getenv(name);
	int v = s && *s ? atoi(s) : dflt;
	return v < lo ? lo : v > hi ? hi : v;
}

extern "C" void bfcg_ec_destroy(bfcg_ec_t *e)
{
	if (!e) return;
	if (e->st) { (void)hipSetDevice(e->device); (void)hipStreamSynchronize(e->st); }
	(void)hipFree(e->d_qual); (void)hipFree(e->d_ec); (void)hipFree(e->d_off); (void)hipFree(e->d_aux); (void)hipFree(e->d_aux2);
	(void)hipFree(e->d_heap); (void)hipFree(e->d_stack); (void)hipFree(e->d_ctr);
	(void)hipFree(e->d_oseq); (void)hipFree(e->d_oaux); (void)hipFree(e->d_oaux2); (void)hipFree(e->d_list);
	if (e->st) { (void)hipEventDestroy(e->e0); (void)hipEventDestroy(e->e1); (void)hipStreamDestroy(e->st); }
	bfcg_kcov_destroy(e->kc);
	free(e);
}

// what both kinds of corrector share, once e->kc (and e->ch) are set: options, capacities, buffers
static bfcg_ec_t *ec_setup(bfcg_ec_t *e, const bfc_opt_t *opt, int mode, uint64_t max_pos, uint64_t max_reads)
{
	e->o = ec_opt(opt, mode);
	e->refine = opt->refine_ec != 0;
	e->tab = bfcg::kcov_table(e->kc, &e->P, &e->device);
	e->max_pos = max_pos; e->max_reads = max_reads;
	e->hcap = env_int("BFCG_EC_HEAP", 16, 1, 1 << 16);
	e->scap = env_int("BFCG_EC_STACK", 1024, 1, 1 << 20);
	e->lmax = env_int("BFCG_EC_LMAX", 512, 1, 1 << 16);
	const uint64_t lanes_max = (uint64_t)env_int("BFCG_EC_LANES", 1 << 17, EC_BT, 1 << 20);
	e->lanes = (max_reads + EC_BT - 1) / EC_BT * EC_BT;
	if (e->lanes > lanes_max) e->lanes = lanes_max / EC_BT * EC_BT;
	BFCG_CKN(bfcg_ec_destroy(e), hipSetDevice(e->device));
	BFCG_CKN(bfcg_ec_destroy(e), hipStreamCreate(&e->st));
	BFCG_CKN(bfcg_ec_destroy(e), hipEventCreate(&e->e0)); BFCG_CKN(bfcg_ec_destroy(e), hipEventCreate(&e->e1));
	BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_qual, max_pos));
	BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_off, (max_reads + 1) * 8));
	BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_aux, max_reads * 4)); BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_aux2, max_reads * 4));
	BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_heap, sizeof(Heap1) * e->lanes * (uint64_t)e->hcap));
	BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_stack, sizeof(Stack1) * e->lanes * (uint64_t)e->scap));
	e->ec_bytes = e->lanes * 2 * (uint64_t)e->lmax;
	BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_ec, e->ec_bytes));
	BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_ctr, 3 * sizeof(unsigned long long)));
	if (e->refine) {
		BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_oseq, max_pos));
		BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_oaux, max_reads * 4)); BFCG_CKN(bfcg_ec_destroy(e), hipMalloc(&e->d_oaux2, max_reads * 4));
	}
	return e;
}

extern "C" bfcg_ec_t *bfcg_ec_create(const bfc_ch_t *ch, const bfc_opt_t *opt, int device, uint64_t max_pos, uint64_t max_reads)
{
	if (!ch || !opt || opt->k != bfc_ch_get_k(ch) || max_pos == 0 || max_reads == 0 || opt->filter_mode) {
		bfcg::fail("bad arguments to bfcg_ec_create (a table-mode bfc_opt_t whose k is the table's)");
		return NULL;
	}
	bfcg_ec_t *e = (bfcg_ec_t *)calloc(1, sizeof(bfcg_ec_t));
	if (!e) { bfcg::fail("out of host memory"); return NULL; }
	e->kc = bfcg_kcov_create(ch, device, max_pos);                 // uploads the table once, or adopts the copy bfc_count left (and says so if there is no GPU)
	if (!e->kc) { free(e); return NULL; }
	uint64_t hist[256], hist_high[64];
	e->ch = ch;
	return ec_setup(e, opt, bfc_ch_hist(ch, hist, hist_high), max_pos, max_reads); // correct.c:627
}

// A corrector on the table of a counting context, where the count kernels built it (bfcg_kcov_attach's contract: the context is drained,
// its segments converted, it must outlive the corrector and must not count meanwhile).  Nothing is exported: the mode comes from one
// pass of k_tab_hist, and the reads k_ec leaves go to k_ec_retry.
extern "C" bfcg_ec_t *bfcg_ec_attach(bfcg_ctx_t *ctx, const bfc_opt_t *opt, uint64_t max_pos, uint64_t max_reads)
{
	if (!ctx || !opt || max_pos == 0 || max_reads == 0 || opt->filter_mode) {
		bfcg::fail("bad arguments to bfcg_ec_attach (a counting context and a table-mode bfc_opt_t)");
		return NULL;
	}
	const int k = bfcg::ctx_table_k(ctx);
	if (k < 0) { bfcg::fail("bfcg_ec_attach needs a table-mode context"); return NULL; }
	if (opt->k != k) { bfcg::fail("bfcg_ec_attach: opt->k is %d, the context counts %d-mers", opt->k, k); return NULL; }
	bfcg_kmers_t *km = bfcg_kmers_attach(ctx);                     // drains the context and converts its segments
	if (!km) return NULL;
	uint64_t hist[256], hist_high[64];
	const int mode = bfcg_kmers_hist(km, hist, hist_high);       // bfc_ch_hist's mode (correct.c:627), read once
	bfcg_kmers_destroy(km);
	if (mode < -1) return NULL;
	bfcg_ec_t *e = (bfcg_ec_t *)calloc(1, sizeof(bfcg_ec_t));
	if (!e) { bfcg::fail("out of host memory"); return NULL; }
	e->kc = bfcg_kcov_attach(ctx, max_pos);
	if (!e->kc) { free(e); return NULL; }
	return ec_setup(e, opt, mode, max_pos, max_reads);
}

// An attached corrector's answer for the reads k_ec left (aux2[r] == BFCG_EC_FALLBACK in the host's copy, which is refreshed here): rounds of
// k_ec_retry over the list of those reads.  Every round has 4x the heap and stack entries per lane of the one before, as host_ec1's loop,
// and an lmax that covers the longest read listed.  The workspace is the corrector's own while a lane's slice fits it -- the arrays are
// lane-major, so a quarter of the lanes get four times the slice -- and a larger one after that, for at most 64 lanes (*big_heap /
// *big_stack: the caller frees them).  An allocation that fails ends the batch with an error that names the read; the host's streams have
// not been written by then.
enum { EC_RETRY_BIG_LANES = 64, EC_RETRY_MAX_CAP = 1 << 28 };
static int ec_retry_rounds(bfcg_ec_t *e, const char *fn, int rf, uint8_t *d_seq, uint8_t *d_qual, const uint16_t *d_cov, const uint64_t *off, uint64_t n_reads,
                           uint32_t *aux2, uint64_t *list, Heap1 **big_heap, Stack1 **big_stack)
{
	uint64_t n_list = 0;
	for (uint64_t r = 0; r < n_reads; ++r) if (aux2[r] == BFCG_EC_FALLBACK) list[n_list++] = r;
	const uint64_t n_first = n_list;
	if (n_list > e->list_cap) {
		(void)hipFree(e->d_list); e->d_list = nullptr; e->list_cap = 0;
		BFCG_CK(hipMalloc(&e->d_list, n_list * 8));
		e->list_cap = n_list;
	}
	uint64_t lanes = e->lanes, hcap = (uint64_t)e->hcap, scap = (uint64_t)e->scap;
	int big = 0;                                                 // the rounds have left the corrector's workspace
	while (n_list) {
		hcap *= 4; scap *= 4;
		if (hcap > EC_RETRY_MAX_CAP || scap > EC_RETRY_MAX_CAP)
			return bfcg::fail("%s: read %llu does not fit a search of 2^28 heap or stack entries", fn, (unsigned long long)list[0]);
		int lmax = e->lmax;
		for (uint64_t i = 0; i < n_list; ++i) {
			const int n = (int)(off[list[i] + 1] - off[list[i]] - 1);
			if (n > lmax) lmax = n;
		}
		Heap1 *heap = e->d_heap;
		Stack1 *stack = e->d_stack;
		if (!big) lanes /= 4;
		if (big || lanes == 0) {                                 // a single lane's slice no longer fits: a larger workspace for the reads that are left
			big = 1;
			lanes = n_list < EC_RETRY_BIG_LANES ? n_list : EC_RETRY_BIG_LANES;
			for (;; lanes = 1) {
				(void)hipFree(*big_heap); (void)hipFree(*big_stack); *big_heap = nullptr; *big_stack = nullptr;
				if (hipMalloc(big_heap, sizeof(Heap1) * lanes * hcap) == hipSuccess && hipMalloc(big_stack, sizeof(Stack1) * lanes * scap) == hipSuccess) break;
				(void)hipGetLastError();
				if (lanes == 1)
					return bfcg::fail("%s: read %llu needs %llu heap and %llu stack entries, which the device cannot allocate", fn, (unsigned long long)list[0],
					              (unsigned long long)hcap, (unsigned long long)scap);
			}
			heap = *big_heap; stack = *big_stack;
		}
		const uint64_t n_lanes = lanes < n_list ? lanes : n_list;
		if (n_lanes * 2 * (uint64_t)lmax > e->ec_bytes) {        // grown for good: k_ec's lanes * 2 * e->lmax bytes still fit
			uint8_t *d = nullptr;
			if (hipMalloc(&d, n_lanes * 2 * (uint64_t)lmax) != hipSuccess) {
				(void)hipGetLastError();
				return bfcg::fail("%s: read %llu: no room for the results of %llu lanes of %d bases", fn, (unsigned long long)list[0], (unsigned long long)n_lanes, lmax);
			}
			(void)hipFree(e->d_ec);
			e->d_ec = d; e->ec_bytes = n_lanes * 2 * (uint64_t)lmax;
		}
		unsigned long long ctr[3];
		BFCG_CK(hipMemsetAsync(e->d_ctr, 0, 3 * sizeof(unsigned long long), e->st));
		BFCG_CK(hipMemcpyAsync(e->d_list, list, n_list * 8, hipMemcpyHostToDevice, e->st));
		BFCG_CK(hipEventRecord(e->e0, e->st));
		hipLaunchKernelGGL(rf ? k_ec_retry<true> : k_ec_retry<false>, dim3((unsigned)((n_lanes + EC_BT - 1) / EC_BT)), dim3(EC_BT), 0, e->st, e->o, e->P.l_pre,
		                   e->P.tab_cshift, e->tab, d_seq, d_qual, d_cov, (const uint64_t *)e->d_off, (const uint64_t *)e->d_list, n_list, e->d_aux, e->d_aux2,
		                   heap, stack, e->d_ec, (int)hcap, (int)scap, lmax, n_lanes, e->d_ctr, (const uint32_t *)e->d_oaux, (const uint32_t *)e->d_oaux2);
		BFCG_CK(hipGetLastError());
		BFCG_CK(hipEventRecord(e->e1, e->st));
		BFCG_CK(hipMemcpyAsync(aux2, e->d_aux2, n_reads * 4, hipMemcpyDeviceToHost, e->st));
		BFCG_CK(hipMemcpyAsync(ctr, e->d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, e->st));
		BFCG_CK(hipStreamSynchronize(e->st));
		float ms = 0;
		BFCG_CK(hipEventElapsedTime(&ms, e->e0, e->e1));
		e->last_ms += ms;
		e->last_lookups += ctr[1];
		uint64_t m = 0;
		for (uint64_t i = 0; i < n_list; ++i) if (aux2[list[i]] == BFCG_EC_FALLBACK) list[m++] = list[i];
		if (m != ctr[2]) return bfcg::fail("%s: the retry kernel left %llu reads, their marks say %llu", fn, ctr[2], (unsigned long long)m);
		n_list = m;
	}
	e->retry_reads += n_first;
	return 0;
}

static int ec_retry(bfcg_ec_t *e, const char *fn, int rf, uint8_t *d_seq, uint8_t *d_qual, const uint16_t *d_cov, const uint64_t *off, uint64_t n_reads,
                    uint32_t *aux2, uint64_t n_left)
{
	uint64_t *list = (uint64_t *)malloc(n_left * 8);
	if (!list) return bfcg::fail("%s: out of host memory", fn);
	Heap1 *big_heap = nullptr;
	Stack1 *big_stack = nullptr;
	const int rc = ec_retry_rounds(e, fn, rf, d_seq, d_qual, d_cov, off, n_reads, aux2, list, &big_heap, &big_stack);
	(void)hipFree(big_heap); (void)hipFree(big_stack);
	free(list);
	return rc;
}

// seq / qual: host streams of n_pos positions in the batch format of PART 2 (qual NULL: no read has a quality string); rewritten in place.
// ori_aux / ori_aux2: NULL for table mode, the reads' earlier stats for refinement.
static int ec_batch(bfcg_ec_t *e, const char *fn, uint8_t *seq, uint8_t *qual, uint64_t n_pos, const uint64_t *off, uint64_t n_reads,
                    const uint32_t *ori_aux, const uint32_t *ori_aux2, uint32_t *aux, uint32_t *aux2)
{
	const int rf = ori_aux != nullptr;
	if (!e || !seq || !off || !aux || !aux2 || (rf && !ori_aux2)) return bfcg::fail("bad arguments to %s", fn);
	if (rf != e->refine)
		return bfcg::fail(rf ? "%s: the corrector was made without refine_ec (bfcg_ec_batch corrects in table mode)"
		                 : "%s: the corrector was made with refine_ec (bfcg_ec_batch_refine takes the reads' earlier stats)", fn);
	if (n_pos > e->max_pos || n_reads > e->max_reads) return bfcg::fail("correction batch exceeds the capacity given to bfcg_ec_create");
	if (n_reads && off[n_reads] != n_pos) return bfcg::fail("%s: off[n_reads] must be n_pos", fn);
	e->last_ms = 0; e->last_lookups = 0; e->last_host = 0;
	if (n_reads == 0) return 0;
	for (uint64_t r = 0; r < n_reads; ++r)                       // every read ends in its separator inside the batch
		if (off[r + 1] <= off[r]) return bfcg::fail("%s: read %llu has no separator", fn, (unsigned long long)r);
	uint8_t *d_seq = (uint8_t *)bfcg_kcov_dev_seq(e->kc);
	const uint16_t *d_cov = (const uint16_t *)bfcg_kcov_dev_out(e->kc);
	uint8_t *d_ec_seq = rf ? e->d_oseq : d_seq;                   // the bytes k_ec rewrites
	float ms_dec = 0;
	BFCG_CK(hipSetDevice(e->device));
	if (!rf) BFCG_CK(hipMemcpy(d_seq, seq, n_pos, hipMemcpyHostToDevice));
	else {                                                       // the coverage pass sees the decoded bases (k_decode into its input buffer)
		BFCG_CK(hipMemcpyAsync(e->d_oseq, seq, n_pos, hipMemcpyHostToDevice, e->st));
		if (qual) BFCG_CK(hipMemcpyAsync(e->d_qual, qual, n_pos, hipMemcpyHostToDevice, e->st));
		BFCG_CK(hipMemcpyAsync(e->d_off, off, (n_reads + 1) * 8, hipMemcpyHostToDevice, e->st));
		BFCG_CK(hipMemcpyAsync(e->d_oaux, ori_aux, n_reads * 4, hipMemcpyHostToDevice, e->st));
		BFCG_CK(hipMemcpyAsync(e->d_oaux2, ori_aux2, n_reads * 4, hipMemcpyHostToDevice, e->st));
		const uint64_t per = DEC_BT / DEC_W;
		BFCG_CK(hipEventRecord(e->e0, e->st));
		hipLaunchKernelGGL(k_decode, dim3((unsigned)((n_reads + per - 1) / per)), dim3(DEC_BT), 0, e->st, e->d_oseq, qual ? e->d_qual : nullptr,
		                   (const uint64_t *)e->d_off, n_reads, d_seq);
		BFCG_CK(hipGetLastError());
		BFCG_CK(hipEventRecord(e->e1, e->st));
		BFCG_CK(hipStreamSynchronize(e->st));                         // bfcg_kcov_batch runs on a stream of its own
		BFCG_CK(hipEventElapsedTime(&ms_dec, e->e0, e->e1));
	}
	if (bfcg_kcov_batch(e->kc, nullptr, d_seq, n_pos, e->o.min_cov, nullptr) != 0) return -1;
	const float ms_cov = bfcg_kcov_last_ms(e->kc) + ms_dec;
	if (!rf) {
		if (qual) BFCG_CK(hipMemcpyAsync(e->d_qual, qual, n_pos, hipMemcpyHostToDevice, e->st));
		BFCG_CK(hipMemcpyAsync(e->d_off, off, (n_reads + 1) * 8, hipMemcpyHostToDevice, e->st));
	}
	BFCG_CK(hipMemsetAsync(e->d_ctr, 0, 3 * sizeof(unsigned long long), e->st));
	uint64_t lanes = (n_reads + EC_BT - 1) / EC_BT * EC_BT;
	if (lanes > e->lanes) lanes = e->lanes;
	BFCG_CK(hipEventRecord(e->e0, e->st));
	hipLaunchKernelGGL(rf ? k_ec<true> : k_ec<false>, dim3((unsigned)(lanes / EC_BT)), dim3(EC_BT), 0, e->st, e->o, e->P.l_pre, e->P.tab_cshift, e->tab,
	                   d_ec_seq, qual ? e->d_qual : nullptr, d_cov, (const uint64_t *)e->d_off, n_reads, e->d_aux, e->d_aux2, e->d_heap, e->d_stack,
	                   e->d_ec, e->hcap, e->scap, e->lmax, e->d_ctr, (const uint32_t *)e->d_oaux, (const uint32_t *)e->d_oaux2);
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipEventRecord(e->e1, e->st));
	unsigned long long ctr[3];
	const int attached = e->ch == nullptr;                       // the streams leave the device behind the retry rounds, if there are any
	if (!attached) {
		BFCG_CK(hipMemcpyAsync(seq, d_ec_seq, n_pos, hipMemcpyDeviceToHost, e->st));
		if (qual) BFCG_CK(hipMemcpyAsync(qual, e->d_qual, n_pos, hipMemcpyDeviceToHost, e->st));
		BFCG_CK(hipMemcpyAsync(aux, e->d_aux, n_reads * 4, hipMemcpyDeviceToHost, e->st));
	}
	BFCG_CK(hipMemcpyAsync(aux2, e->d_aux2, n_reads * 4, hipMemcpyDeviceToHost, e->st));
	BFCG_CK(hipMemcpyAsync(ctr, e->d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, e->st));
	BFCG_CK(hipStreamSynchronize(e->st));
	float ms = 0;
	BFCG_CK(hipEventElapsedTime(&ms, e->e0, e->e1));
	e->last_ms = ms_cov + ms;
	e->last_lookups = ctr[1];
	if (attached) {                                              // no host table: the reads k_ec left are corrected on the device too
		if (ctr[2] && ec_retry(e, fn, rf, d_ec_seq, qual ? e->d_qual : nullptr, d_cov, off, n_reads, aux2, ctr[2]) != 0) return -1;
		BFCG_CK(hipMemcpyAsync(seq, d_ec_seq, n_pos, hipMemcpyDeviceToHost, e->st));
		if (qual) BFCG_CK(hipMemcpyAsync(qual, e->d_qual, n_pos, hipMemcpyDeviceToHost, e->st));
		BFCG_CK(hipMemcpyAsync(aux, e->d_aux, n_reads * 4, hipMemcpyDeviceToHost, e->st));
		BFCG_CK(hipStreamSynchronize(e->st));
		return 0;
	}
	for (uint64_t r = 0; r < n_reads; ++r) {                     // the reads the device left to the host instance
		if (aux2[r] != BFCG_EC_FALLBACK) continue;
		const uint64_t a = off[r];
		uint8_t *s = seq + a, *q = qual ? qual + a : nullptr;
		const int n = (int)(off[r + 1] - a - 1);
		if (rf) { Result ori; ori.aux = ori_aux[r]; ori.aux2 = ori_aux2[r]; host_ec1<true>(e->ch, e->o, s, q, n, ori, &aux[r], &aux2[r]); }
		else host_ec1<false>(e->ch, e->o, s, q, n, Result(), &aux[r], &aux2[r]);
		++e->last_host;
	}
	e->host_reads += e->last_host;
	return 0;
}

extern "C" int bfcg_ec_batch(bfcg_ec_t *e, uint8_t *seq, uint8_t *qual, uint64_t n_pos, const uint64_t *off, uint64_t n_reads, uint32_t *aux, uint32_t *aux2)
{
	return ec_batch(e, "bfcg_ec_batch", seq, qual, n_pos, off, n_reads, nullptr, nullptr, aux, aux2);
}

extern "C" int bfcg_ec_batch_refine(bfcg_ec_t *e, uint8_t *seq, uint8_t *qual, uint64_t n_pos, const uint64_t *off, uint64_t n_reads,
                                    const uint32_t *ori_aux, const uint32_t *ori_aux2, uint32_t *aux, uint32_t *aux2)
{
	if (!ori_aux) return bfcg::fail("bad arguments to bfcg_ec_batch_refine");
	return ec_batch(e, "bfcg_ec_batch_refine", seq, qual, n_pos, off, n_reads, ori_aux, ori_aux2, aux, aux2);
}

extern "C" float bfcg_ec_last_ms(bfcg_ec_t *e) { return e->last_ms; }
extern "C" uint64_t bfcg_ec_host_reads(bfcg_ec_t *e) { return e->host_reads; }
extern "C" uint64_t bfcg_ec_last_lookups(bfcg_ec_t *e) { return e->last_lookups; }
extern "C" uint64_t bfcg_ec_retry_reads(bfcg_ec_t *e) { return e->retry_reads; }
extern "C" int bfcg_ec_adopted(bfcg_ec_t *e) { return bfcg::kcov_adopted(e->kc); }
