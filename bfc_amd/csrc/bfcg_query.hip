// bfcg_query.hip -- the objects that only READ what a counting context built (include/bfc_gpu.h, PART 2): the registry of filters and
// tables left in HBM behind their host objects, the trimmer (bfcg_trim_*) and the coverage pass (bfcg_kcov_*).  No kernel lives here:
// run_query / run_streak / run_kcov are bfcg_kernels.hip's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"

using namespace bfcg;

// ---- filters that stay in HBM behind their host object.  `bfc -1` counts into bf_high and then queries it for every k-mer again
// (correct.c:556): bfc_count hands the host copy the reference's API promises (bfc_bf_t.b is public) AND leaves a device copy here,
// which bfcg_trim_create adopts instead of uploading 2^(b-3) bytes again.  The copy is dropped when the host object is destroyed or
// written to through this library (bfc_bf_destroy / bfc_bf_insert call bfcg_resident_drop).
// A count table has the same arrangement (bfcg_export_table_resident -> bfcg_kcov_create, i.e. bfc_count -> bfc_correct): its entry
// carries k, l_pre and cshift instead of n_shift (k = 0 marks a filter's entry), and the bfc_ch_* functions that write to a table, free
// one or hand out an address call bfcg_resident_drop as the bfc_bf_* ones do.
static resident_t g_res[16];
static std::atomic<int> g_res_n{0};
static std::mutex g_res_mu;

int bfcg::resident_put(const resident_t &r)
{
	std::lock_guard<std::mutex> lk(g_res_mu);
	for (int i = 0; i < 16; ++i) if (!g_res[i].dev) { g_res[i] = r; g_res_n.fetch_add(1); return 0; }
	return -1;
}
// the first taker owns the copy (and frees it), a second one finds nothing
void *bfcg::resident_take(const void *host, int device, int n_shift, int k, int l_pre, int cshift)
{
	if (g_res_n.load(std::memory_order_relaxed) == 0) return 0;
	std::lock_guard<std::mutex> lk(g_res_mu);
	for (int i = 0; i < 16; ++i) {
		resident_t &r = g_res[i];
		if (r.dev && r.host == host && r.device == device && r.n_shift == n_shift && r.k == k && r.l_pre == l_pre && r.cshift == cshift) {
			void *dev = r.dev; r.dev = 0; g_res_n.fetch_sub(1); return dev;
		}
	}
	return 0;
}
extern "C" void bfcg_resident_drop(const void *bf)
{
	if (g_res_n.load(std::memory_order_relaxed) == 0) return;
	for (;;) { // a filter counted on several GPUs has a copy on each of them
		void *dev = 0; int device = 0;
		{
			std::lock_guard<std::mutex> lk(g_res_mu);
			for (int i = 0; i < 16; ++i) if (g_res[i].dev && g_res[i].host == bf) { dev = g_res[i].dev; device = g_res[i].device; g_res[i].dev = 0; g_res_n.fetch_sub(1); break; }
		}
		if (!dev) return;
		int cur = 0; (void)hipGetDevice(&cur); (void)hipSetDevice(device); (void)hipFree(dev); (void)hipSetDevice(cur);
	}
}
// a full copy of host filter `bf` that sits at `dev` on `device` (bfcg_mg.hip: gathered from the ranks' slices); 0, or -1 if the registry is full
extern "C" int bfcg_resident_register(const void *bf, void *dev, int device, int n_shift) { return resident_put(resident_t{bf, dev, device, n_shift}); }

// ---------------------------------------------------------------------------------------------------------------
// trim pass of `bfc -1` on the GPU (config c5): the bloom filter of k-mers seen twice is resident in HBM, every read
// of a batch gets its longest streak of bloom hits and the keep / trim decision of correct.c:557-569

struct bfcg_trim {
	KParams P;
	int device;
	hipStream_t st;
	unsigned int *bloom;
	int adopted;    // the filter was already in HBM (left there by bfc_count), not uploaded
	uint8_t *d_seq, *d_flags;
	uint64_t *d_off;
	int32_t *d_start, *d_end;
	uint64_t max_pos, max_reads;
	hipEvent_t e0, e1;
	float last_ms;
};

// (a failure after the calloc frees what was made so far: the destroy functions of this file take a half-built object)
extern "C" bfcg_trim_t *bfcg_trim_create(int k, const bfc_bf_t *bf, int device, uint64_t max_pos, uint64_t max_reads)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fail("no HIP device available: the trim pass has no CPU fallback here"); return NULL; }
	if (!bf || k < 1 || k > 63 || bf->n_shift < 9 || bf->n_shift > 37 || bf->n_hashes < 1 || bf->n_hashes > 12) { fail("bad arguments to bfcg_trim_create"); return NULL; }
	BFCG_CKN((void)0, hipSetDevice(device));
	bfcg_trim_t *t = (bfcg_trim_t *)calloc(1, sizeof(bfcg_trim_t));
	if (!t) { fail("out of host memory"); return NULL; }
	t->P.k = k; t->P.bf_shift = bf->n_shift; t->P.n_hashes = bf->n_hashes; t->P.q = 0;
	t->device = device; t->max_pos = max_pos; t->max_reads = max_reads;
	BFCG_CKN(bfcg_trim_destroy(t), hipStreamCreate(&t->st));
	BFCG_CKN(bfcg_trim_destroy(t), hipEventCreate(&t->e0)); BFCG_CKN(bfcg_trim_destroy(t), hipEventCreate(&t->e1));
	t->bloom = (unsigned int *)resident_take(bf, device, bf->n_shift, 0, 0, 0); // left in HBM by bfc_count (bfcg_export_bloom_resident)?
	t->adopted = t->bloom != 0;
	if (!t->bloom) {
		BFCG_CKN(bfcg_trim_destroy(t), hipMalloc(&t->bloom, 1ULL << (bf->n_shift - 3)));
		BFCG_CKN(bfcg_trim_destroy(t), hipMemcpy(t->bloom, bf->b, 1ULL << (bf->n_shift - 3), hipMemcpyHostToDevice));
	}
	// d_flags: one bit per position in whole 64-bit words, and k_streak may read the word behind a read's last
	const uint64_t flag_bytes = 8 * (max_pos / 64 + 2);
	BFCG_CKN(bfcg_trim_destroy(t), hipMalloc(&t->d_seq, max_pos)); BFCG_CKN(bfcg_trim_destroy(t), hipMalloc(&t->d_flags, max_pos > flag_bytes ? max_pos : flag_bytes));
	BFCG_CKN(bfcg_trim_destroy(t), hipMalloc(&t->d_off, (max_reads + 1) * 8));
	BFCG_CKN(bfcg_trim_destroy(t), hipMalloc(&t->d_start, max_reads * 4)); BFCG_CKN(bfcg_trim_destroy(t), hipMalloc(&t->d_end, max_reads * 4));
	return t;
}

extern "C" void bfcg_trim_destroy(bfcg_trim_t *t)
{
	if (!t) return;
	(void)hipSetDevice(t->device);
	if (t->st) (void)hipStreamSynchronize(t->st);
	(void)hipFree(t->bloom); (void)hipFree(t->d_seq); (void)hipFree(t->d_flags); (void)hipFree(t->d_off); (void)hipFree(t->d_start); (void)hipFree(t->d_end);
	if (t->e0) (void)hipEventDestroy(t->e0);
	if (t->e1) (void)hipEventDestroy(t->e1);
	if (t->st) (void)hipStreamDestroy(t->st);
	free(t);
}

// device-resident stream (d_seq may be NULL: then h_seq is copied in).  off[n_reads+1] are stream offsets: read r is
// [off[r], off[r+1]-1), byte off[r+1]-1 its separator.  start[r] = -1 if the read is dropped, else keep [start, end).
extern "C" int bfcg_trim_batch(bfcg_trim_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos, const uint64_t *h_off, uint64_t n_reads,
                               float min_frac, int32_t *start, int32_t *end)
{
	if (n_pos > t->max_pos || n_reads > t->max_reads) return fail("trim batch exceeds the capacity given to bfcg_trim_create");
	if (n_reads == 0) return 0;
	BFCG_CK(hipSetDevice(t->device));
	if (!d_seq) { BFCG_CK(hipMemcpyAsync(t->d_seq, h_seq, n_pos, hipMemcpyHostToDevice, t->st)); d_seq = t->d_seq; }
	BFCG_CK(hipMemcpyAsync(t->d_off, h_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, t->st));
	BFCG_CK(hipEventRecord(t->e0, t->st));
	run_query(t->P, d_seq, (int64_t)n_pos, t->bloom, t->d_flags, t->st);
	run_streak(t->P.k, min_frac, t->d_flags, t->d_off, n_reads, t->d_start, t->d_end, t->st);
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(start, t->d_start, n_reads * 4, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(end, t->d_end, n_reads * 4, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&t->last_ms, t->e0, t->e1));
	return 0;
}
extern "C" float bfcg_trim_last_ms(bfcg_trim_t *t) { return t->last_ms; }
extern "C" int bfcg_trim_adopted(bfcg_trim_t *t) { return t->adopted; }
extern "C" void *bfcg_trim_dev_seq(bfcg_trim_t *t) { return t->d_seq; }

// ---------------------------------------------------------------------------------------------------------------
// k-mer coverage for the corrector: bfc_ec_kcov (correct.c:96-117) for a whole batch of reads against the count
// table resident in HBM -- either uploaded from a host bfc_ch_t or borrowed from a counting context that still holds it

struct bfcg_kcov {
	KParams P;
	int device, owns_table;
	int adopted;    // the table was already in HBM (left there by bfc_count), not uploaded
	hipStream_t st;
	unsigned long long *table;
	uint8_t *d_seq, *d_flags;
	uint16_t *d_out;
	uint64_t max_pos;
	hipEvent_t e0, e1;
	float last_ms;
};

// `table` is what the object starts with: an adopted copy it owns (freed with it, also when the buffers below do not fit), a context's
// table it borrows, or nothing yet
static bfcg_kcov_t *kcov_new(int k, int l_pre, int cshift, int device, uint64_t max_pos, unsigned long long *table, int owns_table)
{
	bfcg_kcov_t *t = (bfcg_kcov_t *)calloc(1, sizeof(bfcg_kcov_t));
	if (!t) { fail("out of host memory"); if (owns_table) (void)hipFree(table); return NULL; }
	t->P.k = k; t->P.l_pre = l_pre; t->P.tab_cshift = cshift; t->P.q = 0;
	t->device = device; t->max_pos = max_pos; t->table = table; t->owns_table = owns_table;
	BFCG_CKN(bfcg_kcov_destroy(t), hipSetDevice(device));
	BFCG_CKN(bfcg_kcov_destroy(t), hipStreamCreate(&t->st));
	BFCG_CKN(bfcg_kcov_destroy(t), hipEventCreate(&t->e0)); BFCG_CKN(bfcg_kcov_destroy(t), hipEventCreate(&t->e1));
	BFCG_CKN(bfcg_kcov_destroy(t), hipMalloc(&t->d_seq, max_pos)); BFCG_CKN(bfcg_kcov_destroy(t), hipMalloc(&t->d_flags, max_pos)); BFCG_CKN(bfcg_kcov_destroy(t), hipMalloc(&t->d_out, max_pos * 2));
	return t;
}

extern "C" bfcg_kcov_t *bfcg_kcov_create(const bfc_ch_t *ch, int device, uint64_t max_pos)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { fail("no HIP device available: the k-mer coverage pass has no CPU fallback here"); return NULL; }
	if (!ch || max_pos == 0) { fail("bad arguments to bfcg_kcov_create"); return NULL; }
	const int k = bfc_ch_get_k(ch), l_pre = bfc_ch_get_lpre(ch), cshift = bfc_ch_raw_cshift(ch);
	// left in HBM by bfc_count (bfcg_export_table_resident)?  Taken first, so that the object owns the copy whatever happens next
	unsigned long long *res = (unsigned long long *)resident_take(ch, device, 0, k, l_pre, cshift);
	bfcg_kcov_t *t = kcov_new(k, l_pre, cshift, device, max_pos, res, 1);
	if (!t) return NULL;
	t->adopted = res != 0;
	if (!t->table) {
		const uint64_t bytes = 8ULL << (l_pre + cshift);
		BFCG_CKN(bfcg_kcov_destroy(t), hipMalloc(&t->table, bytes));
		BFCG_CKN(bfcg_kcov_destroy(t), hipMemcpy(t->table, bfc_ch_raw_slots((bfc_ch_t *)ch), bytes, hipMemcpyHostToDevice));
	}
	return t;
}

// the table stays where the count kernels built it; the context must outlive the returned object and must not count meanwhile
extern "C" bfcg_kcov_t *bfcg_kcov_attach(bfcg_ctx_t *c, uint64_t max_pos)
{
	if (!c || ctx_table_k(c) < 0 || max_pos == 0) { fail("bfcg_kcov_attach needs a table-mode context"); return NULL; }
	KParams P; int device;
	const unsigned long long *tab = ctx_borrow_table(c, &P, &device); // drained, in the layout bfc_ch_kmer_occ probes
	if (!tab) return NULL;
	return kcov_new(P.k, P.l_pre, P.tab_cshift, device, max_pos, (unsigned long long *)tab, 0);
}

extern "C" void bfcg_kcov_destroy(bfcg_kcov_t *t)
{
	if (!t) return;
	(void)hipSetDevice(t->device);
	if (t->st) (void)hipStreamSynchronize(t->st);
	if (t->owns_table) (void)hipFree(t->table);
	(void)hipFree(t->d_seq); (void)hipFree(t->d_flags); (void)hipFree(t->d_out);
	if (t->e0) (void)hipEventDestroy(t->e0);
	if (t->e1) (void)hipEventDestroy(t->e1);
	if (t->st) (void)hipStreamDestroy(t->st);
	free(t);
}

// stream = batch format of PART 2; out[p] (host, may be NULL) / the device buffer of bfcg_kcov_dev_out() get one packed u16 per position
extern "C" int bfcg_kcov_batch(bfcg_kcov_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos, int min_occ, uint16_t *out)
{
	if (n_pos > t->max_pos) return fail("k-mer coverage batch exceeds the capacity given at creation");
	if (n_pos == 0) return 0;
	BFCG_CK(hipSetDevice(t->device));
	if (!d_seq) { BFCG_CK(hipMemcpyAsync(t->d_seq, h_seq, n_pos, hipMemcpyHostToDevice, t->st)); d_seq = t->d_seq; }
	BFCG_CK(hipEventRecord(t->e0, t->st));
	run_kcov(t->P, d_seq, (int64_t)n_pos, min_occ, t->table, t->d_flags, t->d_out, t->st);
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	if (out) BFCG_CK(hipMemcpyAsync(out, t->d_out, n_pos * 2, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&t->last_ms, t->e0, t->e1));
	return 0;
}
extern "C" float bfcg_kcov_last_ms(bfcg_kcov_t *t) { return t->last_ms; }
extern "C" void *bfcg_kcov_dev_seq(bfcg_kcov_t *t) { return t->d_seq; }
extern "C" void *bfcg_kcov_dev_out(bfcg_kcov_t *t) { return t->d_out; }
// the corrector (bfcg_ec.hip) runs behind a coverage context: its table in HBM, the probe parameters, the device it lives on
const unsigned long long *bfcg::kcov_table(bfcg_kcov_t *t, KParams *P, int *device) { *P = t->P; *device = t->device; return t->table; }
int bfcg::kcov_adopted(bfcg_kcov_t *t) { return t->adopted; }
