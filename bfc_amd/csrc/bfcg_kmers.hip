// bfcg_kmers.hip -- the count table read out on the GPU: what the reference's hash2cnt prints from a dump (the k-mers with their counts,
// the spectrum, the sub-table sizes), from the table where it lies in HBM.  DESIGN.md section 6d.
//
// The table is the host's layout (bfcg_ctx.hip: B.table): 2^l_pre regions of 2^cshift slots, a slot = key << 14 | high << 8 | count,
// 0 = empty.  Both kernels stream it once, 16 bytes per lane:
//   k_tab_hist   the 256 + 64 bins in LDS (eight copies per wave: the spectrum is peaked, neighbouring lanes hit the same bin), flushed
//                with 64-bit atomics; the non-empty slots of every region in the same pass (wave ballots)
//   k_tab_list   a range of sub-tables in blocks of LIST_BLK slots, count / scan / emit: bfcg_klist.h, shared with bfcg_tabcmp.hip's
//                listing against a second table
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "bfcg_kdec.h"
#include "bfcg_klist.h"

namespace {

enum { HIST_BINS = 256 + 64, HIST_COPIES = 8 /* per wave */, HIST_UNROLL = 4 }; // BT, WAVES, lane_id: bfcg_klist.h

// ---- k_tab_hist -----------------------------------------------------------------------------------------------------------------
// A wave owns one contiguous span of slots (a multiple of 128 * HIST_UNROLL) and walks it 128 slots at a time, lane l holding slots
// 2l and 2l + 1 of the step.  Sub-table sizes: a region of 2^cshift slots is 2^(cshift - 1) lanes of a step; where that is the whole
// wave (cshift >= 7) the count stays in a register until the span leaves the region, else a region's first lane adds its popcount.
__global__ __launch_bounds__(BT) void k_tab_hist(const ulonglong2 *__restrict__ tab, uint64_t n_pairs, uint64_t span_pairs, int cshift,
                                                 unsigned long long *__restrict__ hist, uint32_t *__restrict__ sizes)
{
	__shared__ uint32_t h[WAVES * HIST_COPIES][HIST_BINS];
	for (int i = threadIdx.x; i < WAVES * HIST_COPIES * HIST_BINS; i += BT) (&h[0][0])[i] = 0;
	__syncthreads();
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	uint32_t *mine = h[wave * HIST_COPIES + (lane & (HIST_COPIES - 1))];
	const uint64_t gw = (uint64_t)blockIdx.x * WAVES + wave;
	const uint64_t p_lo = gw * span_pairs, p_hi = p_lo + span_pairs < n_pairs ? p_lo + span_pairs : n_pairs;
	// lanes of one region inside a step, and this lane's region mask (cshift 0: a lane holds two regions)
	const int g = cshift >= 7 ? 64 : cshift >= 1 ? 1 << (cshift - 1) : 1;
	const uint64_t gmask = g == 64 ? ~0ULL : ((1ULL << g) - 1) << (lane & ~(g - 1));
	uint64_t run_sub = ~0ULL; uint32_t run_cnt = 0; // cshift >= 7
	for (uint64_t p = p_lo; p < p_hi; p += 64 * HIST_UNROLL) {
		ulonglong2 v[HIST_UNROLL];
#pragma unroll
		for (int j = 0; j < HIST_UNROLL; ++j) {
			const uint64_t q = p + (uint64_t)j * 64 + lane;
			v[j] = q < p_hi ? tab[q] : make_ulonglong2(0, 0);
		}
#pragma unroll
		for (int j = 0; j < HIST_UNROLL; ++j) {
			const uint64_t q = p + (uint64_t)j * 64 + lane;
			const uint64_t x = v[j].x, y = v[j].y;
			if (x) { atomicAdd(&mine[x & 0xff], 1u); atomicAdd(&mine[256 + (x >> 8 & 0x3f)], 1u); }
			if (y) { atomicAdd(&mine[y & 0xff], 1u); atomicAdd(&mine[256 + (y >> 8 & 0x3f)], 1u); }
			const uint64_t bx = __ballot(x != 0), by = __ballot(y != 0);
			if (cshift == 0) {
				if (x) sizes[2 * q] = 1;
				if (y) sizes[2 * q + 1] = 1;
			} else if (g < 64) {
				const uint32_t n = __popcll(bx & gmask) + __popcll(by & gmask);
				if ((lane & (g - 1)) == 0 && n && q < p_hi) atomicAdd(&sizes[(2 * q) >> cshift], n);
			} else {
				const uint64_t sub = (2 * (p + (uint64_t)j * 64)) >> cshift; // wave-uniform
				if (sub != run_sub) {
					if (lane == 0 && run_cnt) atomicAdd(&sizes[run_sub], run_cnt);
					run_sub = sub; run_cnt = 0;
				}
				run_cnt += __popcll(bx) + __popcll(by);
			}
		}
	}
	if (g == 64 && lane == 0 && run_cnt) atomicAdd(&sizes[run_sub], run_cnt);
	__syncthreads();
	for (int b = threadIdx.x; b < HIST_BINS; b += BT) {
		unsigned long long s = 0;
		for (int c = 0; c < WAVES * HIST_COPIES; ++c) s += h[c][b];
		if (s) atomicAdd(&hist[b], s);
	}
}

} // namespace

// ---- the context ------------------------------------------------------------------------------------------------------------------

// (struct bfcg_kmers: bfcg_internal.h -- bfcg_lookup.hip works on the same object)

// a failure after the calloc frees what was made so far (bfcg_kmers_destroy takes a half-built object)

bfcg_kmers_t *bfcg::kmers_new(int k, int l_pre, int cshift, int device)
{
	if (l_pre + cshift < 1 || l_pre + cshift > 40) { bfcg::fail("a count table of 2^%d slots cannot be read out", l_pre + cshift); return NULL; }
	BFCG_CKN((void)0, hipSetDevice(device));
	bfcg_kmers_t *t = (bfcg_kmers_t *)calloc(1, sizeof(bfcg_kmers_t));
	if (!t) { bfcg::fail("out of host memory"); return NULL; }
	t->k = k; t->l_pre = l_pre; t->cshift = cshift; t->device = device;
	t->q_cap = bfcg::lookup_cap(); t->ut_cap = bfcg::unitig_cap(); t->link_map_min = bfcg::link_map_min();
	BFCG_CKN(bfcg_kmers_destroy(t), hipStreamCreate(&t->st));
	BFCG_CKN(bfcg_kmers_destroy(t), hipEventCreate(&t->e0)); BFCG_CKN(bfcg_kmers_destroy(t), hipEventCreate(&t->e1));
	BFCG_CKN(bfcg_kmers_destroy(t), hipMalloc(&t->d_hist, HIST_BINS * 8));
	BFCG_CKN(bfcg_kmers_destroy(t), hipMalloc(&t->d_sizes, 4ULL << l_pre));
	return t;
}

extern "C" bfcg_kmers_t *bfcg_kmers_create(const bfc_ch_t *ch, int device)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { bfcg::fail("no HIP device available: the table read-out has no CPU fallback here"); return NULL; }
	if (!ch || device < 0 || device >= ndev) { bfcg::fail("bad arguments to bfcg_kmers_create"); return NULL; }
	bfcg_kmers_t *t = bfcg::kmers_new(bfc_ch_get_k(ch), bfc_ch_get_lpre(ch), bfc_ch_raw_cshift(ch), device);
	if (!t) return NULL;
	const uint64_t bytes = 8ULL << (t->l_pre + t->cshift);
	unsigned long long *tab = NULL;
	BFCG_CKN(bfcg_kmers_destroy(t), hipMalloc(&tab, bytes));
	t->table = tab; t->owns_table = 1;
	BFCG_CKN(bfcg_kmers_destroy(t), hipMemcpy(tab, bfc_ch_raw_slots((bfc_ch_t *)ch), bytes, hipMemcpyHostToDevice));
	return t;
}

// the table stays where the count kernels built it (bfcg_kcov_attach's contract): the context must outlive the returned object and must not count meanwhile
extern "C" bfcg_kmers_t *bfcg_kmers_attach(bfcg_ctx_t *c)
{
	bfcg::KParams P; int device;
	const unsigned long long *tab = bfcg::ctx_borrow_table(c, &P, &device);
	if (!tab) return NULL;
	bfcg_kmers_t *t = bfcg::kmers_new(P.k, P.l_pre, P.tab_cshift, device);
	if (!t) return NULL;
	t->table = tab;
	return t;
}

extern "C" void bfcg_kmers_destroy(bfcg_kmers_t *t)
{
	if (!t) return;
	(void)hipSetDevice(t->device);
	if (t->st) (void)hipStreamSynchronize(t->st);
	if (t->owns_table) (void)hipFree((void *)t->table);
	(void)hipFree(t->d_hist); (void)hipFree(t->d_sizes); (void)hipFree(t->d_cnt); (void)hipFree(t->d_off); (void)hipFree(t->d_y); (void)hipFree(t->d_ch);
	(void)hipFree(t->d_qy); (void)hipFree(t->d_qout); (void)hipFree(t->d_pseq); (void)hipFree(t->d_pout); (void)hipFree(t->d_roff); (void)hipFree(t->d_rout);
	(void)hipFree(t->d_oth); (void)hipFree(t->d_joint); (void)hipFree(t->d_jpart); (void)hipFree(t->d_gout); (void)hipFree(t->d_gls);
	for (int i = 0; i < BFCG_UT_NBUF; ++i) (void)hipFree(t->d_ut[i]);
	if (t->e0) (void)hipEventDestroy(t->e0);
	if (t->e1) (void)hipEventDestroy(t->e1);
	if (t->st) (void)hipStreamDestroy(t->st);
	free(t);
}

extern "C" int bfcg_kmers_info(bfcg_kmers_t *t, int out[3])
{
	if (!t || !out) return bfcg::fail("bad arguments to bfcg_kmers_info");
	out[0] = t->k; out[1] = t->l_pre; out[2] = t->cshift;
	return 0;
}

// one pass of k_tab_hist: the bins and the sizes land in d_hist / d_sizes
static int run_hist(bfcg_kmers_t *t)
{
	BFCG_CK(hipSetDevice(t->device));
	const uint64_t n_pairs = 1ULL << (t->l_pre + t->cshift - 1), step = 64 * HIST_UNROLL;
	uint64_t grid = (n_pairs + step * WAVES - 1) / (step * WAVES);
	if (grid > 1024) grid = 1024; // four workgroups on each of the 256 CUs
	const uint64_t waves = grid * WAVES, span = ((n_pairs + waves - 1) / waves + step - 1) / step * step;
	BFCG_CK(hipMemsetAsync(t->d_hist, 0, HIST_BINS * 8, t->st));
	BFCG_CK(hipMemsetAsync(t->d_sizes, 0, 4ULL << t->l_pre, t->st));
	BFCG_CK(hipEventRecord(t->e0, t->st));
	hipLaunchKernelGGL(k_tab_hist, dim3((unsigned)grid), dim3(BT), 0, t->st, (const ulonglong2 *)t->table, n_pairs, span, t->cshift, t->d_hist, t->d_sizes);
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	return 0;
}

// k_tab_hist fills the bins and the sizes in the same pass: one call hands out both (cnt / high together, or sizes, may be NULL)
extern "C" int bfcg_kmers_hist_sizes(bfcg_kmers_t *t, uint64_t cnt[256], uint64_t high[64], uint32_t *sizes)
{
	if (!t || !cnt != !high || (!cnt && !sizes)) { bfcg::fail("bad arguments to bfcg_kmers_hist_sizes"); return -2; }
	uint64_t h[HIST_BINS];
	if (run_hist(t) != 0) return -2;
	hipError_t e = cnt ? hipMemcpyAsync(h, t->d_hist, sizeof(h), hipMemcpyDeviceToHost, t->st) : hipSuccess;
	if (e == hipSuccess && sizes) e = hipMemcpyAsync(sizes, t->d_sizes, 4ULL << t->l_pre, hipMemcpyDeviceToHost, t->st);
	if (e == hipSuccess) e = hipStreamSynchronize(t->st);
	if (e == hipSuccess) e = hipEventElapsedTime(&t->last_ms, t->e0, t->e1);
	if (e != hipSuccess) { bfcg::fail("reading the histogram and the sub-table sizes back failed: %s", hipGetErrorString(e)); return -2; }
	if (!cnt) return -1;
	memcpy(cnt, h, 256 * 8); memcpy(high, h + 256, 64 * 8);
	uint64_t max = 0; int mode = -1; // bfc_ch_hist: the largest bin with i >= 3, the first on ties
	for (int i = 3; i < 256; ++i) if (cnt[i] > max) { max = cnt[i]; mode = i; }
	return mode;
}

extern "C" int bfcg_kmers_hist(bfcg_kmers_t *t, uint64_t cnt[256], uint64_t high[64])
{
	if (!cnt || !high) { bfcg::fail("bad arguments to bfcg_kmers_hist"); return -2; }
	return bfcg_kmers_hist_sizes(t, cnt, high, NULL);
}

extern "C" int bfcg_kmers_sub_sizes(bfcg_kmers_t *t, uint32_t *sizes)
{
	if (!sizes) return bfcg::fail("bad arguments to bfcg_kmers_sub_sizes");
	return bfcg_kmers_hist_sizes(t, NULL, NULL, sizes) == -2 ? -1 : 0;
}

extern "C" int bfcg_kmers_list(bfcg_kmers_t *t, int min_cnt, int min_diff, uint32_t sub_lo, uint32_t sub_hi, uint64_t *y, uint16_t *cnt_high, uint64_t cap, uint64_t *n)
{
	if (!t || !n) return bfcg::fail("bad arguments to bfcg_kmers_list");
	return list_run(t, "bfcg_kmers_list", NoOther(), min_cnt, min_diff, sub_lo, sub_hi, y, cnt_high, NULL, cap, n);
}

extern "C" float bfcg_kmers_last_ms(bfcg_kmers_t *t) { return t ? t->last_ms : 0.0f; }

// ---- the header's host instance, and the text forms ---------------------------------------------------------------------------------

extern "C" int bfcg_kmer_decode_host(int k, int l_pre, uint32_t sub, uint64_t slot, uint64_t y[2])
{
	if (!kdec::decodable(k) || l_pre < 0 || l_pre > BFC_CH_MAXPRE || (k <= 32 ? 2 * k - l_pre < 0 || 2 * k - l_pre > BFC_CH_KEYBITS : k - l_pre < 0)) return -1;
	kdec::decode(k, l_pre, sub, slot, y[0], y[1]);
	uint64_t Y0, Y1, Z0, Z1; // hash(decode(x)) == x
	kdec::slot_to_hash(k, l_pre, sub, slot, Y0, Y1);
	kdec::kmer_to_hash(k, y[0], y[1], Z0, Z1);
	return Y0 == Z0 && Y1 == Z1 ? 0 : -1;
}

extern "C" void bfcg_kmer_2str(int k, const uint64_t y[2], char *buf)
{
	for (int l = 0; l < k; ++l) buf[k - 1 - l] = "ACGT"[(y[1] >> l & 1) << 1 | (y[0] >> l & 1)];
	buf[k] = 0;
}

static inline char *put_u32(char *p, uint32_t v)
{
	char tmp[10]; int n = 0;
	do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
	while (n) *p++ = tmp[--n];
	return p;
}

// hash2cnt's lines, "%s\t%d\t%d\n" per k-mer (count, high), into buf (n * (k + 8) bytes at most); returns the bytes written
extern "C" uint64_t bfcg_kmers_format(int k, const uint64_t *y, const uint16_t *cnt_high, uint64_t n, char *buf)
{
	char *p = buf;
	for (uint64_t i = 0; i < n; ++i) {
		const uint64_t a = y[2 * i], b = y[2 * i + 1];
		for (int l = 0; l < k; ++l) p[k - 1 - l] = "ACGT"[(b >> l & 1) << 1 | (a >> l & 1)];
		p += k; *p++ = '\t';
		p = put_u32(p, cnt_high[i] & 0xff); *p++ = '\t';
		p = put_u32(p, cnt_high[i] >> 8 & 0x3f); *p++ = '\n';
	}
	return (uint64_t)(p - buf);
}

// a listing against a second table (bfcg_kmers_list_vs), "%s\t%d\t%d\t%d\t%d\n" per k-mer: count, high, and the two in the other table
// (0 0 where it is absent there), into buf (n * (k + 16) bytes at most); returns the bytes written
extern "C" uint64_t bfcg_kmers_format_vs(int k, const uint64_t *y, const uint16_t *cnt_high, const int16_t *other, uint64_t n, char *buf)
{
	char *p = buf;
	for (uint64_t i = 0; i < n; ++i) {
		const uint64_t a = y[2 * i], b = y[2 * i + 1];
		const uint32_t o = other[i] < 0 ? 0 : (uint32_t)other[i];
		for (int l = 0; l < k; ++l) p[k - 1 - l] = "ACGT"[(b >> l & 1) << 1 | (a >> l & 1)];
		p += k; *p++ = '\t';
		p = put_u32(p, cnt_high[i] & 0xff); *p++ = '\t';
		p = put_u32(p, cnt_high[i] >> 8 & 0x3f); *p++ = '\t';
		p = put_u32(p, o & 0xff); *p++ = '\t';
		p = put_u32(p, o >> 8 & 0x3f); *p++ = '\n';
	}
	return (uint64_t)(p - buf);
}

// "%d\n" per sub-table (hash2cnt -s), into buf (11 bytes per line at most); returns the bytes written
extern "C" uint64_t bfcg_kmers_format_sizes(const uint32_t *sizes, uint64_t n, char *buf)
{
	char *p = buf;
	for (uint64_t i = 0; i < n; ++i) { p = put_u32(p, sizes[i]); *p++ = '\n'; }
	return (uint64_t)(p - buf);
}
