// bfcg_kmers.hip -- the count table read out on the GPU: what the reference's hash2cnt prints from a dump (the k-mers with their counts,
// the spectrum, the sub-table sizes), from the table where it lies in HBM.  DESIGN.md section 6d.
//
// The table is the host's layout (bfcg_ctx.hip: B.table): 2^l_pre regions of 2^cshift slots, a slot = key << 14 | high << 8 | count,
// 0 = empty.  Both kernels stream it once, 16 bytes per lane:
//   k_tab_hist   the 256 + 64 bins in LDS (eight copies per wave: the spectrum is peaked, neighbouring lanes hit the same bin), flushed
//                with 64-bit atomics; the non-empty slots of every region in the same pass (wave ballots)
//   k_tab_list   a range of sub-tables in blocks of LIST_BLK slots: k_list_count counts the slots that pass the filter per block,
//                k_list_scan turns the counts into offsets, k_list_emit decodes (bfcg_kdec.h) and stores in slot order -- sub-tables
//                ascending, because a sub-table is a contiguous run of slots
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "bfcg_kdec.h"

namespace {

enum { BT = 256, WAVES = BT / 64, HIST_BINS = 256 + 64, HIST_COPIES = 8 /* per wave */, HIST_UNROLL = 4 };
enum { LIST_STEPS = 8, LIST_WAVE = LIST_STEPS * 128 /* slots a wave owns */, LIST_BLK = WAVES * LIST_WAVE /* slots per workgroup: 4096 */ };
enum { SCAN_BT = 1024, SCAN_PER = 8 };

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

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

// ---- k_tab_list -----------------------------------------------------------------------------------------------------------------
// Slots [s_lo, s_hi) of the table in blocks of LIST_BLK, block 0 starting at s_lo rounded down to a pair; a wave owns LIST_WAVE
// consecutive slots of its block, a lane slots 2l, 2l + 1 of each of its LIST_STEPS steps.
struct ListGeom { uint64_t s_lo, s_hi, base; int k, l_pre, cshift, min_cnt, min_diff; };

__device__ __forceinline__ void list_load(const ulonglong2 *__restrict__ tab, const ListGeom &G, uint64_t wave_first, ulonglong2 v[LIST_STEPS])
{
	const int lane = lane_id();
#pragma unroll
	for (int j = 0; j < LIST_STEPS; ++j) {
		const uint64_t s = wave_first + (uint64_t)j * 128 + 2 * lane; // even
		ulonglong2 w = make_ulonglong2(0, 0);
		if (s < G.s_hi) w = tab[s >> 1];   // s_hi is even or the table's end is beyond it: the pair lies inside the table
		if (s < G.s_lo || !kdec::keep(w.x, G.min_cnt, G.min_diff)) w.x = 0;
		if (s + 1 < G.s_lo || s + 1 >= G.s_hi || !kdec::keep(w.y, G.min_cnt, G.min_diff)) w.y = 0;
		v[j] = w;
	}
}

__global__ __launch_bounds__(BT) void k_list_count(const ulonglong2 *__restrict__ tab, ListGeom G, uint32_t *__restrict__ blk_cnt)
{
	__shared__ uint32_t wsum[WAVES];
	const int wave = threadIdx.x >> 6;
	ulonglong2 v[LIST_STEPS];
	list_load(tab, G, G.base + (uint64_t)blockIdx.x * LIST_BLK + (uint64_t)wave * LIST_WAVE, v);
	uint32_t n = 0;
#pragma unroll
	for (int j = 0; j < LIST_STEPS; ++j) n += __popcll(__ballot(v[j].x != 0)) + __popcll(__ballot(v[j].y != 0));
	if (lane_id() == 0) wsum[wave] = n;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t s = 0;
		for (int w = 0; w < WAVES; ++w) s += wsum[w];
		blk_cnt[blockIdx.x] = s;
	}
}

// exclusive scan of cnt[0, n_pad) (n_pad a multiple of SCAN_BT * SCAN_PER, the padding zero) into 64-bit offsets; off[n_pad] = total.  One workgroup:
// the array has one entry per 4096 slots.
__global__ __launch_bounds__(SCAN_BT) void k_list_scan(const uint32_t *__restrict__ cnt, uint64_t n_pad, unsigned long long *__restrict__ off)
{
	__shared__ unsigned long long wtot[SCAN_BT / 64];
	__shared__ unsigned long long carry_s;
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	unsigned long long carry = 0;
	for (uint64_t base = 0; base < n_pad; base += SCAN_BT * SCAN_PER) {
		const uint64_t i0 = base + (uint64_t)threadIdx.x * SCAN_PER;
		uint32_t c[SCAN_PER];
		unsigned long long mine = 0;
#pragma unroll
		for (int j = 0; j < SCAN_PER; ++j) { c[j] = cnt[i0 + j]; mine += c[j]; }
		unsigned long long incl = mine; // inclusive scan over the wave
#pragma unroll
		for (int d = 1; d < 64; d <<= 1) {
			const unsigned long long o = __shfl_up(incl, d, 64);
			if (lane >= d) incl += o;
		}
		if (lane == 63) wtot[wave] = incl;
		__syncthreads();
		unsigned long long before = carry;
		for (int w = 0; w < wave; ++w) before += wtot[w];
		if (threadIdx.x == SCAN_BT - 1) carry_s = before + incl;
		unsigned long long o = before + incl - mine;
#pragma unroll
		for (int j = 0; j < SCAN_PER; ++j) { off[i0 + j] = o; o += c[j]; }
		__syncthreads();
		carry = carry_s;
	}
	if (threadIdx.x == 0) off[n_pad] = carry;
}

__global__ __launch_bounds__(BT) void k_list_emit(const ulonglong2 *__restrict__ tab, ListGeom G, const unsigned long long *__restrict__ blk_off,
                                                  ulonglong2 *__restrict__ out_y, uint16_t *__restrict__ out_ch, uint64_t cap)
{
	__shared__ uint32_t wsum[WAVES];
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	const uint64_t wave_first = G.base + (uint64_t)blockIdx.x * LIST_BLK + (uint64_t)wave * LIST_WAVE;
	ulonglong2 v[LIST_STEPS];
	list_load(tab, G, wave_first, v);
	uint64_t bx[LIST_STEPS], by[LIST_STEPS];
	uint32_t n = 0;
#pragma unroll
	for (int j = 0; j < LIST_STEPS; ++j) { bx[j] = __ballot(v[j].x != 0); by[j] = __ballot(v[j].y != 0); n += __popcll(bx[j]) + __popcll(by[j]); }
	if (lane == 0) wsum[wave] = n;
	__syncthreads();
	uint64_t pos = blk_off[blockIdx.x];
	for (int w = 0; w < wave; ++w) pos += wsum[w];
	const uint64_t below = (1ULL << lane) - 1;
#pragma unroll
	for (int j = 0; j < LIST_STEPS; ++j) {
		const uint64_t s = wave_first + (uint64_t)j * 128 + 2 * lane;
		uint64_t o = pos + __popcll(bx[j] & below) + __popcll(by[j] & below); // slot order: lane-major, x before y
		if (v[j].x) {
			uint64_t a, b;
			kdec::decode(G.k, G.l_pre, (uint32_t)(s >> G.cshift), v[j].x, a, b);
			if (o < cap) { out_y[o] = make_ulonglong2(a, b); out_ch[o] = (uint16_t)(v[j].x & 0x3fff); }
			++o;
		}
		if (v[j].y) {
			uint64_t a, b;
			kdec::decode(G.k, G.l_pre, (uint32_t)((s + 1) >> G.cshift), v[j].y, a, b);
			if (o < cap) { out_y[o] = make_ulonglong2(a, b); out_ch[o] = (uint16_t)(v[j].y & 0x3fff); }
		}
		pos += __popcll(bx[j]) + __popcll(by[j]);
	}
}

} // namespace

// ---- the context ------------------------------------------------------------------------------------------------------------------

// (struct bfcg_kmers: bfcg_internal.h -- bfcg_lookup.hip works on the same object)

// a failure after the calloc frees what was made so far (bfcg_kmers_destroy takes a half-built object)

static bfcg_kmers_t *kmers_new(int k, int l_pre, int cshift, int device)
{
	if (l_pre + cshift < 1 || l_pre + cshift > 40) { bfcg::fail("a count table of 2^%d slots cannot be read out", l_pre + cshift); return NULL; }
	BFCG_CKN((void)0, hipSetDevice(device));
	bfcg_kmers_t *t = (bfcg_kmers_t *)calloc(1, sizeof(bfcg_kmers_t));
	if (!t) { bfcg::fail("out of host memory"); return NULL; }
	t->k = k; t->l_pre = l_pre; t->cshift = cshift; t->device = device;
	t->q_cap = bfcg::lookup_cap();
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
	bfcg_kmers_t *t = kmers_new(bfc_ch_get_k(ch), bfc_ch_get_lpre(ch), bfc_ch_raw_cshift(ch), device);
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
	bfcg_kmers_t *t = kmers_new(P.k, P.l_pre, P.tab_cshift, device);
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
	if (!kdec::decodable(t->k)) return bfcg::fail("k-mers cannot be listed for k=%d: the table's key is lossless only for k <= %d (sizes and histogram work for any k)", t->k, (int)kdec::MAX_K);
	if (sub_lo > sub_hi || (uint64_t)sub_hi > 1ULL << t->l_pre) return bfcg::fail("sub-table range [%u, %u) outside [0, 2^%d]", sub_lo, sub_hi, t->l_pre);
	if (cap && (!y || !cnt_high)) return bfcg::fail("bfcg_kmers_list needs output buffers for cap=%llu", (unsigned long long)cap);
	*n = 0; t->last_ms = 0;
	if (sub_lo == sub_hi) return 0;
	BFCG_CK(hipSetDevice(t->device));
	ListGeom G;
	G.s_lo = (uint64_t)sub_lo << t->cshift; G.s_hi = (uint64_t)sub_hi << t->cshift; G.base = G.s_lo & ~1ULL;
	G.k = t->k; G.l_pre = t->l_pre; G.cshift = t->cshift; G.min_cnt = min_cnt; G.min_diff = min_diff;
	const uint64_t n_blk = (G.s_hi - G.base + LIST_BLK - 1) / LIST_BLK, per = SCAN_BT * SCAN_PER, n_pad = (n_blk + per - 1) / per * per;
	if (n_blk >= 1ULL << 24) return bfcg::fail("sub-table range of %llu slots is too large for one listing: walk it in pieces", (unsigned long long)(G.s_hi - G.s_lo)); // a launch has fewer than 2^32 threads
	if (n_pad > t->blk_cap) {
		(void)hipFree(t->d_cnt); (void)hipFree(t->d_off); t->d_cnt = NULL; t->d_off = NULL; t->blk_cap = 0;
		BFCG_CK(hipMalloc(&t->d_cnt, n_pad * 4)); BFCG_CK(hipMalloc(&t->d_off, (n_pad + 1) * 8));
		t->blk_cap = n_pad;
	}
	float ms1 = 0, ms2 = 0;
	if (n_pad > n_blk) BFCG_CK(hipMemsetAsync(t->d_cnt + n_blk, 0, (n_pad - n_blk) * 4, t->st)); // the scan's padding
	BFCG_CK(hipEventRecord(t->e0, t->st));
	hipLaunchKernelGGL(k_list_count, dim3((unsigned)n_blk), dim3(BT), 0, t->st, (const ulonglong2 *)t->table, G, t->d_cnt);
	hipLaunchKernelGGL(k_list_scan, dim3(1), dim3(SCAN_BT), 0, t->st, t->d_cnt, n_pad, t->d_off);
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	unsigned long long total = 0;
	BFCG_CK(hipMemcpyAsync(&total, t->d_off + n_pad, 8, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&ms1, t->e0, t->e1));
	t->last_ms = ms1;
	*n = total;
	if (total > cap) return 1; // nothing is written: the caller comes back with room for *n
	if (total == 0) return 0;
	if (total > t->out_cap) {
		(void)hipFree(t->d_y); (void)hipFree(t->d_ch); t->d_y = NULL; t->d_ch = NULL; t->out_cap = 0;
		BFCG_CK(hipMalloc(&t->d_y, total * 16)); BFCG_CK(hipMalloc(&t->d_ch, total * 2));
		t->out_cap = total;
	}
	BFCG_CK(hipEventRecord(t->e0, t->st));
	hipLaunchKernelGGL(k_list_emit, dim3((unsigned)n_blk), dim3(BT), 0, t->st, (const ulonglong2 *)t->table, G, t->d_off, t->d_y, t->d_ch, (uint64_t)total);
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(y, t->d_y, total * 16, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(cnt_high, t->d_ch, total * 2, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&ms2, t->e0, t->e1));
	t->last_ms = ms1 + ms2;
	return 0;
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

// "%d\n" per sub-table (hash2cnt -s), into buf (11 bytes per line at most); returns the bytes written
extern "C" uint64_t bfcg_kmers_format_sizes(const uint32_t *sizes, uint64_t n, char *buf)
{
	char *p = buf;
	for (uint64_t i = 0; i < n; ++i) { p = put_u32(p, sizes[i]); *p++ = '\n'; }
	return (uint64_t)(p - buf);
}
