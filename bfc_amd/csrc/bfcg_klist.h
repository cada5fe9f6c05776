// bfcg_klist.h -- the listing of a count table, k_tab_list, for the files that list: bfcg_kmers.hip (bfcg_kmers_list, the table alone),
// bfcg_unitigs.hip (the ends of the graph's paths, left on the device: list_dev), bfcg_tabcmp.hip (bfcg_kmers_list_vs, the table filtered and annotated by a second one) and bfcg_graph.hip (bfcg_kmers_list_graph, by
// its own graph).  The three kernels and the host sequence around them are written once, as templates over what a predicate says about
// a slot:
//   NoOther        nothing: every slot that passes -m / -d is kept, no third output
//   a probing type keep(sub, slot, o): a third output column of its col_t per k-mer
//     VsOther   (bfcg_tabcmp.hip) o = the slot's key looked up in the other table, kept or not by its count
//     GraphPred (bfcg_graph.hip)  o = which of the slot's eight de Bruijn neighbours the table holds, kept or not by its degree cell
//     EndPred   (bfcg_unitigs.hip) o = the stop codes of a node's two sides, kept if one of them is open
//
//   k_tab_list   a range of sub-tables in blocks of LIST_BLK slots: k_list_count counts the slots that pass the filter per block,
//                k_list_scan turns the counts into offsets, k_list_emit decodes (bfcg_kdec.h) and stores in slot order -- sub-tables
//                ascending, because a sub-table is a contiguous run of slots.  The predicate is evaluated in both passes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfcg_internal.h"
#include "bfcg_kdec.h"

namespace {

enum { BT = 256, WAVES = BT / 64 };
enum { LIST_STEPS = 8, LIST_WAVE = LIST_STEPS * 128 /* slots a wave owns */, LIST_BLK = WAVES * LIST_WAVE /* slots per workgroup: 4096 */ };
enum { SCAN_BT = 1024, SCAN_PER = 8 };

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

struct NoOther { static constexpr bool probes = false; using col_t = int16_t; };

// Slots [s_lo, s_hi) of the table in blocks of LIST_BLK, block 0 starting at s_lo rounded down to a pair; a wave owns LIST_WAVE
// consecutive slots of its block, a lane slots 2l, 2l + 1 of each of its LIST_STEPS steps.
struct ListGeom { uint64_t s_lo, s_hi, base; int k, l_pre, cshift, min_cnt, min_diff; };

// ov[2j], ov[2j + 1]: what the other table answered for the two slots of step j (0 without one)
template <class O>
__device__ __forceinline__ void list_load(const ulonglong2 *__restrict__ tab, const ListGeom &G, const O &other, uint64_t wave_first, ulonglong2 v[LIST_STEPS],
                                          typename O::col_t ov[2 * LIST_STEPS])
{
	const int lane = lane_id();
#pragma unroll
	for (int j = 0; j < LIST_STEPS; ++j) {
		const uint64_t s = wave_first + (uint64_t)j * 128 + 2 * lane; // even
		ulonglong2 w = make_ulonglong2(0, 0);
		if (s < G.s_hi) w = tab[s >> 1];   // s_hi is even or the table's end is beyond it: the pair lies inside the table
		if (s < G.s_lo || !kdec::keep(w.x, G.min_cnt, G.min_diff)) w.x = 0;
		if (s + 1 < G.s_lo || s + 1 >= G.s_hi || !kdec::keep(w.y, G.min_cnt, G.min_diff)) w.y = 0;
		ov[2 * j] = ov[2 * j + 1] = 0;
		if constexpr (O::probes) {
			if (w.x && !other.keep((uint32_t)(s >> G.cshift), w.x, ov[2 * j])) w.x = 0;
			if (w.y && !other.keep((uint32_t)((s + 1) >> G.cshift), w.y, ov[2 * j + 1])) w.y = 0;
		}
		v[j] = w;
	}
}

template <class O>
__global__ __launch_bounds__(BT) void k_list_count(const ulonglong2 *__restrict__ tab, ListGeom G, O other, uint32_t *__restrict__ blk_cnt)
{
	__shared__ uint32_t wsum[WAVES];
	const int wave = threadIdx.x >> 6;
	ulonglong2 v[LIST_STEPS];
	typename O::col_t ov[2 * LIST_STEPS];
	list_load(tab, G, other, G.base + (uint64_t)blockIdx.x * LIST_BLK + (uint64_t)wave * LIST_WAVE, v, ov);
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

template <class O>
__global__ __launch_bounds__(BT) void k_list_emit(const ulonglong2 *__restrict__ tab, ListGeom G, O other, const unsigned long long *__restrict__ blk_off,
                                                  ulonglong2 *__restrict__ out_y, uint16_t *__restrict__ out_ch, typename O::col_t *__restrict__ out_other, uint64_t cap)
{
	__shared__ uint32_t wsum[WAVES];
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	const uint64_t wave_first = G.base + (uint64_t)blockIdx.x * LIST_BLK + (uint64_t)wave * LIST_WAVE;
	ulonglong2 v[LIST_STEPS];
	typename O::col_t ov[2 * LIST_STEPS];
	list_load(tab, G, other, wave_first, v, ov);
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
			if (o < cap) {
				out_y[o] = make_ulonglong2(a, b); out_ch[o] = (uint16_t)(v[j].x & 0x3fff);
				if constexpr (O::probes) out_other[o] = ov[2 * j];
			}
			++o;
		}
		if (v[j].y) {
			uint64_t a, b;
			kdec::decode(G.k, G.l_pre, (uint32_t)((s + 1) >> G.cshift), v[j].y, a, b);
			if (o < cap) {
				out_y[o] = make_ulonglong2(a, b); out_ch[o] = (uint16_t)(v[j].y & 0x3fff);
				if constexpr (O::probes) out_other[o] = ov[2 * j + 1];
			}
		}
		pos += __popcll(bx[j]) + __popcll(by[j]);
	}
}


// The device's side of one listing of sub-tables [sub_lo, sub_hi) of t, the arguments checked by the caller (`who` names it in messages;
// `have_bufs`: the caller has somewhere to put `cap` rows): count + scan, the total read back, then -- if it fits `cap` -- emit, after
// which the rows lie in t->d_y / d_ch / d_oth and the stream is idle.  0 / 1 / -1 as bfcg_kmers_list; t->last_ms = its kernels.
template <class O>
int list_dev(bfcg_kmers_t *t, const char *who, const O &other, int min_cnt, int min_diff, uint32_t sub_lo, uint32_t sub_hi, bool have_bufs, uint64_t cap, uint64_t *n)
{
	if (!kdec::decodable(t->k)) return bfcg::fail("k-mers cannot be listed for k=%d: the table's key is lossless only for k <= %d (sizes and histogram work for any k)", t->k, (int)kdec::MAX_K);
	if (sub_lo > sub_hi || (uint64_t)sub_hi > 1ULL << t->l_pre) return bfcg::fail("sub-table range [%u, %u) outside [0, 2^%d]", sub_lo, sub_hi, t->l_pre);
	if (cap && !have_bufs) return bfcg::fail("%s needs output buffers for cap=%llu", who, (unsigned long long)cap);
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
	hipLaunchKernelGGL((k_list_count<O>), dim3((unsigned)n_blk), dim3(BT), 0, t->st, (const ulonglong2 *)t->table, G, other, t->d_cnt);
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
	if (O::probes && bfcg::grow(t->d_oth, t->oth_cap, total * sizeof(typename O::col_t), "a listing's annotation") != 0) return -1;
	BFCG_CK(hipEventRecord(t->e0, t->st));
	hipLaunchKernelGGL((k_list_emit<O>), dim3((unsigned)n_blk), dim3(BT), 0, t->st, (const ulonglong2 *)t->table, G, other, t->d_off, t->d_y, t->d_ch, (typename O::col_t *)t->d_oth, (uint64_t)total);
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&ms2, t->e0, t->e1));
	t->last_ms = ms1 + ms2;
	return 0;
}

// ... and the host's: list_dev, then the rows copied out
template <class O>
int list_run(bfcg_kmers_t *t, const char *who, const O &other, int min_cnt, int min_diff, uint32_t sub_lo, uint32_t sub_hi, uint64_t *y, uint16_t *cnt_high,
             typename O::col_t *oth, uint64_t cap, uint64_t *n)
{
	const int rc = list_dev(t, who, other, min_cnt, min_diff, sub_lo, sub_hi, y && cnt_high && (!O::probes || oth), cap, n);
	if (rc != 0 || *n == 0) return rc;
	BFCG_CK(hipMemcpyAsync(y, t->d_y, *n * 16, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(cnt_high, t->d_ch, *n * 2, hipMemcpyDeviceToHost, t->st));
	if (O::probes) BFCG_CK(hipMemcpyAsync(oth, t->d_oth, *n * sizeof(typename O::col_t), hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipStreamSynchronize(t->st));
	return 0;
}

} // namespace
