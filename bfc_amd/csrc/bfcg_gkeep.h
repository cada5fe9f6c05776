// bfcg_gkeep.h -- the marks-to-table half of a graph-cleaning round, for the files that remove nodes of the count table's de Bruijn graph
// into a new table: bfcg_clip.hip (tips and islands) and bfcg_pop.hip (simple bubbles).  Their walks set one KILL bit per slot of a removed
// node (set_mark, bfcg_glink.h) in d_ut[B_MARK] and count in d_ut[B_CTR]; what follows is the same for both:
//   k_clip_sizes  a streaming pass over the slot pairs: the survivors (count >= min_cnt, no KILL bit) per sub-table, by wave ballots;
//                 they fix the new table's geometry by the union's rule, so a region cannot overflow
//   k_clip_fill   a streaming pass that upserts every survivor into the zeroed new table; the made and full counters are checked as the
//                 union's are
//   clip_keep     the two passes around the new object; `who` names the caller in messages
// and for the host twins HostSlots (bfc_ch_export_sorted of a table), NodeSet (the removed nodes as their smaller strands) and
// clip_keep_host, which inserts the survivors into a table allocated at the same cshift rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <vector>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "kmer_dev.h"
#include "bfcg_klist.h"
#include "bfcg_gprobe.h"
#include "bfcg_glink.h"
#include "bfcg_upsert.h"

namespace {

enum { CLIP_GRID_MAX = 256 * 8, CLIP_MAX_ROUNDS = 64 };
enum { CC_ERR, CC_UNITIGS /* the unitigs a round removed: tips and islands, or a bubble's arm each */, CC_KMERS, CC_MADE, CC_FULL, CC_N }; // the call's counters in d_ut[B_CTR]

// ---- the two streaming passes ----------------------------------------------------------------------------------------------------------------
// the survivors of pair q: slot 2q in s0, slot 2q + 1 in s1 (an empty slot has count 0 < min_cnt)
__device__ __forceinline__ void survivors(const ulonglong2 v, const uint32_t *__restrict__ kill, uint64_t q, int min_cnt, bool &s0, bool &s1)
{
	const uint32_t bits = kill[q >> 4] >> (2 * (q & 15));
	s0 = (int)(v.x & 0xff) >= min_cnt && !(bits & 1); s1 = (int)(v.y & 0xff) >= min_cnt && !(bits & 2);
}

// sizes[sub] += the survivors of sub-table sub.  A wave's step is 128 consecutive slots, aligned: the lanes of one region add one popcount
// (k_tab_hist's ballots, bfcg_kmers.hip)
__global__ __launch_bounds__(BT) void k_clip_sizes(const ulonglong2 *__restrict__ tab, uint64_t n_pairs, int cshift, int min_cnt, const uint32_t *__restrict__ kill,
                                                   uint32_t *__restrict__ sizes)
{
	const int lane = lane_id();
	const int g = cshift >= 7 ? 64 : cshift >= 1 ? 1 << (cshift - 1) : 1; // lanes of one region inside a step
	const uint64_t gmask = g == 64 ? ~0ULL : ((1ULL << g) - 1) << (lane & ~(g - 1));
	for (uint64_t q = (uint64_t)blockIdx.x * BT + threadIdx.x; q < n_pairs; q += (uint64_t)gridDim.x * BT) {
		bool s0, s1;
		survivors(tab[q], kill, q, min_cnt, s0, s1);
		const uint64_t b0 = __ballot(s0), b1 = __ballot(s1);
		if (cshift == 0) { // a lane holds two regions
			if (s0) sizes[2 * q] = 1;
			if (s1) sizes[2 * q + 1] = 1;
		} else {
			const uint32_t n = __popcll(b0 & gmask) + __popcll(b1 & gmask);
			if ((lane & (g - 1)) == 0 && n) atomicAdd(&sizes[(2 * q) >> cshift], n);
		}
	}
}

__global__ __launch_bounds__(BT) void k_clip_fill(const ulonglong2 *__restrict__ src, uint64_t n_pairs, int cshift_src, int min_cnt, const uint32_t *__restrict__ kill,
                                                  unsigned long long *__restrict__ dst, int cshift_dst, unsigned long long *__restrict__ ctr)
{
	uint32_t made = 0, full = 0;
	for (uint64_t q = (uint64_t)blockIdx.x * BT + threadIdx.x; q < n_pairs; q += (uint64_t)gridDim.x * BT) {
		const ulonglong2 v = src[q];
		bool s0, s1;
		survivors(v, kill, q, min_cnt, s0, s1);
		if (s0) { const uint32_t r = union_upsert(dst, cshift_dst, (2 * q) >> cshift_src, v.x); made += r == 1; full += r != 1; }
		if (s1) { const uint32_t r = union_upsert(dst, cshift_dst, (2 * q + 1) >> cshift_src, v.y); made += r == 1; full += r != 1; }
	}
#pragma unroll
	for (int d = 32; d; d >>= 1) { made += __shfl_down(made, d, 64); full += __shfl_down(full, d, 64); }
	if (lane_id() == 0) {
		if (made) atomicAdd(&ctr[CC_MADE], (unsigned long long)made);
		if (full) atomicAdd(&ctr[CC_FULL], (unsigned long long)full);
	}
}

// ---- the host's side ---------------------------------------------------------------------------------------------------------------------------
// the union's rule on the survivors: the smallest table that is at most half full and whose regions take all their keys
int clip_cshift(int l_pre, uint64_t keys, uint64_t most)
{
	int cshift = 2;
	while (cshift < 39 /* kmers_new refuses more than 2^40 slots */ && (1ULL << (l_pre + cshift) < 2 * keys || 1ULL << cshift < most)) ++cshift;
	return cshift;
}

unsigned clip_grid(uint64_t n_pairs)
{
	const uint64_t grid = (n_pairs + BT - 1) / BT;
	return (unsigned)(grid < CLIP_GRID_MAX ? grid : CLIP_GRID_MAX);
}

// the sizes pass over c with its KILL bits as the round's marking left them: sizes[2^l_pre] on the host
int clip_sizes(bfcg_kmers_t *c, int min_cnt, uint32_t *sizes, float *ms)
{
	const uint64_t n_pairs = 1ULL << (c->l_pre + c->cshift - 1);
	BFCG_CK(hipEventRecord(c->e0, c->st));
	BFCG_CK(hipMemsetAsync(c->d_sizes, 0, 4ULL << c->l_pre, c->st));
	hipLaunchKernelGGL(k_clip_sizes, dim3(clip_grid(n_pairs)), dim3(BT), 0, c->st, (const ulonglong2 *)c->table, n_pairs, c->cshift, min_cnt, ut_buf<uint32_t>(c, B_MARK), c->d_sizes);
	BFCG_CK(hipEventRecord(c->e1, c->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(sizes, c->d_sizes, 4ULL << c->l_pre, hipMemcpyDeviceToHost, c->st));
	return ut_lap(c, ms);
}

// The table of c's survivors: a new object that owns it.  The kernels run on c's stream, where the KILL bits were written
bfcg_kmers_t *clip_keep(bfcg_kmers_t *c, const char *who, int min_cnt, float *ms)
{
	const uint64_t n_sub = 1ULL << c->l_pre, n_pairs = 1ULL << (c->l_pre + c->cshift - 1);
	uint32_t *sizes = (uint32_t *)malloc(n_sub * 4);
	if (!sizes) { bfcg::fail("out of host memory"); return NULL; }
	if (clip_sizes(c, min_cnt, sizes, ms) != 0) { free(sizes); return NULL; }
	uint64_t keys = 0, most = 0;
	for (uint64_t s = 0; s < n_sub; ++s) {
		keys += sizes[s];
		if (sizes[s] > most) most = sizes[s];
	}
	free(sizes);
	bfcg_kmers_t *u = bfcg::kmers_new(c->k, c->l_pre, clip_cshift(c->l_pre, keys, most), c->device);
	if (!u) return NULL;
	const uint64_t bytes = 8ULL << (u->l_pre + u->cshift);
	unsigned long long *tab = NULL, ctr[CC_N];
	float d = 0;
	BFCG_CKN(bfcg_kmers_destroy(u), hipMalloc(&tab, bytes));
	u->table = tab; u->owns_table = 1;
	BFCG_CKN(bfcg_kmers_destroy(u), hipEventRecord(c->e0, c->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipMemsetAsync(tab, 0, bytes, c->st));
	hipLaunchKernelGGL(k_clip_fill, dim3(clip_grid(n_pairs)), dim3(BT), 0, c->st, (const ulonglong2 *)c->table, n_pairs, c->cshift, min_cnt, ut_buf<uint32_t>(c, B_MARK), tab, u->cshift,
	                   ut_buf<unsigned long long>(c, B_CTR));
	BFCG_CKN(bfcg_kmers_destroy(u), hipEventRecord(c->e1, c->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipGetLastError());
	BFCG_CKN(bfcg_kmers_destroy(u), hipMemcpyAsync(ctr, c->d_ut[B_CTR], CC_N * 8, hipMemcpyDeviceToHost, c->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipStreamSynchronize(c->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipEventElapsedTime(&d, c->e0, c->e1));
	*ms += d;
	if (ctr[CC_FULL] != 0 || ctr[CC_MADE] != keys) {
		bfcg::fail("%s: %llu slots found their region full or their key there already, %llu keys made of %llu: the table changed under the call", who, ctr[CC_FULL], ctr[CC_MADE],
		           (unsigned long long)keys);
		bfcg_kmers_destroy(u);
		return NULL;
	}
	u->n_keys = keys; u->has_keys = 1;
	return u;
}

// ---- the host twins' side: no GPU ------------------------------------------------------------------------------------------------------------
struct HostSlots { // bfc_ch_export_sorted of a table
	std::vector<uint32_t> sizes; std::vector<uint64_t> slots;
	explicit HostSlots(const bfc_ch_t *ch) : sizes(1ULL << bfc_ch_get_lpre(ch)), slots(bfc_ch_export_sorted(ch, NULL, NULL) + 1) { bfc_ch_export_sorted(ch, sizes.data(), slots.data()); }
};

Planes node_of(int k, uint64_t a, uint64_t b) // a node's smaller strand
{
	uint64_t ra, rb;
	rc_planes(k, a, b, ra, rb);
	return text_less(ra, rb, a, b) ? Planes{ ra, rb } : Planes{ a, b };
}

typedef std::unordered_set<Planes, PlanesHash> NodeSet;

// the table of ch's survivors -- count >= min_cnt, not in kill -- at the union's cshift rule; *keys = its keys.  NULL with the message set
bfc_ch_t *clip_keep_host(const bfc_ch_t *ch, int min_cnt, const NodeSet &kill, uint64_t *keys)
{
	const int k = bfc_ch_get_k(ch), l_pre = bfc_ch_get_lpre(ch);
	const HostSlots S(ch);
	std::vector<uint8_t> keep(S.slots.size(), 0);
	uint64_t most = 0, i = 0;
	*keys = 0;
	for (uint64_t s = 0; s < S.sizes.size(); ++s) {
		uint64_t n = 0;
		for (uint32_t j = 0; j < S.sizes[s]; ++j, ++i) {
			uint64_t a, b;
			if ((int)(S.slots[i] & 0xff) < min_cnt) continue;
			kdec::decode(k, l_pre, (uint32_t)s, S.slots[i], a, b);
			if (kill.empty() || !kill.count(node_of(k, a, b))) { keep[i] = 1; ++n; }
		}
		*keys += n;
		if (n > most) most = n;
	}
	const int cshift = clip_cshift(l_pre, *keys, most);
	bfc_ch_t *out = bfc_ch_alloc_raw(k, l_pre, cshift);
	if (!out) { bfcg::fail("out of host memory for a table of 2^%d slots", l_pre + cshift); return NULL; }
	uint64_t *slots = bfc_ch_raw_slots(out);
	const uint64_t cmask = (1ULL << cshift) - 1;
	i = 0;
	for (uint64_t s = 0; s < S.sizes.size(); ++s)
		for (uint32_t j = 0; j < S.sizes[s]; ++j, ++i) {
			if (!keep[i]) continue;
			uint64_t *reg = slots + (s << cshift), pos = (S.slots[i] >> 14) & cmask;
			while (reg[pos]) pos = (pos + 1) & cmask; // (a region is at most full: 2^cshift >= most)
			reg[pos] = S.slots[i];
		}
	bfc_ch_raw_set_count(out, *keys);
	return out;
}

} // namespace
