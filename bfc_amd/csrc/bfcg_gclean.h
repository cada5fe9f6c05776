// bfcg_gclean.h -- a graph-cleaning round, written once for the files that remove nodes of the count table's de Bruijn graph into a new
// table: bfcg_clip.hip (tips and islands) and bfcg_pop.hip (simple bubbles).  Each of them supplies a RULE and its entry points; the rounds,
// their kernels and the host twin's rounds are here.  A rule is a plain struct that the walk kernel takes by value:
//   min_cnt, max_rounds and the rule's own limits
//   starts(code)           whether a listed node's side with this stop code starts a walk
//   decide(tab, k, a, b)   the unitig that starts at the oriented k-mer (a, b): its k-mers if this start removes it, 0 if not, -1 if a
//                          k-mer of the walk is not in the table.  One __host__ __device__ template over DevGraph and HostGraph
//                          (bfcg_gprobe.h), so the kernel and the host twin apply the same text
//   who_dev, who_host, what_marks, what_ctr   the entry points' names and the two buffers' descriptions, for messages
// A round on a table:
//   k_tab_list    bfcg_klist.h with EndPred: the nodes with an open side and their two stop codes, left on the device
//   k_clean_walk  one lane per (listed node, side) that the rule starts.  A lane whose decide() removes walks the same steps again and sets
//                 one KILL bit per slot (set_mark, bfcg_glink.h: a plain vector atomicOr that returns nothing, so the lane does not wait
//                 for it) in d_ut[B_MARK].  Removed unitigs and k-mers are summed over the wave before one atomic each into d_ut[B_CTR].
//                 Workgroups of one wave, at most `ut_cap` starts a launch (BFCG_UNITIG_CAP), as the unitigs' walks
//   k_clip_sizes  a streaming pass over the slot pairs: the survivors (count >= min_cnt, no KILL bit) per sub-table, by wave ballots;
//                 they fix the new table's geometry by the union's rule, so a region cannot overflow
//   k_clip_fill   a streaming pass that upserts every survivor into the zeroed new table; the made and full counters are checked as the
//                 union's are
// clean_mark is the first two steps, clip_keep the last two around the new object, clean_run the rounds of a call.  For the host twins
// HostSlots (bfc_ch_export_sorted of a table), NodeSet (the removed nodes as their smaller strands), clean_mark_host (decide() from every
// side that starts, through HostGraph), clip_keep_host (the survivors into a table allocated at the same cshift rule) and clean_run_host.
#pragma once
#include <string.h>
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

// ---- k_clean_walk ------------------------------------------------------------------------------------------------------------------------
// start i in [first, end): walk_start's (bfcg_glink.h), as for k_ut_path_count
template <typename W, class Rule>
__global__ __launch_bounds__(UT_BT) void k_clean_walk(TabRef T, Rule A, const ulonglong2 *__restrict__ node_y, const uint8_t *__restrict__ node_code, uint64_t first, uint64_t end,
                                                      uint32_t *__restrict__ kill, unsigned long long *__restrict__ ctr)
{
	const uint64_t i = first + (uint64_t)blockIdx.x * UT_BT + threadIdx.x;
	uint32_t n_rm = 0;
	if (i < end) {
		int code;
		uint64_t a, b, slot = 0;
		if (walk_start(T.k, node_y, node_code, i, A, code, a, b)) {
			DevGraph<W> g; g.T = T;
			const int n = A.decide(g, T.k, a, b);
			bool lost = n < 0;
			for (int j = 0; j < n && !lost; ++j) { // the same steps again
				if (j) succ_planes(T.k, a, b, only_succ(g, a, b, A.min_cnt), a, b);
				if (g.value_at(a, b, slot) < 0) lost = true;
				else set_mark(kill, slot);
			}
			if (lost) atomicOr(&ctr[CC_ERR], 1ULL); // (a listed node is in the table unless the table changed)
			else n_rm = (uint32_t)n;
		}
	}
	uint32_t n_ut = n_rm != 0;
#pragma unroll
	for (int d = 32; d; d >>= 1) { n_ut += __shfl_down(n_ut, d, 64); n_rm += __shfl_down(n_rm, d, 64); }
	if (lane_id() == 0 && n_ut) {
		atomicAdd(&ctr[CC_UNITIGS], (unsigned long long)n_ut);
		atomicAdd(&ctr[CC_KMERS], (unsigned long long)n_rm);
	}
}

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

// The KILL bits and the counters of table c zeroed; with `walk`, the listing of c's open ends and the walks from the sides that the rule
// starts.  ctr = the counters afterwards, *ms += the kernels' time; the stream is idle
template <typename W, class Rule>
int clean_mark(bfcg_kmers_t *c, const Rule &A, bool walk, unsigned long long ctr[CC_N], float *ms)
{
	const TabRef T = tab_ref(c);
	const uint64_t n_slots = 1ULL << (c->l_pre + c->cshift), mark_bytes = (n_slots + 31) / 32 * 4;
	uint64_t n_ends = 0;
	if (walk) {
		EndPred<W> P; P.T = T; P.min_cnt = A.min_cnt;
		if (list_dev(c, Rule::who_dev, P, A.min_cnt, -64, 0, 1u << c->l_pre, true, ~0ULL, &n_ends) != 0) return -1;
		*ms += c->last_ms;
	}
	if (ut_grow(c, B_MARK, mark_bytes, Rule::what_marks) != 0 || ut_grow(c, B_CTR, CC_N * 8, Rule::what_ctr) != 0) return -1;
	BFCG_CK(hipEventRecord(c->e0, c->st));
	BFCG_CK(hipMemsetAsync(c->d_ut[B_MARK], 0, mark_bytes, c->st));
	BFCG_CK(hipMemsetAsync(c->d_ut[B_CTR], 0, CC_N * 8, c->st));
	const uint64_t n_starts = 2 * n_ends;
	for (uint64_t first = 0; first < n_starts; first += c->ut_cap) {
		const uint64_t end = n_starts - first < c->ut_cap ? n_starts : first + c->ut_cap;
		hipLaunchKernelGGL((k_clean_walk<W, Rule>), dim3((unsigned)((end - first + UT_BT - 1) / UT_BT)), dim3(UT_BT), 0, c->st, T, A, (const ulonglong2 *)c->d_y, (const uint8_t *)c->d_oth,
		                   first, end, ut_buf<uint32_t>(c, B_MARK), ut_buf<unsigned long long>(c, B_CTR));
	}
	BFCG_CK(hipEventRecord(c->e1, c->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(ctr, c->d_ut[B_CTR], CC_N * 8, hipMemcpyDeviceToHost, c->st));
	if (ut_lap(c, ms) != 0) return -1;
	if (ctr[CC_ERR]) return bfcg::fail("%s: a walk left the graph it started in: the table changed under the call", Rule::who_dev);
	return 0;
}

// The rounds of a call on t, whose arguments the caller has checked: the table of the last round, a new object; stats and *n_rounds as
// include/bfc_gpu.h says.  NULL with the message set
template <typename W, class Rule>
bfcg_kmers_t *clean_run(bfcg_kmers_t *t, const Rule &A, uint64_t *stats, int *n_rounds)
{
	bfcg_kmers_t *cur = t; // the input, or the table of the last round that removed something: owned here
	unsigned long long ctr[CC_N];
	uint64_t st[3 * CLIP_MAX_ROUNDS];
	float ms = 0;
	int rounds = 0;
	bool marked = false; // clean_mark has run on cur: its KILL bits and counters are in place
	t->last_ms = 0;
	BFCG_CKN((void)0, hipSetDevice(t->device));
	while (rounds < A.max_rounds) {
		if (clean_mark<W>(cur, A, true, ctr, &ms) != 0) goto failed;
		marked = true;
		if (ctr[CC_KMERS] == 0) break;
		bfcg_kmers_t *next = clip_keep(cur, Rule::who_dev, A.min_cnt, &ms);
		if (!next) goto failed;
		if (cur != t) bfcg_kmers_destroy(cur); // an intermediate table goes as soon as the next one stands
		cur = next; marked = false;
		st[3 * rounds] = ctr[CC_UNITIGS]; st[3 * rounds + 1] = ctr[CC_KMERS]; st[3 * rounds + 2] = cur->n_keys;
		++rounds;
	}
	if (cur == t) { // no round removed anything: the nodes at min_cnt
		if (!marked && clean_mark<W>(t, A, false, ctr, &ms) != 0) return NULL;
		if (!(cur = clip_keep(t, Rule::who_dev, A.min_cnt, &ms))) return NULL;
	}
	cur->last_ms = ms;
	if (stats) memcpy(stats, st, (size_t)rounds * 3 * 8);
	if (n_rounds) *n_rounds = rounds;
	return cur;
failed:
	if (cur != t) bfcg_kmers_destroy(cur);
	return NULL;
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

// The walks of one round on ch: the two link rules of every node of bfc_ch_export_sorted's slots, decide() from each side that the rule
// starts.  kill = the nodes they remove, rm[0], rm[1] = the unitigs and k-mers removed.  0, or -1 with the message set
template <class Rule>
int clean_mark_host(const bfc_ch_t *ch, const Rule &A, NodeSet &kill, uint64_t rm[2])
{
	HostGraph g;
	g.ch = ch; g.k = bfc_ch_get_k(ch);
	const int k = g.k, l_pre = bfc_ch_get_lpre(ch);
	const HostSlots S(ch);
	kill.clear();
	rm[0] = rm[1] = 0;
	uint64_t i = 0;
	for (uint64_t s = 0; s < S.sizes.size(); ++s)
		for (uint32_t j = 0; j < S.sizes[s]; ++j, ++i) {
			if ((int)(S.slots[i] & 0xff) < A.min_cnt) continue;
			uint64_t x[2][2], ya, yb;
			kdec::decode(k, l_pre, (uint32_t)s, S.slots[i], x[0][0], x[0][1]);
			rc_planes(k, x[0][0], x[0][1], x[1][0], x[1][1]);
			for (int side = 0; side < 2; ++side) { // the left side of x[side] is the right side of the other strand
				if (!A.starts(link_rule(g, k, x[side ^ 1][0], x[side ^ 1][1], A.min_cnt, ya, yb))) continue;
				uint64_t a = x[side][0], b = x[side][1];
				const int n = A.decide(g, k, a, b);
				if (n < 0) return bfcg::fail("%s: a walk left the graph it started in", Rule::who_host);
				for (int st = 0; st < n; ++st) { // the same steps again
					if (st) succ_planes(k, a, b, only_succ(g, a, b, A.min_cnt), a, b);
					kill.insert(node_of(k, a, b));
				}
				rm[0] += n != 0; rm[1] += (uint64_t)n;
			}
		}
	if (rm[1] != kill.size()) return bfcg::fail("%s: %llu k-mers removed, %llu nodes marked: two walks removed the same node", Rule::who_host, (unsigned long long)rm[1], (unsigned long long)kill.size());
	return 0;
}

// clean_run's rounds on a host table, in the same two steps
template <class Rule>
bfc_ch_t *clean_run_host(const bfc_ch_t *ch, const Rule &A, uint64_t *stats, int *n_rounds)
{
	const bfc_ch_t *cur = ch; // the input, or the table of the last round that removed something: owned here
	uint64_t st[3 * CLIP_MAX_ROUNDS], rm[2], keys = 0;
	NodeSet kill;
	int rounds = 0;
	while (rounds < A.max_rounds) {
		bfc_ch_t *next = NULL;
		if (clean_mark_host(cur, A, kill, rm) != 0 || (!kill.empty() && !(next = clip_keep_host(cur, A.min_cnt, kill, &keys)))) {
			if (cur != ch) bfc_ch_destroy((bfc_ch_t *)cur);
			return NULL;
		}
		if (!next) break;
		if (cur != ch) bfc_ch_destroy((bfc_ch_t *)cur);
		cur = next;
		st[3 * rounds] = rm[0]; st[3 * rounds + 1] = rm[1]; st[3 * rounds + 2] = keys;
		++rounds;
	}
	kill.clear();
	if (cur == ch && !(cur = clip_keep_host(ch, A.min_cnt, kill, &keys))) return NULL; // no round removed anything: the nodes at min_cnt
	if (stats) memcpy(stats, st, (size_t)rounds * 3 * 8);
	*n_rounds = rounds;
	return (bfc_ch_t *)cur;
}

} // namespace
