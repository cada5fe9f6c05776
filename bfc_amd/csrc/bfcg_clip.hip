// bfcg_clip.hip -- the count table's de Bruijn graph cleaned where it lies in HBM: the short, thinly covered dead ends (tips) and, on
// request, the short components that touch nothing (islands) are removed, round by round, into a new table that owns its slots.
// include/bfc_gpu.h defines which unitigs are clippable and what a round is; DESIGN.md section 6e.  The link rule, the listing's predicate
// and the marks are bfcg_glink.h's, the probes bfcg_gprobe.h's, the insert into the new table bfcg_upsert.h's.  A round on a table:
//   k_tab_list    bfcg_klist.h with EndPred: the nodes with an open side and their two stop codes, left on the device
//   k_clip_walk   one lane per (listed node, side) whose code is DEAD (1 or 6).  clip_rule walks away from the dead end for at most max_tip
//                 k-mers and sums the counts; a lane that has not met an open side by then stops -- the unitig is too long --, so no lane
//                 walks more than max_tip steps, however long the graph's unitigs are.  At the far end it knows tip, island or neither;
//                 of an island's two lanes the one text_less picks (the unitigs' rule of which end emits) goes on.  A lane that removes
//                 walks the same steps again and sets one KILL bit per slot (set_mark: a plain vector atomicOr that returns nothing, so
//                 the lane does not wait for it).  Removed unitigs and k-mers are summed over the wave before one atomic each
//   clip_keep     bfcg_gkeep.h, shared with bfcg_pop.hip: two streaming passes (k_clip_sizes, k_clip_fill) put the survivors -- count >=
//                 min_cnt, no KILL bit -- into a new table sized by the union's rule
// The walk kernel runs workgroups of one wave and takes at most `ut_cap` starts a launch (BFCG_UNITIG_CAP), as the unitigs' walks do.
// The host twin at the end of the file applies clip_rule through HostGraph over bfc_ch_export_sorted's slots.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "kmer_dev.h"
#include "bfcg_klist.h"
#include "bfcg_gprobe.h"
#include "bfcg_glink.h"
#include "bfcg_upsert.h"
#include "bfcg_gkeep.h"

namespace {

enum { CLIP_MAX_TIP = 65535 };

struct ClipArgs { int min_cnt, max_tip, max_mean, flags, max_rounds; };

__host__ __device__ __forceinline__ bool is_dead(int code) { return code == 1 || code == 6; }

// The unitig that starts at the oriented k-mer s = (sa, sb), whose left side is open with a DEAD code: its k-mers if this start removes
// it, 0 if not, -1 if a k-mer of the walk is not in the table (it changed under the call).  `tab` answers present4 as for link_rule and
// value_at(a, b, slot)
template <class T>
__host__ __device__ __forceinline__ int clip_rule(const T &tab, int k, uint64_t sa, uint64_t sb, const ClipArgs &A)
{
	uint64_t a = sa, b = sb, ya, yb, slot = 0;
	int v = tab.value_at(a, b, slot), right, n = 1;
	if (v < 0) return -1;
	uint64_t sum = (uint64_t)(v & 0xff);
	while ((right = link_rule(tab, k, a, b, A.min_cnt, ya, yb)) == 0) {
		if (n >= A.max_tip) return 0; // too long
		if ((v = tab.value_at(ya, yb, slot)) < 0) return -1;
		sum += (uint64_t)(v & 0xff); ++n;
		a = ya; b = yb;
	}
	if (is_dead(right)) { // an island: both its ends start a walk
		uint64_t ra, rb;
		rc_planes(k, a, b, ra, rb);
		if (!(A.flags & BFCG_CLIP_ISLANDS) || !text_less(sa, sb, ra, rb)) return 0;
	}
	return sum <= (uint64_t)A.max_mean * (uint64_t)n ? n : 0;
}

// ---- k_clip_walk -------------------------------------------------------------------------------------------------------------------------
// start i in [first, end): side i & 1 of listed node i >> 1, as for k_ut_path_count
template <typename W>
__global__ __launch_bounds__(UT_BT) void k_clip_walk(TabRef T, ClipArgs A, const ulonglong2 *__restrict__ node_y, const uint8_t *__restrict__ node_code, uint64_t first, uint64_t end,
                                                     uint32_t *__restrict__ kill, unsigned long long *__restrict__ ctr)
{
	const uint64_t i = first + (uint64_t)blockIdx.x * UT_BT + threadIdx.x;
	uint32_t n_rm = 0;
	if (i < end) {
		const int side = (int)(i & 1), code = node_code[i >> 1];
		if (is_dead(side ? code >> 3 : code & 7)) {
			DevGraph<W> g; g.T = T;
			const uint64_t m = kdec::mask(T.k);
			const ulonglong2 x = node_y[i >> 1];
			uint64_t a = x.x & m, b = x.y & m, slot = 0;
			if (side) rc_planes(T.k, x.x & m, x.y & m, a, b);
			const int n = clip_rule(g, T.k, a, b, A);
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

// ---- the host's side ---------------------------------------------------------------------------------------------------------------------------
// what both entry points refuse before anything else
int clip_check(const char *who, int k, const ClipArgs &A)
{
	if (check_min_cnt(who, A.min_cnt) != 0 || check_unitig_k(who, k) != 0) return -1;
	if (A.max_tip < 1 || A.max_tip > CLIP_MAX_TIP) return bfcg::fail("%s: max_tip %d is outside [1, %d]: a lane walks a clippable unitig alone", who, A.max_tip, (int)CLIP_MAX_TIP);
	if (A.max_mean < 1 || A.max_mean > 255) return bfcg::fail("%s: max_mean %d is outside [1, 255]: a count is 8 bits (255 switches the rule off)", who, A.max_mean);
	if (A.max_rounds < 0 || A.max_rounds > CLIP_MAX_ROUNDS) return bfcg::fail("%s: max_rounds %d is outside [0, %d]", who, A.max_rounds, (int)CLIP_MAX_ROUNDS);
	if (A.flags & ~BFCG_CLIP_ISLANDS) return bfcg::fail("%s: unknown flag bits 0x%x", who, (unsigned)(A.flags & ~BFCG_CLIP_ISLANDS));
	return 0;
}

// The KILL bits and the counters of table c zeroed; with `walk`, the listing of c's open ends and the walks from the dead ones.  ctr = the
// counters afterwards, *ms += the kernels' time; the stream is idle
template <typename W>
int clip_mark(bfcg_kmers_t *c, const ClipArgs &A, bool walk, unsigned long long ctr[CC_N], float *ms)
{
	const TabRef T = tab_ref(c);
	const uint64_t n_slots = 1ULL << (c->l_pre + c->cshift), mark_bytes = (n_slots + 31) / 32 * 4;
	uint64_t n_ends = 0;
	if (walk) {
		EndPred<W> P; P.T = T; P.min_cnt = A.min_cnt;
		if (list_dev(c, "bfcg_kmers_clip", P, A.min_cnt, -64, 0, 1u << c->l_pre, true, ~0ULL, &n_ends) != 0) return -1;
		*ms += c->last_ms;
	}
	if (ut_grow(c, B_MARK, mark_bytes, "the marks of the clipped k-mers") != 0 || ut_grow(c, B_CTR, CC_N * 8, "the counters of a clipping round") != 0) return -1;
	BFCG_CK(hipEventRecord(c->e0, c->st));
	BFCG_CK(hipMemsetAsync(c->d_ut[B_MARK], 0, mark_bytes, c->st));
	BFCG_CK(hipMemsetAsync(c->d_ut[B_CTR], 0, CC_N * 8, c->st));
	const uint64_t n_starts = 2 * n_ends;
	for (uint64_t first = 0; first < n_starts; first += c->ut_cap) {
		const uint64_t end = n_starts - first < c->ut_cap ? n_starts : first + c->ut_cap;
		hipLaunchKernelGGL((k_clip_walk<W>), dim3((unsigned)((end - first + UT_BT - 1) / UT_BT)), dim3(UT_BT), 0, c->st, T, A, (const ulonglong2 *)c->d_y, (const uint8_t *)c->d_oth,
		                   first, end, ut_buf<uint32_t>(c, B_MARK), ut_buf<unsigned long long>(c, B_CTR));
	}
	BFCG_CK(hipEventRecord(c->e1, c->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(ctr, c->d_ut[B_CTR], CC_N * 8, hipMemcpyDeviceToHost, c->st));
	if (ut_lap(c, ms) != 0) return -1;
	if (ctr[CC_ERR]) return bfcg::fail("bfcg_kmers_clip: a walk left the graph it started in: the table changed under the call");
	return 0;
}


template <typename W>
bfcg_kmers_t *clip_run(bfcg_kmers_t *t, const ClipArgs &A, uint64_t *stats, int *n_rounds)
{
	bfcg_kmers_t *cur = t; // the input, or the table of the last round that removed something: owned here
	unsigned long long ctr[CC_N];
	uint64_t st[3 * CLIP_MAX_ROUNDS];
	float ms = 0;
	int rounds = 0;
	bool marked = false; // clip_mark has run on cur: its KILL bits and counters are in place
	while (rounds < A.max_rounds) {
		if (clip_mark<W>(cur, A, true, ctr, &ms) != 0) goto failed;
		marked = true;
		if (ctr[CC_KMERS] == 0) break;
		bfcg_kmers_t *next = clip_keep(cur, "bfcg_kmers_clip", A.min_cnt, &ms);
		if (!next) goto failed;
		if (cur != t) bfcg_kmers_destroy(cur); // an intermediate table goes as soon as the next one stands
		cur = next; marked = false;
		st[3 * rounds] = ctr[CC_UNITIGS]; st[3 * rounds + 1] = ctr[CC_KMERS]; st[3 * rounds + 2] = cur->n_keys;
		++rounds;
	}
	if (cur == t) { // no round removed anything: the nodes at min_cnt
		if (!marked && clip_mark<W>(t, A, false, ctr, &ms) != 0) return NULL;
		if (!(cur = clip_keep(t, "bfcg_kmers_clip", A.min_cnt, &ms))) return NULL;
	}
	cur->last_ms = ms;
	if (stats) memcpy(stats, st, (size_t)rounds * 3 * 8);
	if (n_rounds) *n_rounds = rounds;
	return cur;
failed:
	if (cur != t) bfcg_kmers_destroy(cur);
	return NULL;
}

} // namespace

extern "C" bfcg_kmers_t *bfcg_kmers_clip(bfcg_kmers_t *t, int min_cnt, int max_tip, int max_mean, int flags, int max_rounds, uint64_t *stats, int *n_rounds)
{
	if (!t || !n_rounds) { bfcg::fail("bad arguments to bfcg_kmers_clip"); return NULL; }
	const ClipArgs A = { min_cnt, max_tip, max_mean, flags, max_rounds };
	if (clip_check("bfcg_kmers_clip", t->k, A) != 0) return NULL;
	t->last_ms = 0;
	BFCG_CKN((void)0, hipSetDevice(t->device));
	return t->k <= 32 ? clip_run<uint32_t>(t, A, stats, n_rounds) : clip_run<uint64_t>(t, A, stats, n_rounds);
}

// ---- the host twin: no GPU -----------------------------------------------------------------------------------------------------------------
// The same rounds on a host table, in the same two steps: clip_mark_host evaluates the two link rules of every node of
// bfc_ch_export_sorted's slots, lets clip_rule walk from each DEAD side and puts the removed nodes into a hash set of their smaller strands;
// clip_keep_host inserts the survivors into a table allocated at the same cshift rule.

namespace {

// the walks of one round on ch: kill = the nodes they remove, rm[0], rm[1] = the unitigs and k-mers removed.  0, or -1 with the message set
int clip_mark_host(const bfc_ch_t *ch, const ClipArgs &A, NodeSet &kill, uint64_t rm[2])
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
				if (!is_dead(link_rule(g, k, x[side ^ 1][0], x[side ^ 1][1], A.min_cnt, ya, yb))) continue;
				uint64_t a = x[side][0], b = x[side][1];
				const int n = clip_rule(g, k, a, b, A);
				if (n < 0) return bfcg::fail("bfcg_clip_host: a walk left the graph it started in");
				for (int st = 0; st < n; ++st) { // the same steps again
					if (st) succ_planes(k, a, b, only_succ(g, a, b, A.min_cnt), a, b);
					kill.insert(node_of(k, a, b));
				}
				rm[0] += n != 0; rm[1] += (uint64_t)n;
			}
		}
	if (rm[1] != kill.size()) return bfcg::fail("bfcg_clip_host: %llu k-mers removed, %llu nodes marked: two walks removed the same node", (unsigned long long)rm[1], (unsigned long long)kill.size());
	return 0;
}


} // namespace

extern "C" bfc_ch_t *bfcg_clip_host(const bfc_ch_t *ch, int min_cnt, int max_tip, int max_mean, int flags, int max_rounds, uint64_t *stats, int *n_rounds)
{
	if (!ch || !n_rounds) { bfcg::fail("bad arguments to bfcg_clip_host"); return NULL; }
	const ClipArgs A = { min_cnt, max_tip, max_mean, flags, max_rounds };
	if (clip_check("bfcg_clip_host", bfc_ch_get_k(ch), A) != 0) return NULL;
	const bfc_ch_t *cur = ch; // the input, or the table of the last round that removed something: owned here
	uint64_t st[3 * CLIP_MAX_ROUNDS], rm[2], keys = 0;
	NodeSet kill;
	int rounds = 0;
	while (rounds < A.max_rounds) {
		bfc_ch_t *next = NULL;
		if (clip_mark_host(cur, A, kill, rm) != 0 || (!kill.empty() && !(next = clip_keep_host(cur, A.min_cnt, kill, &keys)))) {
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
