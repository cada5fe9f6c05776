// bfcg_pop.hip -- the simple bubbles of the count table's de Bruijn graph popped where it lies in HBM: of two parallel unitigs that leave
// one k-mer and meet again in one k-mer (a substitution error seen twice, a heterozygous SNP, a short indel) the one with the lower mean
// count is removed, round by round, into a new table that owns its slots.  include/bfc_gpu.h defines arm, simple bubble, loser and round;
// DESIGN.md section 6f.  The link rule, the listing's predicate and the marks are bfcg_glink.h's, the probes bfcg_gprobe.h's, the
// marks-to-table half of a round bfcg_gkeep.h's, shared with bfcg_clip.hip.  A round on a table:
//   k_tab_list    bfcg_klist.h with EndPred: the nodes with an open side and their two stop codes, left on the device
//   k_pop_walk    one lane per (listed node, side) whose code is 3.  pop_rule walks the arm U from there for at most max_arm k-mers and
//                 sums the counts; it goes on only if the far side's code is 3 too and this end is the one that emits (text_less, the
//                 unitigs' rule), so one lane per arm continues.  It finds the entry p and the exit q, checks that p has two successors
//                 and q two predecessors, takes the sibling s' under p, walks the second arm V from it for at most max_arm k-mers and
//                 checks that V ends at q.  Then the length rule, the loser rule and the mean rule.  A lane decides its own arm only: if
//                 U is to go, it walks U again and sets one KILL bit per slot (set_mark).  No lane takes more than 3 * max_arm steps,
//                 whatever the graph holds.  Removed arms and k-mers are summed over the wave before one atomic each
//   clip_keep     the survivors (count >= min_cnt, no KILL bit) into a new table sized by the union's rule
// The walk kernel runs workgroups of one wave and takes at most `ut_cap` starts a launch (BFCG_UNITIG_CAP), as the unitigs' walks do.
// The host twin at the end of the file applies pop_rule through HostGraph over bfc_ch_export_sorted's slots.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "kmer_dev.h"
#include "bfcg_klist.h"
#include "bfcg_gprobe.h"
#include "bfcg_glink.h"
#include "bfcg_gkeep.h"

namespace {

enum { POP_MAX_ARM = 65535 };

struct PopArgs { int min_cnt, max_arm, max_diff, max_mean, max_rounds; };

// The unitig from the oriented k-mer (a, b), whose left side is open, for at most max_arm k-mers: the stop code of its right end, which
// (a, b) then is, n its k-mers, sum their counts and (ya, yb) the single successor under codes 3 and 6; 0 if it is longer than max_arm;
// -1 if a k-mer of the walk is not in the table
template <class T>
__host__ __device__ __forceinline__ int arm_walk(const T &tab, int k, const PopArgs &A, uint64_t &a, uint64_t &b, uint64_t &ya, uint64_t &yb, int &n, uint64_t &sum)
{
	uint64_t slot = 0;
	int v = tab.value_at(a, b, slot), right;
	if (v < 0) return -1;
	n = 1; sum = (uint64_t)(v & 0xff);
	while ((right = link_rule(tab, k, a, b, A.min_cnt, ya, yb)) == 0) {
		if (n >= A.max_arm) return 0; // too long
		if ((v = tab.value_at(ya, yb, slot)) < 0) return -1;
		sum += (uint64_t)(v & 0xff); ++n;
		a = ya; b = yb;
	}
	return right;
}

// The unitig U that starts at the oriented k-mer s = (sa, sb), whose left side is open with code 3: its k-mers if it is the LOSER of a
// simple bubble and this start is the one that removes it, 0 if not, -1 if the walk met a k-mer that is not in the table or an entry
// that code 3 rules out (the table changed under the call).  `tab` answers present4 as for link_rule and value_at(a, b, slot)
template <class T>
__host__ __device__ __forceinline__ int pop_rule(const T &tab, int k, uint64_t sa, uint64_t sb, const PopArgs &A)
{
	uint64_t ea = sa, eb = sb, qa, qb, ra, rb, sum_u, sum_v;
	int n_u, n_v, code;
	if ((code = arm_walk(tab, k, A, ea, eb, qa, qb, n_u, sum_u)) != 3) return code < 0 ? -1 : 0; // e and the exit q
	rc_planes(k, ea, eb, ra, rb);
	if (!text_less(sa, sb, ra, rb)) return 0;                     // the lane at rc(e) emits U and decides
	const int ip = tab.present4(sa, sb, 1, A.min_cnt);
	if (ip == 0 || (ip & (ip - 1))) return -1;                    // (code 3 on the left: exactly one predecessor)
	uint64_t pa, pb, va, vb, fa, fb, xa, xb;
	pred_planes(k, sa, sb, __builtin_ctz(ip), pa, pb);            // the entry p
	const int mine = (int)(sa & 1) | (int)(sb & 1) << 1, op = tab.present4(pa, pb, 0, A.min_cnt), iq = tab.present4(qa, qb, 1, A.min_cnt);
	if (!(op >> mine & 1)) return -1;
	const int sib = op & ~(1 << mine);
	if (sib == 0 || (sib & (sib - 1)) || __builtin_popcount(iq) != 2) return 0; // three ways or more at either end
	succ_planes(k, pa, pb, __builtin_ctz(sib), va, vb);           // the sibling s'
	if (va == ra && vb == rb) return 0;                           // U read backwards: the inverted case
	rc_planes(k, va, vb, xa, xb);
	if (link_rule(tab, k, xa, xb, A.min_cnt, fa, fb) != 3) return 0; // s' has another way in, or leads back into itself
	const uint64_t first_a = va, first_b = vb;
	if ((code = arm_walk(tab, k, A, va, vb, fa, fb, n_v, sum_v)) != 3) return code < 0 ? -1 : 0; // e' and V's exit
	if (fa != qa || fb != qb) return 0;
	if ((n_u > n_v ? n_u - n_v : n_v - n_u) > A.max_diff) return 0;
	const uint64_t lhs = sum_u * (uint64_t)n_v, rhs = sum_v * (uint64_t)n_u;
	if (lhs > rhs) return 0;
	if (lhs == rhs) { // a tie: the arm whose emitted spelling starts with the larger k-mer goes
		rc_planes(k, va, vb, xa, xb);
		const bool fwd = text_less(first_a, first_b, xa, xb);    // V is emitted from s', not from rc(e')
		if (!text_less(fwd ? first_a : xa, fwd ? first_b : xb, sa, sb)) return 0;
	}
	return sum_u <= (uint64_t)A.max_mean * (uint64_t)n_u ? n_u : 0;
}

// ---- k_pop_walk --------------------------------------------------------------------------------------------------------------------------
// start i in [first, end): side i & 1 of listed node i >> 1, as for k_clip_walk
template <typename W>
__global__ __launch_bounds__(UT_BT) void k_pop_walk(TabRef T, PopArgs A, const ulonglong2 *__restrict__ node_y, const uint8_t *__restrict__ node_code, uint64_t first, uint64_t end,
                                                    uint32_t *__restrict__ kill, unsigned long long *__restrict__ ctr)
{
	const uint64_t i = first + (uint64_t)blockIdx.x * UT_BT + threadIdx.x;
	uint32_t n_rm = 0;
	if (i < end) {
		const int side = (int)(i & 1), code = node_code[i >> 1];
		if ((side ? code >> 3 : code & 7) == 3) {
			DevGraph<W> g; g.T = T;
			const uint64_t m = kdec::mask(T.k);
			const ulonglong2 x = node_y[i >> 1];
			uint64_t a = x.x & m, b = x.y & m, slot = 0;
			if (side) rc_planes(T.k, x.x & m, x.y & m, a, b);
			const int n = pop_rule(g, T.k, a, b, A);
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
int pop_check(const char *who, int k, const PopArgs &A)
{
	if (check_min_cnt(who, A.min_cnt) != 0 || check_unitig_k(who, k) != 0) return -1;
	if (A.max_arm < 1 || A.max_arm > POP_MAX_ARM) return bfcg::fail("%s: max_arm %d is outside [1, %d]: a lane walks both arms of a bubble alone", who, A.max_arm, (int)POP_MAX_ARM);
	if (A.max_diff < 0 || A.max_diff > POP_MAX_ARM) return bfcg::fail("%s: max_diff %d is outside [0, %d]", who, A.max_diff, (int)POP_MAX_ARM);
	if (A.max_mean < 1 || A.max_mean > 255) return bfcg::fail("%s: max_mean %d is outside [1, 255]: a count is 8 bits (255 switches the rule off)", who, A.max_mean);
	if (A.max_rounds < 0 || A.max_rounds > CLIP_MAX_ROUNDS) return bfcg::fail("%s: max_rounds %d is outside [0, %d]", who, A.max_rounds, (int)CLIP_MAX_ROUNDS);
	return 0;
}

// The KILL bits and the counters of table c zeroed; with `walk`, the listing of c's open ends and the walks from the sides with code 3.
// ctr = the counters afterwards, *ms += the kernels' time; the stream is idle
template <typename W>
int pop_mark(bfcg_kmers_t *c, const PopArgs &A, bool walk, unsigned long long ctr[CC_N], float *ms)
{
	const TabRef T = tab_ref(c);
	const uint64_t n_slots = 1ULL << (c->l_pre + c->cshift), mark_bytes = (n_slots + 31) / 32 * 4;
	uint64_t n_ends = 0;
	if (walk) {
		EndPred<W> P; P.T = T; P.min_cnt = A.min_cnt;
		if (list_dev(c, "bfcg_kmers_pop", P, A.min_cnt, -64, 0, 1u << c->l_pre, true, ~0ULL, &n_ends) != 0) return -1;
		*ms += c->last_ms;
	}
	if (ut_grow(c, B_MARK, mark_bytes, "the marks of the popped k-mers") != 0 || ut_grow(c, B_CTR, CC_N * 8, "the counters of a popping round") != 0) return -1;
	BFCG_CK(hipEventRecord(c->e0, c->st));
	BFCG_CK(hipMemsetAsync(c->d_ut[B_MARK], 0, mark_bytes, c->st));
	BFCG_CK(hipMemsetAsync(c->d_ut[B_CTR], 0, CC_N * 8, c->st));
	const uint64_t n_starts = 2 * n_ends;
	for (uint64_t first = 0; first < n_starts; first += c->ut_cap) {
		const uint64_t end = n_starts - first < c->ut_cap ? n_starts : first + c->ut_cap;
		hipLaunchKernelGGL((k_pop_walk<W>), dim3((unsigned)((end - first + UT_BT - 1) / UT_BT)), dim3(UT_BT), 0, c->st, T, A, (const ulonglong2 *)c->d_y, (const uint8_t *)c->d_oth,
		                   first, end, ut_buf<uint32_t>(c, B_MARK), ut_buf<unsigned long long>(c, B_CTR));
	}
	BFCG_CK(hipEventRecord(c->e1, c->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(ctr, c->d_ut[B_CTR], CC_N * 8, hipMemcpyDeviceToHost, c->st));
	if (ut_lap(c, ms) != 0) return -1;
	if (ctr[CC_ERR]) return bfcg::fail("bfcg_kmers_pop: a walk left the graph it started in: the table changed under the call");
	return 0;
}

template <typename W>
bfcg_kmers_t *pop_run(bfcg_kmers_t *t, const PopArgs &A, uint64_t *stats, int *n_rounds)
{
	bfcg_kmers_t *cur = t; // the input, or the table of the last round that removed something: owned here
	unsigned long long ctr[CC_N];
	uint64_t st[3 * CLIP_MAX_ROUNDS];
	float ms = 0;
	int rounds = 0;
	bool marked = false; // pop_mark has run on cur: its KILL bits and counters are in place
	while (rounds < A.max_rounds) {
		if (pop_mark<W>(cur, A, true, ctr, &ms) != 0) goto failed;
		marked = true;
		if (ctr[CC_KMERS] == 0) break;
		bfcg_kmers_t *next = clip_keep(cur, "bfcg_kmers_pop", A.min_cnt, &ms);
		if (!next) goto failed;
		if (cur != t) bfcg_kmers_destroy(cur); // an intermediate table goes as soon as the next one stands
		cur = next; marked = false;
		st[3 * rounds] = ctr[CC_UNITIGS]; st[3 * rounds + 1] = ctr[CC_KMERS]; st[3 * rounds + 2] = cur->n_keys;
		++rounds;
	}
	if (cur == t) { // no round removed anything: the nodes at min_cnt
		if (!marked && pop_mark<W>(t, A, false, ctr, &ms) != 0) return NULL;
		if (!(cur = clip_keep(t, "bfcg_kmers_pop", A.min_cnt, &ms))) return NULL;
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

extern "C" bfcg_kmers_t *bfcg_kmers_pop(bfcg_kmers_t *t, int min_cnt, int max_arm, int max_diff, int max_mean, int max_rounds, uint64_t *stats, int *n_rounds)
{
	if (!t || !n_rounds) { bfcg::fail("bad arguments to bfcg_kmers_pop"); return NULL; }
	const PopArgs A = { min_cnt, max_arm, max_diff, max_mean, max_rounds };
	if (pop_check("bfcg_kmers_pop", t->k, A) != 0) return NULL;
	t->last_ms = 0;
	BFCG_CKN((void)0, hipSetDevice(t->device));
	return t->k <= 32 ? pop_run<uint32_t>(t, A, stats, n_rounds) : pop_run<uint64_t>(t, A, stats, n_rounds);
}

// ---- the host twin: no GPU -----------------------------------------------------------------------------------------------------------------
// The same rounds on a host table, in the same two steps: pop_mark_host evaluates the two link rules of every node of
// bfc_ch_export_sorted's slots, lets pop_rule decide from each side with code 3 and puts the removed nodes into a hash set of their
// smaller strands; clip_keep_host (bfcg_gkeep.h) inserts the survivors into a table allocated at the same cshift rule.

namespace {

// the walks of one round on ch: kill = the nodes they remove, rm[0], rm[1] = the bubbles popped and k-mers removed.  0, or -1 with the message set
int pop_mark_host(const bfc_ch_t *ch, const PopArgs &A, NodeSet &kill, uint64_t rm[2])
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
				if (link_rule(g, k, x[side ^ 1][0], x[side ^ 1][1], A.min_cnt, ya, yb) != 3) continue;
				uint64_t a = x[side][0], b = x[side][1];
				const int n = pop_rule(g, k, a, b, A);
				if (n < 0) return bfcg::fail("bfcg_pop_host: a walk left the graph it started in");
				for (int st = 0; st < n; ++st) { // the same steps again
					if (st) succ_planes(k, a, b, only_succ(g, a, b, A.min_cnt), a, b);
					kill.insert(node_of(k, a, b));
				}
				rm[0] += n != 0; rm[1] += (uint64_t)n;
			}
		}
	if (rm[1] != kill.size()) return bfcg::fail("bfcg_pop_host: %llu k-mers removed, %llu nodes marked: two walks removed the same node", (unsigned long long)rm[1], (unsigned long long)kill.size());
	return 0;
}

} // namespace

extern "C" bfc_ch_t *bfcg_pop_host(const bfc_ch_t *ch, int min_cnt, int max_arm, int max_diff, int max_mean, int max_rounds, uint64_t *stats, int *n_rounds)
{
	if (!ch || !n_rounds) { bfcg::fail("bad arguments to bfcg_pop_host"); return NULL; }
	const PopArgs A = { min_cnt, max_arm, max_diff, max_mean, max_rounds };
	if (pop_check("bfcg_pop_host", bfc_ch_get_k(ch), A) != 0) return NULL;
	const bfc_ch_t *cur = ch; // the input, or the table of the last round that removed something: owned here
	uint64_t st[3 * CLIP_MAX_ROUNDS], rm[2], keys = 0;
	NodeSet kill;
	int rounds = 0;
	while (rounds < A.max_rounds) {
		bfc_ch_t *next = NULL;
		if (pop_mark_host(cur, A, kill, rm) != 0 || (!kill.empty() && !(next = clip_keep_host(cur, A.min_cnt, kill, &keys)))) {
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
