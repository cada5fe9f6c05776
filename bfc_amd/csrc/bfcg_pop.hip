// bfcg_pop.hip -- the simple bubbles of the count table's de Bruijn graph popped where it lies in HBM: of two parallel unitigs that leave
// one k-mer and meet again in one k-mer (a substitution error seen twice, a heterozygous SNP, a short indel) the one with the lower mean
// count is removed, round by round, into a new table that owns its slots.  include/bfc_gpu.h defines arm, simple bubble, loser and round;
// DESIGN.md section 6f.  The round -- the listing of the open ends, k_clean_walk, the survivors into a new table, the rounds of a call and
// the host twin's -- is bfcg_gclean.h's, shared with bfcg_clip.hip; this file holds the rule it applies and the two entry points.
//   PopRule    a side starts a walk if its stop code is 3.  decide() walks the arm U from there for at most max_arm k-mers (arm_walk,
//              bfcg_glink.h) and sums the counts; it goes on only if the far side's code is 3 too and this end is the one that emits
//              (text_less, the unitigs' rule), so one lane per arm continues.  It finds the entry p and the exit q, checks that p has two
//              successors and q two predecessors, takes the sibling s' under p, walks the second arm V from it for at most max_arm k-mers
//              and checks that V ends at q.  Then the length rule, the loser rule and the mean rule.  A lane decides its own arm only,
//              and with the round's second walk of U it takes no more than 3 * max_arm steps, whatever the graph holds
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "bfcg_gprobe.h"
#include "bfcg_glink.h"
#include "bfcg_gclean.h"

namespace {

enum { POP_MAX_ARM = 65535 };

struct PopRule {
	int min_cnt, max_arm, max_diff, max_mean, max_rounds;
	static constexpr const char *who_dev = "bfcg_kmers_pop", *who_host = "bfcg_pop_host";
	static constexpr const char *what_marks = "the marks of the popped k-mers", *what_ctr = "the counters of a popping round";

	__host__ __device__ __forceinline__ bool starts(int code) const { return code == 3; }

	// The unitig U that starts at the oriented k-mer s = (sa, sb), whose left side is open with code 3: its k-mers if it is the LOSER of a
	// simple bubble and this start is the one that removes it, 0 if not, -1 if the walk met a k-mer that is not in the table or an entry
	// that code 3 rules out (the table changed under the call).  `tab` answers present4 as for link_rule and value_at(a, b, slot)
	template <class T>
	__host__ __device__ __forceinline__ int decide(const T &tab, int k, uint64_t sa, uint64_t sb) const
	{
		uint64_t ea = sa, eb = sb, qa, qb, ra, rb, sum_u, sum_v;
		int n_u, n_v, code;
		if ((code = arm_walk(tab, k, min_cnt, max_arm, ea, eb, qa, qb, n_u, sum_u)) != 3) return code < 0 ? -1 : 0; // e and the exit q
		rc_planes(k, ea, eb, ra, rb);
		if (!text_less(sa, sb, ra, rb)) return 0;                     // the lane at rc(e) emits U and decides
		const int ip = tab.present4(sa, sb, 1, min_cnt);
		if (ip == 0 || (ip & (ip - 1))) return -1;                    // (code 3 on the left: exactly one predecessor)
		uint64_t pa, pb, va, vb, fa, fb, xa, xb;
		pred_planes(k, sa, sb, __builtin_ctz(ip), pa, pb);            // the entry p
		const int mine = (int)(sa & 1) | (int)(sb & 1) << 1, op = tab.present4(pa, pb, 0, min_cnt), iq = tab.present4(qa, qb, 1, min_cnt);
		if (!(op >> mine & 1)) return -1;
		const int sib = op & ~(1 << mine);
		if (sib == 0 || (sib & (sib - 1)) || __builtin_popcount(iq) != 2) return 0; // three ways or more at either end
		succ_planes(k, pa, pb, __builtin_ctz(sib), va, vb);           // the sibling s'
		if (va == ra && vb == rb) return 0;                           // U read backwards: the inverted case
		rc_planes(k, va, vb, xa, xb);
		if (link_rule(tab, k, xa, xb, min_cnt, fa, fb) != 3) return 0; // s' has another way in, or leads back into itself
		const uint64_t first_a = va, first_b = vb;
		if ((code = arm_walk(tab, k, min_cnt, max_arm, va, vb, fa, fb, n_v, sum_v)) != 3) return code < 0 ? -1 : 0; // e' and V's exit
		if (fa != qa || fb != qb) return 0;
		if ((n_u > n_v ? n_u - n_v : n_v - n_u) > max_diff) return 0;
		const uint64_t lhs = sum_u * (uint64_t)n_v, rhs = sum_v * (uint64_t)n_u;
		if (lhs > rhs) return 0;
		if (lhs == rhs) { // a tie: the arm whose emitted spelling starts with the larger k-mer goes
			rc_planes(k, va, vb, xa, xb);
			const bool fwd = text_less(first_a, first_b, xa, xb);    // V is emitted from s', not from rc(e')
			if (!text_less(fwd ? first_a : xa, fwd ? first_b : xb, sa, sb)) return 0;
		}
		return sum_u <= (uint64_t)max_mean * (uint64_t)n_u ? n_u : 0;
	}
};

// what both entry points refuse before anything else
int pop_check(const char *who, int k, const PopRule &A)
{
	if (check_min_cnt(who, A.min_cnt) != 0 || check_unitig_k(who, k) != 0) return -1;
	if (A.max_arm < 1 || A.max_arm > POP_MAX_ARM) return bfcg::fail("%s: max_arm %d is outside [1, %d]: a lane walks both arms of a bubble alone", who, A.max_arm, (int)POP_MAX_ARM);
	if (A.max_diff < 0 || A.max_diff > POP_MAX_ARM) return bfcg::fail("%s: max_diff %d is outside [0, %d]", who, A.max_diff, (int)POP_MAX_ARM);
	if (A.max_mean < 1 || A.max_mean > 255) return bfcg::fail("%s: max_mean %d is outside [1, 255]: a count is 8 bits (255 switches the rule off)", who, A.max_mean);
	if (A.max_rounds < 0 || A.max_rounds > CLIP_MAX_ROUNDS) return bfcg::fail("%s: max_rounds %d is outside [0, %d]", who, A.max_rounds, (int)CLIP_MAX_ROUNDS);
	return 0;
}

} // namespace

extern "C" bfcg_kmers_t *bfcg_kmers_pop(bfcg_kmers_t *t, int min_cnt, int max_arm, int max_diff, int max_mean, int max_rounds, uint64_t *stats, int *n_rounds)
{
	if (!t || !n_rounds) { bfcg::fail("bad arguments to bfcg_kmers_pop"); return NULL; }
	const PopRule A = { min_cnt, max_arm, max_diff, max_mean, max_rounds };
	if (pop_check(PopRule::who_dev, t->k, A) != 0) return NULL;
	return t->k <= 32 ? clean_run<uint32_t>(t, A, stats, n_rounds) : clean_run<uint64_t>(t, A, stats, n_rounds);
}

// the host twin: no GPU
extern "C" bfc_ch_t *bfcg_pop_host(const bfc_ch_t *ch, int min_cnt, int max_arm, int max_diff, int max_mean, int max_rounds, uint64_t *stats, int *n_rounds)
{
	if (!ch || !n_rounds) { bfcg::fail("bad arguments to bfcg_pop_host"); return NULL; }
	const PopRule A = { min_cnt, max_arm, max_diff, max_mean, max_rounds };
	if (pop_check(PopRule::who_host, bfc_ch_get_k(ch), A) != 0) return NULL;
	return clean_run_host(ch, A, stats, n_rounds);
}
