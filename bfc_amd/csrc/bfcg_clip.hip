// bfcg_clip.hip -- the count table's de Bruijn graph cleaned where it lies in HBM: the short, thinly covered dead ends (tips) and, on
// request, the short components that touch nothing (islands) are removed, round by round, into a new table that owns its slots.
// include/bfc_gpu.h defines which unitigs are clippable and what a round is; DESIGN.md section 6e.  The round -- the listing of the open
// ends, k_clean_walk, the survivors into a new table, the rounds of a call and the host twin's -- is bfcg_gclean.h's, shared with
// bfcg_pop.hip; this file holds the rule it applies and the two entry points.
//   ClipRule   a side starts a walk if its stop code is DEAD (1 or 6).  decide() walks away from the dead end for at most max_tip k-mers
//              (arm_walk, bfcg_glink.h) and sums the counts; a lane that has not met an open side by then stops -- the unitig is too long
//              --, so no lane walks more than max_tip steps, however long the graph's unitigs are.  At the far end it knows tip, island
//              or neither; of an island's two lanes the one text_less picks (the unitigs' rule of which end emits) goes on.  Then the
//              mean rule
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "bfcg_gprobe.h"
#include "bfcg_glink.h"
#include "bfcg_gclean.h"

namespace {

enum { CLIP_MAX_TIP = 65535 };

struct ClipRule {
	int min_cnt, max_tip, max_mean, flags, max_rounds;
	static constexpr const char *who_dev = "bfcg_kmers_clip", *who_host = "bfcg_clip_host";
	static constexpr const char *what_marks = "the marks of the clipped k-mers", *what_ctr = "the counters of a clipping round";

	__host__ __device__ __forceinline__ bool starts(int code) const { return code == 1 || code == 6; }

	// The unitig that starts at the oriented k-mer s = (sa, sb), whose left side is open with a DEAD code: its k-mers if this start removes
	// it, 0 if not, -1 if a k-mer of the walk is not in the table (it changed under the call).  `tab` answers present4 as for link_rule and
	// value_at(a, b, slot)
	template <class T>
	__host__ __device__ __forceinline__ int decide(const T &tab, int k, uint64_t sa, uint64_t sb) const
	{
		uint64_t a = sa, b = sb, ya, yb, sum;
		int n;
		const int right = arm_walk(tab, k, min_cnt, max_tip, a, b, ya, yb, n, sum);
		if (right <= 0) return right; // too long, or lost
		if (starts(right)) { // an island: both its ends start a walk
			uint64_t ra, rb;
			rc_planes(k, a, b, ra, rb);
			if (!(flags & BFCG_CLIP_ISLANDS) || !text_less(sa, sb, ra, rb)) return 0;
		}
		return sum <= (uint64_t)max_mean * (uint64_t)n ? n : 0;
	}
};

// what both entry points refuse before anything else
int clip_check(const char *who, int k, const ClipRule &A)
{
	if (check_min_cnt(who, A.min_cnt) != 0 || check_unitig_k(who, k) != 0) return -1;
	if (A.max_tip < 1 || A.max_tip > CLIP_MAX_TIP) return bfcg::fail("%s: max_tip %d is outside [1, %d]: a lane walks a clippable unitig alone", who, A.max_tip, (int)CLIP_MAX_TIP);
	if (A.max_mean < 1 || A.max_mean > 255) return bfcg::fail("%s: max_mean %d is outside [1, 255]: a count is 8 bits (255 switches the rule off)", who, A.max_mean);
	if (A.max_rounds < 0 || A.max_rounds > CLIP_MAX_ROUNDS) return bfcg::fail("%s: max_rounds %d is outside [0, %d]", who, A.max_rounds, (int)CLIP_MAX_ROUNDS);
	if (A.flags & ~BFCG_CLIP_ISLANDS) return bfcg::fail("%s: unknown flag bits 0x%x", who, (unsigned)(A.flags & ~BFCG_CLIP_ISLANDS));
	return 0;
}

} // namespace

extern "C" bfcg_kmers_t *bfcg_kmers_clip(bfcg_kmers_t *t, int min_cnt, int max_tip, int max_mean, int flags, int max_rounds, uint64_t *stats, int *n_rounds)
{
	if (!t || !n_rounds) { bfcg::fail("bad arguments to bfcg_kmers_clip"); return NULL; }
	const ClipRule A = { min_cnt, max_tip, max_mean, flags, max_rounds };
	if (clip_check(ClipRule::who_dev, t->k, A) != 0) return NULL;
	return t->k <= 32 ? clean_run<uint32_t>(t, A, stats, n_rounds) : clean_run<uint64_t>(t, A, stats, n_rounds);
}

// the host twin: no GPU
extern "C" bfc_ch_t *bfcg_clip_host(const bfc_ch_t *ch, int min_cnt, int max_tip, int max_mean, int flags, int max_rounds, uint64_t *stats, int *n_rounds)
{
	if (!ch || !n_rounds) { bfcg::fail("bad arguments to bfcg_clip_host"); return NULL; }
	const ClipRule A = { min_cnt, max_tip, max_mean, flags, max_rounds };
	if (clip_check(ClipRule::who_host, bfc_ch_get_k(ch), A) != 0) return NULL;
	return clean_run_host(ch, A, stats, n_rounds);
}
