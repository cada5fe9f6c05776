// bfcg_unitigs.hip -- the compacted de Bruijn graph of the count table where it lies in HBM: every maximal non-branching path (unitig)
// exactly once, as bases.  include/bfc_gpu.h defines nodes, link(x), paths, cycles and which spelling is emitted; DESIGN.md section 6d.
// The k-mer in registers and the probes are bfcg_gprobe.h's, the compaction of the path ends is bfcg_klist.h's.
//   link_rule        (bfcg_glink.h) the rule that joins two nodes, written once for the kernels and bfcg_unitigs_host
//   k_tab_list       bfcg_klist.h with EndPred (bfcg_glink.h): a node is kept if one of its sides is open; the two stop codes are the third column
//   k_ut_path_count  one lane per (path end, side): an open side is a start; the lane walks to the far end, counts k-mers and counts,
//                    marks every node it passes in a bitmap of one bit per slot (a plain vector atomicOr) and decides whether its end
//                    emits (its first k-mer is smaller as text than the reverse complement of the far end's)
//   k_ut_unmarked    a streaming pass: the nodes without a mark have both sides linked and lie on no path -- they are the cycles' nodes
//   k_ut_cycle_count one lane per such node walks its cycle from its smaller strand and gives up at the first oriented k-mer smaller
//                    than that; only the cycle's smallest oriented k-mer completes the lap, and it emits
//   k_list_scan      (bfcg_klist.h) the winners' flags and lengths into unitig indices and base offsets
//   k_ut_fill        one lane per winner walks again and writes the bases at its offset
// The walk kernels run workgroups of one wave: the walks of a wave end when its longest ends, and a long one then holds back 63 lanes and
// no other wave; the bitmap's atomics return nothing and are executed at the memory side, one dword each, so a lane does not wait for
// them.  A launch takes at most `ut_cap` starts (BFCG_UNITIG_CAP when the object is made).
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

namespace {

enum { UT_CAP = 1 << 22, UT_GRID_MAX = 2048 }; // UT_BT, the buffers B_*, link_rule, EndPred, set_mark: bfcg_glink.h
enum { STOP_CYCLE = 64 };
enum { CTR_CAND = 0, CTR_ERR = 1, CTR_N = 2 };

struct Start { uint64_t a, b, sum; uint32_t nk, ends; }; // a winner: the planes of its first oriented k-mer, the sum of the counts, the k-mers, the ends byte

__host__ __device__ __forceinline__ uint8_t base_at(uint64_t a, uint64_t b, int l) { return (uint8_t)"ACGT"[(b >> l & 1) << 1 | (a >> l & 1)]; }

// ---- the counting walks ----------------------------------------------------------------------------------------------------------------
// start i in [first, end): walk_start's (bfcg_glink.h)
template <typename W>
__global__ __launch_bounds__(UT_BT) void k_ut_path_count(TabRef T, int min_cnt, const ulonglong2 *__restrict__ node_y, const uint8_t *__restrict__ node_code, uint64_t first,
                                                         uint64_t end, uint64_t max_steps, uint32_t *__restrict__ mark, Start *__restrict__ rec, uint32_t *__restrict__ win,
                                                         uint32_t *__restrict__ len, unsigned long long *__restrict__ ctr)
{
	const uint64_t i = first + (uint64_t)blockIdx.x * UT_BT + threadIdx.x;
	if (i >= end) return;
	int left;
	uint64_t sa, sb, slot = 0;
	if (!walk_start(T.k, node_y, node_code, i, OpenSide(), left, sa, sb)) return; // this side is linked: the path comes in here, it does not start
	DevGraph<W> g; g.T = T;
	int v = g.value_at(sa, sb, slot);
	if (v < 0) { atomicOr(&ctr[CTR_ERR], 1ULL); return; } // (a listed node is in the table unless the table changed)
	set_mark(mark, slot);
	uint64_t a = sa, b = sb, ya, yb, n = 1, sum = (uint64_t)(v & 0xff);
	int right;
	while ((right = link_rule(g, T.k, a, b, min_cnt, ya, yb)) == 0) {
		v = g.value_at(ya, yb, slot);
		if (v < 0 || n >= max_steps) { atomicOr(&ctr[CTR_ERR], 1ULL); return; }
		set_mark(mark, slot);
		sum += (uint64_t)(v & 0xff); ++n;
		a = ya; b = yb;
	}
	uint64_t ra, rb;
	rc_planes(T.k, a, b, ra, rb);
	if (!text_less(sa, sb, ra, rb)) return; // the other end emits
	Start r;
	r.a = sa; r.b = sb; r.sum = sum; r.nk = (uint32_t)n; r.ends = (uint32_t)(left | right << 3);
	rec[i] = r; win[i] = 1; len[i] = (uint32_t)(T.k + n - 1);
}

// the slots that are nodes and carry no mark, in no particular order: cand[0, min(*n, cap)), ctr[CTR_CAND] = their number
__global__ __launch_bounds__(BT) void k_ut_unmarked(const ulonglong2 *__restrict__ tab, uint64_t n_pairs, int min_cnt, const uint32_t *__restrict__ mark,
                                                    unsigned long long *__restrict__ cand, uint64_t cap, unsigned long long *__restrict__ ctr)
{
	for (uint64_t q = (uint64_t)blockIdx.x * BT + threadIdx.x; q < n_pairs; q += (uint64_t)gridDim.x * BT) {
		const ulonglong2 v = tab[q];
		const uint32_t bits = mark[q >> 4] >> (2 * (q & 15));
		const bool c0 = (int)(v.x & 0xff) >= min_cnt && !(bits & 1), c1 = (int)(v.y & 0xff) >= min_cnt && !(bits & 2); // (an empty slot has count 0 < min_cnt)
		if (c0 || c1) { // rare: the nodes of cycles
			uint64_t at = atomicAdd(&ctr[CTR_CAND], (unsigned long long)c0 + c1);
			if (c0) { if (at < cap) cand[at] = 2 * q; ++at; }
			if (c1 && at < cap) cand[at] = 2 * q + 1;
		}
	}
}

// candidate j in [first, end): the node in slot cand[j]
template <typename W>
__global__ __launch_bounds__(UT_BT) void k_ut_cycle_count(TabRef T, int min_cnt, const unsigned long long *__restrict__ cand, uint64_t first, uint64_t end, uint64_t max_steps,
                                                          Start *__restrict__ rec, uint32_t *__restrict__ win, uint32_t *__restrict__ len, unsigned long long *__restrict__ ctr)
{
	const uint64_t j = first + (uint64_t)blockIdx.x * UT_BT + threadIdx.x;
	if (j >= end) return;
	DevGraph<W> g; g.T = T;
	const uint64_t s = cand[j], word = T.tab[s];
	uint64_t sa, sb, ra, rb, slot = 0;
	kdec::decode(T.k, T.l_pre, (uint32_t)(s >> T.cshift), word, sa, sb);
	rc_planes(T.k, sa, sb, ra, rb);
	if (text_less(ra, rb, sa, sb)) { sa = ra; sb = rb; } // the node's smaller strand
	uint64_t a = sa, b = sb, ya, yb, n = 1, sum = word & 0xff;
	for (;;) {
		if (link_rule(g, T.k, a, b, min_cnt, ya, yb) != 0) { atomicOr(&ctr[CTR_ERR], 2ULL); return; } // (an open side would have been marked)
		if (ya == sa && yb == sb) break; // once round
		rc_planes(T.k, ya, yb, ra, rb);
		if (text_less(ya, yb, sa, sb) || text_less(ra, rb, sa, sb)) return; // a smaller oriented k-mer lies on this cycle: its node leads
		const int v = g.value_at(ya, yb, slot);
		if (v < 0 || n >= max_steps) { atomicOr(&ctr[CTR_ERR], 2ULL); return; }
		sum += (uint64_t)(v & 0xff); ++n;
		a = ya; b = yb;
	}
	Start r;
	r.a = sa; r.b = sb; r.sum = sum; r.nk = (uint32_t)n; r.ends = STOP_CYCLE;
	rec[j] = r; win[j] = 1; len[j] = (uint32_t)(T.k + n - 1);
}

// ---- the fill walk: winner i of a set writes unitig u0 + uidx[i] at base b0 + boff[i] ------------------------------------------------------
template <typename W>
__global__ __launch_bounds__(UT_BT) void k_ut_fill(TabRef T, int min_cnt, const Start *__restrict__ rec, const uint32_t *__restrict__ win, const unsigned long long *__restrict__ uidx,
                                                   const unsigned long long *__restrict__ boff, uint64_t first, uint64_t end, uint64_t u0, uint64_t b0, uint8_t *__restrict__ seq,
                                                   unsigned long long *__restrict__ off, uint32_t *__restrict__ n_kmers, unsigned long long *__restrict__ cnt_sum, uint8_t *__restrict__ ends)
{
	const uint64_t i = first + (uint64_t)blockIdx.x * UT_BT + threadIdx.x;
	if (i >= end || !win[i]) return;
	DevGraph<W> g; g.T = T;
	const Start r = rec[i];
	const uint64_t u = u0 + uidx[i];
	uint64_t p = b0 + boff[i], a = r.a, b = r.b;
	off[u] = p; n_kmers[u] = r.nk; cnt_sum[u] = r.sum; ends[u] = (uint8_t)r.ends;
	for (int l = T.k - 1; l >= 0; --l) seq[p++] = base_at(a, b, l);
	for (uint32_t j = 1; j < r.nk; ++j) { // k + nk - 1 bases in all: what the scan gave this unitig
		succ_planes(T.k, a, b, only_succ(g, a, b, min_cnt), a, b);
		seq[p++] = base_at(a, b, 0);
	}
}

int check_unitig_bufs(const char *who, const uint8_t *seq, uint64_t seq_cap, const void *off, const void *n_kmers, const void *cnt_sum, const void *ends, uint64_t n_cap)
{
	if ((seq_cap && !seq) || (n_cap && (!off || !n_kmers || !cnt_sum || !ends))) return bfcg::fail("%s needs output buffers for seq_cap=%llu, n_cap=%llu", who, (unsigned long long)seq_cap, (unsigned long long)n_cap);
	return 0;
}


// the records, flags, lengths and scans of a set of n starts (flags and lengths zeroed: a start that does not emit writes nothing)
int set_alloc(bfcg_kmers_t *t, int set, uint64_t n, uint64_t &n_pad)
{
	const uint64_t per = SCAN_BT * SCAN_PER;
	n_pad = (n + per - 1) / per * per;
	if (n == 0) return 0;
	if (ut_grow(t, set + B_REC, n * sizeof(Start), "the starts of the unitigs") != 0 || ut_grow(t, set + B_WIN, n_pad * 4, "the starts of the unitigs") != 0 ||
	    ut_grow(t, set + B_LEN, n_pad * 4, "the starts of the unitigs") != 0 || ut_grow(t, set + B_UIDX, (n_pad + 1) * 8, "the starts of the unitigs") != 0 ||
	    ut_grow(t, set + B_BOFF, (n_pad + 1) * 8, "the starts of the unitigs") != 0) return -1;
	BFCG_CK(hipMemsetAsync(t->d_ut[set + B_WIN], 0, n_pad * 4, t->st));
	BFCG_CK(hipMemsetAsync(t->d_ut[set + B_LEN], 0, n_pad * 4, t->st));
	return 0;
}
// the scans of a set, its totals read into tot[0] (unitigs) and tot[1] (bases) when the stream is synchronised
int set_scan(bfcg_kmers_t *t, int set, uint64_t n, uint64_t n_pad, unsigned long long tot[2])
{
	tot[0] = tot[1] = 0;
	if (n == 0) return 0;
	hipLaunchKernelGGL(k_list_scan, dim3(1), dim3(SCAN_BT), 0, t->st, ut_buf<uint32_t>(t, set + B_WIN), n_pad, ut_buf<unsigned long long>(t, set + B_UIDX));
	hipLaunchKernelGGL(k_list_scan, dim3(1), dim3(SCAN_BT), 0, t->st, ut_buf<uint32_t>(t, set + B_LEN), n_pad, ut_buf<unsigned long long>(t, set + B_BOFF));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(&tot[0], ut_buf<unsigned long long>(t, set + B_UIDX) + n_pad, 8, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(&tot[1], ut_buf<unsigned long long>(t, set + B_BOFF) + n_pad, 8, hipMemcpyDeviceToHost, t->st));
	return 0;
}
template <typename W> int set_fill(bfcg_kmers_t *t, const TabRef &T, int min_cnt, int set, uint64_t n, uint64_t u0, uint64_t b0)
{
	for (uint64_t first = 0; first < n; first += t->ut_cap) {
		const uint64_t end = n - first < t->ut_cap ? n : first + t->ut_cap;
		hipLaunchKernelGGL((k_ut_fill<W>), dim3((unsigned)((end - first + UT_BT - 1) / UT_BT)), dim3(UT_BT), 0, t->st, T, min_cnt, ut_buf<Start>(t, set + B_REC),
		                   ut_buf<uint32_t>(t, set + B_WIN), ut_buf<unsigned long long>(t, set + B_UIDX), ut_buf<unsigned long long>(t, set + B_BOFF), first, end, u0, b0,
		                   ut_buf<uint8_t>(t, B_SEQ), ut_buf<unsigned long long>(t, B_OFF), ut_buf<uint32_t>(t, B_NK), ut_buf<unsigned long long>(t, B_SUM), ut_buf<uint8_t>(t, B_ENDS));
	}
	BFCG_CK(hipGetLastError());
	return 0;
}

template <typename W>
int unitigs_run(bfcg_kmers_t *t, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends, uint64_t n_cap, uint64_t n[2])
{
	const TabRef T = tab_ref(t);
	const uint64_t n_slots = 1ULL << (t->l_pre + t->cshift), n_pairs = n_slots >> 1;
	float ms = 0;
	// the path ends: the listing's two passes, the rows left on the device (planes in d_y, the two stop codes in d_oth)
	EndPred<W> P; P.T = T; P.min_cnt = min_cnt;
	uint64_t n_ends = 0;
	if (list_dev(t, "bfcg_kmers_unitigs", P, min_cnt, -64, 0, 1u << t->l_pre, true, ~0ULL, &n_ends) != 0) return -1;
	ms = t->last_ms; t->last_ms = 0;
	// the counting walks of the paths, then the nodes they left unmarked
	const uint64_t n_a = 2 * n_ends;
	uint64_t pad_a = 0, pad_b = 0;
	if (ut_grow(t, B_MARK, (n_slots + 31) / 32 * 4, "the marks of the unitigs' walks") != 0 || ut_grow(t, B_CTR, CTR_N * 8, "the counters of the unitigs' walks") != 0) return -1;
	if (set_alloc(t, 0, n_a, pad_a) != 0) return -1;
	unsigned long long ctr[CTR_N] = { 0, 0 };
	BFCG_CK(hipEventRecord(t->e0, t->st));
	BFCG_CK(hipMemsetAsync(t->d_ut[B_MARK], 0, (n_slots + 31) / 32 * 4, t->st));
	BFCG_CK(hipMemsetAsync(t->d_ut[B_CTR], 0, CTR_N * 8, t->st));
	for (uint64_t first = 0; first < n_a; first += t->ut_cap) {
		const uint64_t end = n_a - first < t->ut_cap ? n_a : first + t->ut_cap;
		hipLaunchKernelGGL((k_ut_path_count<W>), dim3((unsigned)((end - first + UT_BT - 1) / UT_BT)), dim3(UT_BT), 0, t->st, T, min_cnt, (const ulonglong2 *)t->d_y,
		                   (const uint8_t *)t->d_oth, first, end, n_slots, ut_buf<uint32_t>(t, B_MARK), ut_buf<Start>(t, B_REC), ut_buf<uint32_t>(t, B_WIN), ut_buf<uint32_t>(t, B_LEN),
		                   ut_buf<unsigned long long>(t, B_CTR));
	}
	const unsigned grid = (unsigned)((n_pairs + BT - 1) / BT < UT_GRID_MAX ? (n_pairs + BT - 1) / BT : UT_GRID_MAX);
	for (int round = 0; round < 2; ++round) { // the second time with room for all of them
		const uint64_t cap = t->ut_bytes[B_CAND] / 8;
		hipLaunchKernelGGL(k_ut_unmarked, dim3(grid), dim3(BT), 0, t->st, (const ulonglong2 *)t->table, n_pairs, min_cnt, ut_buf<uint32_t>(t, B_MARK), ut_buf<unsigned long long>(t, B_CAND),
		                   cap, ut_buf<unsigned long long>(t, B_CTR));
		BFCG_CK(hipEventRecord(t->e1, t->st));
		BFCG_CK(hipGetLastError());
		BFCG_CK(hipMemcpyAsync(ctr, t->d_ut[B_CTR], sizeof(ctr), hipMemcpyDeviceToHost, t->st));
		if (ut_lap(t, &ms) != 0) return -1;
		if (ctr[CTR_ERR]) return bfcg::fail("bfcg_kmers_unitigs: a walk left the graph it started in (code %llu): the table changed under the call", ctr[CTR_ERR]);
		if (ctr[CTR_CAND] <= cap) break;
		if (ut_grow(t, B_CAND, ctr[CTR_CAND] * 8, "the nodes of the cycles") != 0) return -1;
		BFCG_CK(hipEventRecord(t->e0, t->st));
		BFCG_CK(hipMemsetAsync(t->d_ut[B_CTR], 0, 8, t->st));
	}
	// the cycles' walks, and the scans of both sets
	const uint64_t n_b = ctr[CTR_CAND];
	if (set_alloc(t, SET, n_b, pad_b) != 0) return -1;
	unsigned long long tot_a[2], tot_b[2];
	BFCG_CK(hipEventRecord(t->e0, t->st));
	for (uint64_t first = 0; first < n_b; first += t->ut_cap) {
		const uint64_t end = n_b - first < t->ut_cap ? n_b : first + t->ut_cap;
		hipLaunchKernelGGL((k_ut_cycle_count<W>), dim3((unsigned)((end - first + UT_BT - 1) / UT_BT)), dim3(UT_BT), 0, t->st, T, min_cnt, ut_buf<unsigned long long>(t, B_CAND), first, end,
		                   n_slots, ut_buf<Start>(t, SET + B_REC), ut_buf<uint32_t>(t, SET + B_WIN), ut_buf<uint32_t>(t, SET + B_LEN), ut_buf<unsigned long long>(t, B_CTR));
	}
	if (set_scan(t, 0, n_a, pad_a, tot_a) != 0 || set_scan(t, SET, n_b, pad_b, tot_b) != 0) return -1;
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(ctr, t->d_ut[B_CTR], sizeof(ctr), hipMemcpyDeviceToHost, t->st));
	if (ut_lap(t, &ms) != 0) return -1;
	if (ctr[CTR_ERR]) return bfcg::fail("bfcg_kmers_unitigs: a walk left the graph it started in (code %llu): the table changed under the call", ctr[CTR_ERR]);
	t->last_ms = ms;
	n[0] = tot_a[0] + tot_b[0]; n[1] = tot_a[1] + tot_b[1];
	if (n[0] > n_cap || n[1] > seq_cap) return 1; // nothing is written: the caller comes back with room for n[]
	if (n[0] == 0) { if (off) off[0] = 0; return 0; }
	// the fill walks and the copies
	if (ut_grow(t, B_SEQ, n[1], "the unitigs' bases") != 0 || ut_grow(t, B_OFF, n[0] * 8, "the unitigs' offsets") != 0 || ut_grow(t, B_NK, n[0] * 4, "the unitigs' sizes") != 0 ||
	    ut_grow(t, B_SUM, n[0] * 8, "the unitigs' sums") != 0 || ut_grow(t, B_ENDS, n[0], "the unitigs' ends") != 0) return -1;
	BFCG_CK(hipEventRecord(t->e0, t->st));
	if (set_fill<W>(t, T, min_cnt, 0, n_a, 0, 0) != 0 || set_fill<W>(t, T, min_cnt, SET, n_b, tot_a[0], tot_a[1]) != 0) return -1;
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipMemcpyAsync(seq, t->d_ut[B_SEQ], n[1], hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(off, t->d_ut[B_OFF], n[0] * 8, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(n_kmers, t->d_ut[B_NK], n[0] * 4, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(cnt_sum, t->d_ut[B_SUM], n[0] * 8, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(ends, t->d_ut[B_ENDS], n[0], hipMemcpyDeviceToHost, t->st));
	if (ut_lap(t, &ms) != 0) return -1;
	off[n[0]] = n[1];
	t->last_ms = ms;
	return 0;
}

} // namespace

uint64_t bfcg::unitig_cap()
{
	const char *s = getenv("BFCG_UNITIG_CAP");
	const unsigned long long v = s ? strtoull(s, NULL, 10) : 0;
	return v ? v : UT_CAP;
}

extern "C" int bfcg_kmers_unitigs(bfcg_kmers_t *t, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                                  uint64_t n_cap, uint64_t n[2])
{
	if (!t || !n) return bfcg::fail("bad arguments to bfcg_kmers_unitigs");
	if (check_min_cnt("bfcg_kmers_unitigs", min_cnt) != 0 || check_unitig_k("bfcg_kmers_unitigs", t->k) != 0) return -1;
	if (check_unitig_bufs("bfcg_kmers_unitigs", seq, seq_cap, off, n_kmers, cnt_sum, ends, n_cap) != 0) return -1;
	if (t->l_pre + t->cshift > 31) return bfcg::fail("bfcg_kmers_unitigs: a table of 2^%d slots is too large: a unitig's k-mers and bases are counted in 32 bits", t->l_pre + t->cshift);
	t->last_ms = 0;
	BFCG_CK(hipSetDevice(t->device));
	return t->k <= 32 ? unitigs_run<uint32_t>(t, min_cnt, seq, seq_cap, off, n_kmers, cnt_sum, ends, n_cap, n)
	                  : unitigs_run<uint64_t>(t, min_cnt, seq, seq_cap, off, n_kmers, cnt_sum, ends, n_cap, n);
}

// ---- the host twin: no GPU -----------------------------------------------------------------------------------------------------------------
// Another route to the same set, with link_rule in common: the nodes are looked at in bfc_ch_export_sorted's order, twice.  First every
// node with an open side that no walk has passed yet: one walk from that side to the far end marks the path's nodes (a hash set of
// their smaller strands) and emits the spelling that starts at the smaller of the two ends.  Then every node still unmarked: it lies on
// a cycle, one lap from it marks the cycle and finds its smallest oriented k-mer, from which it is spelled.

#include <unordered_set>
#include <vector>

namespace {


struct HostUnitigs {
	HostGraph g; int min_cnt;
	std::unordered_set<Planes, PlanesHash> seen;
	std::vector<Start> out;
	uint64_t bases;

	bool mark(uint64_t a, uint64_t b) // false if the node was marked before
	{
		uint64_t ra, rb;
		rc_planes(g.k, a, b, ra, rb);
		const Planes c = text_less(ra, rb, a, b) ? Planes{ ra, rb } : Planes{ a, b };
		return seen.insert(c).second;
	}
	void emit(uint64_t a, uint64_t b, uint64_t nk, uint64_t sum, int e)
	{
		Start r;
		r.a = a; r.b = b; r.sum = sum; r.nk = (uint32_t)nk; r.ends = (uint32_t)e;
		out.push_back(r);
		bases += g.k + nk - 1;
	}
	void path(uint64_t sa, uint64_t sb, int cnt, int left) // from s, whose left side is open with code `left`
	{
		uint64_t a = sa, b = sb, ya, yb, ra, rb, nk = 1, sum = (uint64_t)cnt;
		int right;
		while ((right = link_rule(g, g.k, a, b, min_cnt, ya, yb)) == 0) {
			mark(ya, yb);
			sum += (uint64_t)(g.value(ya, yb) & 0xff); ++nk;
			a = ya; b = yb;
		}
		rc_planes(g.k, a, b, ra, rb);
		if (text_less(sa, sb, ra, rb)) emit(sa, sb, nk, sum, left | right << 3);
		else emit(ra, rb, nk, sum, right | left << 3);
	}
	void cycle(uint64_t xa, uint64_t xb, int cnt) // one lap from x
	{
		uint64_t a = xa, b = xb, ya, yb, ra, rb, nk = 1, sum = (uint64_t)cnt;
		rc_planes(g.k, xa, xb, ra, rb);
		Planes least = text_less(ra, rb, xa, xb) ? Planes{ ra, rb } : Planes{ xa, xb };
		while (link_rule(g, g.k, a, b, min_cnt, ya, yb) == 0 && !(ya == xa && yb == xb)) {
			mark(ya, yb);
			rc_planes(g.k, ya, yb, ra, rb);
			if (text_less(ya, yb, least.a, least.b)) least = Planes{ ya, yb };
			if (text_less(ra, rb, least.a, least.b)) least = Planes{ ra, rb };
			sum += (uint64_t)(g.value(ya, yb) & 0xff); ++nk;
			a = ya; b = yb;
		}
		emit(least.a, least.b, nk, sum, STOP_CYCLE);
	}
	int run()
	{
		bases = 0;
		if (each_slot_host(g.ch, [&](uint64_t, uint64_t slot, uint64_t a, uint64_t b) {
			const int cnt = (int)(slot & 0xff);
			uint64_t ra, rb, ya, yb;
			rc_planes(g.k, a, b, ra, rb);
			if (cnt < min_cnt || seen.count(text_less(ra, rb, a, b) ? Planes{ ra, rb } : Planes{ a, b })) return;
			const int left = link_rule(g, g.k, ra, rb, min_cnt, ya, yb), right = left ? 0 : link_rule(g, g.k, a, b, min_cnt, ya, yb);
			if (!left && !right) return;
			mark(a, b);
			if (left) path(a, b, cnt, left);
			else path(ra, rb, cnt, right);
		}) < 0) return -1;
		if (each_slot_host(g.ch, [&](uint64_t, uint64_t slot, uint64_t a, uint64_t b) {
			const int cnt = (int)(slot & 0xff);
			if (cnt >= min_cnt && mark(a, b)) cycle(a, b, cnt);
		}) < 0) return -1;
		return 0;
	}
};

} // namespace

extern "C" int bfcg_unitigs_host(const bfc_ch_t *ch, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                                 uint64_t n_cap, uint64_t n[2])
{
	if (!ch || !n) return bfcg::fail("bad arguments to bfcg_unitigs_host");
	if (check_min_cnt("bfcg_unitigs_host", min_cnt) != 0 || check_unitig_k("bfcg_unitigs_host", bfc_ch_get_k(ch)) != 0) return -1;
	if (check_unitig_bufs("bfcg_unitigs_host", seq, seq_cap, off, n_kmers, cnt_sum, ends, n_cap) != 0) return -1;
	HostUnitigs h;
	h.g.ch = ch; h.g.k = bfc_ch_get_k(ch); h.min_cnt = min_cnt;
	if (h.run() != 0) return -1;
	n[0] = h.out.size(); n[1] = h.bases;
	if (n[0] > n_cap || n[1] > seq_cap) return 1;
	uint64_t p = 0;
	for (uint64_t u = 0; u < n[0]; ++u) {
		const Start &r = h.out[u];
		uint64_t a = r.a, b = r.b;
		off[u] = p; n_kmers[u] = r.nk; cnt_sum[u] = r.sum; ends[u] = (uint8_t)r.ends;
		for (int l = h.g.k - 1; l >= 0; --l) seq[p++] = base_at(a, b, l);
		for (uint32_t j = 1; j < r.nk; ++j) {
			succ_planes(h.g.k, a, b, only_succ(h.g, a, b, min_cnt), a, b);
			seq[p++] = base_at(a, b, 0);
		}
	}
	if (off) off[n[0]] = p;
	return 0;
}
