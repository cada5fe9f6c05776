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
// bfcg_kmers_unitig_graph is the same run with the edges between the oriented unitigs found after the fill:
//   k_ut_fill<W, true>  also writes the planes of the unitig's first and last k-mer and enters the slots of a path's two end nodes
//                    into the end map, an open-addressing table of slot << 32 | unitig with linear probing, twice as large as its
//                    entries at least (BFCG_LINK_MAP_MIN=1 when the object is made: the smallest power of two above them)
//   k_ut_links       one lane per (unitig, side): one present4 on the side's last oriented k-mer, and per present successor its slot,
//                    the map's unitig for that slot and the orientation in which the successor is that unitig's first k-mer
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
enum { LC_EDGES = 0, LC_ERR = 1, LC_N = 2 }; // d_ut[B_LCTR]: the links written, and what went wrong on the way to them
#define MAP_EMPTY (~0ULL) // (a slot index has 31 bits at most: no entry is all ones)

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

// ---- the end map: from the table slot of a path's end node to its unitig -----------------------------------------------------------------
// `mask` + 1 words, a power of two above the number of entries, so a probe always meets an empty word; a probe gives up after one round
// all the same
struct EndMap { unsigned long long *w; uint64_t mask; };
struct FillLinks { EndMap map; ulonglong2 *first, *last; unsigned long long *lctr; }; // what k_ut_fill<W, true> writes besides the unitig

__device__ __forceinline__ uint64_t map_home(const EndMap &M, uint64_t slot) { return (slot * 0x9E3779B97F4A7C15ULL >> 32) & M.mask; }
__device__ __forceinline__ bool map_put(const EndMap &M, uint64_t slot, uint64_t u) // a compare-and-swap on an empty word, as bfcg_upsert.h's
{
	uint64_t pos = map_home(M, slot);
	for (uint64_t probe = 0; probe <= M.mask; ++probe, pos = (pos + 1) & M.mask)
		if (atomicCAS(&M.w[pos], MAP_EMPTY, (unsigned long long)(slot << 32 | u)) == MAP_EMPTY) return true;
	return false;
}
__device__ __forceinline__ int64_t map_get(const EndMap &M, uint64_t slot) // the unitig, or -1
{
	uint64_t pos = map_home(M, slot);
	for (uint64_t probe = 0; probe <= M.mask; ++probe, pos = (pos + 1) & M.mask) {
		const unsigned long long e = M.w[pos];
		if (e == MAP_EMPTY) return -1;
		if (e >> 32 == slot) return (int64_t)(e & 0xffffffffULL);
	}
	return -1;
}

// ---- the fill walk: winner i of a set writes unitig u0 + uidx[i] at base b0 + boff[i] ------------------------------------------------------
// With LINKS it leaves first[u] and last[u] as well, and a path enters the slots of its two end nodes (one entry if they are one node)
// into the end map; a cycle enters nothing: no edge leads into it from outside
template <typename W, bool LINKS>
__global__ __launch_bounds__(UT_BT) void k_ut_fill(TabRef T, int min_cnt, const Start *__restrict__ rec, const uint32_t *__restrict__ win, const unsigned long long *__restrict__ uidx,
                                                   const unsigned long long *__restrict__ boff, uint64_t first, uint64_t end, uint64_t u0, uint64_t b0, uint8_t *__restrict__ seq,
                                                   unsigned long long *__restrict__ off, uint32_t *__restrict__ n_kmers, unsigned long long *__restrict__ cnt_sum, uint8_t *__restrict__ ends,
                                                   FillLinks K)
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
	if constexpr (LINKS) {
		K.first[u] = make_ulonglong2(r.a, r.b); K.last[u] = make_ulonglong2(a, b);
		if (r.ends & STOP_CYCLE) return;
		uint64_t s_first = 0, s_last = 0;
		bool ok = g.value_at(r.a, r.b, s_first) >= 0 && map_put(K.map, s_first, u);
		if (ok && r.nk > 1) ok = g.value_at(a, b, s_last) >= 0 && map_put(K.map, s_last, u);
		if (!ok) atomicOr(&K.lctr[LC_ERR], 1ULL);
	}
}

// ---- the edges: lane i in [lo, end) is side i & 1 of unitig i >> 1 -----------------------------------------------------------------------
// x = the last oriented k-mer of (u, side): last[u], or rc(first[u]).  links[8 u + 4 side + c] = v << 1 | p if succ(x, c) is present and
// is the first oriented k-mer of (v, p) -- first[v] for p = 0, rc(last[v]) for p = 1 --, else -1.  The left side of such a successor is
// open (the symmetry of link, include/bfc_gpu.h), so its node is the end of a path and in the map; a miss means the table changed.
// A cycle's one successor per side is its own first k-mer in that orientation
template <typename W>
__global__ __launch_bounds__(UT_BT) void k_ut_links(TabRef T, int min_cnt, EndMap M, const ulonglong2 *__restrict__ first_km, const ulonglong2 *__restrict__ last_km,
                                                    const uint8_t *__restrict__ ends, uint64_t lo, uint64_t end, longlong2 *__restrict__ links, unsigned long long *__restrict__ lctr)
{
	const uint64_t i = lo + (uint64_t)blockIdx.x * UT_BT + threadIdx.x;
	uint32_t n_e = 0;
	if (i < end) {
		const uint64_t u = i >> 1;
		const int side = (int)(i & 1);
		const ulonglong2 f = first_km[u], l = last_km[u];
		long long out[4] = { -1, -1, -1, -1 };
		uint64_t xa = l.x, xb = l.y, ya, yb, ra, rb;
		if (side) rc_planes(T.k, f.x, f.y, xa, xb);
		if (ends[u] & STOP_CYCLE) {
			ya = f.x; yb = f.y;
			if (side) rc_planes(T.k, l.x, l.y, ya, yb);
			const int c = (int)((yb & 1) << 1 | (ya & 1));
#pragma unroll
			for (int j = 0; j < 4; ++j) if (j == c) out[j] = (long long)(u << 1 | (uint64_t)side);
			n_e = 1;
		} else {
			DevGraph<W> g; g.T = T;
			const int o = g.present4(xa, xb, 0, min_cnt);
			bool bad = false;
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				if (!(o >> c & 1)) continue;
				uint64_t slot = 0;
				succ_planes(T.k, xa, xb, c, ya, yb);
				const int64_t v = g.value_at(ya, yb, slot) >= 0 ? map_get(M, slot) : -1;
				if (v < 0) { bad = true; continue; }
				const ulonglong2 vf = first_km[v], vl = last_km[v];
				rc_planes(T.k, vl.x, vl.y, ra, rb);
				if (ya == vf.x && yb == vf.y) out[c] = (long long)(v << 1);
				else if (ya == ra && yb == rb) out[c] = (long long)(v << 1 | 1);
				else { bad = true; continue; }
				++n_e;
			}
			if (bad) atomicOr(&lctr[LC_ERR], 2ULL);
		}
		links[2 * i] = make_longlong2(out[0], out[1]); links[2 * i + 1] = make_longlong2(out[2], out[3]);
	}
#pragma unroll
	for (int d = 32; d; d >>= 1) n_e += __shfl_down(n_e, d, 64);
	if (lane_id() == 0 && n_e) atomicAdd(&lctr[LC_EDGES], (unsigned long long)n_e);
}

// where a call's edges go: a call without edges (bfcg_kmers_unitigs, bfcg_unitigs_host) passes no LinksOut at all, so that one argument
// says both whether edges are wanted and where they are written (NULL there is the sizing call's, like the other buffers)
struct LinksOut { int64_t *links; };

int check_unitig_bufs(const char *who, const uint8_t *seq, uint64_t seq_cap, const void *off, const void *n_kmers, const void *cnt_sum, const void *ends, uint64_t n_cap,
                      const LinksOut *lo)
{
	if ((seq_cap && !seq) || (n_cap && (!off || !n_kmers || !cnt_sum || !ends || (lo && !lo->links)))) return bfcg::fail("%s needs output buffers for seq_cap=%llu, n_cap=%llu", who, (unsigned long long)seq_cap, (unsigned long long)n_cap);
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
template <typename W, bool LINKS> int set_fill(bfcg_kmers_t *t, const TabRef &T, int min_cnt, int set, uint64_t n, uint64_t u0, uint64_t b0, const FillLinks &K)
{
	for (uint64_t first = 0; first < n; first += t->ut_cap) {
		const uint64_t end = n - first < t->ut_cap ? n : first + t->ut_cap;
		hipLaunchKernelGGL((k_ut_fill<W, LINKS>), dim3((unsigned)((end - first + UT_BT - 1) / UT_BT)), dim3(UT_BT), 0, t->st, T, min_cnt, ut_buf<Start>(t, set + B_REC),
		                   ut_buf<uint32_t>(t, set + B_WIN), ut_buf<unsigned long long>(t, set + B_UIDX), ut_buf<unsigned long long>(t, set + B_BOFF), first, end, u0, b0,
		                   ut_buf<uint8_t>(t, B_SEQ), ut_buf<unsigned long long>(t, B_OFF), ut_buf<uint32_t>(t, B_NK), ut_buf<unsigned long long>(t, B_SUM), ut_buf<uint8_t>(t, B_ENDS), K);
	}
	BFCG_CK(hipGetLastError());
	return 0;
}
// the end map's words for `paths` paths, two entries each at most: the smallest power of two >= twice the entries, or, for tests, the
// smallest one above them
uint64_t map_words(uint64_t paths, int smallest)
{
	const uint64_t entries = 2 * paths, need = smallest ? entries + 1 : 2 * entries;
	uint64_t w = 1;
	while (w < need) w <<= 1;
	return w;
}

// `who` = bfcg_kmers_unitigs (lo is NULL) or bfcg_kmers_unitig_graph, which after the fill finds the edges, writes them to lo->links and
// sets n[2]
template <typename W>
int unitigs_run(bfcg_kmers_t *t, const char *who, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                const LinksOut *lo, uint64_t n_cap, uint64_t *n)
{
	const TabRef T = tab_ref(t);
	const uint64_t n_slots = 1ULL << (t->l_pre + t->cshift), n_pairs = n_slots >> 1;
	float ms = 0;
	// the path ends: the listing's two passes, the rows left on the device (planes in d_y, the two stop codes in d_oth)
	EndPred<W> P; P.T = T; P.min_cnt = min_cnt;
	uint64_t n_ends = 0;
	if (list_dev(t, who, P, min_cnt, -64, 0, 1u << t->l_pre, true, ~0ULL, &n_ends) != 0) return -1;
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
		if (ctr[CTR_ERR]) return bfcg::fail("%s: a walk left the graph it started in (code %llu): the table changed under the call", who, ctr[CTR_ERR]);
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
	if (ctr[CTR_ERR]) return bfcg::fail("%s: a walk left the graph it started in (code %llu): the table changed under the call", who, ctr[CTR_ERR]);
	t->last_ms = ms;
	n[0] = tot_a[0] + tot_b[0]; n[1] = tot_a[1] + tot_b[1];
	if (n[0] > n_cap || n[1] > seq_cap) return 1; // nothing is written: the caller comes back with room for n[]
	if (n[0] == 0) { if (off) off[0] = 0; if (lo) n[2] = 0; return 0; }
	// the fill walks and the copies
	FillLinks K = { { NULL, 0 }, NULL, NULL, NULL };
	if (lo) {
		const uint64_t words = map_words(tot_a[0], t->link_map_min);
		if (ut_grow(t, B_MAP, words * 8, "the unitigs' end map") != 0 || ut_grow(t, B_FIRST, n[0] * 16, "the unitigs' end k-mers") != 0 || ut_grow(t, B_LAST, n[0] * 16, "the unitigs' end k-mers") != 0 ||
		    ut_grow(t, B_LINKS, n[0] * 64, "the unitigs' links") != 0 || ut_grow(t, B_LCTR, LC_N * 8, "the counters of the unitigs' links") != 0) return -1;
		K.map.w = ut_buf<unsigned long long>(t, B_MAP); K.map.mask = words - 1;
		K.first = ut_buf<ulonglong2>(t, B_FIRST); K.last = ut_buf<ulonglong2>(t, B_LAST); K.lctr = ut_buf<unsigned long long>(t, B_LCTR);
	}
	if (ut_grow(t, B_SEQ, n[1], "the unitigs' bases") != 0 || ut_grow(t, B_OFF, n[0] * 8, "the unitigs' offsets") != 0 || ut_grow(t, B_NK, n[0] * 4, "the unitigs' sizes") != 0 ||
	    ut_grow(t, B_SUM, n[0] * 8, "the unitigs' sums") != 0 || ut_grow(t, B_ENDS, n[0], "the unitigs' ends") != 0) return -1;
	unsigned long long lctr[LC_N] = { 0, 0 };
	BFCG_CK(hipEventRecord(t->e0, t->st));
	if (lo) {
		BFCG_CK(hipMemsetAsync(t->d_ut[B_MAP], 0xff, (K.map.mask + 1) * 8, t->st));
		BFCG_CK(hipMemsetAsync(t->d_ut[B_LCTR], 0, LC_N * 8, t->st));
		if (set_fill<W, true>(t, T, min_cnt, 0, n_a, 0, 0, K) != 0 || set_fill<W, true>(t, T, min_cnt, SET, n_b, tot_a[0], tot_a[1], K) != 0) return -1;
		for (uint64_t first = 0; first < 2 * n[0]; first += t->ut_cap) { // the map is complete: the fills came before on this stream
			const uint64_t end = 2 * n[0] - first < t->ut_cap ? 2 * n[0] : first + t->ut_cap;
			hipLaunchKernelGGL((k_ut_links<W>), dim3((unsigned)((end - first + UT_BT - 1) / UT_BT)), dim3(UT_BT), 0, t->st, T, min_cnt, K.map, (const ulonglong2 *)K.first,
			                   (const ulonglong2 *)K.last, (const uint8_t *)ut_buf<uint8_t>(t, B_ENDS), first, end, ut_buf<longlong2>(t, B_LINKS), K.lctr);
		}
		BFCG_CK(hipGetLastError());
		BFCG_CK(hipEventRecord(t->e1, t->st));
		BFCG_CK(hipMemcpyAsync(lctr, t->d_ut[B_LCTR], sizeof(lctr), hipMemcpyDeviceToHost, t->st));
		if (ut_lap(t, &ms) != 0) return -1;
		if (lctr[LC_ERR]) return bfcg::fail("%s: an end of a unitig leads to no unitig (code %llu): the table changed under the call", who, lctr[LC_ERR]);
		BFCG_CK(hipMemcpyAsync(lo->links, t->d_ut[B_LINKS], n[0] * 64, hipMemcpyDeviceToHost, t->st));
	} else {
		if (set_fill<W, false>(t, T, min_cnt, 0, n_a, 0, 0, K) != 0 || set_fill<W, false>(t, T, min_cnt, SET, n_b, tot_a[0], tot_a[1], K) != 0) return -1;
		BFCG_CK(hipEventRecord(t->e1, t->st));
	}
	BFCG_CK(hipMemcpyAsync(seq, t->d_ut[B_SEQ], n[1], hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(off, t->d_ut[B_OFF], n[0] * 8, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(n_kmers, t->d_ut[B_NK], n[0] * 4, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(cnt_sum, t->d_ut[B_SUM], n[0] * 8, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipMemcpyAsync(ends, t->d_ut[B_ENDS], n[0], hipMemcpyDeviceToHost, t->st));
	if (lo) BFCG_CK(hipStreamSynchronize(t->st)); // (the kernels' time is in ms already)
	else if (ut_lap(t, &ms) != 0) return -1;
	off[n[0]] = n[1];
	if (lo) n[2] = lctr[LC_EDGES];
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
int bfcg::link_map_min()
{
	const char *s = getenv("BFCG_LINK_MAP_MIN");
	return s && strtoull(s, NULL, 10) == 1;
}

extern "C" int bfcg_kmers_unitigs(bfcg_kmers_t *t, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                                  uint64_t n_cap, uint64_t n[2])
{
	if (!t || !n) return bfcg::fail("bad arguments to bfcg_kmers_unitigs");
	if (check_min_cnt("bfcg_kmers_unitigs", min_cnt) != 0 || check_unitig_k("bfcg_kmers_unitigs", t->k) != 0) return -1;
	if (check_unitig_bufs("bfcg_kmers_unitigs", seq, seq_cap, off, n_kmers, cnt_sum, ends, n_cap, NULL) != 0) return -1;
	if (t->l_pre + t->cshift > 31) return bfcg::fail("bfcg_kmers_unitigs: a table of 2^%d slots is too large: a unitig's k-mers and bases are counted in 32 bits", t->l_pre + t->cshift);
	t->last_ms = 0;
	BFCG_CK(hipSetDevice(t->device));
	return t->k <= 32 ? unitigs_run<uint32_t>(t, "bfcg_kmers_unitigs", min_cnt, seq, seq_cap, off, n_kmers, cnt_sum, ends, NULL, n_cap, n)
	                  : unitigs_run<uint64_t>(t, "bfcg_kmers_unitigs", min_cnt, seq, seq_cap, off, n_kmers, cnt_sum, ends, NULL, n_cap, n);
}

extern "C" int bfcg_kmers_unitig_graph(bfcg_kmers_t *t, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                                       int64_t *links, uint64_t n_cap, uint64_t n[3])
{
	static const char who[] = "bfcg_kmers_unitig_graph";
	if (!t || !n) return bfcg::fail("bad arguments to %s", who);
	if (check_min_cnt(who, min_cnt) != 0 || check_unitig_k(who, t->k) != 0) return -1;
	const LinksOut lo = { links };
	if (check_unitig_bufs(who, seq, seq_cap, off, n_kmers, cnt_sum, ends, n_cap, &lo) != 0) return -1;
	if (t->l_pre + t->cshift > 31) return bfcg::fail("%s: a table of 2^%d slots is too large: a unitig's k-mers and bases are counted in 32 bits", who, t->l_pre + t->cshift);
	t->last_ms = 0;
	BFCG_CK(hipSetDevice(t->device));
	return t->k <= 32 ? unitigs_run<uint32_t>(t, who, min_cnt, seq, seq_cap, off, n_kmers, cnt_sum, ends, &lo, n_cap, n)
	                  : unitigs_run<uint64_t>(t, who, min_cnt, seq, seq_cap, off, n_kmers, cnt_sum, ends, &lo, n_cap, n);
}

// ---- the host twin: no GPU -----------------------------------------------------------------------------------------------------------------
// Another route to the same set, with link_rule in common: the nodes are looked at in bfc_ch_export_sorted's order, twice.  First every
// node with an open side that no walk has passed yet: one walk from that side to the far end marks the path's nodes (a hash set of
// their smaller strands) and emits the spelling that starts at the smaller of the two ends.  Then every node still unmarked: it lies on
// a cycle, one lap from it marks the cycle and finds its smallest oriented k-mer, from which it is spelled.

#include <unordered_map>
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

// bfcg_unitigs_host and bfcg_unitig_graph_host: the cap protocol, then the spellings; with `lo` the edges between them, by another
// route than the device's -- a hash map from the first oriented k-mer of every oriented unitig (first[u] for (u, 0), rc(last[u]) for
// (u, 1), cycles included) to u << 1 | o, asked for every present successor of every oriented unitig's last k-mer
int host_unitigs(const char *who, const bfc_ch_t *ch, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                 const LinksOut *lo, uint64_t n_cap, uint64_t *n)
{
	if (!ch || !n) return bfcg::fail("bad arguments to %s", who);
	if (check_min_cnt(who, min_cnt) != 0 || check_unitig_k(who, bfc_ch_get_k(ch)) != 0) return -1;
	if (check_unitig_bufs(who, seq, seq_cap, off, n_kmers, cnt_sum, ends, n_cap, lo) != 0) return -1;
	HostUnitigs h;
	h.g.ch = ch; h.g.k = bfc_ch_get_k(ch); h.min_cnt = min_cnt;
	if (h.run() != 0) return -1;
	const uint64_t n0 = h.out.size(), n1 = h.bases;
	if (n0 > n_cap || n1 > seq_cap) { n[0] = n0; n[1] = n1; return 1; }
	// everything is made here first and copied out at the end: a failure on the way writes nothing
	const int k = h.g.k;
	std::vector<uint8_t> bases(n1);
	std::vector<uint64_t> at(n0 + 1);
	std::vector<Planes> last(n0);
	uint64_t p = 0;
	for (uint64_t u = 0; u < n0; ++u) {
		const Start &r = h.out[u];
		uint64_t a = r.a, b = r.b;
		at[u] = p;
		for (int l = k - 1; l >= 0; --l) bases[p++] = base_at(a, b, l);
		for (uint32_t j = 1; j < r.nk; ++j) {
			succ_planes(k, a, b, only_succ(h.g, a, b, min_cnt), a, b);
			bases[p++] = base_at(a, b, 0);
		}
		last[u] = Planes{ a, b };
	}
	at[n0] = p;
	std::vector<int64_t> found(lo ? 8 * n0 : 0, -1);
	uint64_t edges = 0;
	if (lo) {
		std::unordered_map<Planes, int64_t, PlanesHash> head;
		uint64_t ra, rb, ya, yb;
		for (uint64_t u = 0; u < n0; ++u) {
			rc_planes(k, last[u].a, last[u].b, ra, rb);
			const bool fresh0 = head.emplace(Planes{ h.out[u].a, h.out[u].b }, (int64_t)(u << 1)).second, fresh1 = head.emplace(Planes{ ra, rb }, (int64_t)(u << 1 | 1)).second;
			if (!fresh0 || !fresh1) return bfcg::fail("%s: two oriented unitigs start with one k-mer: the table changed under the call", who);
		}
		for (uint64_t u = 0; u < n0; ++u)
			for (int o = 0; o < 2; ++o) {
				uint64_t xa = last[u].a, xb = last[u].b;
				if (o) rc_planes(k, h.out[u].a, h.out[u].b, xa, xb);
				const int succ = h.g.present4(xa, xb, 0, min_cnt);
				for (int c = 0; c < 4; ++c) {
					if (!(succ >> c & 1)) continue;
					succ_planes(k, xa, xb, c, ya, yb);
					const auto it = head.find(Planes{ ya, yb });
					if (it == head.end()) return bfcg::fail("%s: an end of a unitig leads to no unitig: the table changed under the call", who);
					found[8 * u + 4 * o + c] = it->second;
					++edges;
				}
			}
	}
	n[0] = n0; n[1] = n1;
	if (n1) memcpy(seq, bases.data(), n1);
	if (off) memcpy(off, at.data(), 8 * (n0 + 1));
	for (uint64_t u = 0; u < n0; ++u) { n_kmers[u] = h.out[u].nk; cnt_sum[u] = h.out[u].sum; ends[u] = (uint8_t)h.out[u].ends; }
	if (lo) {
		if (n0) memcpy(lo->links, found.data(), 64 * n0);
		n[2] = edges;
	}
	return 0;
}

} // namespace

extern "C" int bfcg_unitigs_host(const bfc_ch_t *ch, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                                 uint64_t n_cap, uint64_t n[2])
{
	return host_unitigs("bfcg_unitigs_host", ch, min_cnt, seq, seq_cap, off, n_kmers, cnt_sum, ends, NULL, n_cap, n);
}

extern "C" int bfcg_unitig_graph_host(const bfc_ch_t *ch, int min_cnt, uint8_t *seq, uint64_t seq_cap, uint64_t *off, uint32_t *n_kmers, uint64_t *cnt_sum, uint8_t *ends,
                                      int64_t *links, uint64_t n_cap, uint64_t n[3])
{
	const LinksOut lo = { links };
	return host_unitigs("bfcg_unitig_graph_host", ch, min_cnt, seq, seq_cap, off, n_kmers, cnt_sum, ends, &lo, n_cap, n);
}
