// bfcg_glink.h -- the link rule of the compacted graph and what goes with it, for the files that walk the count table's de Bruijn graph from
// its open ends: bfcg_unitigs.hip (every unitig as bases) and, through bfcg_gclean.h's round, bfcg_clip.hip (tips and islands removed into
// a new table) and bfcg_pop.hip (the weaker arm of every simple bubble removed likewise).  include/bfc_gpu.h
// defines nodes, link(x), paths and the stop codes; the k-mer in registers and the probes are bfcg_gprobe.h's, the listing bfcg_klist.h's.
//   rc_planes, text_less, succ_planes, pred_planes   oriented k-mers as planes, for the device and the host
//   link_rule        the rule that joins two nodes, written once for the kernels and the host twins
//   arm_walk         the unitig from an open side for a bounded number of k-mers: its length, the sum of its counts, its far end's stop code
//   EndPred          the listing's predicate: a node is kept if one of its sides is open; the two stop codes are the third column
//   walk_start       start i of such a listing as a side, its stop code and an oriented k-mer, for the kernels with one lane per start
//   set_mark         one bit per slot, a plain vector atomicOr that returns nothing
//   B_*, ut_buf ...  the object's buffers for these calls (bfcg_kmers.d_ut), grown on demand
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <unordered_set>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "kmer_dev.h"
#include "bfcg_klist.h"
#include "bfcg_gprobe.h"

namespace {

enum { UT_BT = 64 /* a lane walks a start: a workgroup is one wave */ };
// the object's buffers (bfcg_kmers.d_ut): the marks, the cycles' nodes, counters; per set of starts (paths at +0, cycles at +SET) a
// record, the winner flag, the length in bases and their scans; the call's five outputs.  A cleaning round (bfcg_gclean.h) uses the
// marks (its KILL bits) and the counters.  bfcg_kmers_unitig_graph adds the end map (slot << 32 | unitig), the planes of every unitig's
// first and last k-mer, the eight links of every unitig and its own two counters
enum { B_MARK, B_CAND, B_CTR, B_REC, B_WIN, B_LEN, B_UIDX, B_BOFF, SET = 5, B_SEQ = B_REC + 2 * SET, B_OFF, B_NK, B_SUM, B_ENDS,
       B_MAP, B_FIRST, B_LAST, B_LINKS, B_LCTR, B_N };
static_assert(B_N <= BFCG_UT_NBUF, "bfcg_kmers.d_ut is too short");

// ---- oriented k-mers as planes, for the device and the host ----------------------------------------------------------------------------
__host__ __device__ __forceinline__ void rc_planes(int k, uint64_t a, uint64_t b, uint64_t &ra, uint64_t &rb) // a, b hold nothing at and above bit k
{
	ra = __builtin_bitreverse64(~a) >> (64 - k); rb = __builtin_bitreverse64(~b) >> (64 - k);
}
// x < y as text, A < C < G < T from the 5' end (bit k - 1 of the planes; the high plane is the high code bit)
__host__ __device__ __forceinline__ bool text_less(uint64_t xa, uint64_t xb, uint64_t ya, uint64_t yb)
{
	const uint64_t d = (xa ^ ya) | (xb ^ yb);
	if (d == 0) return false;
	const int h = 63 - __builtin_clzll(d);
	return ((xb >> h & 1) << 1 | (xa >> h & 1)) < ((yb >> h & 1) << 1 | (ya >> h & 1));
}
__host__ __device__ __forceinline__ void succ_planes(int k, uint64_t a, uint64_t b, int c, uint64_t &ya, uint64_t &yb)
{
	const uint64_t m = kdec::mask(k);
	ya = (a << 1 | (uint64_t)(c & 1)) & m; yb = (b << 1 | (uint64_t)(c >> 1)) & m;
}
__host__ __device__ __forceinline__ void pred_planes(int k, uint64_t a, uint64_t b, int c, uint64_t &ya, uint64_t &yb) // a, b masked
{
	ya = a >> 1 | (uint64_t)(c & 1) << (k - 1); yb = b >> 1 | (uint64_t)(c >> 1) << (k - 1);
}

// link(x) of include/bfc_gpu.h for the oriented k-mer (a, b), masked: 0 and y = (ya, yb), or the stop code 1, 2, 3, 6; with 3 and 6
// (ya, yb) is the single successor all the same.  `tab` answers present4(a, b, pred, min_cnt) as for extend_rule (bfcg_graph.hip)
template <class T>
__host__ __device__ __forceinline__ int link_rule(const T &tab, int k, uint64_t a, uint64_t b, int min_cnt, uint64_t &ya, uint64_t &yb)
{
	const int o = tab.present4(a, b, 0, min_cnt);
	if (o == 0) return 1;
	if (o & (o - 1)) return 2;
	succ_planes(k, a, b, __builtin_ctz(o), ya, yb);
	const int i = tab.present4(ya, yb, 1, min_cnt); // x is one of them
	if (i & (i - 1)) return 3;
	uint64_t ra, rb;
	rc_planes(k, a, b, ra, rb);
	if ((ya == a && yb == b) || (ya == ra && yb == rb)) return 6;
	return 0;
}
// the next base of a walk that link_rule allowed: the single present successor (0 if the table changed meanwhile)
template <class T> __host__ __device__ __forceinline__ int only_succ(const T &tab, uint64_t a, uint64_t b, int min_cnt)
{
	const int o = tab.present4(a, b, 0, min_cnt);
	return o ? __builtin_ctz(o) : 0;
}

// The unitig from the oriented k-mer (a, b), whose left side is open, for at most max_n k-mers: the stop code of its right end, which
// (a, b) then is, n its k-mers, sum their counts and (ya, yb) the single successor under codes 3 and 6; 0 if it is longer than max_n;
// -1 if a k-mer of the walk is not in the table
template <class T>
__host__ __device__ __forceinline__ int arm_walk(const T &tab, int k, int min_cnt, int max_n, uint64_t &a, uint64_t &b, uint64_t &ya, uint64_t &yb, int &n, uint64_t &sum)
{
	uint64_t slot = 0;
	int v = tab.value_at(a, b, slot), right;
	if (v < 0) return -1;
	n = 1; sum = (uint64_t)(v & 0xff);
	while ((right = link_rule(tab, k, a, b, min_cnt, ya, yb)) == 0) {
		if (n >= max_n) return 0; // too long
		if ((v = tab.value_at(ya, yb, slot)) < 0) return -1;
		sum += (uint64_t)(v & 0xff); ++n;
		a = ya; b = yb;
	}
	return right;
}

// ---- the listing's predicate: a node with an open side -----------------------------------------------------------------------------------
template <typename W> struct EndPred {
	static constexpr bool probes = true;
	using col_t = uint8_t;
	TabRef T; int min_cnt;
	__device__ __forceinline__ bool keep(uint32_t sub, uint64_t slot, uint8_t &o) const // o = left stop | right stop << 3 of the stored strand
	{
		DevGraph<W> g; g.T = T;
		uint64_t a, b, ra, rb, ya, yb;
		kdec::decode(T.k, T.l_pre, sub, slot, a, b);
		rc_planes(T.k, a, b, ra, rb);
		const int right = link_rule(g, T.k, a, b, min_cnt, ya, yb), left = link_rule(g, T.k, ra, rb, min_cnt, ya, yb);
		o = (uint8_t)(left | right << 3);
		return o != 0;
	}
};

// Start i of a listing with EndPred: side i & 1 of listed node i >> 1 (0: the stored strand x, its left side; 1: rc(x), whose left side is
// x's right).  code = that side's stop code; if r.starts(code), true and (a, b) = the oriented k-mer whose left side it is
template <class R>
__device__ __forceinline__ bool walk_start(int k, const ulonglong2 *__restrict__ node_y, const uint8_t *__restrict__ node_code, uint64_t i, const R &r, int &code, uint64_t &a, uint64_t &b)
{
	const int side = (int)(i & 1), both = node_code[i >> 1];
	code = side ? both >> 3 : both & 7;
	if (!r.starts(code)) return false;
	const uint64_t m = kdec::mask(k);
	const ulonglong2 x = node_y[i >> 1];
	a = x.x & m; b = x.y & m;
	if (side) rc_planes(k, x.x & m, x.y & m, a, b);
	return true;
}
struct OpenSide { __device__ __forceinline__ bool starts(int code) const { return code != 0; } }; // every open side starts: a linked one is where a path comes in

__device__ __forceinline__ void set_mark(uint32_t *mark, uint64_t slot) { atomicOr(&mark[slot >> 5], 1u << (slot & 31)); }

int check_unitig_k(const char *who, int k)
{
	if (k > (int)kdec::MAX_K) return check_decodable(k);
	if (k % 2 == 0) return bfcg::fail("%s: k=%d is even: the strand rule leaves some k-mers undecided, a k-mer and its reverse complement can be two keys, and there is no strand-free graph to compact (odd k <= %d only)", who, k, (int)kdec::MAX_K);
	return 0;
}

template <typename T> T *ut_buf(bfcg_kmers_t *t, int which) { return (T *)t->d_ut[which]; }
int ut_grow(bfcg_kmers_t *t, int which, uint64_t bytes, const char *what) { return bfcg::grow(t->d_ut[which], t->ut_bytes[which], bytes, what); }
// the time between the object's two events added to *ms; the stream is idle afterwards
int ut_lap(bfcg_kmers_t *t, float *ms)
{
	float d = 0;
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&d, t->e0, t->e1));
	*ms += d;
	return 0;
}

// ---- the host twins' set of nodes: the planes of a node's smaller strand -----------------------------------------------------------------
struct Planes { uint64_t a, b; bool operator==(const Planes &o) const { return a == o.a && b == o.b; } };
struct PlanesHash { size_t operator()(const Planes &p) const { return (size_t)kdec::mix(p.a ^ kdec::mix(p.b, ~0ULL), ~0ULL); } };

} // namespace
