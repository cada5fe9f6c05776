// bfcg_gprobe.h -- a k-mer of the graph view in registers and the probes of its neighbours, for the files that read the count table as a
// de Bruijn graph: bfcg_graph.hip (neighbours, census, listing by degree, extension), bfcg_unitigs.hip (the compacted graph) and
// bfcg_clip.hip and bfcg_pop.hip (the graph cleaned), the last three through bfcg_glink.h.
//
// A k-mer is the two planes a listing hands out (bit l = the base l from the 3' end); succ(x, c) shifts both planes left and puts base c
// at the 3' end, pred(x, c) shifts them right and puts c at the 5' end.  The VALUE of a k-mer is what bfcg_kmers_lookup answers for it, on
// the strand as constructed.  A kernel holds a k-mer as k_lookup does, as the two windows of its strand (oldest base at bit 0): a
// neighbour's windows are the k-mer's shifted by one with one bit pair replaced, so the bit reversal is done once per k-mer and the
// eight hashes start from there (kmer_hash_windows, kmer_dev.h).  All home slots of a group of probes are loaded before the first is
// looked at.  DevGraph answers for planes on the device what HostGraph answers on the host from bfcg_kmer_occ_host: the rules that walk
// the graph (extend_rule, link_rule, arm_walk, the cleaning rules' decide) are templates over the two.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "kmer_dev.h"
#include "bfcg_kdec.h"

namespace {

struct TabRef { const unsigned long long *tab; int k, l_pre, cshift; };

__host__ __device__ __forceinline__ bool present(int v, int min_cnt) { return v >= 0 && (v & 0xff) >= min_cnt; }

// ---- a k-mer as windows, its neighbours, the probes -------------------------------------------------------------------------------
template <typename W> struct Win { W lo, hi; }; // low / high code bit, the base at the 5' end in bit 0; bits at and above k are 0

template <typename W> __device__ __forceinline__ Win<W> win_of_planes(int k, uint64_t a, uint64_t b) // bits of the planes at and above k fall out
{
	constexpr int nb = 8 * (int)sizeof(W);
	Win<W> w;
	w.lo = bfcg::brev_w((W)a) >> (nb - k); w.hi = bfcg::brev_w((W)b) >> (nb - k);
	return w;
}
template <typename W> __device__ __forceinline__ Win<W> win_succ(int k, const Win<W> w, int c) // the 5' base falls out, c is the new 3' base
{
	Win<W> r;
	r.lo = (w.lo >> 1) | (W)(c & 1) << (k - 1); r.hi = (w.hi >> 1) | (W)(c >> 1) << (k - 1);
	return r;
}
template <typename W> __device__ __forceinline__ Win<W> win_pred(int k, const Win<W> w, int c) // the 3' base falls out, c is the new 5' base
{
	const W m = bfcg::kmask<W>(k);
	Win<W> r;
	r.lo = ((w.lo << 1) & m) | (W)(c & 1); r.hi = ((w.hi << 1) & m) | (W)(c >> 1);
	return r;
}

// ch_get_dev (kmer_dev.h) in two halves: the hash, the home slot and its load; then the rest of the chain.  A caller starts all its
// probes before it finishes the first.
struct Probe { const unsigned long long *reg; uint64_t key; uint32_t pos, cmask; unsigned long long cur; };

template <typename W> __device__ __forceinline__ Probe probe_first(const TabRef &T, const Win<W> w)
{
	uint64_t y0, y1, key;
	bfcg::kmer_hash_windows<W>(T.k, w.lo, w.hi, y0, y1);
	const uint32_t sub = bfcg::ch_subkey(T.k, T.l_pre, y0, y1, key);
	Probe p;
	p.key = key >> 14; p.cmask = (1u << T.cshift) - 1;
	p.reg = T.tab + ((uint64_t)sub << T.cshift);
	p.pos = (uint32_t)p.key & p.cmask;
	p.cur = p.reg[p.pos];
	return p;
}
// -1, or high << 8 | count: it ends at the key, at an empty slot, or after a whole region.  *at (may be NULL) = the slot where the key lies
__device__ __forceinline__ int probe_rest(Probe p, const unsigned long long **at = NULL)
{
	for (uint32_t probe = 0;;) {
		if (p.cur == 0) return -1;
		if ((p.cur >> 14) == p.key) { if (at) *at = p.reg + p.pos; return (int)(p.cur & 0x3fff); }
		if (++probe > p.cmask) return -1;
		p.pos = (p.pos + 1) & p.cmask;
		p.cur = p.reg[p.pos];
	}
}

// v[c] = the value of succ(x, c), v[4 + c] = that of pred(x, c)
template <typename W> __device__ __forceinline__ void values8(const TabRef &T, const Win<W> w, int v[8])
{
	Probe p[8];
#pragma unroll
	for (int c = 0; c < 4; ++c) { p[c] = probe_first<W>(T, win_succ<W>(T.k, w, c)); p[4 + c] = probe_first<W>(T, win_pred<W>(T.k, w, c)); }
#pragma unroll
	for (int j = 0; j < 8; ++j) v[j] = probe_rest(p[j]);
}
// bit c: succ(x, c) is present at min_cnt (pred = 0), or pred(x, c) (pred = 1)
template <typename W> __device__ __forceinline__ int present4(const TabRef &T, const Win<W> w, int pred, int min_cnt)
{
	Probe p[4];
#pragma unroll
	for (int c = 0; c < 4; ++c) p[c] = probe_first<W>(T, pred ? win_pred<W>(T.k, w, c) : win_succ<W>(T.k, w, c));
	int r = 0;
#pragma unroll
	for (int c = 0; c < 4; ++c) r |= (int)present(probe_rest(p[c]), min_cnt) << c;
	return r;
}
// the neighbour bits of the k-mer in `slot` of sub-table `sub`: bit c succ by c present, bit 4 + c pred by c present
template <typename W> __device__ __forceinline__ uint32_t node_nb(const TabRef &T, uint32_t sub, uint64_t slot, int min_cnt)
{
	uint64_t a, b;
	kdec::decode(T.k, T.l_pre, sub, slot, a, b);
	int v[8];
	values8<W>(T, win_of_planes<W>(T.k, a, b), v);
	uint32_t nb = 0;
#pragma unroll
	for (int j = 0; j < 8; ++j) nb |= (uint32_t)present(v[j], min_cnt) << j;
	return nb;
}

// the table asked by planes, on the device ...
template <typename W> struct DevGraph {
	TabRef T;
	__device__ __forceinline__ bool present(uint64_t a, uint64_t b, int min_cnt) const
	{
		return ::present(probe_rest(probe_first<W>(T, win_of_planes<W>(T.k, a, b))), min_cnt);
	}
	__device__ __forceinline__ int present4(uint64_t a, uint64_t b, int pred, int min_cnt) const { return ::present4<W>(T, win_of_planes<W>(T.k, a, b), pred, min_cnt); }
	// the value of a k-mer and the index of its slot in the table (untouched if it is absent)
	__device__ __forceinline__ int value_at(uint64_t a, uint64_t b, uint64_t &slot) const
	{
		const unsigned long long *at = NULL;
		const int v = probe_rest(probe_first<W>(T, win_of_planes<W>(T.k, a, b)), &at);
		if (at) slot = (uint64_t)(at - T.tab);
		return v;
	}
};

// ... and on the host, without a GPU
struct HostGraph {
	const bfc_ch_t *ch; int k;
	int value(uint64_t a, uint64_t b) const
	{
		const uint64_t y[2] = { a, b };
		return bfcg_kmer_occ_host(ch, y);
	}
	bool present(uint64_t a, uint64_t b, int min_cnt) const { return ::present(value(a, b), min_cnt); }
	int value_at(uint64_t a, uint64_t b, uint64_t &) const { return value(a, b); } // DevGraph's, for a rule that needs no slot
	int value(uint64_t a, uint64_t b, int pred, int c) const // of succ or pred by c
	{
		const uint64_t m = kdec::mask(k);
		a &= m; b &= m;
		return value(pred ? a >> 1 | (uint64_t)(c & 1) << (k - 1) : (a << 1 | (uint64_t)(c & 1)) & m,
		             pred ? b >> 1 | (uint64_t)(c >> 1) << (k - 1) : (b << 1 | (uint64_t)(c >> 1)) & m);
	}
	int present4(uint64_t a, uint64_t b, int pred, int min_cnt) const
	{
		int r = 0;
		for (int c = 0; c < 4; ++c) r |= (int)::present(value(a, b, pred, c), min_cnt) << c;
		return r;
	}
};

// every slot of bfc_ch_export_sorted, in its order: fn(i, slot, a, b) with the slot's planes.  The number of slots, or -1 with the message set
template <class F> int64_t each_slot_host(const bfc_ch_t *ch, const F &fn)
{
	const int k = bfc_ch_get_k(ch), l_pre = bfc_ch_get_lpre(ch);
	const uint64_t n = bfc_ch_export_sorted(ch, NULL, NULL);
	uint32_t *sizes = (uint32_t *)malloc(4ULL << l_pre);
	uint64_t *slots = (uint64_t *)malloc(n ? n * 8 : 8);
	if (!sizes || !slots) { free(sizes); free(slots); return bfcg::fail("out of host memory"); }
	bfc_ch_export_sorted(ch, sizes, slots);
	uint64_t i = 0;
	for (uint64_t s = 0; s < 1ULL << l_pre; ++s)
		for (uint32_t j = 0; j < sizes[s]; ++j, ++i) {
			uint64_t a, b;
			kdec::decode(k, l_pre, (uint32_t)s, slots[i], a, b);
			fn(i, slots[i], a, b);
		}
	free(sizes); free(slots);
	return (int64_t)n;
}

TabRef tab_ref(const bfcg_kmers_t *t)
{
	TabRef T;
	T.tab = t->table; T.k = t->k; T.l_pre = t->l_pre; T.cshift = t->cshift;
	return T;
}

int check_min_cnt(const char *who, int min_cnt)
{
	if (min_cnt < 1 || min_cnt > 255) return bfcg::fail("%s: min_cnt %d is outside [1, 255]: a count is 8 bits, and a key the table holds was counted at least once", who, min_cnt);
	return 0;
}
int check_decodable(int k)
{
	if (!kdec::decodable(k)) return bfcg::fail("k-mers cannot be listed for k=%d: the table's key is lossless only for k <= %d (sizes and histogram work for any k)", k, (int)kdec::MAX_K);
	return 0;
}

} // namespace
