// bfcg_graph.hip -- the count table read as a de Bruijn graph where it lies in HBM: which of a k-mer's eight neighbours the table holds, the
// degree census of all its k-mers, the k-mers of chosen degree cells, the unambiguous path from a seed.  DESIGN.md section 6d.
//
// The k-mer in registers, the probes of its neighbours and the table asked by planes on the device and on the host are bfcg_gprobe.h's,
// shared with bfcg_unitigs.hip (the compacted graph).
//   k_neighbors    one k-mer per lane, eight values out as one 16-byte store (every k: only the forward hash is needed)
//   k_graph_census  k_tab_hist's walk (a wave on a contiguous span, 16 bytes per lane); a slot that is a node is decoded (bfcg_kdec.h,
//                   k <= 37), its neighbours probed, cell 5 o + i counted in the wave's 25 LDS bins; a workgroup flushes its non-zero
//                   bins with one 64-bit atomic each
//   k_tab_list      bfcg_klist.h with GraphPred: the eight probes are the predicate of both passes, the neighbour bits the third column
//   k_extend        one seed per lane, walked while exactly one successor is present and that one has no second predecessor
//                   (extend_rule, written once for this kernel and bfcg_extend_host)
// The host twins at the end of the file use no GPU: bfcg_kmer_occ_host per neighbour, bfc_ch_export_sorted and the decode's host instance.
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

namespace {

enum { NB_BT = 256, NB_GRID_MAX = 256 * 8 /* eight workgroups on each of the 256 CUs */ };
enum { CENSUS_UNROLL = 2, CENSUS_CELLS = 25, CENSUS_ROW = 32 /* a wave's bins, padded */, CENSUS_GRID_MAX = 1024 }; // BT, WAVES, lane_id: bfcg_klist.h
enum { EXT_BT = 64 /* a lane walks a seed: short workgroups spread few seeds over many CUs */, EXT_MAX_LEN = 65535 };

__host__ __device__ __forceinline__ int cell_of(uint32_t nb) { return 5 * __builtin_popcount(nb & 15) + __builtin_popcount(nb >> 4); }

// ---- k_neighbors ------------------------------------------------------------------------------------------------------------------
template <typename W>
__global__ __launch_bounds__(NB_BT) void k_neighbors(TabRef T, const ulonglong2 *__restrict__ y, uint64_t n, uint4 *__restrict__ out)
{
	for (uint64_t i = (uint64_t)blockIdx.x * NB_BT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * NB_BT) {
		const ulonglong2 x = y[i];
		int v[8];
		values8<W>(T, win_of_planes<W>(T.k, x.x, x.y), v);
		out[i] = make_uint4((uint32_t)(uint16_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)(uint16_t)v[2] | (uint32_t)v[3] << 16,
		                    (uint32_t)(uint16_t)v[4] | (uint32_t)v[5] << 16, (uint32_t)(uint16_t)v[6] | (uint32_t)v[7] << 16);
	}
}

// ---- k_graph_census ---------------------------------------------------------------------------------------------------------------
// slot s of the table lies in sub-table s >> cshift; the spans are k_tab_hist's (bfcg_kmers.hip)
template <typename W>
__global__ __launch_bounds__(BT) void k_graph_census(const ulonglong2 *__restrict__ tab, uint64_t n_pairs, uint64_t span_pairs, TabRef T, int min_cnt,
                                                     unsigned long long *__restrict__ deg)
{
	__shared__ uint32_t h[WAVES][CENSUS_ROW];
	if (threadIdx.x < WAVES * CENSUS_ROW) (&h[0][0])[threadIdx.x] = 0;
	__syncthreads();
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	const uint64_t gw = (uint64_t)blockIdx.x * WAVES + wave;
	const uint64_t p_lo = gw * span_pairs, p_hi = p_lo + span_pairs < n_pairs ? p_lo + span_pairs : n_pairs;
	for (uint64_t p = p_lo; p < p_hi; p += 64 * CENSUS_UNROLL) {
		ulonglong2 v[CENSUS_UNROLL];
#pragma unroll
		for (int j = 0; j < CENSUS_UNROLL; ++j) {
			const uint64_t q = p + (uint64_t)j * 64 + lane;
			v[j] = q < p_hi ? tab[q] : make_ulonglong2(0, 0);
		}
#pragma unroll
		for (int j = 0; j < CENSUS_UNROLL; ++j) {
			const uint64_t q = p + (uint64_t)j * 64 + lane;
			if ((int)(v[j].x & 0xff) >= min_cnt) atomicAdd(&h[wave][cell_of(node_nb<W>(T, (uint32_t)((2 * q) >> T.cshift), v[j].x, min_cnt))], 1u); // (an empty slot has count 0 < min_cnt)
			if ((int)(v[j].y & 0xff) >= min_cnt) atomicAdd(&h[wave][cell_of(node_nb<W>(T, (uint32_t)((2 * q + 1) >> T.cshift), v[j].y, min_cnt))], 1u);
		}
	}
	__syncthreads();
	if (threadIdx.x < CENSUS_CELLS) {
		unsigned long long s = 0;
		for (int w = 0; w < WAVES; ++w) s += h[w][threadIdx.x];
		if (s) atomicAdd(&deg[threadIdx.x], s);
	}
}

// ---- the listing's predicate ------------------------------------------------------------------------------------------------------
template <typename W> struct GraphPred {
	static constexpr bool probes = true;
	using col_t = uint8_t;
	TabRef T; int min_cnt; uint32_t cell_mask;
	__device__ __forceinline__ bool keep(uint32_t sub, uint64_t slot, uint8_t &o) const
	{
		const uint32_t nb = node_nb<W>(T, sub, slot, min_cnt);
		o = (uint8_t)nb;
		return cell_mask >> cell_of(nb) & 1;
	}
};

// ---- the walk from a seed, for the device and the host ------------------------------------------------------------------------------
// `tab` answers present(a, b, min_cnt) for a k-mer's planes and present4(a, b, pred, min_cnt) for its four successors or predecessors.
// bases[0, max_len) is zero when the walk starts.  include/bfc_gpu.h states the rule.
template <class T>
__host__ __device__ __forceinline__ void extend_rule(const T &tab, int k, uint64_t a, uint64_t b, int min_cnt, int max_len, uint8_t *bases, int32_t *len_stop)
{
	const uint64_t m = kdec::mask(k), sa = a & m, sb = b & m;
	int len = 0, stop;
	a = sa; b = sb;
	if (!tab.present(a, b, min_cnt)) stop = 4;
	else for (;;) {
		if (len == max_len) { stop = 0; break; }
		const int o = tab.present4(a, b, 0, min_cnt);
		if (o == 0) { stop = 1; break; }
		if (o & (o - 1)) { stop = 2; break; }
		const int c = __builtin_ctz(o);
		const uint64_t na = (a << 1 | (uint64_t)(c & 1)) & m, nb = (b << 1 | (uint64_t)(c >> 1)) & m;
		const int i = tab.present4(na, nb, 1, min_cnt); // the current k-mer is one of them
		if (i & (i - 1)) { stop = 3; break; }
		if (na == sa && nb == sb) { stop = 5; break; }
		bases[len++] = (uint8_t)"ACGT"[c];
		a = na; b = nb;
	}
	len_stop[0] = len; len_stop[1] = stop;
}

template <typename W>
__global__ __launch_bounds__(EXT_BT) void k_extend(TabRef T, const ulonglong2 *__restrict__ y, uint64_t n, int min_cnt, int max_len, uint8_t *__restrict__ bases,
                                                   int32_t *__restrict__ len_stop)
{
	const uint64_t i = (uint64_t)blockIdx.x * EXT_BT + threadIdx.x;
	if (i >= n) return;
	DevGraph<W> g; g.T = T;
	const ulonglong2 x = y[i];
	extend_rule(g, T.k, x.x, x.y, min_cnt, max_len, bases + i * (uint64_t)max_len, len_stop + 2 * i);
}

int check_cell_mask(const char *who, uint32_t cell_mask)
{
	if (cell_mask == 0 || cell_mask >> CENSUS_CELLS) return bfcg::fail("%s: cell_mask 0x%x names no cell or one beyond bit 24 (bit 5 o + i: o successors, i predecessors)", who, cell_mask);
	return 0;
}
int check_max_len(const char *who, int max_len)
{
	if (max_len < 1 || max_len > EXT_MAX_LEN) return bfcg::fail("%s: max_len %d is outside [1, %d]", who, max_len, (int)EXT_MAX_LEN);
	return 0;
}

} // namespace

extern "C" int bfcg_kmers_neighbors(bfcg_kmers_t *t, const uint64_t *y, uint64_t n, int16_t *out)
{
	if (!t || (n && (!y || !out))) return bfcg::fail("bad arguments to bfcg_kmers_neighbors");
	t->last_ms = 0;
	if (n == 0) return 0;
	BFCG_CK(hipSetDevice(t->device));
	if (bfcg::lookup_stage(t) != 0) return -1;
	if (bfcg::grow(t->d_gout, t->gout_cap, t->q_cap * 16, "the neighbours' values") != 0) return -1;
	const TabRef T = tab_ref(t);
	float total = 0;
	for (uint64_t done = 0; done < n; ) {
		const uint64_t m = n - done < t->q_cap ? n - done : t->q_cap;
		uint64_t grid = (m + NB_BT - 1) / NB_BT;
		if (grid > NB_GRID_MAX) grid = NB_GRID_MAX;
		float ms = 0;
		BFCG_CK(hipMemcpyAsync(t->d_qy, y + 2 * done, m * 16, hipMemcpyHostToDevice, t->st));
		BFCG_CK(hipEventRecord(t->e0, t->st));
		if (t->k <= 32) hipLaunchKernelGGL((k_neighbors<uint32_t>), dim3((unsigned)grid), dim3(NB_BT), 0, t->st, T, t->d_qy, m, (uint4 *)t->d_gout);
		else hipLaunchKernelGGL((k_neighbors<uint64_t>), dim3((unsigned)grid), dim3(NB_BT), 0, t->st, T, t->d_qy, m, (uint4 *)t->d_gout);
		BFCG_CK(hipEventRecord(t->e1, t->st));
		BFCG_CK(hipGetLastError());
		BFCG_CK(hipMemcpyAsync(out + 8 * done, t->d_gout, m * 16, hipMemcpyDeviceToHost, t->st));
		BFCG_CK(hipStreamSynchronize(t->st));
		BFCG_CK(hipEventElapsedTime(&ms, t->e0, t->e1));
		total += ms;
		done += m;
	}
	t->last_ms = total;
	return 0;
}

extern "C" int bfcg_kmers_graph_census(bfcg_kmers_t *t, int min_cnt, uint64_t deg[25])
{
	if (!t || !deg) return bfcg::fail("bad arguments to bfcg_kmers_graph_census");
	if (check_min_cnt("bfcg_kmers_graph_census", min_cnt) != 0 || check_decodable(t->k) != 0) return -1;
	t->last_ms = 0;
	BFCG_CK(hipSetDevice(t->device));
	const uint64_t n_pairs = 1ULL << (t->l_pre + t->cshift - 1), step = 64 * CENSUS_UNROLL;
	uint64_t grid = (n_pairs + step * WAVES - 1) / (step * WAVES);
	if (grid > CENSUS_GRID_MAX) grid = CENSUS_GRID_MAX; // four workgroups on each of the 256 CUs
	const uint64_t waves = grid * WAVES, span = ((n_pairs + waves - 1) / waves + step - 1) / step * step;
	const TabRef T = tab_ref(t);
	uint64_t h[CENSUS_CELLS];
	BFCG_CK(hipMemsetAsync(t->d_hist, 0, CENSUS_CELLS * 8, t->st));
	BFCG_CK(hipEventRecord(t->e0, t->st));
	if (t->k <= 32) hipLaunchKernelGGL((k_graph_census<uint32_t>), dim3((unsigned)grid), dim3(BT), 0, t->st, (const ulonglong2 *)t->table, n_pairs, span, T, min_cnt, t->d_hist);
	else hipLaunchKernelGGL((k_graph_census<uint64_t>), dim3((unsigned)grid), dim3(BT), 0, t->st, (const ulonglong2 *)t->table, n_pairs, span, T, min_cnt, t->d_hist);
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(h, t->d_hist, sizeof(h), hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&t->last_ms, t->e0, t->e1));
	memcpy(deg, h, sizeof(h));
	return 0;
}

extern "C" int bfcg_kmers_list_graph(bfcg_kmers_t *t, int min_cnt, uint32_t cell_mask, uint32_t sub_lo, uint32_t sub_hi, uint64_t *y, uint16_t *cnt_high, uint8_t *nb,
                                     uint64_t cap, uint64_t *n)
{
	if (!t || !n) return bfcg::fail("bad arguments to bfcg_kmers_list_graph");
	if (check_min_cnt("bfcg_kmers_list_graph", min_cnt) != 0 || check_cell_mask("bfcg_kmers_list_graph", cell_mask) != 0) return -1;
	// (-64: every slot passes hash2cnt's -d)
	if (t->k <= 32) {
		GraphPred<uint32_t> P; P.T = tab_ref(t); P.min_cnt = min_cnt; P.cell_mask = cell_mask;
		return list_run(t, "bfcg_kmers_list_graph", P, min_cnt, -64, sub_lo, sub_hi, y, cnt_high, nb, cap, n);
	}
	GraphPred<uint64_t> P; P.T = tab_ref(t); P.min_cnt = min_cnt; P.cell_mask = cell_mask;
	return list_run(t, "bfcg_kmers_list_graph", P, min_cnt, -64, sub_lo, sub_hi, y, cnt_high, nb, cap, n);
}

extern "C" int bfcg_kmers_extend(bfcg_kmers_t *t, const uint64_t *y, uint64_t n, int min_cnt, int max_len, uint8_t *bases, int32_t *len_stop)
{
	if (!t || (n && (!y || !bases || !len_stop))) return bfcg::fail("bad arguments to bfcg_kmers_extend");
	if (check_min_cnt("bfcg_kmers_extend", min_cnt) != 0 || check_max_len("bfcg_kmers_extend", max_len) != 0) return -1;
	t->last_ms = 0;
	if (n == 0) return 0;
	BFCG_CK(hipSetDevice(t->device));
	if (bfcg::lookup_stage(t) != 0) return -1;
	// the staging room of the paths is that of the neighbours' values, 16 bytes per staged k-mer, and one path at least
	const uint64_t room = t->q_cap * 16 > (uint64_t)max_len ? t->q_cap * 16 : (uint64_t)max_len;
	uint64_t per = room / (uint64_t)max_len;
	if (per > t->q_cap) per = t->q_cap;
	if (bfcg::grow(t->d_gout, t->gout_cap, room, "the paths of an extension") != 0) return -1;
	if (bfcg::grow(t->d_gls, t->gls_cap, per * 8, "the lengths of an extension") != 0) return -1;
	const TabRef T = tab_ref(t);
	float total = 0;
	for (uint64_t done = 0; done < n; ) {
		const uint64_t m = n - done < per ? n - done : per;
		float ms = 0;
		BFCG_CK(hipMemcpyAsync(t->d_qy, y + 2 * done, m * 16, hipMemcpyHostToDevice, t->st));
		BFCG_CK(hipMemsetAsync(t->d_gout, 0, m * (uint64_t)max_len, t->st));
		BFCG_CK(hipEventRecord(t->e0, t->st));
		const unsigned grid = (unsigned)((m + EXT_BT - 1) / EXT_BT);
		if (t->k <= 32) hipLaunchKernelGGL((k_extend<uint32_t>), dim3(grid), dim3(EXT_BT), 0, t->st, T, t->d_qy, m, min_cnt, max_len, t->d_gout, t->d_gls);
		else hipLaunchKernelGGL((k_extend<uint64_t>), dim3(grid), dim3(EXT_BT), 0, t->st, T, t->d_qy, m, min_cnt, max_len, t->d_gout, t->d_gls);
		BFCG_CK(hipEventRecord(t->e1, t->st));
		BFCG_CK(hipGetLastError());
		BFCG_CK(hipMemcpyAsync(bases + done * (uint64_t)max_len, t->d_gout, m * (uint64_t)max_len, hipMemcpyDeviceToHost, t->st));
		BFCG_CK(hipMemcpyAsync(len_stop + 2 * done, t->d_gls, m * 8, hipMemcpyDeviceToHost, t->st));
		BFCG_CK(hipStreamSynchronize(t->st));
		BFCG_CK(hipEventElapsedTime(&ms, t->e0, t->e1));
		total += ms;
		done += m;
	}
	t->last_ms = total;
	return 0;
}

// ---- the host twins: no GPU ---------------------------------------------------------------------------------------------------------

extern "C" int bfcg_kmer_revcomp(int k, const uint64_t y_in[2], uint64_t y_out[2])
{
	if (k < 1 || k > 63 || !y_in || !y_out) return -1;
	uint64_t a = 0, b = 0;
	for (int l = 0; l < k; ++l) { // the base l from the 3' end becomes the complement at k - 1 - l
		a |= (~y_in[0] >> l & 1) << (k - 1 - l);
		b |= (~y_in[1] >> l & 1) << (k - 1 - l);
	}
	y_out[0] = a; y_out[1] = b;
	return 0;
}

extern "C" int bfcg_neighbors_host(const bfc_ch_t *ch, const uint64_t *y, uint64_t n, int16_t *out)
{
	if (!ch || (n && (!y || !out))) return bfcg::fail("bad arguments to bfcg_neighbors_host");
	HostGraph g; g.ch = ch; g.k = bfc_ch_get_k(ch);
	for (uint64_t i = 0; i < n; ++i)
		for (int c = 0; c < 4; ++c) {
			out[8 * i + c] = (int16_t)g.value(y[2 * i], y[2 * i + 1], 0, c);
			out[8 * i + 4 + c] = (int16_t)g.value(y[2 * i], y[2 * i + 1], 1, c);
		}
	return 0;
}

extern "C" int64_t bfcg_graph_nb_host(const bfc_ch_t *ch, int min_cnt, uint64_t *y, uint8_t *nb)
{
	if (!ch) return bfcg::fail("bad arguments to bfcg_graph_nb_host");
	if (check_min_cnt("bfcg_graph_nb_host", min_cnt) != 0 || check_decodable(bfc_ch_get_k(ch)) != 0) return -1;
	if (!y && !nb) return (int64_t)bfc_ch_export_sorted(ch, NULL, NULL);
	HostGraph g; g.ch = ch; g.k = bfc_ch_get_k(ch);
	return each_slot_host(ch, [&](uint64_t i, uint64_t slot, uint64_t a, uint64_t b) {
		if (y) { y[2 * i] = a; y[2 * i + 1] = b; }
		if (nb) nb[i] = (int)(slot & 0xff) >= min_cnt ? (uint8_t)(g.present4(a, b, 0, min_cnt) | g.present4(a, b, 1, min_cnt) << 4) : 0;
	});
}

extern "C" int bfcg_graph_census_host(const bfc_ch_t *ch, int min_cnt, uint64_t deg[25])
{
	if (!ch || !deg) return bfcg::fail("bad arguments to bfcg_graph_census_host");
	if (check_min_cnt("bfcg_graph_census_host", min_cnt) != 0 || check_decodable(bfc_ch_get_k(ch)) != 0) return -1;
	HostGraph g; g.ch = ch; g.k = bfc_ch_get_k(ch);
	uint64_t h[CENSUS_CELLS] = { 0 };
	if (each_slot_host(ch, [&](uint64_t, uint64_t slot, uint64_t a, uint64_t b) {
		if ((int)(slot & 0xff) >= min_cnt) ++h[cell_of((uint32_t)(g.present4(a, b, 0, min_cnt) | g.present4(a, b, 1, min_cnt) << 4))];
	}) < 0) return -1;
	memcpy(deg, h, sizeof(h));
	return 0;
}

extern "C" int bfcg_extend_host(const bfc_ch_t *ch, const uint64_t *y, uint64_t n, int min_cnt, int max_len, uint8_t *bases, int32_t *len_stop)
{
	if (!ch || (n && (!y || !bases || !len_stop))) return bfcg::fail("bad arguments to bfcg_extend_host");
	if (check_min_cnt("bfcg_extend_host", min_cnt) != 0 || check_max_len("bfcg_extend_host", max_len) != 0) return -1;
	HostGraph g; g.ch = ch; g.k = bfc_ch_get_k(ch);
	if (n) memset(bases, 0, n * (uint64_t)max_len);
	for (uint64_t i = 0; i < n; ++i) extend_rule(g, g.k, y[2 * i], y[2 * i + 1], min_cnt, max_len, bases + i * (uint64_t)max_len, len_stop + 2 * i);
	return 0;
}
