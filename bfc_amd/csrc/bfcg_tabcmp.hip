// bfcg_tabcmp.hip -- two count tables compared and merged where they lie in HBM: the joint spectrum, one table listed against the other,
// the union.  DESIGN.md section 6d.
//
// Two tables of equal k and l_pre share the sub-table index and the 50-bit key: slot i of table A belongs to sub-table i >> cshift_A, its
// key is v >> 14, and its partner in B, if any, lies in B's region sub << cshift_B on the probe chain from (v >> 14) & cmask_B.  Neither a
// hash nor a decode is needed, so everything but the listing's planes works for every k up to 63, the lossy keys of k >= 38 included.
// Both tables are walked in ascending sub-table order: the join is two sequential streams.
//   k_tab_join    k_tab_hist's walk (a wave on a contiguous span, 16 bytes per lane) over one table, every non-empty slot probing the
//                 other; the 128 x 128 low corner of the 256 x 256 bins in LDS, the rest by 64-bit atomics in HBM.  Launched twice: A
//                 against B fills the rows i >= 1, B against A counts only B's private keys, row 0.  A workgroup stores its corner as
//                 a slice of its own and k_join_sum adds the slices up: a joint spectrum is a ridge of a few dozen cache lines, and
//                 a thousand workgroups flushing into those with atomics took longer than the walk (profiles/kmers_rate.md)
//   k_tab_list    bfcg_klist.h with VsOther: the probe of B is part of the predicate of both passes, its answer the third column
//   k_tab_union   a lane per pair of source slots, inserted into the output's region from home (v >> 14) & cmask_U by table_upsert's
//                 protocol (bfcg_kernels.hip) written on (sub, key): union_upsert, bfcg_upsert.h; the output's geometry is fixed from the inputs' sub-table sizes
//                 before the launch, so a region cannot overflow and there is no retry
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"
#include "bfcg_klist.h"
#include "bfcg_upsert.h"

namespace {

enum { JOIN_LOW = 128 /* counts below it are binned in LDS: 64 KiB */, JOIN_CELLS = JOIN_LOW * JOIN_LOW, JOIN_BT = 1024, JOIN_WAVES = JOIN_BT / 64, JOIN_UNROLL = 4 };
enum { JOIN_GRID_MAX = 512 /* two workgroups of sixteen waves on each of the 256 CUs */, JOIN_SUM_BT = 256, JOIN_SUM_Y = 8 };
enum { JOINT_BINS = 256 * 256, CTR_KEYS = JOINT_BINS, CTR_FULL = JOINT_BINS + 1, JOINT_WORDS = JOINT_BINS + 2 };
enum { UNION_GRID_MAX = 256 * 8 };

// ch_get_dev's loop (kmer_dev.h) on (sub, key): -1, or high << 8 | count.  It ends at the key, at an empty slot, or after a whole region.
__device__ __forceinline__ int probe_sub(const unsigned long long *__restrict__ tab, int cshift, uint32_t sub, uint64_t key)
{
	const uint64_t cmask = (1ULL << cshift) - 1;
	const unsigned long long *reg = tab + ((uint64_t)sub << cshift);
	uint64_t pos = key & cmask;
	for (uint64_t probe = 0; probe <= cmask; ++probe, pos = (pos + 1) & cmask) {
		const unsigned long long cur = reg[pos];
		if (cur == 0) return -1;
		if ((cur >> 14) == key) return (int)(cur & 0x3fff);
	}
	return -1;
}

// ---- k_tab_join -----------------------------------------------------------------------------------------------------------------
// The walked table `w` (spans as in k_tab_hist), the probed table `p`.  rows == 1: w is A, bin (count in w, count in p or 0).
// rows == 0: w is B, only the keys p does not hold are counted, bin (0, count in w).
__device__ __forceinline__ void join_bin(uint32_t *__restrict__ low, unsigned long long *__restrict__ joint, uint32_t ca, uint32_t cb)
{
	if (ca < JOIN_LOW && cb < JOIN_LOW) atomicAdd(&low[ca * JOIN_LOW + cb], 1u);
	else atomicAdd(&joint[ca * 256 + cb], 1ULL);
}

__device__ __forceinline__ void join_slot(uint64_t v, uint64_t slot, int cshift_w, const unsigned long long *__restrict__ p, int cshift_p, int rows,
                                          uint32_t *__restrict__ low, unsigned long long *__restrict__ joint)
{
	if (!v) return;
	const int r = probe_sub(p, cshift_p, (uint32_t)(slot >> cshift_w), v >> 14);
	if (rows) join_bin(low, joint, (uint32_t)(v & 0xff), r < 0 ? 0u : (uint32_t)(r & 0xff));
	else if (r < 0) join_bin(low, joint, 0u, (uint32_t)(v & 0xff));
}

__global__ __launch_bounds__(JOIN_BT) void k_tab_join(const ulonglong2 *__restrict__ w, uint64_t n_pairs, uint64_t span_pairs, int cshift_w,
                                                      const unsigned long long *__restrict__ p, int cshift_p, int rows, unsigned long long *__restrict__ joint,
                                                      uint32_t *__restrict__ part)
{
	__shared__ uint32_t low[JOIN_CELLS];
	for (int i = threadIdx.x; i < JOIN_CELLS; i += JOIN_BT) low[i] = 0;
	__syncthreads();
	const int lane = lane_id(), wave = threadIdx.x >> 6;
	const uint64_t gw = (uint64_t)blockIdx.x * JOIN_WAVES + wave;
	const uint64_t p_lo = gw * span_pairs, p_hi = p_lo + span_pairs < n_pairs ? p_lo + span_pairs : n_pairs;
	for (uint64_t q0 = p_lo; q0 < p_hi; q0 += 64 * JOIN_UNROLL) {
		ulonglong2 v[JOIN_UNROLL];
#pragma unroll
		for (int j = 0; j < JOIN_UNROLL; ++j) {
			const uint64_t q = q0 + (uint64_t)j * 64 + lane;
			v[j] = q < p_hi ? w[q] : make_ulonglong2(0, 0);
		}
#pragma unroll
		for (int j = 0; j < JOIN_UNROLL; ++j) {
			const uint64_t q = q0 + (uint64_t)j * 64 + lane;
			join_slot(v[j].x, 2 * q, cshift_w, p, cshift_p, rows, low, joint);      // with cshift_w == 0 the two slots of a pair
			join_slot(v[j].y, 2 * q + 1, cshift_w, p, cshift_p, rows, low, joint);  // belong to different sub-tables
		}
	}
	__syncthreads();
	part += (uint64_t)blockIdx.x * JOIN_CELLS; // this workgroup's slice
	for (int b = threadIdx.x; b < JOIN_CELLS; b += JOIN_BT) part[b] = low[b];
}

// the slices of both launches added up: a thread per cell of the corner, blockIdx.y a share of the slices
__global__ __launch_bounds__(JOIN_SUM_BT) void k_join_sum(const uint32_t *__restrict__ part, uint32_t n_part, unsigned long long *__restrict__ joint)
{
	const uint32_t b = blockIdx.x * JOIN_SUM_BT + threadIdx.x; // < JOIN_CELLS: the grid is exact
	unsigned long long s = 0;
	for (uint32_t i = blockIdx.y; i < n_part; i += gridDim.y) s += part[(uint64_t)i * JOIN_CELLS + b];
	if (s) atomicAdd(&joint[(b / JOIN_LOW) * 256 + b % JOIN_LOW], s);
}

// ---- the listing's predicate ------------------------------------------------------------------------------------------------------
struct VsOther {
	static constexpr bool probes = true;
	using col_t = int16_t;
	const unsigned long long *tab; int cshift, lo, hi;
	__device__ __forceinline__ bool keep(uint32_t sub, uint64_t slot, int16_t &o) const
	{
		const int r = probe_sub(tab, cshift, sub, slot >> 14), c = r < 0 ? 0 : r & 0xff;
		o = (int16_t)r;
		return c >= lo && c <= hi;
	}
};

// ---- k_tab_union ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BT) void k_tab_union(const ulonglong2 *__restrict__ src, uint64_t n_pairs, int cshift_src, unsigned long long *__restrict__ dst,
                                                  int cshift_dst, unsigned long long *__restrict__ ctr)
{
	uint32_t made = 0, full = 0;
	for (uint64_t q = (uint64_t)blockIdx.x * BT + threadIdx.x; q < n_pairs; q += (uint64_t)gridDim.x * BT) {
		const ulonglong2 v = src[q];
		if (v.x) { const uint32_t r = union_upsert(dst, cshift_dst, (2 * q) >> cshift_src, v.x); made += r == 1; full += r == 2; }
		if (v.y) { const uint32_t r = union_upsert(dst, cshift_dst, (2 * q + 1) >> cshift_src, v.y); made += r == 1; full += r == 2; }
	}
#pragma unroll
	for (int d = 32; d; d >>= 1) { made += __shfl_down(made, d, 64); full += __shfl_down(full, d, 64); }
	if (lane_id() == 0) {
		if (made) atomicAdd(&ctr[CTR_KEYS], (unsigned long long)made);
		if (full) atomicAdd(&ctr[CTR_FULL], (unsigned long long)full);
	}
}

// what every entry point refuses before any launch
int pair_check(const bfcg_kmers_t *a, const bfcg_kmers_t *b, const char *who)
{
	if (!a || !b) return bfcg::fail("bad arguments to %s", who);
	if (a->k != b->k) return bfcg::fail("%s: the tables differ in k (%d and %d)", who, a->k, b->k);
	if (a->l_pre != b->l_pre) return bfcg::fail("%s: the tables differ in l_pre (%d and %d): joining them needs a rehash", who, a->l_pre, b->l_pre);
	if (a->device != b->device) return bfcg::fail("%s: the tables lie on different devices (%d and %d)", who, a->device, b->device);
	return 0;
}

int joint_stage(bfcg_kmers_t *t)
{
	if (t->d_joint) return 0;
	hipError_t e = hipMalloc(&t->d_joint, JOINT_WORDS * 8);
	if (e != hipSuccess) { t->d_joint = NULL; (void)hipGetLastError(); return bfcg::fail("no room for the bins of a joint spectrum: %s", hipGetErrorString(e)); }
	return 0;
}

// workgroups of one launch of k_tab_join over w's table
uint32_t join_grid(const bfcg_kmers_t *w)
{
	const uint64_t n_pairs = 1ULL << (w->l_pre + w->cshift - 1), step = 64 * JOIN_UNROLL, grid = (n_pairs + step * JOIN_WAVES - 1) / (step * JOIN_WAVES);
	return grid > JOIN_GRID_MAX ? (uint32_t)JOIN_GRID_MAX : (uint32_t)grid;
}

// one launch of k_tab_join over w's table on stream st, its join_grid(w) slices from `part` on
void launch_join(const bfcg_kmers_t *w, const bfcg_kmers_t *p, int rows, unsigned long long *joint, uint32_t *part, hipStream_t st)
{
	const uint64_t n_pairs = 1ULL << (w->l_pre + w->cshift - 1), step = 64 * JOIN_UNROLL;
	const uint64_t grid = join_grid(w), waves = grid * JOIN_WAVES, span = ((n_pairs + waves - 1) / waves + step - 1) / step * step;
	hipLaunchKernelGGL(k_tab_join, dim3((unsigned)grid), dim3(JOIN_BT), 0, st, (const ulonglong2 *)w->table, n_pairs, span, w->cshift, p->table, p->cshift, rows, joint, part);
}

void launch_union(const bfcg_kmers_t *src, bfcg_kmers_t *u)
{
	const uint64_t n_pairs = 1ULL << (src->l_pre + src->cshift - 1);
	uint64_t grid = (n_pairs + BT - 1) / BT;
	if (grid > UNION_GRID_MAX) grid = UNION_GRID_MAX;
	hipLaunchKernelGGL(k_tab_union, dim3((unsigned)grid), dim3(BT), 0, u->st, (const ulonglong2 *)src->table, n_pairs, src->cshift, (unsigned long long *)u->table, u->cshift,
	                   u->d_joint);
}

} // namespace

extern "C" int bfcg_kmers_joint_hist(bfcg_kmers_t *a, bfcg_kmers_t *b, uint64_t *joint, uint64_t n[3])
{
	if (!joint || !n) return bfcg::fail("bad arguments to bfcg_kmers_joint_hist");
	if (pair_check(a, b, "bfcg_kmers_joint_hist") != 0) return -1;
	a->last_ms = 0;
	BFCG_CK(hipSetDevice(a->device));
	if (joint_stage(a) != 0) return -1;
	const uint32_t ga = join_grid(a), gb = join_grid(b);
	if (bfcg::grow(a->d_jpart, a->jpart_cap, (uint64_t)(ga + gb) * JOIN_CELLS * 4, "the workgroups' slices of a joint spectrum") != 0) return -1;
	BFCG_CK(hipMemsetAsync(a->d_joint, 0, JOINT_BINS * 8, a->st));
	BFCG_CK(hipEventRecord(a->e0, a->st));
	launch_join(a, b, 1, a->d_joint, a->d_jpart, a->st);
	launch_join(b, a, 0, a->d_joint, a->d_jpart + (uint64_t)ga * JOIN_CELLS, a->st);
	hipLaunchKernelGGL(k_join_sum, dim3(JOIN_CELLS / JOIN_SUM_BT, JOIN_SUM_Y), dim3(JOIN_SUM_BT), 0, a->st, a->d_jpart, ga + gb, a->d_joint);
	BFCG_CK(hipEventRecord(a->e1, a->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(joint, a->d_joint, JOINT_BINS * 8, hipMemcpyDeviceToHost, a->st));
	BFCG_CK(hipStreamSynchronize(a->st));
	BFCG_CK(hipEventElapsedTime(&a->last_ms, a->e0, a->e1));
	n[0] = n[1] = n[2] = 0;
	for (int i = 1; i < 256; ++i) {
		n[1] += joint[i * 256]; n[2] += joint[i];
		for (int j = 1; j < 256; ++j) n[0] += joint[i * 256 + j];
	}
	return 0;
}

extern "C" int bfcg_kmers_list_vs(bfcg_kmers_t *a, bfcg_kmers_t *b, int min_cnt, int min_diff, int other_min, int other_max, uint32_t sub_lo, uint32_t sub_hi,
                                  uint64_t *y, uint16_t *cnt_high, int16_t *other, uint64_t cap, uint64_t *n)
{
	if (!n) return bfcg::fail("bad arguments to bfcg_kmers_list_vs");
	if (pair_check(a, b, "bfcg_kmers_list_vs") != 0) return -1;
	VsOther O;
	O.tab = b->table; O.cshift = b->cshift; O.lo = other_min; O.hi = other_max;
	return list_run(a, "bfcg_kmers_list_vs", O, min_cnt, min_diff, sub_lo, sub_hi, y, cnt_high, other, cap, n);
}

extern "C" bfcg_kmers_t *bfcg_kmers_union(bfcg_kmers_t *a, bfcg_kmers_t *b)
{
	if (pair_check(a, b, "bfcg_kmers_union") != 0) return NULL;
	const uint64_t n_sub = 1ULL << a->l_pre;
	uint32_t *sa = (uint32_t *)malloc(n_sub * 4 * 2), *sb = sa ? sa + n_sub : NULL;
	if (!sa) { bfcg::fail("out of host memory"); return NULL; }
	float ms = 0;
	if (bfcg_kmers_sub_sizes(a, sa) != 0) { free(sa); return NULL; }
	ms += a->last_ms;
	if (bfcg_kmers_sub_sizes(b, sb) != 0) { free(sa); return NULL; }
	ms += b->last_ms;
	uint64_t keys = 0, most = 0;
	for (uint64_t s = 0; s < n_sub; ++s) {
		const uint64_t both = (uint64_t)sa[s] + sb[s];
		keys += both;
		if (both > most) most = both;
	}
	free(sa);
	int cshift = 2; // the smallest table that is at most half full and whose regions take all their keys whatever the overlap
	while (cshift < 39 /* kmers_new refuses more than 2^40 slots */ && (1ULL << (a->l_pre + cshift) < 2 * keys || 1ULL << cshift < most)) ++cshift;
	bfcg_kmers_t *u = bfcg::kmers_new(a->k, a->l_pre, cshift, a->device);
	if (!u) return NULL;
	const uint64_t bytes = 8ULL << (u->l_pre + u->cshift);
	unsigned long long *tab = NULL, ctr[2] = { 0, 0 };
	BFCG_CKN(bfcg_kmers_destroy(u), hipMalloc(&tab, bytes));
	u->table = tab; u->owns_table = 1;
	if (joint_stage(u) != 0) { bfcg_kmers_destroy(u); return NULL; }
	BFCG_CKN(bfcg_kmers_destroy(u), hipEventRecord(u->e0, u->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipMemsetAsync(tab, 0, bytes, u->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipMemsetAsync(u->d_joint + CTR_KEYS, 0, 16, u->st));
	launch_union(a, u);
	launch_union(b, u);
	BFCG_CKN(bfcg_kmers_destroy(u), hipEventRecord(u->e1, u->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipGetLastError());
	BFCG_CKN(bfcg_kmers_destroy(u), hipMemcpyAsync(ctr, u->d_joint + CTR_KEYS, 16, hipMemcpyDeviceToHost, u->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipStreamSynchronize(u->st));
	BFCG_CKN(bfcg_kmers_destroy(u), hipEventElapsedTime(&u->last_ms, u->e0, u->e1));
	if (ctr[1] != 0 || ctr[0] > keys) {
		bfcg::fail("bfcg_kmers_union: %llu slots found their region full, %llu keys made of at most %llu: an input changed under the union", ctr[1], ctr[0], (unsigned long long)keys);
		bfcg_kmers_destroy(u);
		return NULL;
	}
	u->n_keys = ctr[0]; u->has_keys = 1;
	u->last_ms += ms; // the two size passes and the fill: all the kernels of the call
	return u;
}

extern "C" bfc_ch_t *bfcg_kmers_export(bfcg_kmers_t *t, uint64_t *n_keys)
{
	if (!t) { bfcg::fail("bad arguments to bfcg_kmers_export"); return NULL; }
	uint64_t keys = t->n_keys;
	if (!t->has_keys) { // one pass of k_tab_hist: the spectrum's sum
		uint64_t cnt[256], high[64];
		if (bfcg_kmers_hist(t, cnt, high) == -2) return NULL;
		keys = 0;
		for (int i = 0; i < 256; ++i) keys += cnt[i];
	}
	BFCG_CKN((void)0, hipSetDevice(t->device));
	bfc_ch_t *ch = bfc_ch_alloc_raw(t->k, t->l_pre, t->cshift);
	if (!ch) { bfcg::fail("out of host memory for a table of 2^%d slots", t->l_pre + t->cshift); return NULL; }
	BFCG_CKN(bfc_ch_destroy(ch), hipMemcpy(bfc_ch_raw_slots(ch), t->table, 8ULL << (t->l_pre + t->cshift), hipMemcpyDeviceToHost));
	bfc_ch_raw_set_count(ch, keys);
	if (n_keys) *n_keys = keys;
	return ch;
}
