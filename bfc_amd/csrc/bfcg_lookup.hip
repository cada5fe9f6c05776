// bfcg_lookup.hip -- the count table asked by k-mer, where it lies in HBM: "here are my k-mers, or my sequence; what did you count for
// them?"  The other direction of bfcg_kmers.hip's listing, on the same object (bfcg_kmers_t).  DESIGN.md section 6d.
//
//   k_lookup    one k-mer per lane, given as the two bit planes a listing hands out (either strand): the planes turned into the stream's
//               windows (bit-reversed over k), from which kmer_hash_from_windows / _windows2 build both strands, pick one by the middle
//               base (kmer.h:81) and hash it -- the arithmetic k_occ runs on a window cut from the bases --, then ch_get_dev's probe
//   k_profile   k_occ's skeleton (occ_tile, bfcg_k1.h) over a batch stream, keeping the probe's value: 2 bytes per position
//
// Neither kernel has a hash or a probe of its own.  A query larger than the object's staging buffers is cut into pieces inside the call.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfcg_k1.h"

namespace {

enum { LOOKUP_BT = 256, LOOKUP_GRID_MAX = 256 * 8 /* eight workgroups on each of the 256 CUs */ };
enum : uint64_t { LOOKUP_CAP = 1ULL << 22 /* k-mers a piece: 64 MiB of planes, 8 MiB of answers */ };

// W = uint32_t for k <= 32, uint64_t above, as k_occ is instantiated.  Bits of the planes at and above k fall out of the reversal.
template <typename W>
__global__ __launch_bounds__(LOOKUP_BT) void k_lookup(int k, int l_pre, int cshift, const unsigned long long *__restrict__ tab,
                                                      const ulonglong2 *__restrict__ y, uint64_t n, int16_t *__restrict__ out)
{
	constexpr int nb = 8 * (int)sizeof(W);
	for (uint64_t i = (uint64_t)blockIdx.x * LOOKUP_BT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LOOKUP_BT) {
		const ulonglong2 v = y[i];
		// a plane has the base at the 3' end in bit 0, a window of the stream the oldest base: the given strand's windows
		const W w_lo = brev_w((W)v.x) >> (nb - k), w_hi = brev_w((W)v.y) >> (nb - k);
		uint64_t y0, y1;
		kmer_hash_windows<W>(k, w_lo, w_hi, y0, y1);
		out[i] = (int16_t)ch_get_dev(k, l_pre, cshift, tab, y0, y1);
	}
}

template <typename W, int TILE, int BT>
__global__ __launch_bounds__(BT) void k_profile(KParams P, const uint8_t *__restrict__ seq, int64_t n_pos, const unsigned long long *__restrict__ tab,
                                                int16_t *__restrict__ out)
{
	constexpr int PW = (TILE + 64) / 32 + 2;
	__shared__ uint32_t planes[4 * PW];
	occ_tile<W, TILE, BT>(P, seq, n_pos, tab, planes, [&](int64_t e, int occ) { out[e] = (int16_t)occ; });
}

} // namespace

// the staging buffers of a lookup, both or none
int bfcg::lookup_stage(bfcg_kmers_t *t)
{
	if (t->d_qy) return 0;
	ulonglong2 *qy = NULL; int16_t *qout = NULL;
	hipError_t e = hipMalloc(&qy, t->q_cap * 16);
	if (e == hipSuccess) e = hipMalloc(&qout, t->q_cap * 2);
	if (e != hipSuccess) {
		(void)hipFree(qy); (void)hipFree(qout); (void)hipGetLastError();
		return bfcg::fail("no room for a lookup's staging buffers (%llu k-mers a piece): %s", (unsigned long long)t->q_cap, hipGetErrorString(e));
	}
	t->d_qy = qy; t->d_qout = qout;
	return 0;
}

uint64_t bfcg::lookup_cap()
{
	const char *s = getenv("BFCG_LOOKUP_CAP");
	const unsigned long long v = s ? strtoull(s, NULL, 10) : 0;
	return v ? v : LOOKUP_CAP;
}

extern "C" int bfcg_kmers_lookup(bfcg_kmers_t *t, const uint64_t *y, uint64_t n, int16_t *out, uint64_t *n_found)
{
	if (!t || (n && (!y || !out))) return bfcg::fail("bad arguments to bfcg_kmers_lookup");
	if (n_found) *n_found = 0;
	t->last_ms = 0;
	if (n == 0) return 0;
	BFCG_CK(hipSetDevice(t->device));
	if (bfcg::lookup_stage(t) != 0) return -1;
	float total = 0;
	for (uint64_t done = 0; done < n; ) {
		const uint64_t m = n - done < t->q_cap ? n - done : t->q_cap;
		uint64_t grid = (m + LOOKUP_BT - 1) / LOOKUP_BT;
		if (grid > LOOKUP_GRID_MAX) grid = LOOKUP_GRID_MAX;
		float ms = 0;
		BFCG_CK(hipMemcpyAsync(t->d_qy, y + 2 * done, m * 16, hipMemcpyHostToDevice, t->st));
		BFCG_CK(hipEventRecord(t->e0, t->st));
		if (t->k <= 32) hipLaunchKernelGGL((k_lookup<uint32_t>), dim3((unsigned)grid), dim3(LOOKUP_BT), 0, t->st, t->k, t->l_pre, t->cshift, t->table, t->d_qy, m, t->d_qout);
		else hipLaunchKernelGGL((k_lookup<uint64_t>), dim3((unsigned)grid), dim3(LOOKUP_BT), 0, t->st, t->k, t->l_pre, t->cshift, t->table, t->d_qy, m, t->d_qout);
		BFCG_CK(hipEventRecord(t->e1, t->st));
		BFCG_CK(hipGetLastError());
		BFCG_CK(hipMemcpyAsync(out + done, t->d_qout, m * 2, hipMemcpyDeviceToHost, t->st));
		BFCG_CK(hipStreamSynchronize(t->st));
		BFCG_CK(hipEventElapsedTime(&ms, t->e0, t->e1));
		total += ms;
		done += m;
	}
	t->last_ms = total;
	if (n_found) {
		uint64_t f = 0;
		for (uint64_t i = 0; i < n; ++i) f += out[i] >= 0;
		*n_found = f;
	}
	return 0;
}

// the first half of a profile, shared with bfcg_kmers_read_stats (bfcg_readstats.hip): everything up to and including k_profile's launch
int bfcg::profile_launch(bfcg_kmers_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos)
{
	if (n_pos >= 1ULL << 40) return bfcg::fail("a stream of %llu positions is too long for one profile: walk it in pieces that overlap by k - 1", (unsigned long long)n_pos);
	BFCG_CK(hipSetDevice(t->device));
	if (h_seq && bfcg::grow(t->d_pseq, t->pseq_cap, n_pos, "a profile") != 0) return -1;
	if (bfcg::grow(t->d_pout, t->pout_cap, n_pos * 2, "a profile") != 0) return -1;
	if (h_seq) { BFCG_CK(hipMemcpyAsync(t->d_pseq, h_seq, n_pos, hipMemcpyHostToDevice, t->st)); d_seq = t->d_pseq; }
	bfcg::KParams P = {};
	P.k = t->k; P.l_pre = t->l_pre; P.tab_cshift = t->cshift;
	const int64_t tiles = ((int64_t)n_pos + BFCG_TILE1 - 1) / BFCG_TILE1;
	const unsigned g = (unsigned)(((tiles + 7) / 8) * 8); // xcd_tile deals whole rounds of the eight XCDs
	BFCG_CK(hipEventRecord(t->e0, t->st));
	if (t->k <= 32) hipLaunchKernelGGL((k_profile<uint32_t, BFCG_TILE1, BFCG_BT1>), dim3(g), dim3(BFCG_BT1), 0, t->st, P, d_seq, (int64_t)n_pos, t->table, t->d_pout);
	else hipLaunchKernelGGL((k_profile<uint64_t, BFCG_TILE1, BFCG_BT1>), dim3(g), dim3(BFCG_BT1), 0, t->st, P, d_seq, (int64_t)n_pos, t->table, t->d_pout);
	return 0;
}

// the stream is the batch format of PART 2, on the host or on the device; out[p] (host) describes the k-mer ending at position p
extern "C" int bfcg_kmers_profile(bfcg_kmers_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos, int16_t *out)
{
	if (!t || !h_seq == !d_seq || (n_pos && !out)) return bfcg::fail("bad arguments to bfcg_kmers_profile (exactly one of h_seq / d_seq, and a result buffer)");
	t->last_ms = 0;
	if (n_pos == 0) return 0;
	if (bfcg::profile_launch(t, h_seq, d_seq, n_pos) != 0) return -1;
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(out, t->d_pout, n_pos * 2, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&t->last_ms, t->e0, t->e1));
	return 0;
}
