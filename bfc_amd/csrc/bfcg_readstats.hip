// bfcg_readstats.hip -- a read set screened against the count table where it lies in HBM: eight words per read instead of two bytes per
// base.  On the same object as the listing and the lookups (bfcg_kmers_t).  DESIGN.md section 6d.
//
// Two stages, the idiom of k_query4 -> k_streak:
//   k_profile      (bfcg_lookup.hip, launched unchanged through bfcg::profile_launch) the probe's value under every stream position
//   k_read_stats   a segmented reduction of that profile, one wavefront per read and RS_WAVES reads per workgroup: the read's positions
//                  in strides of 64, one 2-byte load per lane.  The counters come from the popcounts of wave ballots; the counts are
//                  8 bits, so minimum, median and maximum come from a 256-bin histogram per wave in LDS (an absent k-mer is bin 0) and
//                  a wave-wide prefix over the bins, four per lane, with no sort; the longest solid run is walked RUN by run on each
//                  stride's ballot of "solid" in wave-uniform registers, the open run carried from stride to stride as k_streak carries
//                  it from word to word.  No atomics in global memory.
// A wave walks its read alone, however long: a megabase contig is one wave crawling over it at 64 positions a step while the other waves
// of its workgroup wait at the barrier.  The kernel is meant for reads of 50 to 300 bases.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfc_gpu.h"
#include "bfcg_internal.h"
#include "bfc_host.h"

namespace {

enum { RS_BT = 256, RS_WAVES = RS_BT / 64, RS_BINS = 256 };

// prof[p]: -2 no k-mer ends at p, -1 absent, else high << 8 | count.  Read r is positions [off[r], off[r + 1] - 1) (the host has checked
// that the offsets ascend and end at the profile's length); out[8 r ..] as include/bfc_gpu.h says.
__global__ __launch_bounds__(RS_BT) void k_read_stats(int k, int min_cov, const int16_t *__restrict__ prof, const unsigned long long *__restrict__ off,
                                                      uint64_t n_reads, int32_t *__restrict__ out)
{
	__shared__ uint32_t hist[RS_WAVES][RS_BINS];
	const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
	const uint64_t r = (uint64_t)blockIdx.x * RS_WAVES + wave;
	uint32_t *h = hist[wave];
	*reinterpret_cast<uint4 *>(&h[4 * lane]) = make_uint4(0, 0, 0, 0);
	__syncthreads(); // (every wave passes both barriers once, whatever its read's length, also a wave behind the last read)
	uint64_t p0 = 0;
	int len = 0;
	if (r < n_reads) { p0 = off[r]; len = (int)(off[r + 1] - p0) - 1; }
	uint32_t n_def = 0, n_present = 0, n_solid = 0, sum = 0; // the first three wave-uniform, sum per lane
	// k_streak's walk: t = open run's length << 32 | its first position, mx the maximum -- the longest run, of equal ones the later
	unsigned long long mx = 0, t = 0;
	for (int i = 0; i < len; i += 64) {
		const int nb = len - i < 64 ? len - i : 64;
		const int v = lane < nb ? (int)prof[p0 + (uint64_t)i + lane] : -2;
		const int c = v >= 0 ? v & 0xff : 0;
		if (v != -2) atomicAdd(&h[c], 1u);
		sum += (uint32_t)c;
		n_def += __popcll(__ballot(v != -2));
		n_present += __popcll(__ballot(v >= 0));
		const unsigned long long w = __ballot(v >= 0 && c >= min_cov); // lanes at and beyond nb are not solid
		n_solid += __popcll(w);
		int pos = 0;
		while (pos < nb) {
			const unsigned long long x = w >> pos;
			if (x & 1ULL) { // a run of solid positions
				int ones = ~x ? __builtin_ctzll(~x) : 64;
				if (ones > nb - pos) ones = nb - pos;
				t += (unsigned long long)ones << 32;
				mx = mx > t ? mx : t;
				pos += ones;
			} else { // everything up to the next solid position restarts the run behind it
				int zeros = x ? __builtin_ctzll(x) : 64;
				if (zeros > nb - pos) zeros = nb - pos;
				pos += zeros;
				t = (unsigned long long)(i + pos);
			}
		}
	}
	__syncthreads();
	const uint4 b = *reinterpret_cast<const uint4 *>(&h[4 * lane]);
	const uint32_t s = b.x + b.y + b.z + b.w;
	uint32_t incl = s; // bins [0, 4 lane + 4)
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = __shfl_up(incl, d, 64);
		if (lane >= d) incl += o;
	}
#pragma unroll
	for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d, 64);
	int32_t word4 = 0;
	if (n_def) {
		const uint32_t m = (n_def - 1) >> 1, excl = incl - s; // the lower median is element m of the sorted counts
		const int first = b.x ? 0 : b.y ? 1 : b.z ? 2 : 3, last = b.w ? 3 : b.z ? 2 : b.y ? 1 : 0; // of this lane's bins, where s > 0
		const int med = m < excl + b.x ? 0 : m < excl + b.x + b.y ? 1 : m < excl + b.x + b.y + b.z ? 2 : 3; // where excl <= m < incl
		const unsigned long long nz = __ballot(s > 0), holds = __ballot(excl <= m && m < incl);
		const int lo = __shfl(4 * lane + first, __builtin_ctzll(nz), 64), hi = __shfl(4 * lane + last, 63 - __builtin_clzll(nz), 64);
		const int md = __shfl(4 * lane + med, __builtin_ctzll(holds), 64);
		word4 = lo | md << 8 | hi << 16;
	}
	if (r < n_reads && lane == 0) {
		const int streak = (int)(mx >> 32), start = streak ? (int)(uint32_t)mx - (k - 1) : -1;
		int4 *o = reinterpret_cast<int4 *>(out + 8 * r);
		o[0] = make_int4((int)n_def, (int)n_present, (int)n_solid, (int)sum);
		o[1] = make_int4(word4, streak, start, streak ? start + streak + k - 1 : -1);
	}
}

} // namespace

// the stream and off[] as bfcg_trim_batch / bfcg_ec_batch take them; out (host): eight words per read
extern "C" int bfcg_kmers_read_stats(bfcg_kmers_t *t, const uint8_t *h_seq, const uint8_t *d_seq, uint64_t n_pos, const uint64_t *h_off, uint64_t n_reads,
                                     int min_cov, int32_t *out)
{
	if (!t) return bfcg::fail("bad arguments to bfcg_kmers_read_stats");
	t->last_ms = 0;
	if (bfcg_read_stats_check(n_pos, h_off, n_reads, min_cov) != 0) return -1;
	if (n_reads == 0 || n_pos == 0) return 0;
	if (!h_seq == !d_seq || !out) return bfcg::fail("bad arguments to bfcg_kmers_read_stats (exactly one of h_seq / d_seq, and a result buffer)");
	BFCG_CK(hipSetDevice(t->device));
	if (bfcg::grow(t->d_roff, t->roff_cap, (n_reads + 1) * 8, "the reads' offsets") != 0) return -1;
	if (bfcg::grow(t->d_rout, t->rout_cap, n_reads * 32, "the reads' statistics") != 0) return -1;
	BFCG_CK(hipMemcpyAsync(t->d_roff, h_off, (n_reads + 1) * 8, hipMemcpyHostToDevice, t->st));
	if (bfcg::profile_launch(t, h_seq, d_seq, n_pos) != 0) return -1;
	hipLaunchKernelGGL(k_read_stats, dim3((unsigned)((n_reads + RS_WAVES - 1) / RS_WAVES)), dim3(RS_BT), 0, t->st, t->k, min_cov, t->d_pout, t->d_roff, n_reads, t->d_rout);
	BFCG_CK(hipEventRecord(t->e1, t->st));
	BFCG_CK(hipGetLastError());
	BFCG_CK(hipMemcpyAsync(out, t->d_rout, n_reads * 32, hipMemcpyDeviceToHost, t->st));
	BFCG_CK(hipStreamSynchronize(t->st));
	BFCG_CK(hipEventElapsedTime(&t->last_ms, t->e0, t->e1));
	return 0;
}
