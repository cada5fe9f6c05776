// bfcg_upsert.h -- a whole slot inserted into a device table that is being built, for the files that make one: bfcg_tabcmp.hip (the
// union of two tables) and bfcg_clip.hip (the survivors of a round).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// table_upsert (bfcg_kernels.hip) on (sub, key), the increment a whole slot: 1 key created, 0 counts added (saturating, order
// independent), 2 region full -- which the geometry rules out; the host checks the counter all the same
__device__ __forceinline__ uint32_t union_upsert(unsigned long long *__restrict__ tab, int cshift, uint64_t sub, unsigned long long v)
{
	const uint64_t cmask = (1ULL << cshift) - 1;
	unsigned long long *reg = tab + (sub << cshift);
	uint64_t pos = (v >> 14) & cmask;
	const uint32_t c = (uint32_t)(v & 0xff), h = (uint32_t)(v >> 8 & 0x3f);
	for (uint64_t probe = 0; probe <= cmask; ++probe, pos = (pos + 1) & cmask) {
		unsigned long long cur = __hip_atomic_load(&reg[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == 0) {
			cur = atomicCAS(&reg[pos], 0ULL, v);
			if (cur == 0) return 1;
		}
		if ((cur >> 14) == (v >> 14)) {
			for (;;) {
				const uint32_t nc = (uint32_t)(cur & 0xff) + c, nh = (uint32_t)(cur >> 8 & 0x3f) + h;
				const unsigned long long nv = (cur & ~0x3fffULL) | (nc < 255 ? nc : 255) | ((uint64_t)(nh < 63 ? nh : 63) << 8);
				if (nv == cur) return 0;
				const unsigned long long old = atomicCAS(&reg[pos], cur, nv);
				if (old == cur) return 0;
				cur = old;
			}
		}
	}
	return 2;
}

} // namespace
