// bfcg_kdec.h -- from a slot of the count table back to the k-mer, as ONE piece of code for the host and the device (the pattern of
// bfcg_ec1.h).  It is the inverse of what kmer_dev.h computes forwards:
//
//   k-mer planes (a, b) of the canonical strand            kmer_hash_from_windows:  h0 = mix(a + b), h1 = mix(h0 ^ b)
//   table hash (Y0, Y1) = ((h0 + h1) & m, h1)              ch_subkey:               (sub-table, key) from (Y0, Y1)
//   slot = key << 14 | high << 8 | count
//
// slot_to_hash() undoes ch_subkey, hash_to_kmer() undoes the two sums and the two mixes.  The key keeps every bit of (Y0, Y1) only for
// k <= 37: a key has 50 bits (BFC_CH_KEYBITS), for k <= 32 the sub-table index supplies the rest of Y0 << k | Y1 (l_pre is clamped so
// that 2k - l_pre <= 50), for 33 <= k <= 37 the key is (low k - l_pre bits of Y0) << k ^ Y1 with (k - l_pre) + k <= 50, i.e. no
// overlap.  From k = 38 on the shift is 50 - (k - l_pre) < k and the xor folds bits of Y0 into Y1: decodable() says no.
//
// mix_k (kmer_dev.h:30-40) is four multiplications by odd constants modulo 2^k, (2^21 - 1) v - 1, 265 v, 21 v, (2^31 + 1) v, with three
// v ^= v >> s between them.  An odd constant has an inverse modulo 2^64, which is also its inverse modulo 2^k (minv64: Newton's
// iteration, evaluated by the compiler); v ^= v >> s is undone by folding the known top bits down s at a time.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define KD_HD __host__ __device__ __forceinline__
#else
#define KD_HD static inline
#endif

namespace kdec {

enum { MAX_K = 37 }; // the last k whose key is lossless

constexpr uint64_t minv64(uint64_t a) // a odd: x with a * x = 1 (mod 2^64); every step doubles the number of correct low bits (a * a = 1 mod 8)
{
	uint64_t x = a;
	for (int i = 0; i < 5; ++i) x *= 2 - a * x;
	return x;
}

KD_HD uint64_t mask(int k) { return k >= 64 ? ~0ULL : (1ULL << k) - 1; }

KD_HD uint64_t mix(uint64_t v, uint64_t m) // the forward function (kmer_dev.h: mix_k), for the checks
{
	v = (~v + (v << 21)) & m;
	v ^= v >> 24;
	v = (v + (v << 3) + (v << 8)) & m;
	v ^= v >> 14;
	v = (v + (v << 2) + (v << 4)) & m;
	v ^= v >> 28;
	v = (v + (v << 31)) & m;
	return v;
}

template <int S> KD_HD uint64_t unxorshift(uint64_t w) // v with v ^ (v >> S) = w: the top S bits of v are w's, every fold fixes S more
{
	uint64_t v = w;
#pragma unroll
	for (int done = S; done < 64; done += S) v = w ^ (v >> S);
	return v;
}

KD_HD uint64_t unmix(uint64_t v, uint64_t m)
{
	constexpr uint64_t i31 = minv64(0x80000001ULL), i21 = minv64(21), i265 = minv64(265), i2m = minv64(0x1FFFFFULL);
	v = (v * i31) & m;
	v = unxorshift<28>(v);
	v = (v * i21) & m;
	v = unxorshift<14>(v);
	v = (v * i265) & m;
	v = unxorshift<24>(v);
	v = ((v + 1) * i2m) & m; // w = (2^21 - 1) v - 1
	return v;
}

KD_HD bool decodable(int k) { return k >= 1 && k <= MAX_K; }

// the inverse of ch_subkey (kmer_dev.h) for a decodable k: the table hash (Y0, Y1) of the k-mer in `slot` of sub-table `sub`
KD_HD void slot_to_hash(int k, int l_pre, uint32_t sub, uint64_t slot, uint64_t &Y0, uint64_t &Y1)
{
	const uint64_t key = slot >> 14, m = mask(k);
	if (k <= 32) {
		const int t = 2 * k - l_pre;
		const uint64_t z = (t < 64 ? (uint64_t)sub << t : 0) | key;
		Y0 = z >> k; Y1 = z & m;
	} else {
		Y0 = (uint64_t)sub << (k - l_pre) | key >> k;
		Y1 = key & m;
	}
}

// the inverse of kmer_hash_from_windows: the two bit planes of the strand the forward hash chose (bit l = the base l from the 3' end)
KD_HD void hash_to_kmer(int k, uint64_t Y0, uint64_t Y1, uint64_t &a, uint64_t &b)
{
	const uint64_t m = mask(k), h1 = Y1, h0 = (Y0 - Y1) & m;
	b = unmix(h1, m) ^ h0;            // h1 = mix(h0 ^ b)
	a = (unmix(h0, m) - b) & m;       // h0 = mix(a + b)
}

KD_HD void kmer_to_hash(int k, uint64_t a, uint64_t b, uint64_t &Y0, uint64_t &Y1) // forwards again, for hash(decode(x)) == x
{
	const uint64_t m = mask(k), h0 = mix((a + b) & m, m), h1 = mix(h0 ^ b, m);
	Y0 = (h0 + h1) & m; Y1 = h1;
}

KD_HD void decode(int k, int l_pre, uint32_t sub, uint64_t slot, uint64_t &a, uint64_t &b)
{
	uint64_t Y0, Y1;
	slot_to_hash(k, l_pre, sub, slot, Y0, Y1);
	hash_to_kmer(k, Y0, Y1, a, b);
}

// hash2cnt's -m / -d on a slot's fields: count >= min_cnt and min(count, 63) - high >= min_diff
KD_HD bool keep(uint64_t slot, int min_cnt, int min_diff)
{
	const int cnt = (int)(slot & 0xff), high = (int)(slot >> 8 & 0x3f);
	return slot != 0 && cnt >= min_cnt && (cnt < 63 ? cnt : 63) - high >= min_diff;
}

} // namespace kdec
