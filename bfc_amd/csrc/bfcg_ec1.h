// bfcg_ec1.h -- BFC's per-read error correction (bfc_ec1, correct.c:388-476, with bfc_ec1dir, correct.c:249-386) as ONE piece of
// code for the host and the device.  It is templated on the k-mer lookup: table_get on the device table (bfcg_ec.hip), bfc_ch_get
// on the host table (the host instance, also in bfcg_ec.hip).  Results are byte-identical to the reference's worker_ec in table mode.
//
// What a read is made of (bfc_seq_conv, correct.c:23-38): base code b = seq_nt6_table[c] - 1 (ACGTacgt -> 0..3, any other byte -> 4),
// q = 1 without a quality string, else (signed char)qual - 33 >= opt.q, and q = 0 where b > 3.  Nothing is copied per read: ec_base()
// derives b / ob / q / lcov / hcov of position i in either orientation from the read's bytes and its packed k-mer coverage words
// (lcov | hcov << 6 | solid_end << 12, bfcg_kcov_batch's format).  The one base the brute path may change (bfc_ec_greedy_k) is an
// override (pos, base).
//
// Refinement (`bfc -R`, opt.refine_ec) is the template parameter RF of every function that reads a base: the table-mode instances are
// the code they were before.  With RF a base comes from the quality string where bfc wrote it there (bfc_seq_conv's b_from_q,
// correct.c:31): (signed char)qual - 33 <= 5 gives b = (qual - 34) & 7, every other position decodes its sequence byte as above.  Values
// 5..7 come only from quality bytes <= 33 (e.g. '!'), which bfc never writes; the reference then indexes past "ACGTN" (correct.c:457,
// undefined), here they are folded to 4 (N).  The read's earlier stats (worker_ec's ori_st, correct.c:543) come in as the (aux, aux2) pair
// worker_ec packs, and end the correction as correct.c:438-442 / 470 do: rf_code 2 (the earlier stats, the read untouched) when they say
// ec_code 0 with fewer absent k-mers than the new path, else rf_code 3 after a correction; the early exits keep rf_code 1.
//
// The search keeps the reference's data: a binary heap ordered by tot_pen with ksort's tie behaviour (pop: the last element to the
// root and sift down, taking the right child only if the left one is "less"; push: append and sift up, stopping when the new element is
// "less" than its parent; "less" = larger tot_pen) and a stack of extension steps linked by parent index.  A heap entry holds the two
// forward planes of its k-mer only: the reverse planes are their complement, bit-reversed over k bits, whenever the k-mer is full --
// and a lookup never sees any other.  Both arrays have a fixed capacity; a read that would overflow either reports EC_OVERFLOW and
// its bytes are left untouched, so the caller can run it again with more room (the host instance grows and retries; the device flags
// the read for the host).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define EC_HD __host__ __device__ __forceinline__
#else
#define EC_HD static inline
#endif

namespace ec1k {

enum { MAX_PATHS = 4, HIST = 5, HIST_HIGH = 2 };              // bfc.h:11-13
enum { CODE_MISC = 1, CODE_MANY_N = 2, CODE_NO_SOLID = 3, CODE_UNCORR_N = 4, CODE_MANY_FAIL = 5 };
enum { EC_OK = 0, EC_OVERFLOW = 1 };
// aux2 of a read left to the host.  No result can have it: it would be n_absent 2^22 - 1 with rf_code 3, but rf_code 3 only follows a
// correction on the device, where a read has at most lmax <= 2^16 bases and so fewer absent k-mers; rf_code 2 sets bit 9 alone.
#define BFCG_EC_FALLBACK 0xffffffffu

struct Opt {                                                   // the bfc_opt_t fields the corrector reads, and the count table's mode
	int k, q, max_end_ext, win_multi_ec, min_cov;
	int w_ec, w_ec_high, w_absent, w_absent_high, max_path_diff, max_heap;
	int mode;                                                  // bfc_ch_hist's mode (correct.c:627), for the brute path
};

struct Heap1 {                                                 // 56 bytes (the reference's entry: 72)
	uint64_t x0, x1;                                           // forward planes of the k-mer
	int32_t tot_pen, i, k;                                     // penalty so far, next base position, stack index (-1: root)
	int32_t ecpos_high[HIST_HIGH], ecpos[HIST];
};
struct Stack1 { int32_t parent, i, tot_pen; uint8_t b, pen; uint16_t pad; }; // pen: ec | ec_high<<1 | absent<<2 | absent_high<<3

struct Read {                                                  // one read as the corrector sees it
	const uint8_t *seq, *qual;                                 // qual NULL: no quality string
	const uint16_t *cov;                                       // packed kcov word per base (lcov | hcov << 6 | solid_end << 12)
	int n;
	int brute_pos, brute_b;                                    // b of brute_pos is brute_b (-1: none)
};

EC_HD int nt4(uint8_t c)                                       // seq_nt6_table - 1 (bseq.c:9-26)
{
	const int u = c & 0xdf;                                    // upper case; bytes >= 128 stay apart
	return c >= 128 ? 4 : u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

// base code of position p (bfc_seq_conv, correct.c:31); with RF, from the quality byte where bfc wrote one there
template <bool RF> EC_HD int base_at(const uint8_t *seq, const uint8_t *qual, int p)
{
	if (RF && qual) {
		const int q = (int)(signed char)qual[p] - 33;
		if (q <= 5) { const int b = (q - 1) & 7; return b > 4 ? 4 : b; }
	}
	return nt4(seq[p]);
}

struct Base { int b, ob, q, lcov, hcov; };

// position i of the read in orientation dir (1: the reverse complement of the whole read)
template <bool RF> EC_HD Base ec_base(const Opt &o, const Read &r, int dir, int i)
{
	Base c;
	const int p = dir ? r.n - 1 - i : i;
	const int ob = base_at<RF>(r.seq, r.qual, p);
	int b = p == r.brute_pos ? r.brute_b : ob;
	c.q = ob > 3 ? 0 : !r.qual ? 1 : (int)(signed char)r.qual[p] - 33 >= o.q ? 1 : 0;
	c.ob = dir && ob < 4 ? 3 - ob : ob;
	c.b = dir && b < 4 ? 3 - b : b;
	c.lcov = r.cov[p] & 0x3f; c.hcov = r.cov[p] >> 6 & 0x3f;
	return c;
}

EC_HD uint64_t kmask(int k) { return (1ULL << k) - 1; }
EC_HD void kmer_append(int k, uint64_t &x0, uint64_t &x1, int c) { const uint64_t m = kmask(k); x0 = (x0 << 1 | (uint64_t)(c & 1)) & m; x1 = (x1 << 1 | (uint64_t)(c >> 1)) & m; }
EC_HD void kmer_change(uint64_t &x0, uint64_t &x1, int d, int c)
{
	const uint64_t t = ~(1ULL << d);
	x0 = (uint64_t)(c & 1) << d | (x0 & t); x1 = (uint64_t)(c >> 1) << d | (x1 & t);
}
EC_HD uint64_t mix(uint64_t v, uint64_t m)                     // Thomas Wang's 64-bit mix reduced to k bits (kmer.h:30-40)
{
	v = (~v + (v << 21)) & m; v ^= v >> 24;
	v = (v + (v << 3) + (v << 8)) & m; v ^= v >> 14;
	v = (v + (v << 2) + (v << 4)) & m; v ^= v >> 28;
	v = (v + (v << 31)) & m;
	return v;
}
// the table key (y0, y1) of a full k-mer given by its forward planes (kmer.h:79-88 on the four planes)
EC_HD void kmer_y(int k, uint64_t x0, uint64_t x1, uint64_t &y0, uint64_t &y1)
{
	const uint64_t m = kmask(k);
	const uint64_t x2 = __builtin_bitreverse64(~x0 & m) >> (64 - k), x3 = __builtin_bitreverse64(~x1 & m) >> (64 - k);
	const int t = k >> 1, rev = (x1 >> t & 1) > (x3 >> t & 1);
	const uint64_t a = rev ? x2 : x0, b = rev ? x3 : x1;
	const uint64_t h0 = mix((a + b) & m, m), h1 = mix(h0 ^ b, m);
	y0 = (h0 + h1) & m; y1 = h1;
}
template <class Lookup> EC_HD int occ(const Lookup &lk, int k, uint64_t x0, uint64_t x1)
{
	uint64_t y0, y1;
	kmer_y(k, x0, x1, y0, y1);
	return lk(y0, y1);
}

// bfc_ec_kcov (correct.c:96-117) into packed words: the host instance's coverage (the device has k_occ / k_cov)
template <bool RF, class Lookup> EC_HD void kcov(const Opt &o, const uint8_t *seq, const uint8_t *qual, int n, const Lookup &lk, uint16_t *cov)
{
	uint64_t x0 = 0, x1 = 0;
	for (int i = 0; i < n; ++i) cov[i] = 0;
	for (int i = 0, l = 0; i < n; ++i) {
		const int c = base_at<RF>(seq, qual, i);
		if (c > 3) { l = 0; x0 = x1 = 0; continue; }
		kmer_append(o.k, x0, x1, c);
		if (++l < o.k) continue;
		const int r = occ(lk, o.k, x0, x1);
		if (r < 0) continue;
		const int high = (r >> 8 & 0x3f) >= o.min_cov + 1;
		if (high) cov[i] |= 1 << 13;
		if ((r & 0xff) >= o.min_cov) {
			cov[i] |= 1 << 12;
			for (int j = i - o.k + 1; j <= i; ++j) cov[j] += 1 + (high << 6);
		}
	}
}

EC_HD int weighted(const Opt &o, int pen)
{
	return o.w_ec * (pen & 1) + o.w_ec_high * (pen >> 1 & 1) + o.w_absent * (pen >> 2 & 1) + o.w_absent_high * (pen >> 3 & 1);
}

// ksort's heap (ksort.h: ks_heapup / ks_heapdown) with lt(a, b) = a.tot_pen > b.tot_pen
EC_HD void heap_up(Heap1 *h, int n)
{
	int k = n - 1;
	const Heap1 tmp = h[k];
	while (k) {
		const int i = (k - 1) >> 1;
		if (tmp.tot_pen > h[i].tot_pen) break;
		h[k] = h[i]; k = i;
	}
	h[k] = tmp;
}
EC_HD void heap_down(Heap1 *h, int n)
{
	int i = 0, k = 0;
	const Heap1 tmp = h[0];
	while ((k = (k << 1) + 1) < n) {
		if (k != n - 1 && h[k].tot_pen > h[k + 1].tot_pen) ++k;
		if (h[k].tot_pen > tmp.tot_pen) break;
		h[i] = h[k]; i = k;
	}
	h[i] = tmp;
}

struct Work { Heap1 *heap; Stack1 *stack; int hcap, scap; };

// buf_update (correct.c:198-233): one extension step onto the stack and its successor into the heap
EC_HD int push(const Opt &o, Work &w, int &hn, int &sn, const Heap1 &z, int pen, int b)
{
	if (sn == w.scap || hn == w.hcap) return EC_OVERFLOW;
	Stack1 &q = w.stack[sn++];
	q.parent = z.k; q.i = z.i; q.b = (uint8_t)b; q.pen = (uint8_t)pen; q.pad = 0;
	q.tot_pen = z.tot_pen + weighted(o, pen);
	Heap1 &r = w.heap[hn++];
	r.i = z.i + 1; r.k = sn - 1; r.x0 = z.x0; r.x1 = z.x1;
	if (pen & 2) { r.ecpos_high[1] = z.ecpos_high[0]; r.ecpos_high[0] = z.i; }
	else { r.ecpos_high[0] = z.ecpos_high[0]; r.ecpos_high[1] = z.ecpos_high[1]; }
	if (pen & 1) { for (int j = HIST - 1; j > 0; --j) r.ecpos[j] = z.ecpos[j - 1]; r.ecpos[0] = z.i; }
	else for (int j = 0; j < HIST; ++j) r.ecpos[j] = z.ecpos[j];
	r.tot_pen = q.tot_pen;
	kmer_append(o.k, r.x0, r.x1, b);
	heap_up(w.heap, hn);
	return EC_OK;
}

// bfc_ec1dir (correct.c:249-386) in orientation dir from `start`; end is the read's length.  ec[i] (this orientation) gets the chosen
// path's base or 4 where the read is not corrected.  *rv: n_absent of the path (>= 0), -2 (heap ran empty), -3 (too many failures),
// -1 (no path).  Returns EC_OK or EC_OVERFLOW.
template <bool RF, class Lookup>
EC_HD int ec1dir(const Opt &o, const Read &r, int dir, int start, const Lookup &lk, Work &w, uint8_t *ec, int *max_heap, int *rv)
{
	const int n = r.n, end = n, k = o.k;
	int path[MAX_PATHS], n_paths = 0, min_path = -1, min_path_pen = 0x7fffffff, n_failures = 0, hn = 0, sn = 0;
	Heap1 z;
	*rv = -1; *max_heap = 0;
	z.x0 = z.x1 = 0; z.tot_pen = 0; z.k = -1;
	for (int j = 0; j < HIST; ++j) z.ecpos[j] = -1;
	for (int j = 0; j < HIST_HIGH; ++j) z.ecpos_high[j] = -1;
	int l = 0;
	for (z.i = start; z.i < end; ++z.i) {                      // the first k-1 bases of the first k-mer
		const int c = ec_base<RF>(o, r, dir, z.i).b;
		if (c < 4) {
			if (++l == k) break;
			kmer_append(k, z.x0, z.x1, c);
		} else { l = 0; z.x0 = z.x1 = 0; }
	}
	w.heap[hn++] = z;
	for (;;) {
		int stop = 0;
		*max_heap = *max_heap > 255 ? 255 : *max_heap > hn ? *max_heap : hn;
		if (hn == 0) { *rv = -2; break; }
		z = w.heap[0];
		w.heap[0] = w.heap[--hn];
		heap_down(w.heap, hn);
		if (min_path >= 0 && z.tot_pen > min_path_pen + o.max_path_diff) break;
		if (z.i - end > o.max_end_ext) stop = 1;
		if (!stop) {
			const int has_c = z.i < n;
			Base c; c.b = 4; c.ob = 4; c.q = 0; c.lcov = c.hcov = 0;
			if (has_c) c = ec_base<RF>(o, r, dir, z.i);
			int os = -1, fixed = 0, other_ext = 0, n_added = 0, added[4], added_b[4];
			if (z.i > end) fixed = 1;
			if (has_c && c.b < 4) {
				uint64_t x0 = z.x0, x1 = z.x1;
				kmer_append(k, x0, x1, c.b);
				os = occ(lk, k, x0, x1);
				if (c.q && (os & 0xff) >= o.min_cov + 1 && c.lcov >= o.min_cov + 1) fixed = 1;
				else if (c.hcov > k * .75) fixed = 1;
			}
			for (int b = 0; b < 4; ++b) {
				if (fixed && has_c && b != c.b) continue;
				if (!has_c || b != c.b) {
					if (has_c) {
						if (c.q && z.ecpos_high[HIST_HIGH - 1] >= 0 && z.i - z.ecpos_high[HIST_HIGH - 1] < o.win_multi_ec) continue;
						if (z.ecpos[HIST - 1] >= 0 && z.i - z.ecpos[HIST - 1] < o.win_multi_ec) continue;
					}
					uint64_t x0 = z.x0, x1 = z.x1;
					kmer_append(k, x0, x1, b);
					const int s = occ(lk, k, x0, x1);
					if (s < 0 || (s & 0xff) < o.min_cov) continue;
					const int pe = has_c && c.b < 4 ? 1 : 0;
					const int ph = pe ? c.q : 0;                // oq == q without refine_ec
					const int pah = (s >> 8 & 0xff) < o.min_cov;
					added[n_added] = pe | ph << 1 | pah << 3; added_b[n_added++] = b;
					++other_ext;
				} else {
					const int pa = os < 0 || (os & 0xff) < o.min_cov, pah = os < 0 || (os >> 8 & 0xff) < o.min_cov;
					added[n_added] = pa << 2 | pah << 3; added_b[n_added++] = b;
				}
			}
			if (fixed == 0 && other_ext == 0) ++n_failures;
			if (n_failures > n * 2) { *rv = -3; break; }
			if (has_c || n_added == 1) {
				if (n_added > 1 && hn > o.max_heap) {          // heap explosion: only the first cheapest step
					int min_b = -1, mn = 0x7fffffff;
					for (int b = 0; b < n_added; ++b) { const int t = weighted(o, added[b]); if (mn > t) mn = t, min_b = b; }
					if (push(o, w, hn, sn, z, added[min_b], added_b[min_b]) != EC_OK) return EC_OVERFLOW;
				} else {
					for (int b = 0; b < n_added; ++b)
						if (push(o, w, hn, sn, z, added[b], added_b[b]) != EC_OK) return EC_OVERFLOW;
				}
			} else {
				if (n_added == 0) w.stack[z.k].tot_pen += o.w_absent * (o.max_end_ext - (z.i - end));
				stop = 1;
			}
		}
		if (stop) {
			if (w.stack[z.k].tot_pen < min_path_pen) min_path_pen = w.stack[z.k].tot_pen, min_path = n_paths;
			path[n_paths++] = z.k;
			if (n_paths == MAX_PATHS) break;
		}
	}
	for (int i = 0; i < n; ++i) ec[i] = (uint8_t)ec_base<RF>(o, r, dir, i).b;
	if (n_paths == 0) return EC_OK;
	int n_absent = 0;                                          // buf_backtrack (correct.c:235-247)
	for (int e = path[min_path]; e >= 0; e = w.stack[e].parent) {
		const int i = w.stack[e].i;
		if (i < n) { ec[i] = w.stack[e].b; n_absent += w.stack[e].pen >> 2 & 1; }
	}
	for (int i = 0; i < n && i < start + k; ++i) ec[i] = 4;   // i >= end never holds: end is the read's length
	*rv = n_absent;
	return EC_OK;
}

struct Result { uint32_t aux, aux2; };

// bfc_ec1 (correct.c:388-476) and worker_ec's packing (correct.c:552-553).  seq / qual are rewritten in place when ec_code is 0 (and,
// with RF, the earlier stats `ori` do not keep the read).  ec0 / ec1 hold n bytes each.  Returns EC_OK or EC_OVERFLOW (nothing written then).
template <bool RF, class Lookup>
EC_HD int ec1(const Opt &o, uint8_t *seq, uint8_t *qual, const uint16_t *cov, int n, const Lookup &lk, Work &w, uint8_t *ec0, uint8_t *ec1b, Result *res,
              Result ori)
{
	const int k = o.k;
	int ec_code = CODE_MISC, brute = 0, n_ec = 0, n_ec_high = 0, n_absent = 0, mh = 0, n_n = 0, start = 0, end = 0;
	Read r; r.seq = seq; r.qual = qual; r.cov = cov; r.n = n; r.brute_pos = r.brute_b = -1;
	for (int i = 0; i < n; ++i) n_n += base_at<RF>(seq, qual, i) > 3;
	if (n_n > n * .05) { ec_code = CODE_MANY_N; goto done; }
	{                                                          // bfc_ec_best_island (correct.c:119-130) on the coverage words
		int l = 0, mx = 0, mx_i = -1, i;
		for (i = k - 1; i < n; ++i) {
			if (!(cov[i] >> 12 & 1)) { if (l > mx) mx = l, mx_i = i; l = 0; }
			else ++l;
		}
		if (l > mx) mx = l, mx_i = i;
		if (mx > 0) start = mx_i - mx - k + 1, end = mx_i;
		else {                                                 // no solid k-mer: bfc_ec_first_kmer + bfc_ec_greedy_k (correct.c:63-94)
			int ec = -1;
			for (;;) {
				uint64_t x0 = 0, x1 = 0;
				int ll = 0;
				for (end = start; end < n; ++end) {
					const int c = base_at<RF>(seq, qual, end);
					if (c < 4) { kmer_append(k, x0, x1, c); if (++ll == k) break; }
					else ll = 0, x0 = x1 = 0;
				}
				if (end >= n) break;
				int mxo = 0, mx2 = 0;
				ec = -1;
				for (int d = 0; d < k; ++d) {
					const int cb = (int)((x1 >> d & 1) << 1 | (x0 >> d & 1));
					for (int j = 0; j < 4; ++j) {
						if (j == cb) continue;
						uint64_t y0 = x0, y1 = x1;
						kmer_change(y0, y1, d, j);
						const int t = occ(lk, k, y0, y1);
						if (t < 0) continue;
						if ((mxo & 0xff) < (t & 0xff)) mx2 = mxo, mxo = t, ec = d << 2 | j;
						else if ((mx2 & 0xff) < (t & 0xff)) mx2 = t;
					}
				}
				ec = (mxo & 0xff) * 3 > o.mode && (mx2 & 0xff) < 3 ? ec : -1;
				if (ec >= 0) break;
				if (end + (k >> 1) >= n) break;
				start = end - (k >> 1);
			}
			if (ec < 0) { ec_code = CODE_NO_SOLID; goto done; }
			r.brute_pos = end - (ec >> 2); r.brute_b = ec & 3;
			++end; start = end - k;
			brute = 1;
		}
	}
	{
		int rv0, rv1, mh0, mh1;
		if (ec1dir<RF>(o, r, 0, start, lk, w, ec0, &mh0, &rv0) != EC_OK) return EC_OVERFLOW;
		if (rv0 < 0) { ec_code = rv0 == -2 ? CODE_UNCORR_N : rv0 == -3 ? CODE_MANY_FAIL : CODE_MISC; goto done; }
		if (ec1dir<RF>(o, r, 1, n - end, lk, w, ec1b, &mh1, &rv1) != EC_OK) return EC_OVERFLOW;
		if (rv1 < 0) { ec_code = rv1 == -2 ? CODE_UNCORR_N : rv1 == -3 ? CODE_MANY_FAIL : CODE_MISC; goto done; }
		mh = mh0 > mh1 ? mh0 : mh1;
		ec_code = 0; n_absent = rv0 + rv1;
	}
	if (RF && (ori.aux & 7) == 0 && (uint32_t)(n_absent & 0x3fffff) > ori.aux2 >> 10) { // correct.c:438-442: the earlier stats stand
		res->aux = ori.aux; res->aux2 = (ori.aux2 & ~0x300u) | 2u << 8;
		return EC_OK;
	}
	for (int i = 0; i < n; ++i) {                              // merge the two directions, rewrite the read (position i is read before it is written)
		const Base c = ec_base<RF>(o, r, 0, i);
		const int e0 = ec0[i], t = ec1b[n - 1 - i], e1 = t < 4 ? 3 - t : 4;
		const int b = e0 == e1 ? (e0 > 3 ? c.b : e0) : e1 > 3 ? e0 : e0 > 3 ? e1 : c.ob;
		const int diff = b != c.ob;
		n_ec += diff; n_ec_high += diff && c.q;
		seq[i] = (uint8_t)(diff ? "acgtn"[b] : "ACGTN"[b]);
		if (qual) qual[i] = (uint8_t)(diff ? 34 + c.ob : "+?"[c.q]);
	}
done:
	res->aux = (uint32_t)(n_ec & 0x3fff) << 18 | (uint32_t)(n_ec_high & 0x3fff) << 4 | (uint32_t)brute << 3 | (uint32_t)ec_code;
	res->aux2 = (uint32_t)(n_absent & 0x3fffff) << 10 | (uint32_t)(mh & 0xff);
	if (RF) res->aux2 |= (ec_code == 0 ? 3u : 1u) << 8;        // rf_code: 3 after a correction (correct.c:470), else bfc_ec1's initial 1
	return EC_OK;
}

} // namespace ec1k
