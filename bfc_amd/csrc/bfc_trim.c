/* bfc_trim.c -- `bfc -1` trim pass behind the reference's own entry point
 *     void bfc_correct(const char *fn, const bfc_opt_t *opt, const void *ptr)        (bfc.h:40, correct.c:620)
 * for opt->filter_mode: per read, one bloom query per k-mer (max_streak, correct.c:478-497), keep the longest streak if
 * (streak + k) / length > min_frac (correct.c:557-569), print kept reads (correct.c:605-611).  The queries and the streak
 * scan run on the GPU (bfcg_trim_batch); the host parses and prints.
 *
 * An unmodified correct.c can never call a batched kernel, so this object provides `bfc_correct` itself; the reference's
 * corrector is linked under another name (compile correct.c with -Dbfc_correct=bfc_correct_cpu, source untouched, see
 * INTEGRATION.md) and is what this function forwards to when filter_mode is off -- unless BFC_GPU_EC=1 is set or bfc_correct_cpu is not
 * linked: then table-mode correction, `-R` included, runs on the GPU (correct_gpu below).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <ctype.h>
#include <unistd.h>
#include <sys/time.h>
#include <sys/resource.h>
#include "bfc_gpu.h"

extern double bfc_real_time __attribute__((weak));
extern int bfc_verbose __attribute__((weak));
void bfc_correct_cpu(const char *fn, const bfc_opt_t *opt, const void *ptr) __attribute__((weak));
void *bfcg_host_alloc(uint64_t bytes);
void bfcg_host_free(void *p);

static double t_real(void) { struct timeval tp; gettimeofday(&tp, 0); return tp.tv_sec + tp.tv_usec * 1e-6; }
static double t_cpu(void)
{
	struct rusage r; getrusage(RUSAGE_SELF, &r);
	return r.ru_utime.tv_sec + r.ru_stime.tv_sec + 1e-6 * (r.ru_utime.tv_usec + r.ru_stime.tv_usec);
}

#include "bfc_ingest.h"
#include <pthread.h>

int bfcg_env_devices(int *dev, int max); /* bfc_count.c: BFC_GPU_DEVICES */

/* the trim pass is embarrassingly parallel over reads: with several GPUs every batch's reads are dealt to them in
 * contiguous ranges, one host thread per device; each device holds the whole of bf_high (left there by bfc_count, or uploaded) */
typedef struct { bfcg_trim_t *tr; const uint8_t *seq; uint64_t n_pos; uint64_t *off; uint64_t n; float min_frac; int32_t *st, *en; int rc; char err[256]; } trim_job_t;
static void *trim_worker(void *p)
{
	trim_job_t *j = (trim_job_t*)p;
	j->rc = j->n ? bfcg_trim_batch(j->tr, j->seq, 0, j->n_pos, j->off, j->n, j->min_frac, j->st, j->en) : 0;
	if (j->rc != 0) { strncpy(j->err, bfcg_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; } /* the message is thread-local: it dies with this thread */
	return 0;
}

typedef struct { uint64_t off_hdr, off_cmt; int has_comment, has_qual; } rinfo_t; /* name and comment (as bseq_read copied them) in hdrs[] */

/* one batch as bseq_read makes it (bseq.c:52-76): records until chunk_size bases, max_reads reads or a full stream; names (and comments) go to
 * hdrs / ri, stream offsets to off[0..n].  The batch ends at the end of the input or at a malformed record; an empty batch is the last. */
static uint64_t read_batch(parser_t *ps, batch_t *b, uint64_t *off, uint64_t max_reads, rinfo_t *ri, char **hdrs, size_t *m_hdrs)
{
	uint64_t bases = 0, n = 0;
	size_t l_hdrs = 0;
	batch_clear(b);
	off[0] = 0;
	for (;;) {
		if (!ps->have_rec) {
			int rc = next_record(ps);
			if (rc <= 0) break;
			ps->have_rec = 1;
		}
		if (ps->l_seq + 1 > b->cap) { fprintf(stderr, "[E::%s] a read of %zu bases does not fit a GPU batch\n", "bfc_correct", ps->l_seq); abort(); }
		if (n == max_reads || !batch_put(b, ps->seq, ps->rec_has_qual ? ps->qual : 0, ps->l_seq)) break;
		ps->have_rec = 0;
		if (l_hdrs + ps->l_hdr + ps->l_cmt + 2 > *m_hdrs) { *m_hdrs = (l_hdrs + ps->l_hdr + ps->l_cmt + 2) * 2; *hdrs = (char*)realloc(*hdrs, *m_hdrs); }
		memcpy(*hdrs + l_hdrs, ps->hdr, ps->l_hdr + 1);
		ri[n].off_hdr = l_hdrs; l_hdrs += ps->l_hdr + 1;
		ri[n].has_comment = ps->have_cmt; ri[n].has_qual = ps->rec_has_qual; ri[n].off_cmt = l_hdrs;
		if (ps->have_cmt) { memcpy(*hdrs + l_hdrs, ps->cmt, ps->l_cmt + 1); l_hdrs += ps->l_cmt + 1; } /* bseq.c:64: whatever kseq's comment buffer holds now */
		off[++n] = b->n_pos;
		bases += ps->l_seq;
		if (bases >= ps->chunk_size) break;
	}
	return n;
}

/* worker_ec's test and parse_stats (correct.c:517-531, 542-543) with ecstat_t's bit-fields (correct.c:144-147) as masks, packed as
 * worker_ec packs a result (correct.c:552-553).  Where the reference's strtol(p + 1, ...) would step over the comment's NUL, the fields
 * left are 0. */
int bfcg_ec_parse_stats(const char *comment, uint32_t *aux, uint32_t *aux2)
{
	long v[6] = {0, 0, 0, 0, 0, 0}; /* ec_code, n_absent, max_heap, brute, n_ec, n_ec_high: the order of the ec:Z: tag */
	char *p;
	int i;
	if (!comment || strncmp(comment, "ec:Z:", 5) != 0) return 0;
	v[0] = strtol(comment + 5, &p, 10);
	if (((uint32_t)v[0] & 7) == 0)
		for (i = 1; i < 6 && *p; ++i) v[i] = strtol(p + 1, &p, 10);
	*aux = ((uint32_t)v[4] & 0x3fff) << 18 | ((uint32_t)v[5] & 0x3fff) << 4 | ((uint32_t)v[3] & 1) << 3 | ((uint32_t)v[0] & 7);
	*aux2 = ((uint32_t)v[1] & 0x3fffff) << 10 | 1u << 8 | ((uint32_t)v[2] & 0xff); /* rf_code 1 */
	return 1;
}

/* Error correction of table mode on the GPU (bfcg_ec_*): bfc_ec_cb's pipeline (correct.c:575-612) batch by batch -- parse as
 * bseq_read(..., keep_comment = 0, ...) does, correct every read (bfc_ec1 through worker_ec, correct.c:532-553), print.  With several
 * devices (BFC_GPU_DEVICES) each batch's reads are dealt to them as in the trim pass, one host thread per device.
 * With refine_ec (`-R`) comments are kept (correct.c:578) and worker_ec's first step runs here on the host, read by read in stream order
 * (what `-t1` does): a comment that starts with ec:Z: becomes the stats the following reads are held to (ori_st, carried across batches),
 * and its read is printed as it came if they say ec_code 0 and max_heap < 50.  The others go to the GPU as a batch of their own, so the
 * coverage pass sees only reads that are corrected. */
typedef struct { bfcg_ec_t *e; uint8_t *seq, *qual; uint64_t n_pos; uint64_t *off; uint64_t n; const uint32_t *oaux, *oaux2; uint32_t *aux, *aux2; int rc; char err[256]; } ec_job_t;
static int ec_run(bfcg_ec_t *e, uint8_t *seq, uint8_t *qual, uint64_t n_pos, uint64_t *off, uint64_t n, const uint32_t *oaux, const uint32_t *oaux2,
                  uint32_t *aux, uint32_t *aux2)
{
	return oaux ? bfcg_ec_batch_refine(e, seq, qual, n_pos, off, n, oaux, oaux2, aux, aux2) : bfcg_ec_batch(e, seq, qual, n_pos, off, n, aux, aux2);
}
static void *ec_worker(void *p)
{
	ec_job_t *j = (ec_job_t*)p;
	j->rc = j->n ? ec_run(j->e, j->seq, j->qual, j->n_pos, j->off, j->n, j->oaux, j->oaux2, j->aux, j->aux2) : 0;
	if (j->rc != 0) { strncpy(j->err, bfcg_last_error(), sizeof(j->err) - 1); j->err[sizeof(j->err) - 1] = 0; }
	return 0;
}

/* one batch (n reads, off[0] = 0) corrected: by the host instance where records without a quality string meet q > 93 (below), else on the
 * GPU(s).  ri[idx[r]] (ri[r] without idx) describes read r; oaux / oaux2: NULL, or the reads' earlier stats (refinement) */
typedef struct {
	const bfc_opt_t *opt;
	const bfc_ch_t *ch;
	bfcg_ec_t *ecs[64];
	int devs[64], n_dev;
	uint64_t *off2;
	double gpu_ms;
	uint64_t n_host;
} ec_devs_t;
static void ec_correct(ec_devs_t *g, uint8_t *seq, uint8_t *qual, int has_qual, int any_noq, uint64_t n_pos, uint64_t *off, uint64_t n,
                       const rinfo_t *ri, const uint64_t *idx, const uint32_t *oaux, const uint32_t *oaux2, uint32_t *aux, uint32_t *aux2)
{
	const bfc_opt_t *opt = g->opt;
	uint64_t r;
	int d;
	/* a record without a quality string has '~' in the stream (batch_put): q = (93 >= opt->q), which is what no quality string means
	 * (correct.c:32) unless q > 93 -- then a batch that mixes both kinds of record takes the host instance, read by read */
	uint8_t *q_all = has_qual ? qual : 0;
	if (n == 0) return;
	if (q_all && any_noq && opt->q > 93) {
		uint64_t hist[256], high[64];
		const int mode = bfc_ch_hist(g->ch, hist, high);
		for (r = 0; r < n; ++r) {
			uint8_t *s = seq + off[r], *q = qual + off[r];
			const uint64_t l = off[r + 1] - off[r] - 1;
			const uint8_t sep_s = s[l], sep_q = q[l];
			char *rq = ri[idx ? idx[r] : r].has_qual ? (char*)q : 0;
			s[l] = 0; q[l] = 0;
			if (oaux) bfcg_ec1_host_refine(g->ch, opt, mode, (char*)s, rq, oaux[r], oaux2[r], &aux[r], &aux2[r]);
			else bfcg_ec1_host(g->ch, opt, mode, (char*)s, rq, &aux[r], &aux2[r]);
			s[l] = sep_s; q[l] = sep_q;
		}
		g->n_host += n;
	} else if (g->n_dev == 1) {
		if (ec_run(g->ecs[0], seq, q_all, n_pos, off, n, oaux, oaux2, aux, aux2) != 0) {
			fprintf(stderr, "[E::%s] GPU error correction failed: %s\n", "bfc_correct", bfcg_last_error()); abort();
		}
		g->gpu_ms += bfcg_ec_last_ms(g->ecs[0]);
	} else { /* as the trim pass: device d takes the reads up to the boundary nearest to d+1 N-ths of the batch's positions */
		ec_job_t job[64];
		pthread_t th[64];
		uint64_t o2 = 0, r1 = 0;
		for (d = 0; d < g->n_dev; ++d) {
			const uint64_t r0 = r1, want = d + 1 == g->n_dev ? n_pos : n_pos / (uint64_t)g->n_dev * (uint64_t)(d + 1);
			uint64_t q;
			if (d + 1 == g->n_dev) r1 = n;
			else {
				uint64_t lo = r0, hi = n;
				while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] < want) lo = mid + 1; else hi = mid; }
				r1 = lo;
				if (r1 > r0 && off[r1] - want > want - off[r1 - 1]) --r1;
			}
			job[d].e = g->ecs[d]; job[d].seq = seq + off[r0]; job[d].qual = q_all ? q_all + off[r0] : 0; job[d].n_pos = off[r1] - off[r0];
			job[d].n = r1 - r0; job[d].off = g->off2 + o2; job[d].aux = aux + r0; job[d].aux2 = aux2 + r0; job[d].rc = 0;
			job[d].oaux = oaux ? oaux + r0 : 0; job[d].oaux2 = oaux2 ? oaux2 + r0 : 0;
			for (q = r0; q <= r1; ++q) g->off2[o2++] = off[q] - off[r0];
			pthread_create(&th[d], 0, ec_worker, &job[d]);
		}
		for (d = 0; d < g->n_dev; ++d) {
			pthread_join(th[d], 0);
			if (job[d].rc != 0) { fprintf(stderr, "[E::%s] GPU error correction failed on device %d: %s\n", "bfc_correct", g->devs[d], job[d].err); abort(); }
		}
	}
}

static void correct_gpu(const char *fn, const bfc_opt_t *opt, const bfc_ch_t *ch)
{
	parser_t ps;
	batch_t b;
	ec_devs_t g;
	int d, empties = 0;
	int n_adopted = 0;
	uint64_t cap, max_reads, *off, n_total = 0, n_refined = 0, n_kept = 0;
	uint32_t *aux, *aux2;
	rinfo_t *ri;
	char *hdrs = 0; size_t m_hdrs = 0;
	const char *env;
	double t0 = (&bfc_real_time && bfc_real_time > 0.) ? bfc_real_time : t_real();
	/* refinement: the sub-batch of the reads to correct (stream, offsets, their reads in the batch, earlier stats, results), kept reads */
	uint8_t *r_seq = 0, *r_qual = 0, *kept = 0;
	uint64_t *r_off = 0, *r_idx = 0;
	uint32_t *r_oaux = 0, *r_oaux2 = 0, *r_aux = 0, *r_aux2 = 0, ori_aux = 0, ori_aux2 = 0; /* ori_st: calloc'd (correct.c:185) */

	if (!(&bfc_verbose) || bfc_verbose >= 3)
		fprintf(stderr, "[M::%s @%.1f*%.1f%%] Starting...\n", "bfc_correct", t_real() - t0, 100. * t_cpu() / (t_real() - t0 + 1e-6));
	memset(&g, 0, sizeof(g));
	g.opt = opt; g.ch = ch;
	cap = (uint64_t)(opt->chunk_size > 0 ? opt->chunk_size : 100000000);
	if ((env = getenv("BFC_GPU_BATCH")) != 0) cap = strtoull(env, 0, 10);
	if (cap < (1u << 16)) cap = 1u << 16;
	cap += cap / 64 + (1u << 20);
	max_reads = cap / 16 + 1024;
	g.n_dev = bfcg_env_devices(g.devs, 64);
	if (g.n_dev == 0) { g.n_dev = 1; g.devs[0] = (env = getenv("BFC_GPU_DEVICE")) ? atoi(env) : 0; }
	for (d = 0; d < g.n_dev; ++d) { /* a device's share of a batch: 1/N of its positions (cut at the nearest read boundary), up to all of its reads */
		g.ecs[d] = bfcg_ec_create(ch, opt, g.devs[d], g.n_dev > 1 ? cap / (uint64_t)g.n_dev + cap / 64 + (1u << 16) : cap, max_reads);
		if (!g.ecs[d]) { fprintf(stderr, "[E::%s] cannot set up error correction on the GPU: %s\n", "bfc_correct", bfcg_last_error()); abort(); }
		n_adopted += bfcg_ec_adopted(g.ecs[d]); /* the copy bfc_count left in HBM (bfcg_export_table_resident): the first corrector on its device takes it */
	}
	if (g.n_dev > 1) g.off2 = (uint64_t*)malloc((max_reads + 1 + (uint64_t)g.n_dev) * 8);

	memset(&ps, 0, sizeof(ps));
	ps.keep_hdr = 1;
	ps.chunk_size = (uint64_t)(opt->chunk_size > 0 ? opt->chunk_size : 100000000);
	if (ps.chunk_size > cap - cap / 32) ps.chunk_size = cap - cap / 32;
	ps.rd.fp = fn && strcmp(fn, "-") ? gzopen(fn, "r") : gzdopen(fileno(stdin), "r");
	if (ps.rd.fp == 0) { fprintf(stderr, "[E::%s] cannot open '%s'\n", "bfc_correct", fn ? fn : "-"); abort(); }
	ps.rd.buf = (uint8_t*)malloc(RD_BUF);
	memset(&b, 0, sizeof(b));
	b.cap = cap;
	b.seq = (uint8_t*)bfcg_host_alloc(cap); b.qual = (uint8_t*)bfcg_host_alloc(cap);
	off = (uint64_t*)malloc((max_reads + 1) * 8); aux = (uint32_t*)malloc(max_reads * 4); aux2 = (uint32_t*)malloc(max_reads * 4);
	ri = (rinfo_t*)malloc(max_reads * sizeof(rinfo_t));
	if (!b.seq || !b.qual || !off || !aux || !aux2 || !ri) { fprintf(stderr, "[E::%s] out of memory\n", "bfc_correct"); abort(); }
	if (opt->refine_ec) {
		r_seq = (uint8_t*)bfcg_host_alloc(cap); r_qual = (uint8_t*)bfcg_host_alloc(cap); kept = (uint8_t*)malloc(max_reads);
		r_off = (uint64_t*)malloc((max_reads + 1) * 8); r_idx = (uint64_t*)malloc(max_reads * 8);
		r_oaux = (uint32_t*)malloc(max_reads * 4); r_oaux2 = (uint32_t*)malloc(max_reads * 4);
		r_aux = (uint32_t*)malloc(max_reads * 4); r_aux2 = (uint32_t*)malloc(max_reads * 4);
		if (!r_seq || !r_qual || !kept || !r_off || !r_idx || !r_oaux || !r_oaux2 || !r_aux || !r_aux2) { fprintf(stderr, "[E::%s] out of memory\n", "bfc_correct"); abort(); }
	}

	for (;;) { /* one batch: parse (keep_comment = refine_ec, correct.c:578-580), correct on the GPU, print */
		uint64_t r, n = read_batch(&ps, &b, off, max_reads, ri, &hdrs, &m_hdrs);
		int last = 0;
		fprintf(stderr, "[M::%s] read %d sequences\n", "bfc_ec_cb", (int)n);
		if (n == 0 && ++empties >= (opt->no_mt_io ? 1 : 2)) last = 1;
		if (n) {
			if (!opt->refine_ec) ec_correct(&g, b.seq, b.qual, b.has_qual, b.n_noq > 0, b.n_pos, off, n, ri, 0, 0, 0, aux, aux2);
			else {
				uint64_t m = 0, any_noq = 0;
				r_off[0] = 0;
				for (r = 0; r < n; ++r) { /* worker_ec, correct.c:542-550 */
					const uint64_t l = off[r + 1] - off[r];
					uint32_t a, a2;
					kept[r] = 0;
					if (ri[r].has_comment && bfcg_ec_parse_stats(hdrs + ri[r].off_cmt, &a, &a2)) {
						ori_aux = a; ori_aux2 = a2;
						if ((a & 7) == 0 && (a2 & 0xff) < 50) { kept[r] = 1; aux[r] = aux2[r] = 0; continue; }
					}
					memcpy(r_seq + r_off[m], b.seq + off[r], l); memcpy(r_qual + r_off[m], b.qual + off[r], l);
					r_idx[m] = r; r_oaux[m] = ori_aux; r_oaux2[m] = ori_aux2; any_noq |= !ri[r].has_qual;
					r_off[m + 1] = r_off[m] + l; ++m;
				}
				ec_correct(&g, r_seq, r_qual, b.has_qual, any_noq != 0, r_off[m], r_off, m, ri, r_idx, r_oaux, r_oaux2, r_aux, r_aux2);
				for (r = 0; r < m; ++r) { /* the results back into the batch */
					const uint64_t i = r_idx[r], l = off[i + 1] - off[i] - 1;
					memcpy(b.seq + off[i], r_seq + r_off[r], l); memcpy(b.qual + off[i], r_qual + r_off[r], l);
					aux[i] = r_aux[r]; aux2[i] = r_aux2[r];
				}
				n_refined += m; n_kept += n - m;
			}
			fprintf(stderr, "[M::%s @%.1f*%.1f%%] processed %d sequences\n", "bfc_ec_cb", t_real() - t0, 100. * t_cpu() / (t_real() - t0 + 1e-6), (int)n);
			for (r = 0; r < n; ++r) { /* correct.c:595-604, 609-611 */
				const int is_fq = ri[r].has_qual && !opt->no_qual;
				const uint64_t l = off[r + 1] - off[r] - 1;
				if (opt->discard && (aux[r] & 7)) continue;
				putchar(is_fq ? '@' : '>');
				fputs(hdrs + ri[r].off_hdr, stdout);
				if (kept && kept[r]) { putchar('\t'); fputs(hdrs + ri[r].off_cmt, stdout); } /* the comment worker_ec left (correct.c:604) */
				else {
					printf("\tec:Z:%d", aux[r] & 7);
					if ((aux[r] & 7) == 0)
						printf("_%d:%d_%d_%d:%d_%d", aux2[r] >> 10, aux2[r] & 0xff, aux[r] >> 3 & 1, aux[r] >> 18 & 0x3fff, aux[r] >> 4 & 0x3fff, aux2[r] >> 8 & 3);
				}
				putchar('\n');
				fwrite(b.seq + off[r], 1, (size_t)l, stdout); putchar('\n');
				if (is_fq) { puts("+"); fwrite(b.qual + off[r], 1, (size_t)l, stdout); putchar('\n'); }
			}
			n_total += n;
		}
		if (last) break;
	}
	for (d = 0; d < g.n_dev; ++d) { g.n_host += bfcg_ec_host_reads(g.ecs[d]); bfcg_ec_destroy(g.ecs[d]); }
	fprintf(stderr, "[M::%s] error correction ran on the GPU (%d device(s), %.1f ms of kernels): %llu reads, %llu of them by the host fallback",
	        "bfc_correct", g.n_dev, g.gpu_ms, (unsigned long long)n_total, (unsigned long long)g.n_host);
	if (opt->refine_ec) fprintf(stderr, "; -R: %llu reads refined, %llu skipped", (unsigned long long)n_refined, (unsigned long long)n_kept);
	if (n_adopted == g.n_dev) fprintf(stderr, "; count table found in HBM");
	else if (n_adopted == 0) fprintf(stderr, "; count table uploaded");
	else fprintf(stderr, "; count table found in HBM by %d corrector(s), uploaded by %d", n_adopted, g.n_dev - n_adopted);
	fputc('\n', stderr);
	free(g.off2);
	gzclose(ps.rd.fp);
	free(ps.rd.buf); free(ps.rd.line); free(ps.seq); free(ps.qual); free(ps.hdr); free(ps.cmt);
	bfcg_host_free(b.seq); bfcg_host_free(b.qual); free(b.kind_cut); free(off); free(aux); free(aux2); free(ri); free(hdrs);
	if (r_seq) bfcg_host_free(r_seq);
	if (r_qual) bfcg_host_free(r_qual);
	free(kept); free(r_off); free(r_idx); free(r_oaux); free(r_oaux2); free(r_aux); free(r_aux2);
}

void bfc_correct(const char *fn, const bfc_opt_t *opt, const void *ptr)
{
	const bfc_bf_t *bf = (const bfc_bf_t*)ptr;
	parser_t ps;
	batch_t b;
	bfcg_trim_t *tr, *trs[64];
	int devs[64], n_dev, d;
	uint64_t cap, max_reads, *off, *off2 = 0;
	int32_t *st, *en;
	rinfo_t *ri;
	char *hdrs = 0; size_t m_hdrs = 0;
	const char *env;
	double t0 = (&bfc_real_time && bfc_real_time > 0.) ? bfc_real_time : t_real();

	if (!opt->filter_mode) {
		if (((env = getenv("BFC_GPU_EC")) != 0 && strcmp(env, "1") == 0) || !bfc_correct_cpu) correct_gpu(fn, opt, (const bfc_ch_t*)ptr);
		else bfc_correct_cpu(fn, opt, ptr);
		return;
	}
	if (!(&bfc_verbose) || bfc_verbose >= 3)
		fprintf(stderr, "[M::%s @%.1f*%.1f%%] Starting...\n", __func__, t_real() - t0, 100. * t_cpu() / (t_real() - t0 + 1e-6));
	cap = (uint64_t)(opt->chunk_size > 0 ? opt->chunk_size : 100000000);
	if ((env = getenv("BFC_GPU_BATCH")) != 0) cap = strtoull(env, 0, 10);
	if (cap < (1u << 16)) cap = 1u << 16;
	cap += cap / 64 + (1u << 20);
	max_reads = cap / 16 + 1024;
	n_dev = bfcg_env_devices(devs, 64);
	if (n_dev == 0) { n_dev = 1; devs[0] = (env = getenv("BFC_GPU_DEVICE")) ? atoi(env) : 0; }
	for (d = 0; d < n_dev; ++d) {
		int dup = 0, j;
		for (j = 0; j < d; ++j) if (devs[j] == devs[d]) dup = 1; /* a device named twice: its first context serves both shares' turns */
		(void)dup;
		/* a device's share of a batch: 1/N of its positions (cut at the nearest read boundary) -- and up to all of its reads, if they are short there */
		trs[d] = bfcg_trim_create(opt->k, bf, devs[d], n_dev > 1 ? cap / (uint64_t)n_dev + cap / 64 + (1u << 16) : cap, max_reads);
		if (!trs[d]) { fprintf(stderr, "[E::%s] cannot set up the GPU trim pass: %s\n", __func__, bfcg_last_error()); abort(); }
	}
	tr = trs[0];
	if (n_dev > 1) off2 = (uint64_t*)malloc((max_reads + 1 + (uint64_t)n_dev) * 8);

	memset(&ps, 0, sizeof(ps));
	ps.keep_hdr = 1;
	ps.chunk_size = (uint64_t)(opt->chunk_size > 0 ? opt->chunk_size : 100000000);
	if (ps.chunk_size > cap - cap / 32) ps.chunk_size = cap - cap / 32;
	ps.rd.fp = fn && strcmp(fn, "-") ? gzopen(fn, "r") : gzdopen(fileno(stdin), "r");
	if (ps.rd.fp == 0) { fprintf(stderr, "[E::%s] cannot open '%s'\n", __func__, fn ? fn : "-"); abort(); }
	/* (no gzbuffer: zlib is asked for kseq's own 16 KiB pieces through its default buffers, so that a damaged gzip file ends where it ends for
	 * the reference -- rd_fill in bfc_ingest.h) */
	ps.rd.buf = (uint8_t*)malloc(RD_BUF);
	memset(&b, 0, sizeof(b));
	b.cap = cap;
	b.seq = (uint8_t*)bfcg_host_alloc(cap); b.qual = (uint8_t*)malloc(cap);
	off = (uint64_t*)malloc((max_reads + 1) * 8); st = (int32_t*)malloc(max_reads * 4); en = (int32_t*)malloc(max_reads * 4);
	ri = (rinfo_t*)malloc(max_reads * sizeof(rinfo_t));
	if (!b.seq || !b.qual || !off || !st || !en || !ri) { fprintf(stderr, "[E::%s] out of memory\n", __func__); abort(); }

	int empties = 0;
	for (;;) { /* one batch: parse (keeping headers), trim on the GPU, print */
		uint64_t r, n;
		int last = 0;
		n = read_batch(&ps, &b, off, max_reads, ri, &hdrs, &m_hdrs);
		fprintf(stderr, "[M::%s] read %d sequences\n", "bfc_ec_cb", (int)n); /* correct.c:582, once per bseq_read call */
		if (n == 0 && ++empties >= (opt->no_mt_io ? 1 : 2)) last = 1; /* each of the pipeline's workers ends on its own empty batch (kthread.c:88-106, correct.c:644) */
		if (n) {
			if (n_dev == 1) {
				if (bfcg_trim_batch(tr, b.seq, 0, b.n_pos, off, n, opt->min_frac, st, en) != 0) {
					fprintf(stderr, "[E::%s] GPU trim pass failed: %s\n", __func__, bfcg_last_error()); abort();
				}
			} else { /* device d takes the reads up to the boundary nearest to d+1 N-ths of the batch's POSITIONS (the contexts are sized by positions:
			          * dealt by read count, a batch of reads sorted by length would overflow one of them): their part of the stream, offsets rebased */
				trim_job_t job[64];
				pthread_t th[64];
				uint64_t o2 = 0, r1 = 0;
				for (d = 0; d < n_dev; ++d) {
					const uint64_t r0 = r1, want = d + 1 == n_dev ? b.n_pos : b.n_pos / (uint64_t)n_dev * (uint64_t)(d + 1);
					uint64_t q;
					if (d + 1 == n_dev) r1 = n;
					else { /* first boundary at or behind `want` (off[] ascends), or the one before it if that is nearer */
						uint64_t lo = r0, hi = n;
						while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (off[mid] < want) lo = mid + 1; else hi = mid; }
						r1 = lo;
						if (r1 > r0 && off[r1] - want > want - off[r1 - 1]) --r1;
					}
					job[d].tr = trs[d]; job[d].seq = b.seq + off[r0]; job[d].n_pos = off[r1] - off[r0]; job[d].n = r1 - r0;
					job[d].off = off2 + o2; job[d].min_frac = opt->min_frac; job[d].st = st + r0; job[d].en = en + r0; job[d].rc = 0;
					for (q = r0; q <= r1; ++q) off2[o2++] = off[q] - off[r0];
					pthread_create(&th[d], 0, trim_worker, &job[d]);
				}
				for (d = 0; d < n_dev; ++d) {
					pthread_join(th[d], 0);
					if (job[d].rc != 0) { fprintf(stderr, "[E::%s] GPU trim pass failed on device %d: %s\n", __func__, devs[d], job[d].err); abort(); }
				}
			}
			fprintf(stderr, "[M::%s @%.1f*%.1f%%] processed %d sequences\n", "bfc_ec_cb", t_real() - t0, 100. * t_cpu() / (t_real() - t0 + 1e-6), (int)n);
			for (r = 0; r < n; ++r) { /* correct.c:595-611 */
				char *h = hdrs + ri[r].off_hdr;
				int is_fq = ri[r].has_qual && !opt->no_qual;
				if (st[r] < 0) continue;
				putchar(is_fq ? '@' : '>');
				fputs(h, stdout);
				if (ri[r].has_comment) { putchar('\t'); fputs(hdrs + ri[r].off_cmt, stdout); }
				putchar('\n');
				fwrite(b.seq + off[r] + st[r], 1, (size_t)(en[r] - st[r]), stdout); putchar('\n');
				if (is_fq) { puts("+"); fwrite(b.qual + off[r] + st[r], 1, (size_t)(en[r] - st[r]), stdout); putchar('\n'); }
			}
		}
		if (last) break;
	}
	for (d = 0; d < n_dev; ++d) bfcg_trim_destroy(trs[d]);
	free(off2);
	gzclose(ps.rd.fp);
	free(ps.rd.buf); free(ps.rd.line); free(ps.seq); free(ps.qual); free(ps.hdr); free(ps.cmt);
	bfcg_host_free(b.seq); free(b.qual); free(b.kind_cut); free(off); free(st); free(en); free(ri); free(hdrs);
}
