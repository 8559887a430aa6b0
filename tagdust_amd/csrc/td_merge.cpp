// td_merge.cpp -- include/tagdust_merge.h without the kernel: the pow() / log() tables, the host path (a restatement of
// overlap_reads(), src/merge.c:399-688, over those tables), one batch on either path, and the command line of `tagdust-merge`.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <vector>

#include "td_merge_internal.h"

namespace {
thread_local std::string g_merge_error;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}

void td_merge_set_error(const std::string& msg) { g_merge_error = msg; }
extern "C" const char* td_merge_last_error(void) { return g_merge_error.c_str(); }

extern "C" void td_merge_opts_default(td_merge_opts* o)
{
	if (!o) return;
	memset(o, 0, sizeof *o);
	o->min_overlap = 16;       // interface.c: minlen
	o->threshold = 0.0f;
	o->n_threads = 0;
	o->batch_pairs = 0;
	o->device = 0;
	o->table_placement = TD_MERGE_TABLE_AUTO;
}

// ---- the tables ----
td_merge_tables* td_merge_tables_from_set(const bool* present)
{
	td_merge_tables* t = (td_merge_tables*)calloc(1, sizeof(td_merge_tables));
	if (!t) return nullptr;
	for (int c = 0; c < 256; c++) t->qindex[c] = -1;
	for (int c = 0; c < 256; c++)
		if (present[c]) { t->qindex[c] = (int16_t)t->nq; t->qchar[t->nq++] = (uint8_t)c; }
	if (t->nq == 0) { t->qindex['I'] = 0; t->qchar[0] = 'I'; t->nq = 1; }     // (a batch without a base: any table will do)
	const int nq = t->nq, dim = 5 * nq;
	t->dim = dim;
	t->profile = (float*)malloc(sizeof(float) * 2 * (size_t)nq);
	t->T = (float*)malloc(sizeof(float) * (size_t)dim * (size_t)dim);
	if (!t->profile || !t->T) { td_merge_tables_free(t); return nullptr; }
	for (int q = 0; q < nq; q++) {
		// merge.c:428: the quality is a (signed) char
		float score = 1.0 - pow(10.0, -((int)(signed char)t->qchar[q] - 33) / 10.0);
		t->profile[2 * q] = score;
		t->profile[2 * q + 1] = (1.0 - score) / 3.0;                         // merge.c:444, with the float score
	}
	std::vector<float> prof((size_t)dim * 4);
	for (int q = 0; q < nq; q++)
		for (int x = 0; x < 5; x++)
			for (int c = 0; c < 4; c++)
				prof[(size_t)(5 * q + x) * 4 + (size_t)c] = x > 3 ? 0.25f : (c == x ? t->profile[2 * q] : t->profile[2 * q + 1]);
	for (int a = 0; a < dim; a++)
		for (int b = 0; b < dim; b++) {
			float sum = 0.0f;
			for (int c = 0; c < 4; c++) sum += prof[(size_t)a * 4 + (size_t)c] * prof[(size_t)b * 4 + (size_t)c];   // merge.c:492-495 (no FMA: -ffp-contract=off)
			t->T[(size_t)a * (size_t)dim + (size_t)b] = sum == 0.0f ? -INFINITY : (float)log((double)sum);   // misc.c:85-92
		}
	return t;
}

extern "C" int td_merge_tables_build(const uint8_t* qual, int64_t n, td_merge_tables** out)
{
	if (!out || (n > 0 && !qual)) { td_merge_set_error("td_merge_tables_build: bad arguments"); return TD_FAIL; }
	bool present[256] = { false };
	for (int64_t i = 0; i < n; i++) present[qual[i]] = true;
	*out = td_merge_tables_from_set(present);
	if (!*out) { td_merge_set_error("td_merge_tables_build: out of memory"); return TD_FAIL; }
	return TD_OK;
}

extern "C" void td_merge_tables_free(td_merge_tables* t)
{
	if (!t) return;
	free(t->profile);
	free(t->T);
	free(t);
}

// ---- overlap_reads() for one pair ----
void td_merge_pair_host(const TdMergeView& v, int64_t p, const td_merge_tables& t, int min_overlap, float threshold,
                        td_merge_record* rec, char* seq, char* qual)
{
	const int64_t o1 = v.offs1[p], o2 = v.offs2[p];
	const int len_f = (int)(v.offs1[p + 1] - o1), len_r = (int)(v.offs2[p + 1] - o2);
	const int dim = t.dim;
	// one number per base: 5 q + x; read 2 reverse-complemented, its qualities reversed (merge.c:314-315)
	std::vector<uint16_t> buf((size_t)len_f + (size_t)len_r + 1);
	uint16_t* ef = buf.data();
	uint16_t* er = ef + len_f;
	for (int i = 0; i < len_f; i++) ef[i] = (uint16_t)(5 * t.qindex[v.qual1[o1 + i]] + v.codes1[o1 + i]);
	for (int j = 0; j < len_r; j++) {
		const int64_t s = o2 + (len_r - 1 - j);
		er[j] = (uint16_t)(5 * t.qindex[v.qual2[s]] + td_merge_rc(v.codes2[s]));
	}
	float max_score = -INFINITY;
	int best_d = -1, d = 0;
	for (int i = 0; i < len_f; i++, d++) {                              // merge.c:480-516
		if (!(len_f - i > min_overlap && len_r > min_overlap)) continue;
		float score = 0.0f;
		const int n = std::min(len_f - i, len_r);
		for (int k = 0; k < n; k++) score = score + t.T[(size_t)ef[i + k] * (size_t)dim + er[k]];
		if (td_merge_better(score, d, max_score, best_d)) { max_score = score; best_d = d; }
	}
	for (int j = 0; j < len_r; j++, d++) {                              // merge.c:517-558
		if (!(len_f > min_overlap && len_r - j > min_overlap)) continue;
		float score = 0.0f;
		const int n = std::min(len_f, len_r - j);
		for (int k = 0; k < n; k++) score = score + t.T[(size_t)ef[k] * (size_t)dim + er[j + k]];
		if (td_merge_better(score, d, max_score, best_d)) { max_score = score; best_d = d; }
	}
	rec->best_d = best_d;
	if (best_d < 0) { rec->out_len = 0; rec->id = 0; rec->aligned = 0; rec->status = TD_MERGE_NO_CANDIDATE; return; }
	// the consensus, merge.c:561-676
	static const char letter[] = "ACGTC";
	const int i0 = best_d < len_f ? best_d : 0, j0 = best_d < len_f ? 0 : best_d - len_f;
	int o = 0, id = 0;
	auto plain = [&](uint16_t e) { seq[o] = letter[e % 5]; qual[o] = (char)t.qchar[e / 5]; o++; };
	for (int i = 0; i < i0; i++) plain(ef[i]);
	for (int j = 0; j < j0; j++) plain(er[j]);
	const int aligned = std::min(len_f - i0, len_r - j0);
	for (int k = 0; k < aligned; k++) {
		const int xf = ef[i0 + k] % 5, qf = ef[i0 + k] / 5, xr = er[j0 + k] % 5, qr = er[j0 + k] / 5;
		if (xf == xr) { seq[o] = letter[xf]; id++; }
		else seq[o] = letter[td_merge_pick(t.profile, qf, xf, qr, xr)];
		qual[o] = (char)t.qchar[qf > qr ? qf : qr];                      // (the characters are numbered in ascending order)
		o++;
	}
	for (int i = i0 + aligned; i < len_f; i++) plain(ef[i]);
	for (int j = j0 + aligned; j < len_r; j++) plain(er[j]);
	rec->id = id;
	rec->aligned = aligned;
	const bool pass = td_merge_passes(id, aligned, threshold);
	rec->out_len = pass ? o : 0;
	rec->status = pass ? TD_MERGE_WRITTEN : TD_MERGE_BELOW;
}

// ---- one batch ----
namespace {
// task(k) for k in [0, n): on the pool of the stream that owns one for its run, or (pool NULL: the one-batch entry) on n_threads
// threads made and joined here, the calling one included -- a pool made for one call's two sections measured 12 % behind this
void run_chunks(TdWorkers* pool, int n_threads, int64_t n, const std::function<void(int64_t)>& task)
{
	if (pool) { pool->run(n, task); return; }
	std::atomic<int64_t> next(0);
	auto work = [&] { for (int64_t k; (k = next.fetch_add(1)) < n;) task(k); };
	std::vector<std::thread> th;
	for (int t = 1; t < n_threads && t < n; t++) th.emplace_back(work);
	work();
	for (auto& t : th) t.join();
}

void scan_bytes(const uint8_t* codes, const uint8_t* qual, int64_t lo, int64_t hi, bool* present, bool& bad)
{
	for (int64_t i = lo; i < hi; i++) { present[qual[i]] = true; if (codes[i] > 4) bad = true; }
}
}

bool td_merge_batch(const TdMergeView& v, const td_merge_opts& o, TdMergeDevice* dev, TdWorkers* pool, td_merge_result* res, double* tables_s, std::string& err)
{
	memset(res, 0, sizeof *res);
	if (o.min_overlap < 0) { err = "td_merge: min_overlap must not be negative"; return false; }
	const int64_t n = v.n;
	const int64_t nb1 = n ? v.offs1[n] : 0, nb2 = n ? v.offs2[n] : 0;
	const int T = td_stage_threads(o.n_threads, 64);
	for (int64_t p = 0; p < n; p++)
		if (v.offs1[p + 1] - v.offs1[p] > (1 << 24) || v.offs2[p + 1] - v.offs2[p] > (1 << 24)) { err = "td_merge: a read of more than 2^24 bases"; return false; }
	// the quality characters of the batch, and the one base code the reference cannot reverse-complement
	const double t0 = now_s();
	bool present[256] = { false };
	{
		struct A { const TdMergeView* v; int64_t nb1; std::atomic<int> bad; std::atomic<uint64_t> bits[4]; } a{ &v, nb1, { 0 }, {} };
		for (auto& b : a.bits) b = 0;
		const int64_t nb = nb1 + nb2, chunk = (int64_t)1 << 20;
		run_chunks(pool, T, (nb + chunk - 1) / chunk, [&](int64_t k) {
			const int64_t lo = k * chunk, hi = std::min(nb, (k + 1) * chunk);
			bool pr[256] = { false }, bad = false;
			if (lo < a.nb1) scan_bytes(a.v->codes1, a.v->qual1, lo, std::min(hi, a.nb1), pr, bad);
			if (hi > a.nb1) scan_bytes(a.v->codes2, a.v->qual2, std::max(lo, a.nb1) - a.nb1, hi - a.nb1, pr, bad);
			if (bad) a.bad = 1;
			for (int w = 0; w < 4; w++) {
				uint64_t m = 0;
				for (int b = 0; b < 64; b++) if (pr[w * 64 + b]) m |= (uint64_t)1 << b;
				if (m) a.bits[w].fetch_or(m);
			}
		});
		if (a.bad) { err = "td_merge: a read holds '.' (base code 5), which the reference's reverse complement does not define"; return false; }
		for (int c = 0; c < 256; c++) present[c] = (a.bits[c / 64].load() >> (c % 64)) & 1;
	}
	td_merge_tables* t = td_merge_tables_from_set(present);
	if (!t) { err = "td_merge: out of memory"; return false; }
	if (tables_s) *tables_s += now_s() - t0;
	res->n_pairs = n;
	res->rec = (td_merge_record*)malloc(sizeof(td_merge_record) * (size_t)(n ? n : 1));
	res->out_off = (int64_t*)malloc(sizeof(int64_t) * (size_t)(n + 1));
	res->seq = (char*)malloc((size_t)(nb1 + nb2) + 1);
	res->qual = (char*)malloc((size_t)(nb1 + nb2) + 1);
	if (!res->rec || !res->out_off || !res->seq || !res->qual) { td_merge_tables_free(t); err = "td_merge: out of memory"; return false; }
	res->out_off[0] = 0;
	for (int64_t p = 0; p < n; p++) res->out_off[p + 1] = v.offs1[p + 1] + v.offs2[p + 1];
	bool ok = true;
	if (dev) ok = td_merge_device_run(dev, v, *t, o.min_overlap, o.threshold, o.table_placement, res->rec, res->seq, res->qual, &res->table_in_lds, &res->kernel_ms, err);
	if (ok) {
		run_chunks(pool, T, (n + 255) / 256, [&](int64_t k) {
			for (int64_t p = k * 256; p < std::min(n, (k + 1) * 256); p++) {
				const bool is_long = v.offs1[p + 1] - v.offs1[p] > TD_MERGE_STAGE_BASES || v.offs2[p + 1] - v.offs2[p] > TD_MERGE_STAGE_BASES;
				if (dev && !is_long) continue;
				td_merge_pair_host(v, p, *t, o.min_overlap, o.threshold, &res->rec[p], res->seq + res->out_off[p], res->qual + res->out_off[p]);
			}
		});
		for (int64_t p = 0; p < n; p++) {
			const int s = res->rec[p].status;
			if (s == TD_MERGE_WRITTEN) res->n_written++; else if (s == TD_MERGE_BELOW) res->n_below++; else res->n_too_short++;
			if (dev && (v.offs1[p + 1] - v.offs1[p] > TD_MERGE_STAGE_BASES || v.offs2[p + 1] - v.offs2[p] > TD_MERGE_STAGE_BASES)) res->n_on_host++;
		}
	}
	td_merge_tables_free(t);
	return ok;
}

extern "C" void td_merge_result_free(td_merge_result* r)
{
	if (!r) return;
	free(r->rec); free(r->out_off); free(r->seq); free(r->qual);
	free(r);
}

namespace {
// the quality bytes of a td_reads batch, contiguous under its offsets
bool pack_qual(const td_reads* r, std::vector<uint8_t>& q, std::string& err)
{
	q.resize((size_t)(r->n_reads ? r->offs[r->n_reads] : 0) + 1);
	for (int64_t i = 0; i < r->n_reads; i++) {
		if (r->qual_off[i] < 0) { err = "td_merge: FASTA input: the reads have no base qualities"; return false; }
		memcpy(q.data() + r->offs[i], r->text + r->qual_off[i], (size_t)(r->offs[i + 1] - r->offs[i]));
	}
	return true;
}

int merge_reads(const td_reads* r1, const td_reads* r2, const td_merge_opts* opts, bool device, td_merge_result** out)
{
	if (!r1 || !r2 || !out) { td_merge_set_error("td_merge: bad arguments"); return TD_FAIL; }
	td_merge_opts o;
	if (opts) o = *opts; else td_merge_opts_default(&o);
	if (r1->n_reads != r2->n_reads) { td_merge_set_error("td_merge: the two batches differ in their number of records"); return TD_FAIL; }
	std::string err;
	std::vector<uint8_t> q1, q2;
	if (!pack_qual(r1, q1, err) || !pack_qual(r2, q2, err)) { td_merge_set_error(err); return TD_FAIL; }
	TdMergeView v;
	v.n = r1->n_reads;
	v.codes1 = r1->codes; v.qual1 = q1.data(); v.offs1 = r1->offs;
	v.codes2 = r2->codes; v.qual2 = q2.data(); v.offs2 = r2->offs;
	TdMergeDevice* dev = nullptr;
	if (device) {
		dev = td_merge_device_open(o.device, err);
		if (!dev) { td_merge_set_error(err); return TD_FAIL; }
	}
	td_merge_result* res = (td_merge_result*)calloc(1, sizeof(td_merge_result));
	const bool ok = res && td_merge_batch(v, o, dev, nullptr, res, nullptr, err);
	if (dev) td_merge_device_close(dev);
	if (!ok) { td_merge_result_free(res); td_merge_set_error(res ? err : "td_merge: out of memory"); return TD_FAIL; }
	*out = res;
	return TD_OK;
}
}

extern "C" int td_merge_host(const td_reads* r1, const td_reads* r2, const td_merge_opts* opts, td_merge_result** out)
{
	return merge_reads(r1, r2, opts, false, out);
}

extern "C" int td_merge_device(const td_reads* r1, const td_reads* r2, const td_merge_opts* opts, td_merge_result** out)
{
	if (opts && opts->device < 0) { td_merge_set_error("td_merge_device: no device given (td_merge_host is the host path)"); return TD_FAIL; }
	return merge_reads(r1, r2, opts, true, out);
}

// ---- two files of any size ----
extern "C" int td_merge_stream(const char* in1, const char* in2, const char* out_path, const td_merge_opts* opts, td_merge_stats* stats)
{
	if (stats) memset(stats, 0, sizeof *stats);
	if (!in1 || !in2 || !out_path) { td_merge_set_error("td_merge_stream: two input files and an output path are needed"); return TD_FAIL; }
	td_merge_opts mo;
	if (opts) mo = *opts; else td_merge_opts_default(&mo);
	if (mo.min_overlap < 0) { td_merge_set_error("td_merge_stream: min_overlap must not be negative"); return TD_FAIL; }
	mo.n_threads = td_stage_threads(mo.n_threads, 64);
	std::string err;
	TdMergeDevice* dev = nullptr;
	if (mo.device >= 0) {
		dev = td_merge_device_open(mo.device, err);
		if (!dev) { td_merge_set_error(err); return TD_FAIL; }
	}
	td_merge_stats st{};
	double tables_s = 0.0;
	const int rc = td_merge_stream_run(in1, in2, out_path, mo.n_threads, mo.batch_pairs, dev != nullptr,
		[&](const TdMergeView& v, TdWorkers& pool, td_merge_result* res, std::string& e) { return td_merge_batch(v, mo, dev, &pool, res, &tables_s, e); }, &st, err);
	td_merge_device_close(dev);
	st.tables_s = tables_s;
	if (stats) *stats = st;
	if (rc != TD_OK) { td_merge_set_error(err); return TD_FAIL; }
	return TD_OK;
}

// ---- the command line ----
extern "C" const char* td_merge_usage(void)
{
	return "Usage: tagdust-merge [options] <read1.fq> <read2.fq>\n"
	       "Merges overlapping paired-end reads; the records go to stdout (or --out) in input order.\n"
	       "  -t <n>                    host threads\n"
	       "  -minlen <n>               a candidate offset needs more than n bases left in both reads [16]\n"
	       "  -Q | -q | -threshold <x>  write a record when identical / aligned positions >= x [0]\n"
	       "  --out <file>              output file [- = stdout]\n"
	       "  --device <n>              the GPU to use [0]\n"
	       "  --host                    run on the host instead (no GPU needed)\n"
	       "  --batch-pairs <n>         pairs per batch [262144]\n"
	       "Input may be plain, .gz or .bz2 FASTQ.\n";
}

extern "C" int td_merge_parse_args(int argc, const char* const* argv, td_merge_args* out, char* err, size_t errcap)
{
	auto fail = [&](const std::string& m) { if (err && errcap) snprintf(err, errcap, "%s", m.c_str()); return TD_FAIL; };
	if (!out) return fail("td_merge_parse_args: bad arguments");
	memset(out, 0, sizeof *out);
	td_merge_opts_default(&out->opts);
	out->out_path = "-";
	int n_in = 0;
	for (int k = 1; k < argc; k++) {
		const char* a = argv[k];
		if (a[0] != '-' || !a[1]) {                       // an input file ("-" included), wherever it stands
			if (n_in == 0) out->in1 = a; else if (n_in == 1) out->in2 = a;
			n_in++;
			continue;
		}
		const std::string name = a + (a[1] == '-' ? 2 : 1);
		auto value = [&](const char** v) { if (k + 1 >= argc) return false; *v = argv[++k]; return true; };
		auto number = [&](const char* v, long lo, long* x) { char* e = nullptr; *x = strtol(v, &e, 10); return e != v && !*e && *x >= lo && *x <= 0x7fffffffL; };
		const char* v = nullptr;
		long x = 0;
		if (name == "h" || name == "help") out->help = 1;
		else if (name == "host") out->opts.device = -1;
		else if (name == "t" || name == "minlen" || name == "device" || name == "batch-pairs") {
			if (!value(&v)) return fail(std::string("option ") + a + " needs a value");
			if (!number(v, name == "t" || name == "batch-pairs" ? 1 : 0, &x)) return fail(std::string("option ") + a + ": bad value " + v);
			if (name == "t") out->opts.n_threads = (int32_t)x;
			else if (name == "minlen") out->opts.min_overlap = (int32_t)x;
			else if (name == "device") out->opts.device = (int32_t)x;
			else out->opts.batch_pairs = (int32_t)x;
		} else if (name == "Q" || name == "q" || name == "threshold") {
			if (!value(&v)) return fail(std::string("option ") + a + " needs a value");
			char* e = nullptr;
			out->opts.threshold = (float)strtod(v, &e);            // interface.c: atof
			if (e == v || *e) return fail(std::string("option ") + a + ": bad value " + v);
		} else if (name == "out") {
			if (!value(&v)) return fail(std::string("option ") + a + " needs a value");
			out->out_path = v;
		} else return fail(std::string("unknown option ") + a);
	}
	if (argc < 2) out->help = 1;
	if (!out->help && n_in != 2) return fail("two input files are needed (read 1 and read 2), " + std::to_string(n_in) + " given");
	return TD_OK;
}
