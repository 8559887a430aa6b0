// td_run.cpp -- the whole-run driver (include/tagdust_run.h), the run itself: what the reference's hmm_controller_multiple()
// (src/barcode_hmm.c:51-460) and test_architectures() (src/test_architectures.c:20-289) do, on this library's own entry points.
// Options, plan and report texts are td_run_opts.cpp, td_run_plan.cpp and td_run_report.cpp (td_run_internal.h).
// Host code; the device work is behind td_sequence_stats_device, td_compare_architectures, td_estimate_threshold and the
// streaming pipelines.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include <unistd.h>

#include "../../include/tagdust_multi.h"
#include "td_run_internal.h"
#include "td_io_internal.h"

using namespace tdrun;

namespace {

double now_s()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + (double)ts.tv_nsec * 1e-9;
}

struct CtxDeleter { void operator()(td_ctx* c) const { td_ctx_destroy(c); } };
struct TablesDeleter { void operator()(td_model_tables* t) const { td_model_tables_free(t); } };
struct FastaDeleter { void operator()(td_fasta* f) const { td_fasta_free(f); } };

struct FileState {
	ArchPtr arch;
	std::vector<std::string> segs;
	std::vector<uint8_t> codes;            // the head of the file: what the statistics (and -arch) look at
	std::vector<int64_t> offs;
	td_seq_stats stats{};
	float threshold = 0.0f;
	std::vector<std::unique_ptr<td_ctx, CtxDeleter>> ctx;   // one per listed device
	std::vector<td_ctx*> raw;
};

bool read_whole_file(const char* path, std::string& out)
{
	FILE* f = fopen(path, "rb");
	if (!f) return false;
	char buf[1 << 16];
	size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, n);
	fclose(f);
	return true;
}

struct Run {
	const td_run_opts* o;
	td_run_report* rep;
	Log log;
	std::vector<FileState> files;
	std::unique_ptr<td_fasta, FastaDeleter> fasta;
	int dust = 0;
	bool use_ref = false;
	float error_rate = 0.05f;
	RunRoles roles;                       // which file plays which part, once every architecture is known
	bool device_counts = false;           // rep->counts are a context's own tally (td_counts_get), not the combined records'

	int head_limit() const { return o->flavour ? 1001000 : 1000001; }   // io.c:125-188 with num_query 1000 / 1 000 001

	__attribute__((format(printf, 2, 3))) int fail(const char* fmt, ...)
	{
		char buf[1024];
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(buf, sizeof buf, fmt, ap);
		va_end(ap);
		g_run_error = buf;
		log.add(std::string(buf) + "\n");
		return TD_FAIL;
	}

	int load_head(int k)
	{
		FileState& f = files[(size_t)k];
		if (!f.offs.empty()) return TD_OK;
		std::string why;
		if (td_stream_head(o->infile[k], head_limit(), o->host_threads, f.codes, f.offs, why) != TD_OK) return fail("%s", why.c_str());
		if (f.offs.size() < 2) return fail("Input file:%s holds no reads.", o->infile[k]);
		if (f.codes.empty()) f.codes.push_back(0);   // (reads without bases: a valid pointer all the same)
		return TD_OK;
	}

	td_ctx* first_ctx(int k)
	{
		FileState& f = files[(size_t)k];
		if (f.ctx.empty()) {
			for (int d = 0; d < o->n_devices; d++) {
				td_ctx* c = nullptr;
				if (td_ctx_create(o->devices[d], &c) != TD_OK) { fail("%s", td_last_error(nullptr)); return nullptr; }
				f.ctx.emplace_back(c);
				f.raw.push_back(c);
				if (o->host_threads > 0) (void)td_set_option(c, "host_threads", o->host_threads > 16 ? 16 : o->host_threads);
			}
		}
		return f.raw[0];
	}

	// test_architectures(), test_architectures.c:20-289
	int select_architecture(int k, const ArchFile& af)
	{
		FileState& f = files[(size_t)k];
		log.addf("Looking at file:%s\n", o->infile[k]);
		log.addf("Searching for best architecture in file '%s'\n", o->arch_file);
		size_t best = 0;
		if (af.segs.size() > 1) {
			if (load_head(k) != TD_OK) return TD_FAIL;
			std::vector<ArchPtr> cand(af.segs.size());
			std::vector<const td_arch*> ptr;
			std::string why;
			for (size_t c = 0; c < af.segs.size(); c++) {
				if (!parse_arch(af.segs[c], cand[c], why)) return fail("%s", why.c_str());
				ptr.push_back(cand[c].get());
			}
			td_ctx* ctx = first_ctx(k);
			if (!ctx) return TD_FAIL;
			const int64_t n = std::min<int64_t>((int64_t)f.offs.size() - 1, 100000);   // param->num_query, :38-42
			std::vector<float> post(ptr.size());
			int32_t b = -1;
			if (td_compare_architectures(ctx, ptr.data(), (int32_t)ptr.size(), f.codes.data(), f.offs.data(), n, o->sequencer_error_rate,
			                             o->indel_frequency, o->num_threads, post.data(), &b) != TD_OK || b < 0)
				return fail("Test architecture on file %s failed: %s", o->infile[k], td_last_error(ctx));
			best = (size_t)b;
			log.add("Using: " + segments_text(af.segs[best]) + " \n");
			log.addf("%0.2f Confidence.\n", (double)post[best]);
		} else {
			log.add("Using: " + segments_text(af.segs[0]) + " \n");
			log.addf("Confidence: %0.2f\n", 1.0);
		}
		f.segs = af.segs[best];
		return TD_OK;
	}

	int execute();
	int run_files(td_stream_stats& st);
	int unknown_barcodes();
	int molecules();
	int samples();
	int quality();

	// a report file, whole
	int write_text(const std::string& name, const std::string& text)
	{
		FILE* out = fopen(name.c_str(), "w");
		if (!out) return fail("Failed to open file:%s", name.c_str());
		fwrite(text.data(), 1, text.size(), out);
		fclose(out);
		return TD_OK;
	}

	// Every device's entries of a file, merged: acc[n_acc] is the caller's to td_census_free (NULL after a failure), per[d] the
	// totals of device d.  `get` is td_census_get or td_mol_entries.
	template <typename Totals>
	int merged_entries(const FileState& f, int (*get)(td_ctx*, td_census_entry*, int64_t, int64_t*, Totals*), td_census_entry*& acc, int64_t& n_acc,
	                   std::vector<Totals>& per)
	{
		acc = nullptr; n_acc = 0;
		for (td_ctx* c : f.raw) {
			int64_t n = 0, n_merged = 0;
			Totals t{};
			td_census_entry* merged = nullptr;
			bool ok = get(c, nullptr, 0, &n, &t) == TD_OK;
			std::vector<td_census_entry> part((size_t)std::max<int64_t>(n, 1));
			ok = ok && get(c, part.data(), n, &n, &t) == TD_OK;
			if (!ok) fail("%s", td_last_error(c));
			else if (!(ok = td_census_merge(acc, n_acc, part.data(), n, &merged, &n_merged) == TD_OK)) fail("%s", td_last_error(nullptr));
			td_census_free(acc);
			acc = merged; n_acc = n_merged;
			if (!ok) return TD_FAIL;
			per.push_back(t);
		}
		return TD_OK;
	}
};

int Run::execute()
{
	const int K = o->n_infiles;
	td_run_plan_t* plan_raw = nullptr;
	// the banner and the cmd: line, interface.c:384-412; "Start Run", main.c:127
	log.add("Tagdust 2.33, Copyright (C) 2013-2019 Timo Lassmann <timolassmann@gmail.com>\n");
	{
		std::string cmd = "cmd: ";
		for (int k = 0; k < o->argc; k++) { cmd += o->argv[k]; cmd += ' '; }
		log.add(cmd + "\n");
	}
	if (td_run_plan(o, &plan_raw) != TD_OK) { log.add(g_run_error + "\n"); return TD_FAIL; }
	std::unique_ptr<td_run_plan_t> plan(plan_raw);
	for (auto& w : plan->warnings) log.add(w + "\n");
	dust = plan->dust;
	use_ref = plan->use_ref;
	log.add("Start Run\n--------------------------------------------------\n");
	files.resize((size_t)K);
	rep->n_files = K;

	// 1. architectures per file, barcode_hmm.c:105-138
	double t0 = now_s();
	std::string why;
	for (int k = 0; k < K; k++) {
		FileState& f = files[(size_t)k];
		if (plan->source[(size_t)k] == SRC_ARCH_FILE) { if (select_architecture(k, plan->arch_file) != TD_OK) return TD_FAIL; }
		else f.segs = plan->segs[(size_t)k];
		if (!parse_arch(f.segs, f.arch, why)) return fail("%s", why.c_str());
		rep->architectures[k] = dup_str(segments_text(f.segs).c_str());
	}
	rep->arch_s = now_s() - t0;
	{
		std::vector<const td_arch*> view;
		for (auto& f : files) view.push_back(f.arch.get());
		if (decide_roles(o, view, roles) != TD_OK || mate_filter_files(o, dust, use_ref, roles) != TD_OK) { log.add(g_run_error + "\n"); return TD_FAIL; }
	}
	const SampleSheet& sheet = roles.sheet;
	std::vector<const char*> sample_names;   // (as td_samples_enable takes them)
	for (const std::string& s : sheet.names) sample_names.push_back(s.c_str());

	// 2. sequence statistics over the head of every file, io.c:52-300
	t0 = now_s();
	for (int k = 0; k < K; k++) {
		FileState& f = files[(size_t)k];
		if (load_head(k) != TD_OK) return TD_FAIL;
		const int64_t n = (int64_t)f.offs.size() - 1;
		if (o->stats_on_host) {
			if (td_sequence_stats_limit(f.arch.get(), f.codes.data(), f.offs.data(), n, head_limit(), o->matchstart, o->matchend, &f.stats) != TD_OK)
				return fail("sequence statistics of %s failed", o->infile[k]);
		} else {
			td_ctx* ctx = first_ctx(k);
			if (!ctx) return TD_FAIL;
			if (td_sequence_stats_device(ctx, f.arch.get(), f.codes.data(), f.offs.data(), n, head_limit(), o->matchstart, o->matchend, &f.stats) != TD_OK)
				return fail("%s", td_last_error(ctx));
		}
		std::vector<uint8_t>().swap(f.codes);   // the run opens the file again, as the reference does
		std::vector<int64_t>().swap(f.offs);
		f.offs.push_back(0);
	}
	rep->stats_on_device = !o->stats_on_host;
	rep->stats_s = now_s() - t0;

	// contexts, window (param->matchstart / matchend apply to every run_pHMM call, calibration included)
	for (int k = 0; k < K; k++) {
		if (!first_ctx(k)) return TD_FAIL;
		for (td_ctx* c : files[(size_t)k].raw)
			if (td_set_window(c, o->matchstart, o->matchend) != TD_OK) return fail("%s", td_last_error(c));
	}

	// 3. thresholds, barcode_hmm.c:190-200 (estimateQthreshold, calibrateQ.c:17-235): srand(seed) once per file
	t0 = now_s();
	error_rate = o->sequencer_error_rate;
	if (!o->confidence_threshold) {
		const uint32_t seed = o->seed ? o->seed : (uint32_t)(time(nullptr) * 42);   // calibrateQ.c:27-31
		for (int k = 0; k < K; k++) {
			FileState& f = files[(size_t)k];
			log.addf("Determining threshold for read%d.\n", k);
			if (td_estimate_threshold(f.raw[0], f.arch.get(), &f.stats, o->indel_frequency, seed, o->flavour ? 4000 : 400000, o->flavour ? 1 : 0,
			                          &f.threshold) != TD_OK)
				return fail("estimateQthreshold failed: %s", td_last_error(f.raw[0]));
			log.addf("Selected Threshold:: %f\n", (double)f.threshold);
		}
		error_rate = 0.05f;   // calibrateQ.c:65, :117: for the rest of the run
	}
	for (int k = 0; k < K; k++) { rep->thresholds[k] = files[(size_t)k].threshold; rep->selected_threshold = files[(size_t)k].threshold; }
	rep->calibration_s = now_s() - t0;

	// -ref, barcode_hmm.c:209-215
	if (use_ref) {
		std::string text;
		if (!read_whole_file(o->reference_fasta, text)) return fail("Failed to open file:%s", o->reference_fasta);
		td_fasta* fa = nullptr;
		if (td_fasta_parse(text.data(), (int64_t)text.size(), &fa) != TD_OK || !fa) return fail("Failed to read the sequences of %s", o->reference_fasta);
		fasta.reset(fa);
		rep->n_artifacts = fa->n_seq;
		rep->artifact_hits = (int64_t*)calloc((size_t)std::max(1, fa->n_seq), sizeof(int64_t));
		rep->artifact_names = (char**)calloc((size_t)std::max(1, fa->n_seq), sizeof(char*));
		for (int j = 0; j < fa->n_seq; j++) rep->artifact_names[j] = dup_str(fa->names[j]);
	}

	// 4. models and parameters, barcode_hmm.c:203-206
	t0 = now_s();
	for (int k = 0; k < K; k++) {
		FileState& f = files[(size_t)k];
		std::unique_ptr<td_model_tables, TablesDeleter> tables;
		if (!is_read_only(f.arch.get())) {   // (an R:N file goes through run_rna_dust: no model on the device)
			td_model_tables* t = nullptr;
			if (td_model_build(f.arch.get(), &f.stats, error_rate, o->indel_frequency, &t) != TD_OK) return fail("building the model of %s failed", o->infile[k]);
			tables.reset(t);
		}
		for (td_ctx* c : f.raw) {
			if (tables) {
				if (td_set_option(c, "async_compile", o->sync_compile ? 0 : 1) != TD_OK || td_model_upload(c, &tables->desc) != TD_OK) return fail("%s", td_last_error(c));
			}
			if (td_set_params(c, f.threshold, o->minlen, dust) != TD_OK) return fail("%s", td_last_error(c));
			if (td_set_artifacts(c, fasta ? fasta->string : nullptr, fasta ? fasta->s_index : nullptr, fasta ? fasta->n_seq : 0, o->filter_error, o->num_threads) != TD_OK)
				return fail("%s", td_last_error(c));
			if (td_counts_reset(c) != TD_OK) return fail("%s", td_last_error(c));
			// --unknown-barcodes: the contexts of the barcode file count what their reads spell in the last 'B' segment
			if (o->unknown_barcodes > 0 && k == roles.bar_file &&
			    td_census_enable(c, -1, TD_CENSUS_DEFAULT_MASK, o->unknown_slots_log2) != TD_OK) return fail("%s", td_last_error(c));
			// --samples: the contexts of the barcode file assign every extracted read by all its barcodes, in front of census and count
			if (sheet.n() > 0 && k == roles.bar_file && !o->join_barcodes &&
			    td_samples_enable(c, sheet.tuples.data(), sample_names.data(), sheet.n(), 16) != TD_OK) return fail("%s", td_last_error(c));
			// --join-barcodes: the first barcode file's contexts hold the sheet over the columns of all barcode files and join the calls
			// that the contexts of every other barcode file export (td_stream_run_multi carries the words from file to file)
			if (o->join_barcodes)
				for (size_t q = 0; q < roles.bar_files.size(); q++) {
					if (roles.bar_files[q] != k) continue;
					const int rc = q == 0 ? td_samples_join_enable(c, sheet.tuples.data(), sample_names.data(), sheet.n(), 16, (int32_t)roles.column_hmms.size(),
					                                               roles.first_column[q], roles.column_hmms.data())
					                      : td_samples_export_enable(c, roles.first_column[q]);
					if (rc != TD_OK) return fail("%s", td_last_error(c));
				}
			// --min-base-quality: the context of the one decoded file drops extracted reads with low-quality barcode / UMI bases, in front
			// of samples, census and count (the streaming run names every batch's quality lines)
			if (k == roles.qual_file &&
			    td_qual_enable(c, o->min_base_quality, o->quality_offset, o->max_low_bases, o->quality_segments) != TD_OK) return fail("%s", td_last_error(c));
			// --molecules: the contexts of the one input file (with --mate-bases: of the one decoded file) count its extracted reads per
			// barcode, fingerprint and start of the read
			if (k != roles.mol_file) continue;
			if (o->molecules && td_mol_enable(c, o->molecules_prefix, o->molecules_slots_log2) != TD_OK) return fail("%s", td_last_error(c));
			// --dedup: ... and mark every read that is not the first of its molecule; the writer leaves those out
			if (o->dedup && td_mol_dedup_enable(c) != TD_OK) return fail("%s", td_last_error(c));
			// --collapse-umis: ... and keep what every key was made of, for the collapse behind the run
			if (o->collapse_umis && td_mol_collapse_enable(c) != TD_OK) return fail("%s", td_last_error(c));
			// --mate-bases: ... and take the first bases of every read's mate into the key (td_stream_run_multi names the mate batches)
			if (o->mate_bases && td_mol_mate_enable(c, o->mate_bases) != TD_OK) return fail("%s", td_last_error(c));
			// --mate-filter: ... and judge every mate with this context's DUST and -ref, its outcome joined to the read's in front of the count
			if (o->mate_filter && td_mol_mate_filter_enable(c) != TD_OK) return fail("%s", td_last_error(c));
		}
	}
	rep->compile_wait_s = now_s() - t0;

	// 5. the run
	t0 = now_s();
	td_stream_stats st{};
	const int rc = run_files(st);
	rep->stream = st;
	rep->stream_s = now_s() - t0;
	if (rc != TD_OK) {
		const std::string msg = g_run_error;
		return fail("%s -- the run failed after it had started: the output files are incomplete and were left as they are", msg.c_str());
	}

	if (roles.qual_file >= 0 && quality() != TD_OK) return TD_FAIL;
	if (sheet.n() > 0 && samples() != TD_OK) return TD_FAIL;
	if (o->unknown_barcodes > 0 && unknown_barcodes() != TD_OK) return TD_FAIL;
	if (o->molecules && molecules() != TD_OK) return TD_FAIL;

	// 6. the summary, barcode_hmm.c:387-430
	for (auto& m : summary_messages(o, rep)) log.add(m);
	return TD_OK;
}

// --unknown-barcodes: every device's census of the barcode file, merged (nothing of it enters the log), and <out>_unknown_barcodes.txt
int Run::unknown_barcodes()
{
	FileState& f = files[(size_t)roles.bar_file];
	td_census_entry* acc = nullptr;
	int64_t n_acc = 0;
	td_census_totals sum{};
	std::vector<td_census_totals> per;
	if (merged_entries(f, td_census_get, acc, n_acc, per) != TD_OK) return TD_FAIL;
	for (const td_census_totals& t : per) {
		sum.eligible += t.eligible; sum.counted += t.counted; sum.skipped_empty += t.skipped_empty; sum.skipped_long += t.skipped_long;
		sum.skipped_n += t.skipped_n; sum.overflow += t.overflow;
	}
	sum.distinct = n_acc;
	rep->unknown = acc; rep->n_unknown = n_acc; rep->unknown_totals = sum;

	std::string text;
	const bool ok = unknown_barcodes_text(o, f.arch.get(), f.segs, o->infile[roles.bar_file], *rep, text);
	if (write_text(unknown_file_name(o), text) != TD_OK) return TD_FAIL;
	return ok ? TD_OK : fail("%s", td_last_error(nullptr));
}

// --min-base-quality: the totals of the decoded file's context (one device); behind the summary's counts in the log
int Run::quality()
{
	td_ctx* c = files[(size_t)roles.qual_file].raw[0];
	td_qual_totals t{};
	if (td_qual_get(c, &t) != TD_OK) return fail("%s", td_last_error(c));
	rep->quality = 1;
	rep->quality_totals = t;
	// a context's own tally is the decode kernel's: the reads that lost their extraction here move to "barcode / UMI not found"
	if (device_counts) {
		rep->counts[TD_EXTRACT_SUCCESS] -= t.failed;
		rep->counts[TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND] += t.failed;
	}
	return TD_OK;
}

// --samples: every device's combination count of the barcode file, merged with td_census_merge, the totals summed (nothing of it
// enters the log), and <out>_samples.txt
int Run::samples()
{
	FileState& f = files[(size_t)roles.bar_file];
	td_census_entry* acc = nullptr;
	int64_t n_acc = 0;
	td_samples_totals sum{};
	std::vector<td_samples_totals> per;
	if (o->join_barcodes) {   // (one device: the join's totals are the one context's, partner_failed among them)
		std::vector<td_samples_join_totals> jper;
		if (merged_entries(f, td_samples_join_get, acc, n_acc, jper) != TD_OK) return TD_FAIL;
		for (const td_samples_join_totals& t : jper) { per.push_back(t.t); rep->partner_failed += t.partner_failed; }
	} else if (merged_entries(f, td_samples_get, acc, n_acc, per) != TD_OK) return TD_FAIL;
	for (const td_samples_totals& t : per) {
		sum.eligible += t.eligible; sum.assigned += t.assigned; sum.unlisted += t.unlisted; sum.incomplete += t.incomplete; sum.overflow += t.overflow;
	}
	rep->samples = acc; rep->n_sample_keys = n_acc; rep->samples_totals = sum; rep->n_samples = roles.sheet.n();
	// a context's own tally is the decode kernel's: the reads that lost their extraction here move to "barcode / UMI not found"
	if (device_counts) {
		rep->counts[TD_EXTRACT_SUCCESS] -= sum.unlisted + sum.incomplete;
		rep->counts[TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND] += sum.unlisted + sum.incomplete;
	}
	std::string text;
	bool ok;
	if (o->join_barcodes) {
		std::vector<const td_arch*> archs;
		std::vector<std::vector<std::string>> segs;
		for (const FileState& g : files) { archs.push_back(g.arch.get()); segs.push_back(g.segs); }
		ok = samples_text_join(o, archs, segs, o->infile, roles.sheet, *rep, text);
	} else ok = samples_text(o, f.arch.get(), f.segs, o->infile[roles.bar_file], roles.sheet, *rep, text);
	if (write_text(samples_file_name(o), text) != TD_OK) return TD_FAIL;
	return ok ? TD_OK : fail("%s", std::string(g_run_error).c_str());
}

// --molecules: one device's own summary, or every device's entries merged and summarised on the host (nothing of it enters the
// log), and <out>_molecules.txt
int Run::molecules()
{
	FileState& f = files[(size_t)roles.mol_file];
	td_mol_row* rows = (td_mol_row*)calloc(TD_NUM_BARCODE_BINS, sizeof(td_mol_row));
	if (!rows) return fail("--molecules: out of memory");
	rep->molecules = rows;
	td_mol_totals sum{};
	if (f.raw.size() == 1) {
		if (td_mol_get(f.raw[0], rows, &sum) != TD_OK) return fail("%s", td_last_error(f.raw[0]));
	} else {
		td_census_entry* acc = nullptr;
		int64_t n_acc = 0;
		std::vector<td_mol_totals> per;
		if (merged_entries(f, td_mol_entries, acc, n_acc, per) != TD_OK) return TD_FAIL;
		for (const td_mol_totals& t : per) {
			sum.eligible += t.eligible; sum.counted += t.counted; sum.skipped_empty += t.skipped_empty; sum.skipped_n += t.skipped_n;
			sum.overflow += t.overflow;
		}
		sum.molecules = n_acc;
		const int rc = td_mol_summarise(acc, n_acc, rows);
		td_census_free(acc);
		if (rc != TD_OK) return fail("%s", td_last_error(nullptr));
	}
	rep->molecules_totals = sum;
	// --collapse-umis: one device's own collapse, or every device's molecules with their origins collapsed on the host
	if (o->collapse_umis) {
		td_mol_row* crows = (td_mol_row*)calloc(TD_NUM_BARCODE_BINS, sizeof(td_mol_row));
		if (!crows) return fail("--collapse-umis: out of memory");
		rep->molecules_collapsed = crows;
		if (f.raw.size() == 1) {
			if (td_mol_collapse_get(f.raw[0], crows, &rep->collapse_totals) != TD_OK) return fail("%s", td_last_error(f.raw[0]));
		} else {
			std::vector<td_census_entry> all;
			std::vector<td_mol_origin> all_o;
			for (td_ctx* c : f.raw) {
				int64_t n = 0;
				if (td_mol_origins(c, nullptr, nullptr, 0, &n, nullptr) != TD_OK) return fail("%s", td_last_error(c));
				const size_t at = all.size();
				all.resize(at + (size_t)n); all_o.resize(at + (size_t)n);
				if (n > 0 && td_mol_origins(c, all.data() + at, all_o.data() + at, n, &n, nullptr) != TD_OK) return fail("%s", td_last_error(c));
			}
			td_census_entry* roots = nullptr;
			td_mol_origin* roots_o = nullptr;
			int64_t n_roots = 0;
			if (td_mol_collapse_host(all.data(), all_o.data(), (int64_t)all.size(), &roots, &roots_o, &n_roots, &rep->collapse_totals) != TD_OK)
				return fail("%s", td_last_error(nullptr));
			const int rc = td_mol_summarise(roots, n_roots, crows);
			td_census_free(roots);
			free(roots_o);
			if (rc != TD_OK) return fail("%s", td_last_error(nullptr));
		}
		rep->collapse = 1;
	}
	if (o->dedup) {   // (one device: td_run_plan saw to it)
		if (td_mol_dedup_get(f.raw[0], &rep->dedup_totals) != TD_OK) return fail("%s", td_last_error(f.raw[0]));
		rep->dedup = 1;
		rep->dedup_collapsed = o->dedup_collapsed != 0;
	}
	const char* mate_infile = roles.mate_file >= 0 ? o->infile[roles.mate_file] : nullptr;
	return write_text(molecules_file_name(o), molecules_text(o, f.arch.get(), o->infile[roles.mol_file], mate_infile, dust, use_ref, roles.sheet, *rep));
}

int Run::run_files(td_stream_stats& st)
{
	const int K = o->n_infiles;
	td_stream_opts so{};
	so.fingerprint_text = o->fingerprint_seq;
	so.batch_reads = o->batch_reads > 0 ? o->batch_reads : (o->flavour ? 1000 : 0);
	so.n_threads = o->host_threads;
	if (K == 1 && o->n_devices == 1 && !is_read_only(files[0].arch.get())) {
		td_ctx* c = files[0].raw[0];
		if (o->dedup_collapsed) {
			// Survey, freeze, replay (tagdust_molecules.h).  The survey decodes the whole file for the molecule table alone; every other
			// accumulator of the context -- outcome counters, artifact hits, the census of --unknown-barcodes -- is reset behind it, so
			// that it reports exactly one pass, the second.
			td_stream_stats survey{};
			const double t0 = now_s();
			if (td_stream_survey(c, o->infile[0], &so, &survey) != TD_OK) return run_fail("%s", td_io_last_error());
			if (td_mol_dedup_freeze(c, nullptr) != TD_OK || td_counts_reset(c) != TD_OK || (o->unknown_barcodes > 0 && td_census_reset(c) != TD_OK) ||
			    (roles.sheet.n() > 0 && td_samples_reset(c) != TD_OK) || (o->min_base_quality && td_qual_reset(c) != TD_OK))
				return run_fail("%s", td_last_error(c));
			rep->survey_s = now_s() - t0;
		}
		if (td_stream_run(c, o->infile[0], files[0].arch.get(), o->outfile, &so, &st) != TD_OK) return run_fail("%s", td_io_last_error());
		if (td_counts_get(c, rep->counts) != TD_OK) return run_fail("%s", td_last_error(c));
		device_counts = true;
		if (rep->n_artifacts && td_artifact_hits_get(c, rep->artifact_hits, rep->n_artifacts) != TD_OK) return run_fail("%s", td_last_error(c));
		return TD_OK;
	}
	std::vector<td_stream_file> sf((size_t)K);
	for (int k = 0; k < K; k++) {
		sf[(size_t)k].path = o->infile[k];
		sf[(size_t)k].arch = files[(size_t)k].arch.get();
		// (--mate-bases: the other files get no contexts -- their reads are uploaded once, as mates, by the decoded file's context)
		sf[(size_t)k].ctx = o->mate_bases && k != roles.mol_file ? nullptr : files[(size_t)k].raw.data();
	}
	if (td_stream_run_multi_hits(sf.data(), K, o->n_devices, o->outfile, dust, &so, &st, rep->counts, rep->artifact_hits, rep->n_artifacts) != TD_OK)
		return run_fail("%s", td_io_last_error());
	return TD_OK;
}

}   // namespace

extern "C" int td_run_execute(const td_run_opts* o, td_run_report* report)
{
	if (!o) return run_fail("td_run_execute: NULL options");
	td_run_report local{};
	td_run_report* rep = report ? report : &local;
	memset(rep, 0, sizeof *rep);
	int rc;
	{
		Run run{ o, rep };
		run.log.echo = o->echo_log != 0;
		rc = run.execute();
		run.log.write(o->outfile);
		rep->log = dup_str(run.log.text.c_str());
	}   // (contexts and their compile jobs are gone here)
	if (rc != TD_OK) snprintf(rep->error, sizeof rep->error, "%s", g_run_error.c_str());
	if (!report) td_run_report_clear(&local);
	return rc;
}
