// td_stream.cpp -- input files of any size through the decode path as a pipeline (include/tagdust_io.h): td_stream_run, one
// input file on one device (td_stream_survey: the same without a write stage), and td_stream_run_multi, the K input files of a paired / multi-read run in lock-step on N devices.
//
//   reader / parser thread (per file) caller's thread                     writer thread
//   block k+1: read or map, find      batch k: td_submit ... td_wait      batch k-1: format per output file, append
//   records, base-code them into      (several batches in flight on the
//   the next batch's pinned buffers   devices)
//
// It replaces the reference's batch loop around run_pHMM (src/barcode_hmm.c:244-385): read_fasta_fastq() of <= 1 000 001
// records of every file (io.c:1684-1815, through popen("cat|zcat|bzcat"), io.c:382-608) -> run_pHMM -> print_all() appending
// to the per-barcode files (io.c:757-1016) -- with the three steps of consecutive batches running side by side, each of the
// two host steps on several threads.  Batches hold exactly `batch_reads` records like the reference's (the -ref artifact
// filter's per-thread read ranges are taken over a batch, barcode_hmm.c:2478-2583, so the boundaries are part of the result).
//
// The pieces: a Reader per input file (td_stream_reader.cpp: Source, parse pool, the batches it owns, its allocator and producer
// threads), one run_stages() for both entry points, here (the device stage over tuples of one batch per file, the write-stage
// thread, the teardown), one Writer (td_stream_writer.cpp: output files, format pool, appender thread) and one RunError that all
// of them share (td_stream_internal.h, with the queues between the stages): the first failure anywhere is the run's message and
// ends every stage.  An entry point validates its arguments, sets these up and gives run_stages what is its own: the check of a
// tuple and what the write stage does with a finished one.  td_merge_stream.cpp is the `merge` controller on the same readers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/tagdust_molecules.h"   // td_mol_mate_next: pair mode of td_stream_run_multi
#include "../../include/tagdust_samples.h"     // td_samples_name: the output files of a run with sample assignment on
#include "../../include/tagdust_quality.h"     // td_qual_next: the quality lines of a file whose context has the base-quality filter on
#include "td_stream_internal.h"

using namespace tdstream;

// ---- td_stream_opts as the run uses them (the defaults of include/tagdust_io.h) ----
// The reference reads 1 000 001 records at a time (param->num_query, barcode_hmm.c:172).  Per-read results do not depend on how
// a file is cut into batches -- except through the -ref artifact filter, whose per-thread read ranges are taken over a batch:
// with a filter set (and in a parse-only run) the batches are the reference's (reference_batches), otherwise they are 2^18
// reads (one tile per wave slot of the device; a quarter of the page-locked memory and a pipeline that fills four times sooner).
td_stream_opts tdstream::resolve_opts(const td_stream_opts* opts, bool reference_batches)
{
	td_stream_opts o{};
	if (opts) o = *opts;
	if (o.batch_reads <= 0) o.batch_reads = reference_batches ? 1000001 : (1 << 18);
	if (o.block_bytes <= 0) o.block_bytes = (int64_t)64 << 20;
	if (o.block_bytes < 4096) o.block_bytes = 4096;
	o.n_threads = td_stage_threads(o.n_threads, 32);
	return o;
}

// Sample assignment (tagdust_samples.h): the decoded file's contexts say whether it is on, the way pair mode reads "mate_bases"; the
// output files are then the sheet's.  Contexts of one file that disagree about the sheet cannot write one file set.
bool td_stream_sample_names(td_ctx* const* ctx, int n_ctx, std::vector<std::string>& samples, std::string& why)
{
	samples.clear();
	for (int d = 0; d < n_ctx; d++) {
		int32_t n = 0;
		(void)td_get_option(ctx[d], "samples", &n);
		std::vector<std::string> mine;
		for (int32_t s = 0; s < n; s++) { const char* name = td_samples_name(ctx[d], s); mine.push_back(name ? name : ""); }
		if (d == 0) samples = mine;
		else if (mine != samples) {
			why = "the contexts of one input file disagree about the sample sheet (td_samples_enable): context 0 has " + std::to_string(samples.size()) +
			      " samples, context " + std::to_string(d) + " has " + std::to_string(mine.size()) + (mine.size() == samples.size() ? " with other names" : "");
			return false;
		}
	}
	return true;
}

namespace {

// batches (record ranges of every file) in flight on the devices: the option of a context of the run, 3 when it has none
int pipeline_depth(td_ctx* ctx)
{
	int32_t depth = 3;
	if (ctx) (void)td_get_option(ctx, "pipeline_depth", &depth);
	return depth;
}

// the base-quality filter (tagdust_quality.h) is on in this context: its batches carry the records' quality lines
bool quality_active(td_ctx* ctx)
{
	int32_t on = 0;
	(void)td_get_option(ctx, "quality_filter", &on);
	return on != 0;
}

bool artifacts_active(td_ctx* ctx)
{
	int32_t art = 0;
	(void)td_get_option(ctx, "artifacts_active", &art);
	return art != 0;
}

// ---- the three stages of a run over K input files in lock-step and N devices (td_stream_run: K = 1, N = 1) ----
struct Tuple {                        // batch j of every input file: records [j * batch_reads, ...) of each
	std::vector<Batch*> b;            // [file]; the batches stay their readers'
	std::vector<int64_t> tickets;     // [file * N + device]; 0: nothing was submitted
	std::vector<std::vector<uint32_t>> words;   // [file] the join across input files: an exporter's words, the primary's partner words
	Tuple(int K, int N) : b((size_t)K, nullptr), tickets((size_t)(K * N), 0), words((size_t)K) {}
};

enum { JOIN_NONE = 0, JOIN_EXPORTER, JOIN_PRIMARY };   // a file's side of the join across input files (tagdust_samples.h)

struct Target {                       // where the batches of one input file go
	td_ctx* const* ctx;               // its context on each of the N devices; NULL: no device sees this file
	bool rna;                         // run_rna_dust (TD_MODE_RNA_DUST: the reads come back unchanged) instead of the HMM
	int mate = -1;                    // pair mode: the file whose batch is this file's mate batch (td_mol_mate_next), else -1
	bool qual = false;                // the base-quality filter is on in ctx[0]: the batch's quality lines are named (td_qual_next)
	int join = JOIN_NONE;             // its contexts export their barcode calls / join the exporters' (one device)
};

// Starts the readers, runs the write stage on a thread of its own (`write` for every finished tuple in input order, then the
// wait for the writer's appends; writer == NULL: a parse-only run, no output files) and the device stage on the calling thread
// (a context is driven from one thread): a ready batch of every reader -> `check` (an error message, or empty) -> submit, at most
// `depth` tuples in flight, waited for in order.  Then the teardown, the same after a failure at any point: every ticket still
// outstanding waited for, write stage and appender ended, files closed, readers stopped, batches released.  The run's error, if
// any, is in `err`; `prefix` starts the messages of this function.
void run_stages(const std::string& prefix, RunError& err, const std::vector<std::unique_ptr<Reader>>& readers, const std::vector<Target>& dev,
                const int N, const int depth, Writer* writer, const std::function<std::string(const Tuple&)>& check,
                const std::function<bool(Tuple&)>& write, td_stream_stats& st)
{
	const int K = (int)readers.size();
	const int n_batches = depth + 4;
	Queue<std::unique_ptr<Tuple>> done((size_t)n_batches);      // (tuples left in it by a failed run are freed with it)
	err.watch(&done);
	for (auto& r : readers)
		if (!r->start(n_batches)) { err.fail(prefix + "page-locked memory exhausted"); break; }
	std::thread t_write([&] {
		std::unique_ptr<Tuple> t;
		while (done.pop(t)) {
			const double t0 = now_s();
			if (!write(*t)) return;
			st.n_reads += t->b[0]->n; st.n_batches++;
			for (Batch* b : t->b) b->pieces.clear();               // releases the blocks
			st.write_s += now_s() - t0;
			for (int k = 0; k < K; k++) if (!readers[(size_t)k]->free_list->push(t->b[(size_t)k])) return;
		}
		const double t0 = now_s();
		if (writer) (void)writer->finish();
		st.write_s += now_s() - t0;
	});
	std::deque<std::unique_ptr<Tuple>> flying;
	auto wait_for = [&](const Tuple& t) -> bool {   // every ticket of the tuple, also after one of them has failed
		bool ok = true;
		for (int k = 0; k < K; k++)
			for (int d = 0; d < N; d++) {
				const int64_t ticket = t.tickets[(size_t)(k * N + d)];
				if (dev[(size_t)k].ctx && ticket && td_wait(dev[(size_t)k].ctx[d], ticket) != TD_OK) {
					if (ok) err.fail(prefix + td_last_error(dev[(size_t)k].ctx[d]));
					ok = false;
				}
			}
		return ok;
	};
	auto retire = [&]() -> bool {
		std::unique_ptr<Tuple> t = std::move(flying.front());
		flying.pop_front();
		const double t0 = now_s();
		const bool ok = wait_for(*t);
		st.decode_s += now_s() - t0;
		return ok && done.push(std::move(t));
	};
	while (!err.failed()) {
		std::unique_ptr<Tuple> t(new Tuple(K, N));
		int n_closed = 0;
		bool bad = false;
		// With nothing ready from a reader and tuples in flight the oldest one is retired instead of waiting: the reader may be
		// waiting for exactly that tuple's buffers.  (The allocator thread "runs with what it has" when page-locking fails part-way
		// -- a memlock limit, a container -- and with fewer than depth + 2 batches in all a loop that only retires at full depth
		// leaves the reader waiting for a free batch, this thread for a ready one and the writer for a finished one, forever.)
		for (int k = 0; k < K && !bad; k++)
			for (;;) {
				const Reader& r = *readers[(size_t)k];
				Batch* b = nullptr;
				const int got = flying.empty() ? (r.ready->pop(b) ? 1 : -1) : r.ready->try_pop(b);
				if (got == 1) { t->b[(size_t)k] = b; break; }
				if (got < 0) { n_closed++; break; }
				if (!retire()) { bad = true; break; }
			}
		if (bad || n_closed == K) break;
		const std::string objection = check(*t);
		if (!objection.empty()) { err.fail(objection); break; }
		if ((int)flying.size() >= depth && !retire()) break;
		const double t0 = now_s();
		const int64_t n = t->b[0]->n;
		bool ok = true;
		auto submit_file = [&](const int k) {
			Batch* b = t->b[(size_t)k];
			const Target& tg = dev[(size_t)k];
			for (int d = 0; d < N && ok; d++) {      // run_pHMM's contiguous ranges over the devices (barcode_hmm.c:1911-1922)
				td_ctx* ctx = tg.ctx[d];
				const int64_t interval = n / N, lo = (int64_t)d * interval, hi = (d == N - 1) ? n : lo + interval;
				if (hi <= lo) continue;
				const bool r = tg.rna;
				// (the window: the artifact filter's thread ranges are those of the whole batch, not of a device's range)
				// (pair mode, one device: the tuple's batch of the mate file goes up with this one, on the same upload stream)
				// (the join across input files, one device: an exporter's words come back into the tuple, the primary's go up with its batch)
				ok = (N == 1 || td_set_batch_window(ctx, lo, n) == TD_OK) &&
				     (tg.mate < 0 || td_mol_mate_next(ctx, t->b[(size_t)tg.mate]->codes, t->b[(size_t)tg.mate]->offs, n) == TD_OK) &&
				     (!tg.qual || r || td_qual_next(ctx, b->qual, hi - lo) == TD_OK) &&
				     (tg.join != JOIN_EXPORTER || td_samples_export_next(ctx, t->words[(size_t)k].data() + lo, hi - lo) == TD_OK) &&
				     (tg.join != JOIN_PRIMARY || td_samples_join_next(ctx, t->words[(size_t)k].data() + lo, hi - lo) == TD_OK) &&
				     td_submit(ctx, b->codes, 0, b->offs + lo, hi - lo, r ? TD_MODE_RNA_DUST : TD_MODE_GET_LABEL, b->res + lo, nullptr,
				               r ? nullptr : b->seq_out + b->offs[lo], &t->tickets[(size_t)(k * N + d)]) == TD_OK;
				if (!ok) err.fail(prefix + td_last_error(ctx));
			}
		};
		// The join across input files (tagdust_samples.h): the exporters first, their words waited for and OR-ed into the primary's,
		// then the primary, then every other file as ever.  A ticket waited for here is zeroed: the teardown does not wait twice.
		int primary = -1;
		for (int k = 0; k < K; k++) {
			if (dev[(size_t)k].join == JOIN_NONE) continue;
			t->words[(size_t)k].assign((size_t)(n > 0 ? n : 1), 0u);
			if (dev[(size_t)k].join == JOIN_PRIMARY) primary = k;
		}
		for (int k = 0; k < K && ok; k++) if (dev[(size_t)k].join == JOIN_EXPORTER) submit_file(k);
		for (int k = 0; k < K; k++) {
			if (dev[(size_t)k].join != JOIN_EXPORTER) continue;
			for (int d = 0; d < N; d++) {
				int64_t& ticket = t->tickets[(size_t)(k * N + d)];
				if (ticket && td_wait(dev[(size_t)k].ctx[d], ticket) != TD_OK) {
					if (ok) err.fail(prefix + td_last_error(dev[(size_t)k].ctx[d]));
					ok = false;
				}
				ticket = 0;
			}
			if (ok && primary >= 0) for (int64_t i = 0; i < n; i++) t->words[(size_t)primary][(size_t)i] |= t->words[(size_t)k][(size_t)i];
		}
		if (primary >= 0 && ok) submit_file(primary);
		for (int k = 0; k < K && ok; k++) if (dev[(size_t)k].ctx && dev[(size_t)k].join == JOIN_NONE) submit_file(k);

		st.decode_s += now_s() - t0;
		flying.push_back(std::move(t));     // (also after a failed submit: the ranges already on other devices are waited for below)
		if (!ok) break;
	}
	while (!flying.empty() && !err.failed()) if (!retire()) break;
	if (err.failed()) {                     // nothing of ours may stay queued on the devices
		for (auto& t : flying) (void)wait_for(*t);
		flying.clear();
	}
	done.close();
	t_write.join();
	if (writer) {
		const int e = writer->close();
		if (e) err.fail(prefix + "close failed: " + strerror(e));
	}
	if (N > 1) for (const Target& tg : dev) if (tg.ctx) for (int d = 0; d < N; d++) (void)td_set_batch_window(tg.ctx[d], 0, 0);
	finish_readers(readers, !err.failed(), st.bytes_in, st.parse_s, st.read_s);
	if (writer) st.bytes_out = writer->bytes_out;
}

} // namespace

extern "C" int td_stream_run(td_ctx* ctx, const char* in_path, const td_arch* arch, const char* out_prefix,
                             const td_stream_opts* opts, td_stream_stats* stats)
{
	if (!in_path) { td_io_set_error("td_stream_run: NULL input path"); return TD_FAIL; }
	if (ctx && (!arch || !out_prefix)) { td_io_set_error("td_stream_run: a decoding run needs the architecture and an output prefix"); return TD_FAIL; }
	const td_stream_opts o = resolve_opts(opts, !ctx || artifacts_active(ctx));
	const double t_start = now_s();
	RunError err;
	std::vector<std::unique_ptr<Reader>> readers;
	readers.emplace_back(new Reader(err, o, ctx == nullptr, true, o.n_threads));
	const bool judged = ctx && quality_active(ctx);
	readers[0]->want_qual = judged; readers[0]->path = in_path;
	std::string why;
	if (!readers[0]->src.open(in_path, o.block_bytes, why)) { td_io_set_error(why); return TD_FAIL; }
	std::unique_ptr<Writer> w;
	if (ctx) {
		std::vector<std::string> names;
		int num_alternatives = 2;
		std::vector<std::string> samples;
		td_ctx* const own[1] = { ctx };
		if (!td_stream_sample_names(own, 1, samples, why)) { td_io_set_error("td_stream_run: " + why); return TD_FAIL; }
		if (samples.empty()) td_writer_file_names(out_prefix, arch, names, &num_alternatives);
		else {
			int n_r = 0;
			for (int j = 0; j < arch->n_segments; j++) n_r += arch->type[j] == 'R';
			td_writer_file_names_samples(out_prefix, samples, n_r, names, &num_alternatives);
		}
		w.reset(new Writer(err, o.n_threads, num_alternatives));
		w->fingerprint_text = o.fingerprint_text != 0;
		if (!w->open(names, why)) { td_io_set_error("td_stream_run: cannot create " + why); return TD_FAIL; }
	}
	td_stream_stats st{};
	uint64_t fnv = 1469598103934665603ULL;
	std::function<bool(Tuple&)> write;
	if (ctx) write = [&](Tuple& t) { return w->write_batch(t.b[0], nullptr, nullptr, 0); };
	else write = [&](Tuple& t) {
		// parse-only run: a checksum over what would have gone to the device (lengths and codes, in order)
		const Batch* b = t.b[0];
		for (int64_t i = 0; i < b->n; i++) {
			const int64_t l = b->offs[i + 1] - b->offs[i];
			fnv = (fnv ^ (uint64_t)l) * 1099511628211ULL;
			const uint8_t* s = b->codes + b->offs[i];
			for (int64_t j = 0; j < l; j++) fnv = (fnv ^ s[j]) * 1099511628211ULL;
		}
		return true;
	};
	td_ctx* const one[1] = { ctx };
	run_stages("td_stream_run: ", err, readers, { Target{ ctx ? one : nullptr, false, -1, judged } }, 1, pipeline_depth(ctx), w.get(),
	           [](const Tuple&) { return std::string(); }, write, st);
	if (!err.failed() && getenv("TD_STREAM_DEBUG"))
		fprintf(stderr, "td_stream: formatting %.3f s, appends %.3f s beside it (write stage %.3f s)\n", w ? w->dbg_format : 0.0, w ? w->dbg_pwrite : 0.0, st.write_s);
	st.wall_s = now_s() - t_start;
	st.codes_fnv = ctx ? 0 : fnv;
	if (stats) *stats = st;
	if (err.failed()) { td_io_set_error(err.message()); return TD_FAIL; }
	return TD_OK;
}

// A decode-only run: reader, then submit and wait, no writer and no output files -- what the context accumulates (its counters, a
// census, the molecule count's survey) is the result.
extern "C" int td_stream_survey(td_ctx* ctx, const char* in_path, const td_stream_opts* opts, td_stream_stats* stats)
{
	if (!ctx || !in_path) { td_io_set_error("td_stream_survey: needs a context and an input path"); return TD_FAIL; }
	const td_stream_opts o = resolve_opts(opts, artifacts_active(ctx));
	const double t_start = now_s();
	RunError err;
	std::vector<std::unique_ptr<Reader>> readers;
	readers.emplace_back(new Reader(err, o, false, true, o.n_threads));
	const bool judged = quality_active(ctx);
	readers[0]->want_qual = judged; readers[0]->path = in_path;
	std::string why;
	if (!readers[0]->src.open(in_path, o.block_bytes, why)) { td_io_set_error(why); return TD_FAIL; }
	td_stream_stats st{};
	td_ctx* const one[1] = { ctx };
	run_stages("td_stream_survey: ", err, readers, { Target{ one, false, -1, judged } }, 1, pipeline_depth(ctx), nullptr,
	           [](const Tuple&) { return std::string(); }, [](Tuple&) { return true; }, st);
	st.wall_s = now_s() - t_start;
	if (stats) *stats = st;
	if (err.failed()) { td_io_set_error(err.message()); return TD_FAIL; }
	return TD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Several input files of one run, several devices: the controller's loop for paired / three-read data
// (hmm_controller_multiple, src/barcode_hmm.c:244-385).
// ---------------------------------------------------------------------------------------------------------
namespace {

// dust_sequences(), src/barcode_hmm.c:2407-2467, on a read that nothing was removed from (run_rna_dust: the read as it was read)
bool rna_dust_low(const uint8_t* s, int64_t len, int dust_cut)
{
	if (len < 1) return false;
	int trip[64];
	for (int j = 0; j < 64; j++) trip[j] = 0;
	auto at = [&](int64_t k) -> unsigned { return k < len ? (unsigned)s[k] : 0u; };   // (the reference's sequences end in a 0 byte)
	unsigned key = ((at(0) & 3u) << 2) | (at(1) & 3u);
	const int64_t n = len > 64 ? 64 : len;
	int64_t c = 2;
	for (int64_t j = 2; j < n; j++) {
		key = ((key << 2) | (at(j) & 3u)) & 0x3Fu;
		trip[key]++;
		c++;
	}
	double sc = 0.0;
	for (int j = 0; j < 64; j++) sc += (double)trip[j] * ((double)trip[j] - 1.0) / 2.0;
	sc = sc / (double)(c - 3) * 10.0;
	return sc > (double)dust_cut;
}

// what the architectures and contexts of the input files say about the run (barcode_hmm.c:105-153)
struct MultiPlan {
	int bar_file = -1;                // the file that holds the barcode (at most one may), -1: none
	int num_out_reads = 0;            // read segments over all files
	int n_art = 0;                    // files whose contexts have a -ref artifact filter: none or all
	std::vector<int> read_present;    // read segments of every file
	std::vector<char> rna;            // run_rna_dust on the file's devices (TD_MODE_RNA_DUST)
	// pair mode (tagdust_molecules.h, mate mode): the contexts of the one decoded file report mate_bases > 0
	int mol_file = -1, mate_file = -1;   // the decoded file and its mate: the first file in call order other than it (-1: no pair mode)
	bool mate_filter = false;            // ... and its contexts report "mate_filter": the mate's outcome is joined on the device
	int qual_file = -1;                  // the decoded file whose contexts report "quality_filter" (tagdust_quality.h), -1: none
	// the join across input files (tagdust_samples.h): several files hold barcodes, bar_file is the primary; [file] JOIN_*
	std::vector<int> join;
};

// Several files hold barcodes: they make a join when there is one device, every one of them has contexts, exactly one of them
// reports "samples_join" and every other one "samples_export".  roles: [file] JOIN_*; *primary: the joining file.
bool join_roles(const td_stream_file* files, const int K, const int N, std::vector<int>& roles, int* primary)
{
	roles.assign((size_t)K, JOIN_NONE);
	*primary = -1;
	if (N != 1) return false;
	for (int k = 0; k < K; k++) {
		const td_arch* a = files[k].arch;
		bool has_bar = false;
		if (a) for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'B') has_bar = true;
		if (!has_bar) continue;
		if (!files[k].ctx || !files[k].ctx[0]) return false;
		int32_t joins = 0, exports = 0;
		(void)td_get_option(files[k].ctx[0], "samples_join", &joins);
		(void)td_get_option(files[k].ctx[0], "samples_export", &exports);
		if (joins > 0 && *primary < 0) { roles[(size_t)k] = JOIN_PRIMARY; *primary = k; }
		else if (exports != 0 && joins == 0) roles[(size_t)k] = JOIN_EXPORTER;
		else return false;
	}
	return *primary >= 0;
}

// false: the files cannot make a run (td_io_set_error says why)
bool plan_multi(const td_stream_file* files, const int K, const int N, const int32_t dust, MultiPlan& m)
{
	m.read_present.assign((size_t)K, 0);
	m.rna.assign((size_t)K, 0);
	m.join.assign((size_t)K, JOIN_NONE);
	int join_primary = -1;
	for (int k = 0; k < K; k++) {
		const td_arch* a = files[k].arch;
		if (!files[k].path || !a || a->n_segments < 1) { td_io_set_error("td_stream_run_multi: every input file needs a path and an architecture"); return false; }
		bool has_bar = false;
		for (int j = 0; j < a->n_segments; j++) { if (a->type[j] == 'B') has_bar = true; if (a->type[j] == 'R') m.read_present[(size_t)k]++; }
		if (has_bar) {
			// a second barcode file: only as a side of the join across input files, which its contexts and the others' must say
			if (m.bar_file >= 0 && join_primary < 0 && !join_roles(files, K, N, m.join, &join_primary)) {
				td_io_set_error("td_stream_run_multi: barcodes seem to be in both architectures (barcode_hmm.c:140-145)");
				return false;
			}
			if (m.bar_file < 0) m.bar_file = k;
		}
		m.num_out_reads += m.read_present[(size_t)k];
		// run_rna_dust (barcode_hmm.c:315-319) is what the controller runs instead of the HMM for an architecture that is one read segment
		const bool one_read = a->n_segments == 1 && a->type[0] == 'R';
		if (!files[k].ctx) {
			if (!one_read) { td_io_set_error("td_stream_run_multi: a file without contexts must have the architecture R:N"); return false; }
		} else {
			for (int d = 0; d < N; d++) if (!files[k].ctx[d]) { td_io_set_error("td_stream_run_multi: NULL context"); return false; }
			m.rna[(size_t)k] = one_read;
			m.n_art += artifacts_active(files[k].ctx[0]);
			if (one_read) {   // the devices run the DUST of this call
				int32_t cd = 0;
				(void)td_get_option(files[k].ctx[0], "dust", &cd);
				if (cd != dust) {
					td_io_set_error(std::string("td_stream_run_multi: ") + files[k].path + " (R:N) has contexts with dust " + std::to_string(cd) +
					                ", the call has dust " + std::to_string(dust));
					return false;
				}
			}
		}
	}
	if (join_primary >= 0) m.bar_file = join_primary;   // the file whose contexts hold the sheet names the output files and the samples
	// pair mode: a decoded file whose contexts are in mate mode takes the first other file's batches as its mate batches
	int n_decoded = 0, decoded = -1;
	for (int k = 0; k < K; k++) {
		if (!files[k].ctx || m.rna[(size_t)k]) continue;
		n_decoded++;
		for (int d = 0; d < N; d++) if (quality_active(files[k].ctx[d]) && m.qual_file < 0) m.qual_file = k;
		int32_t mb = 0;
		(void)td_get_option(files[k].ctx[0], "mate_bases", &mb);
		if (mb > 0 && decoded < 0) decoded = k;
	}
	int32_t mate_dust = 0;
	if (decoded >= 0) {
		int32_t mf = 0;
		(void)td_get_option(files[decoded].ctx[0], "mate_filter", &mf);
		(void)td_get_option(files[decoded].ctx[0], "dust", &mate_dust);
		m.mate_filter = mf != 0;
	}
	// the join across input files stands alone yet: a mate batch or a quality verdict of one file is not carried to the others
	if (join_primary >= 0 && decoded >= 0) {
		td_io_set_error(std::string("td_stream_run_multi: barcode calls are joined across input files (td_samples_join_enable) and mate mode is on in the contexts of ") +
		                files[decoded].path + ": the join and mate mode do not go together yet (td_mol_mate_disable)");
		return false;
	}
	if (join_primary >= 0 && m.qual_file >= 0) {
		td_io_set_error(std::string("td_stream_run_multi: barcode calls are joined across input files (td_samples_join_enable) and the base-quality filter is on in the "
		                            "contexts of ") + files[m.qual_file].path + ": the join and the filter do not go together yet (td_qual_disable)");
		return false;
	}
	// the base-quality filter: a batch's quality lines travel with its reads to one context, and one file's verdicts are the run's
	if (m.qual_file >= 0 && (N > 1 || n_decoded != 1)) {
		td_io_set_error("td_stream_run_multi: the base-quality filter is on (td_qual_enable) and " + (N > 1 ? std::to_string(N) + " devices are given: one device"
		                : std::to_string(n_decoded) + " files are decoded: exactly one may be, every other file must be R:N"));
		return false;
	}
	const int mate = decoded < 0 ? -1 : (decoded == 0 ? 1 : 0);
	// the mate filter (tagdust_molecules.h): one mate's outcome is joined in front of the count, a third file's would come behind it
	if (m.mate_filter && K >= 3 && (m.n_art > 0 || dust != 0 || mate_dust != 0)) {
		int third = 0;
		while (third == decoded || third == mate) third++;
		td_io_set_error(std::string("td_stream_run_multi: the mate filter is on with a -ref filter or DUST and ") + std::to_string(K) + " files are given: the outcome of " +
		                files[third].path + " would be joined behind the count, so a read of it that could fail would take a molecule's one kept read out of "
		                "the files (two files, or dust 0 and no filter)");
		return false;
	}
	// -ref (hmm_controller_multiple, barcode_hmm.c:209-214, :313-325): the controller hands the one FASTA to every file's step
	if (m.n_art > 0) {
		for (int k = 0; k < K; k++) {
			if (m.mate_filter && k == mate) continue;   // (the decoded file's contexts filter its reads as their mates)
			if (!files[k].ctx) {
				td_io_set_error(std::string("td_stream_run_multi: a -ref artifact filter is set, but ") + files[k].path +
				                " (R:N) has no contexts: its reads must be filtered too (give it contexts: TD_MODE_RNA_DUST)");
				return false;
			}
			if (!artifacts_active(files[k].ctx[0])) { td_io_set_error(std::string("td_stream_run_multi: a -ref artifact filter is set for some files but not for ") + files[k].path); return false; }
		}
	}
	if (decoded >= 0) {
		if (N > 1) { td_io_set_error("td_stream_run_multi: mate mode is on and " + std::to_string(N) + " devices are given: a mate batch travels with its reads to one context (one device)"); return false; }
		if (n_decoded != 1 || K < 2) {
			td_io_set_error("td_stream_run_multi: mate mode is on and " + std::to_string(n_decoded) + " of " + std::to_string(K) +
			                " files are decoded: exactly one may be, and every other file, at least one, must be R:N");
			return false;
		}
		for (int k = 0; k < K; k++) {
			const td_arch* a = files[k].arch;
			if (k != decoded && !(a->n_segments == 1 && a->type[0] == 'R')) {
				td_io_set_error(std::string("td_stream_run_multi: mate mode is on and ") + files[k].path + " is not R:N: every file but the decoded one must be");
				return false;
			}
		}
		const int32_t cd = mate_dust;
		if (m.mate_filter && cd != dust) {   // (the decoded file's contexts run the DUST of this call over the mates)
			td_io_set_error(std::string("td_stream_run_multi: the mate filter is on and ") + files[decoded].path + " has contexts with dust " + std::to_string(cd) +
			                ", the call has dust " + std::to_string(dust));
			return false;
		}
		if (!m.mate_filter && (m.n_art > 0 || dust != 0 || cd != 0)) {
			td_io_set_error("td_stream_run_multi: mate mode is on with a -ref filter or DUST: the mate's own outcome is not joined to the count, so a mate "
			                "that could fail would take a molecule's one kept read out of the files (run with dust 0 and without a filter)");
			return false;
		}
		m.mol_file = decoded;
		m.mate_file = mate;
	}
	if (m.num_out_reads == 0) { td_io_set_error("td_stream_run_multi: no read segment in any architecture: no output files to create (io.c:846-852)"); return false; }
	return true;
}

} // namespace

extern "C" int td_stream_run_multi(const td_stream_file* files, int32_t n_files, int32_t n_devices, const char* out_prefix, int32_t dust,
                                   const td_stream_opts* opts, td_stream_stats* stats, int64_t* counts)
{
	return td_stream_run_multi_hits(files, n_files, n_devices, out_prefix, dust, opts, stats, counts, nullptr, 0);
}

extern "C" int td_stream_run_multi_hits(const td_stream_file* files, int32_t n_files, int32_t n_devices, const char* out_prefix, int32_t dust,
                                        const td_stream_opts* opts, td_stream_stats* stats, int64_t* counts, int64_t* artifact_hits,
                                        int32_t n_artifacts)
{
	if (!files || n_files < 1 || n_files > 8 || !out_prefix) { td_io_set_error("td_stream_run_multi: bad arguments (1..8 input files, an output prefix)"); return TD_FAIL; }
	if (n_devices < 1) n_devices = 1;
	const int K = n_files, N = n_devices;
	MultiPlan m;
	if (!plan_multi(files, K, N, dust, m)) return TD_FAIL;
	const td_stream_opts o = resolve_opts(opts, m.n_art > 0);
	td_ctx* first_ctx = nullptr;
	for (int k = 0; k < K && !first_ctx; k++) if (files[k].ctx) first_ctx = files[k].ctx[0];
	const double t_start = now_s();

	RunError err;
	// print_all() names its files after param->read_structure: the barcode file's architecture, else the last file's
	std::vector<std::string> names;
	int num_alternatives = 2;
	std::string why;
	std::vector<std::string> samples;   // sample assignment: on in the contexts of the barcode file
	if (m.bar_file >= 0 && files[m.bar_file].ctx && !td_stream_sample_names(files[m.bar_file].ctx, N, samples, why)) {
		td_io_set_error("td_stream_run_multi: " + why);
		return TD_FAIL;
	}
	if (samples.empty()) td_writer_file_names_n(out_prefix, files[m.bar_file >= 0 ? m.bar_file : K - 1].arch, m.num_out_reads, names, &num_alternatives);
	else td_writer_file_names_samples(out_prefix, samples, m.num_out_reads, names, &num_alternatives);
	Writer w(err, o.n_threads, num_alternatives);
	w.fingerprint_text = o.fingerprint_text != 0;
	if (!w.open(names, why)) { td_io_set_error("td_stream_run_multi: cannot create " + why); return TD_FAIL; }
	std::vector<size_t> file_base((size_t)K, 0);      // io.c:917-1001: c
	{ size_t c = 0; for (int k = 0; k < K; k++) { file_base[(size_t)k] = c; c += (size_t)num_alternatives * (size_t)m.read_present[(size_t)k]; } }
	std::vector<std::unique_ptr<Reader>> readers;
	std::vector<Target> dev;
	for (int k = 0; k < K; k++) {
		// (a file that is not decoded needs no page-locked buffers, nor does one whose reads come back unchanged need room for rewritten ones)
		// (... but the mate file of pair mode does: its batches are uploaded from where they lie)
		readers.emplace_back(new Reader(err, o, files[k].ctx == nullptr && k != m.mate_file, files[k].ctx != nullptr && !m.rna[(size_t)k], std::max(1, o.n_threads / K)));
		dev.push_back(Target{ files[k].ctx, m.rna[(size_t)k] != 0, k == m.mol_file ? m.mate_file : -1, k == m.qual_file, m.join[(size_t)k] });
		readers.back()->want_qual = k == m.qual_file; readers.back()->path = files[k].path;
		if (!readers.back()->src.open(files[k].path, o.block_bytes, why)) { td_io_set_error(why); return TD_FAIL; }
	}

	// barcode_hmm.c:257-289: the files hold the same number of records, and the first 1000 names of every pair of files name the same reads
	bool first = true;
	int name_format = -1;
	std::vector<const char*> paths;
	for (int k = 0; k < K; k++) paths.push_back(files[k].path);
	auto check = [&](const Tuple& t) { return lockstep_objection("td_stream_run_multi: ", t.b.data(), paths.data(), K, first, name_format); };
	// the write stage: run_rna_dust for the files that no device sees, the per-record combination, print_all
	int64_t cnt[TD_NUM_COUNTERS];
	for (int q = 0; q < TD_NUM_COUNTERS; q++) cnt[q] = 0;
	if (artifact_hits) for (int32_t q = 0; q < n_artifacts; q++) artifact_hits[q] = 0;
	std::vector<int32_t> ctype, cbar;
	auto write = [&](Tuple& t) -> bool {
		const int64_t n = t.b[0]->n;
		for (int k = 0; k < K; k++) {
			Batch* b = t.b[(size_t)k];
			if (files[k].ctx && !m.rna[(size_t)k]) { b->seq_src = nullptr; continue; }
			b->seq_src = b->codes;
			if (files[k].ctx) continue;             // (TD_MODE_RNA_DUST ran on the file's devices)
			const int64_t chunk = 16384, nch = (n + chunk - 1) / chunk;
			w.pool.run(nch, [&](int64_t c) {        // do_rna_dust, barcode_hmm.c:2370-2395 (no -ref filter: a run with one has contexts here)
				for (int64_t i = c * chunk; i < std::min(n, (c + 1) * chunk); i++) {
					td_read_result& r = b->res[i];
					memset(&r, 0, sizeof r);
					r.mapq = -1.0f; r.barcode = -1; r.fingerprint = -1;        // read_fasta_fastq's defaults, io.c:1698-1702
					r.read_type = TD_EXTRACT_SUCCESS;
					// (the mate filter: the device has judged this file's reads as mates, and the decoded record carries the maximum)
					if (m.mate_filter && k == m.mate_file) continue;
					if (dust && rna_dust_low(b->codes + b->offs[i], b->offs[i + 1] - b->offs[i], dust)) r.read_type = TD_EXTRACT_FAIL_LOW_COMPLEXITY;
				}
			});
		}
		ctype.resize((size_t)n); cbar.resize((size_t)n);
		for (int64_t i = 0; i < n; i++) {          // barcode_hmm.c:329-351
			int32_t c = -100000;
			for (int k = 0; k < K; k++) c = std::max(c, t.b[(size_t)k]->res[i].read_type);
			ctype[(size_t)i] = c;
			cbar[(size_t)i] = t.b[(size_t)(m.bar_file >= 0 ? m.bar_file : 0)]->res[i].barcode;
			// the controller's counting, :354-384; a duplicate (dedup, tagdust_molecules.h) counts as the extracted read it was decoded
			// as, under its barcode bin: what the single-file run's device counters do
			// ... and a read the base-quality filter dropped (tagdust_quality.h) as what its file says it is, not extracted: slot 3
			const int32_t cc = (c & 0xFF) == TD_EXTRACT_DUPLICATE ? TD_EXTRACT_SUCCESS : (c == TD_EXTRACT_FAIL_LOW_BASE_QUALITY ? TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND : c);
			cnt[cc & (TD_NUM_OUTCOME_SLOTS - 1)]++;
			if (cc == TD_EXTRACT_SUCCESS && cbar[(size_t)i] >= 0) cnt[TD_NUM_OUTCOME_SLOTS + (cbar[(size_t)i] & 0xFF)]++;
			// reference_fasta->mer_hash (:381): on the combined outcome, which is the largest of the files' -- of two files' hits the later sequence
			if (artifact_hits && (c & 0xFF) == TD_EXTRACT_FAIL_MATCHES_ARTIFACTS && (c >> 8) >= 1 && (c >> 8) <= n_artifacts) artifact_hits[(c >> 8) - 1]++;
		}
		bool ok = true;
		for (int k = 0; k < K && ok; k++)
			if (m.read_present[(size_t)k] > 0) ok = w.write_batch(t.b[(size_t)k], ctype.data(), cbar.data(), file_base[(size_t)k]);
		for (Batch* b : t.b) b->seq_src = nullptr;
		return ok;
	};
	td_stream_stats st{};
	run_stages("td_stream_run_multi: ", err, readers, dev, N, pipeline_depth(first_ctx), &w, check, write, st);
	st.wall_s = now_s() - t_start;
	if (stats) *stats = st;
	if (counts) for (int q = 0; q < TD_NUM_COUNTERS; q++) counts[q] = cnt[q];
	if (err.failed()) { td_io_set_error(err.message()); return TD_FAIL; }
	return TD_OK;
}
