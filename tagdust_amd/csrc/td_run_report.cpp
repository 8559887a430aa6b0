// td_run_report.cpp -- what a whole run (include/tagdust_run.h) says: the log (append_message(), src/misc.c:285-335; free_param(),
// src/interface.c:715-726), the summary block (src/barcode_hmm.c:387-430) and the texts of <out>_unknown_barcodes.txt,
// <out>_samples.txt and <out>_molecules.txt, each a pure function of what the run gathered into its report.  Plain C++ over
// td_census_host.cpp (td_census_key_text, td_census_free) and td_samples_host.cpp (td_samples_key, td_samples_key_calls).
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "td_run_internal.h"

namespace tdrun {

void Log::add(const std::string& msg)
{
	char stamp[64];
	const time_t now = time(nullptr);
	struct tm tmv;
	localtime_r(&now, &tmv);
	strftime(stamp, sizeof stamp, "[%F %H:%M:%S]\t", &tmv);
	if (echo) fprintf(stderr, "%s%s", stamp, msg.c_str());
	text += stamp;
	text += msg;
}

void Log::addf(const char* fmt, ...)
{
	char buf[2048];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	add(buf);
}

void Log::write(const char* outfile) const
{
	if (!outfile) return;
	const std::string name = std::string(outfile) + "_logfile.txt";
	if (FILE* f = fopen(name.c_str(), "w")) { fprintf(f, "%s\n", text.c_str()); fclose(f); }
}

std::vector<std::string> summary_messages(const td_run_opts* o, const td_run_report* r)
{
	std::vector<std::string> m;
	char b[2048];
	auto addf = [&](const char* fmt, ...) {
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(b, sizeof b, fmt, ap);
		va_end(ap);
		m.push_back(b);
	};
	int64_t total = 0;
	for (int q = 0; q < TD_NUM_OUTCOME_SLOTS; q++) total += r->counts[q];
	const int64_t ok = r->counts[TD_EXTRACT_SUCCESS];
	addf("Done.\n\n");
	for (int k = 0; k < o->n_infiles; k++) addf("%s\tInput file %d.\n", o->infile[k], k);
	addf("%d\ttotal input reads\n", (int)total);
	addf("%0.2f\tselected threshold\n", (double)r->selected_threshold);
	addf("%d\tsuccessfully extracted\n", (int)ok);
	addf("%0.1f%%\textracted\n", (double)((float)ok / (float)total * 100.0f));
	addf("%d\tproblems with architecture\n", (int)r->counts[TD_EXTRACT_FAIL_ARCHITECTURE_MISMATCH]);
	addf("%d\tbarcode / UMI not found\n", (int)r->counts[TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND]);
	addf("%d\ttoo short\n", (int)r->counts[TD_EXTRACT_FAIL_READ_TOO_SHORT]);
	addf("%d\tlow complexity\n", (int)r->counts[TD_EXTRACT_FAIL_LOW_COMPLEXITY]);
	addf("%d\tmatch artifacts:\n", (int)r->counts[TD_EXTRACT_FAIL_MATCHES_ARTIFACTS]);
	for (int j = 0; j < r->n_artifacts; j++)
		if (r->artifact_hits && r->artifact_hits[j]) addf("%d\t%s\n", (int)r->artifact_hits[j], r->artifact_names && r->artifact_names[j] ? r->artifact_names[j] : "");
	// --min-base-quality: one line behind the counts (only with the option: a report made without it may end in front of these fields)
	if (o->min_base_quality && r->quality)
		addf("%d\tlow base quality in barcode / UMI (Q < %d, more than %d bases)\n", (int)r->quality_totals.failed, o->min_base_quality, o->max_low_bases);
	return m;
}

namespace {

// printf behind a text of any length
void appendf(std::string& s, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void appendf(std::string& s, const char* fmt, ...)
{
	va_list ap, ap2;
	va_start(ap, fmt);
	va_copy(ap2, ap);
	const int n = vsnprintf(nullptr, 0, fmt, ap);
	va_end(ap);
	const size_t at = s.size();
	s.resize(at + (size_t)n + 1);
	vsnprintf(&s[at], (size_t)n + 1, fmt, ap2);
	va_end(ap2);
	s.resize(at + (size_t)n);
}

// Levenshtein distance of two short words
int edit_distance(const std::string& a, const std::string& b)
{
	std::vector<int> row(b.size() + 1);
	for (size_t j = 0; j <= b.size(); j++) row[j] = (int)j;
	for (size_t i = 1; i <= a.size(); i++) {
		int diag = row[0];
		row[0] = (int)i;
		for (size_t j = 1; j <= b.size(); j++) {
			const int up = row[j];
			row[j] = std::min(std::min(row[j] + 1, row[j - 1] + 1), diag + (a[i - 1] != b[j - 1]));
			diag = up;
		}
	}
	return row[b.size()];
}

}   // namespace

// --unknown-barcodes: the K most frequent spellings of the last 'B' segment, each with the listed barcode nearest to it
bool unknown_barcodes_text(const td_run_opts* o, const td_arch* a, const std::vector<std::string>& segs, const char* infile, const td_run_report& r, std::string& out)
{
	const td_census_totals& sum = r.unknown_totals;
	const int seg = last_barcode_segment(a);
	appendf(out, "# unknown barcodes: what the reads that were not extracted spell in segment %d (%s) of %s\n", seg + 1, segs[(size_t)seg].c_str(), infile);
	appendf(out, "# eligible reads\t%lld\n# counted\t%lld\n# distinct sequences\t%lld\n# no base in the segment\t%lld\n# more than %d bases\t%lld\n# with N\t%lld\n",
	        (long long)sum.eligible, (long long)sum.counted, (long long)sum.distinct, (long long)sum.skipped_empty, TD_CENSUS_MAX_WORD,
	        (long long)sum.skipped_long, (long long)sum.skipped_n);
	if (sum.overflow > 0)
		appendf(out, "# the counting table was too small: %lld reads were not counted (the counts below are exact; --unknown-barcodes-slots %d or more)\n",
		        (long long)sum.overflow, o->unknown_slots_log2 + 1);
	appendf(out, "# count\tsequence\tnearest\tdistance\n");
	const int n_listed = a->n_seq[seg] - 1;   // (the last one is the all-N wildcard)
	for (int64_t i = 0; i < r.n_unknown && i < o->unknown_barcodes; i++) {
		char word[32];
		if (td_census_key_text(r.unknown[i].key, word) != TD_OK) return false;
		int best = -1, best_d = 0;
		for (int q = 0; q < n_listed; q++) {
			const int d = edit_distance(word, a->seqs[seg][q]);
			if (best < 0 || d < best_d) { best = q; best_d = d; }   // (ties go to the lower index)
		}
		appendf(out, "%lld\t%s\t%s\t%d\n", (long long)r.unknown[i].count, word, best >= 0 ? a->seqs[seg][best] : "-", best >= 0 ? best_d : -1);
	}
	return true;
}

// --samples: one line per sample of the sheet, then the combinations no sample has
// One text for both forms: column t of the sheet is segment sheet.segs[t] of col_arch[t], spelled col_segs[t]; col_file != NULL: the
// join across input files, every column is named with its file and the reads whose partner failed get a line
static bool samples_text_columns(const td_run_opts* o, const std::vector<const td_arch*>& col_arch, const std::vector<std::string>& col_segs,
                                 const std::vector<const char*>* col_file, const char* infile, const SampleSheet& sheet, const td_run_report& r, std::string& out)
{
	const td_samples_totals& sum = r.samples_totals;
	const td_census_entry* acc = r.samples;
	const int64_t n_acc = r.n_sample_keys;
	const int m = (int)sheet.segs.size();
	appendf(out, "# samples: the extracted reads of %s by all their barcodes\n# sheet\t%s\n# samples\t%d\n# segments", infile, o->samples_file, sheet.n());
	for (int t = 0; t < m; t++) {
		if (!col_file) appendf(out, "\t%d (%s)", sheet.segs[(size_t)t] + 1, col_segs[(size_t)t].c_str());
		else appendf(out, "\t%d of %s (%s)", sheet.segs[(size_t)t] + 1, (*col_file)[(size_t)t], col_segs[(size_t)t].c_str());
	}
	appendf(out, "\n# extracted reads\t%lld\n# assigned\t%lld\n# not in the sheet\t%lld\n# incomplete\t%lld\n# not counted\t%lld\n", (long long)sum.eligible,
	        (long long)sum.assigned, (long long)sum.unlisted, (long long)sum.incomplete, (long long)sum.overflow);
	if (col_file) appendf(out, "# partner failed\t%lld\n", (long long)r.partner_failed);
	if (sum.overflow > 0) appendf(out, "# the counting table was too small: the counts below are exact, %lld reads are in none of them\n", (long long)sum.overflow);
	out += "# sample";
	for (int t = 0; t < m; t++) appendf(out, "\tbarcode %d", t + 1);
	out += "\treads\tshare\n";
	std::vector<char> listed((size_t)std::max<int64_t>(n_acc, 1), 0);
	for (int s = 0; s < sheet.n(); s++) {
		const uint64_t key = td_samples_key(sheet.tuples.data() + (size_t)s * m, m);
		int64_t reads = 0;
		for (int64_t i = 0; i < n_acc; i++) if (acc[i].key == key) { reads = acc[i].count; listed[(size_t)i] = 1; }
		out += sheet.names[(size_t)s];
		for (int t = 0; t < m; t++) appendf(out, "\t%s", col_arch[(size_t)t]->seqs[sheet.segs[(size_t)t]][sheet.tuples[(size_t)s * m + t]]);
		appendf(out, "\t%lld\t%0.4f\n", (long long)reads, sum.eligible > 0 ? (double)reads / (double)sum.eligible : 0.0);
	}
	out += "# combinations not in the sheet\n";
	for (int64_t i = 0; i < n_acc; i++) {   // (td_samples_get's order: count descending, then key ascending)
		if (listed[(size_t)i]) continue;
		int32_t calls[TD_SAMPLES_MAX_SEGMENTS], km = 0;
		if (td_samples_key_calls(acc[i].key, calls, &km) != TD_OK || km != m) { run_fail("--samples: 0x%llx is no key of %d segments", (unsigned long long)acc[i].key, m); return false; }
		for (int t = 0; t < m; t++) {
			const int seg = sheet.segs[(size_t)t];
			const td_arch* a = col_arch[(size_t)t];
			appendf(out, "%s%s", t ? "\t" : "", calls[t] < 0 || calls[t] >= a->n_seq[seg] ? "-" : a->seqs[seg][calls[t]]);   // (the decoy's own spelling is its N's)
		}
		appendf(out, "\t%lld\t%0.4f\n", (long long)acc[i].count, sum.eligible > 0 ? (double)acc[i].count / (double)sum.eligible : 0.0);
	}
	return true;
}

bool samples_text(const td_run_opts* o, const td_arch* a, const std::vector<std::string>& segs, const char* infile, const SampleSheet& sheet,
                  const td_run_report& r, std::string& out)
{
	std::vector<std::string> col_segs;
	for (const int seg : sheet.segs) col_segs.push_back(segs[(size_t)seg]);
	return samples_text_columns(o, std::vector<const td_arch*>(sheet.segs.size(), a), col_segs, nullptr, infile, sheet, r, out);
}

bool samples_text_join(const td_run_opts* o, const std::vector<const td_arch*>& archs, const std::vector<std::vector<std::string>>& segs,
                       const char* const* infile, const SampleSheet& sheet, const td_run_report& r, std::string& out)
{
	std::vector<const td_arch*> col_arch;
	std::vector<std::string> col_segs;
	std::vector<const char*> col_file;
	for (size_t t = 0; t < sheet.segs.size(); t++) {
		const size_t k = (size_t)sheet.files[t];
		col_arch.push_back(archs[k]); col_segs.push_back(segs[k][(size_t)sheet.segs[t]]); col_file.push_back(infile[k]);
	}
	return samples_text_columns(o, col_arch, col_segs, &col_file, infile[sheet.files[0]], sheet, r, out);
}

// --molecules: one row per sample, per listed barcode of the last 'B' segment, or one "-" row; then the total
std::string molecules_text(const td_run_opts* o, const td_arch* a, const char* infile, const char* mate_infile, int dust, bool use_ref,
                           const SampleSheet& sheet, const td_run_report& r)
{
	const td_mol_totals& sum = r.molecules_totals;
	const td_mol_row* rows = r.molecules;
	const td_mol_row* crows = r.molecules_collapsed;   // (--collapse-umis: the rows after the collapse)
	std::string out;
	appendf(out, "# molecules: the extracted reads of %s by barcode, fingerprint and the first bases of the read\n", infile);
	appendf(out, "# prefix bases\t%d\n", o->molecules_prefix);
	if (o->mate_bases) appendf(out, "# mate bases\t%d\n# mate file\t%s\n", o->mate_bases, mate_infile);
	if (o->mate_filter) appendf(out, "# mate filter\tdust %d, -ref %s\n", dust, use_ref ? o->reference_fasta : "none");
	appendf(out, "# extracted reads\t%lld\n# counted\t%lld\n# molecules\t%lld\n# no read base\t%lld\n# N in the prefix\t%lld\n",
	        (long long)sum.eligible, (long long)sum.counted, (long long)sum.molecules, (long long)sum.skipped_empty, (long long)sum.skipped_n);
	if (sum.overflow > 0)
		appendf(out, "# the counting table was too small: %lld reads were not counted (the counts below are exact; --molecules-slots %d or more)\n",
		        (long long)sum.overflow, o->molecules_slots_log2 + 1);
	if (o->dedup_collapsed) out += "# dedup\tcollapsed molecules\n";
	if (o->dedup)
		appendf(out, "# written\t%lld\n# duplicates removed\t%lld\n", (long long)r.dedup_totals.kept, (long long)r.dedup_totals.duplicates);
	if (crows)
		appendf(out, "# UMI collapse\tfingerprints one mismatch apart, directional rule\n# molecules after collapse\t%lld\n# absorbed\t%lld\n",
		        (long long)r.collapse_totals.molecules_after, (long long)r.collapse_totals.absorbed);
	appendf(out, "# barcode\treads\tmolecules\tduplication\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10+%s\n", crows ? "\tcollapsed\tduplication_collapsed" : "");
	// (collapsed: the molecules of the row after the collapse, with --collapse-umis)
	auto line = [&](const char* label, const td_mol_row& row, int64_t collapsed) {
		appendf(out, "%s\t%lld\t%lld\t%0.4f", label, (long long)row.reads, (long long)row.molecules,
		        row.reads > 0 ? 1.0 - (double)row.molecules / (double)row.reads : 0.0);
		for (int q = 0; q < TD_MOL_LEVELS; q++) appendf(out, "\t%lld", (long long)row.levels[q]);
		if (crows) appendf(out, "\t%lld\t%0.4f", (long long)collapsed, row.reads > 0 ? 1.0 - (double)collapsed / (double)row.reads : 0.0);
		out += "\n";
	};
	const int seg = last_barcode_segment(a);
	if (sheet.n() > 0 && seg >= 0) {   // --samples: a bin is a sample
		for (int q = 0; q < sheet.n(); q++) line(sheet.names[(size_t)q].c_str(), rows[q], crows ? crows[q].molecules : 0);
	} else if (seg >= 0) {
		const int n_listed = std::min(a->n_seq[seg] - 1, (int)TD_NUM_BARCODE_BINS);   // (the last one is the all-N wildcard)
		for (int q = 0; q < n_listed; q++) line(a->seqs[seg][q], rows[q], crows ? crows[q].molecules : 0);
	} else {
		line("-", rows[0], crows ? crows[0].molecules : 0);
	}
	td_mol_row total{};
	int64_t total_collapsed = 0;
	for (int b = 0; b < TD_NUM_BARCODE_BINS; b++) {
		total.reads += rows[b].reads; total.molecules += rows[b].molecules;
		for (int q = 0; q < TD_MOL_LEVELS; q++) total.levels[q] += rows[b].levels[q];
		if (crows) total_collapsed += crows[b].molecules;
	}
	line("total", total, total_collapsed);
	return out;
}

}   // namespace tdrun

using namespace tdrun;

extern "C" int64_t td_run_format_summary(const td_run_opts* o, const td_run_report* r, char* buf, int64_t cap)
{
	if (!o || !r) return 0;
	std::string s;
	for (auto& m : summary_messages(o, r)) s += m;
	return copy_out(s, buf, cap);
}

extern "C" void td_run_report_clear(td_run_report* r)
{
	if (!r) return;
	if (r->artifact_names) for (int j = 0; j < r->n_artifacts; j++) free(r->artifact_names[j]);
	free(r->artifact_names); free(r->artifact_hits); free(r->log);
	td_census_free(r->unknown);
	td_census_free(r->samples);
	free(r->molecules);
	free(r->molecules_collapsed);
	for (int k = 0; k < TD_RUN_MAX_FILES; k++) free(r->architectures[k]);
	memset(r, 0, sizeof *r);
}
