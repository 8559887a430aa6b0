// td_run_internal.h -- what the units of the whole-run driver (include/tagdust_run.h) share: td_run_opts.cpp (options),
// td_run_plan.cpp (architectures, sample sheet, which file plays which part, the plan), td_run_report.cpp (log, summary, the texts
// of the report files) and td_run.cpp (the run itself).  The first three are plain C++ over plain C++ units: no HIP header, no call
// into a .hip unit; tools/run_host_check.cpp links them without the device layer.  Nothing here is part of the library's interface.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tagdust_run.h"

namespace tdrun {

// ---- the message of a failed call (td_run_last_error), per thread: td_run_opts.cpp ----
extern thread_local std::string g_run_error;
int run_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

inline char* dup_str(const char* s) { return s ? strdup(s) : nullptr; }
inline bool file_exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }   // misc.c:file_exists

// a text into a caller's buffer: at most cap - 1 bytes + NUL; the whole length is returned
inline int64_t copy_out(const std::string& s, char* buf, int64_t cap)
{
	if (buf && cap > 0) {
		const int64_t n = std::min<int64_t>((int64_t)s.size(), cap - 1);
		memcpy(buf, s.data(), (size_t)n);
		buf[n] = 0;
	}
	return (int64_t)s.size();
}

// ---- architectures: td_run_plan.cpp ----
struct ArchDeleter { void operator()(td_arch* a) const { td_arch_free(a); } };
typedef std::unique_ptr<td_arch, ArchDeleter> ArchPtr;

// segments as "-1 B:ACGT -2 R:N" (pretty_print_selected_architecture's form, without "Using: ")
std::string segments_text(const std::vector<std::string>& segs);
// QC_read_structure (interface.c:759-829) as far as it can fail, and td_arch_parse's own checks: no segment skipped, one length per segment
bool parse_arch(const std::vector<std::string>& segs, ArchPtr& out, std::string& why);

inline bool is_read_only(const td_arch* a) { return a->n_segments == 1 && a->type[0] == 'R'; }
inline bool has_fingerprint(const td_arch* a) { for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'F') return true; return false; }
inline bool has_barcode(const td_arch* a) { for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'B') return true; return false; }
inline int read_segments(const td_arch* a) { int n = 0; for (int j = 0; j < a->n_segments; j++) n += a->type[j] == 'R'; return n; }
inline int last_barcode_segment(const td_arch* a) { int seg = -1; for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'B') seg = j; return seg; }

struct ArchFile {
	std::vector<std::string> lines;                    // the candidates' lines as read (duplicates are an error)
	std::vector<std::vector<std::string>> segs;
};
bool read_arch_file(const char* path, ArchFile& af, std::string& why);

// --samples FILE (tagdust_samples.h): one sample per line -- the name, then one barcode spelling per 'B' segment as the architecture
// lists them, separated by white space; '#' lines and blank lines are skipped
struct SampleSheet {
	std::vector<int> segs;                 // the 'B' segments of the architecture, in order (--join-barcodes: of every barcode file, files first)
	std::vector<int> files;                // --join-barcodes: the input file of every column (empty without the option: all of the barcode file)
	std::vector<std::string> names;
	std::vector<int32_t> tuples;           // [names.size() * segs.size()]
	int n() const { return (int)names.size(); }
};
// TD_FAIL with a message that names the line.  The sheet's own rules (rows and names pairwise different, the name's characters) are
// checked here too, so that the plan refuses what td_samples_enable would.
int read_sample_sheet(const char* path, const td_arch* a, SampleSheet& sh);
// --join-barcodes: the sheet's columns are the 'B' segments of the files `bar_files` (indices into archs and infile), files first;
// a message names file and segment of the column it is about
int read_sample_sheet_join(const char* path, const std::vector<const td_arch*>& archs, const std::vector<int>& bar_files, const char* const* infile,
                           SampleSheet& sh);

// Which file plays which part, once every file's architecture is known (barcode_hmm.c:130-159): decided in one place, for the plan,
// for td_run_output_files_describe and for the run.
struct RunRoles {
	int bar_file = -1;                     // the one file whose architecture has a barcode segment (-1: none)
	int num_out_reads = 0;                 // read segments of all files together
	std::vector<std::string> out_files;    // every file the run writes, the reports among them
	int mol_file = 0;                      // the file whose contexts count molecules: file 0, or with --mate-bases the one decoded file
	int mate_file = -1;                    // ... its mate with --mate-bases, else -1
	int qual_file = -1;                    // --min-base-quality: the one decoded file, whose context judges (-1 without the option)
	std::vector<int> bar_files;            // --join-barcodes: every file whose architecture has a barcode segment, in call order; bar_file is
	                                       // the first of them, whose contexts hold the sheet (empty without the option)
	std::vector<int> first_column;         // ... [bar_files.size()] the sheet column of each one's first 'B' segment
	std::vector<int32_t> column_hmms;      // ... [columns] the HMMs of every column's segment (its barcodes and the all-N decoy)
	std::string join_line;                 // ... the plan's "join:" line
	SampleSheet sheet;                     // --samples, resolved against the barcode file's architecture (no sample without the option)
};
// TD_FAIL with the reference's message, or this library's for its own options
int decide_roles(const td_run_opts* o, const std::vector<const td_arch*>& archs, RunRoles& r);
// --mate-filter with DUST or -ref: the outcome of one mate is joined on the device, a third file's is not
int mate_filter_files(const td_run_opts* o, int dust, bool use_ref, const RunRoles& r);

inline std::string samples_file_name(const td_run_opts* o) { return std::string(o->outfile) + "_samples.txt"; }
inline std::string unknown_file_name(const td_run_opts* o) { return std::string(o->outfile) + "_unknown_barcodes.txt"; }
inline std::string molecules_file_name(const td_run_opts* o) { return std::string(o->outfile) + "_molecules.txt"; }

enum { SRC_CMDLINE = 0, SRC_ARCH_FILE = 1, SRC_DEFAULT = 2 };

// ---- log and report texts: td_run_report.cpp ----
// append_message(), misc.c:285-335: "[YYYY-MM-DD HH:MM:SS]\t" in front of every message; the messages end in '\n' themselves
struct Log {
	std::string text;
	bool echo = false;
	void add(const std::string& msg);
	void addf(const char* fmt, ...) __attribute__((format(printf, 2, 3)));
	void write(const char* outfile) const;   // free_param(), interface.c:715-726
};

// the messages of barcode_hmm.c:387-430
std::vector<std::string> summary_messages(const td_run_opts* o, const td_run_report* r);

// The bytes of <out>_unknown_barcodes.txt, <out>_samples.txt and <out>_molecules.txt from what the run gathered into the report.
// a / segs / infile: the architecture, segment strings and name of the file the report is about (the barcode file; for the molecules
// the counting file, mate_infile its mate with --mate-bases).  false: an entry's key cannot be read; `out` holds the text up to it,
// and the message is td_census_key_text's own (the caller's to fetch) or, for the samples, in g_run_error.
bool unknown_barcodes_text(const td_run_opts* o, const td_arch* a, const std::vector<std::string>& segs, const char* infile, const td_run_report& r, std::string& out);
bool samples_text(const td_run_opts* o, const td_arch* a, const std::vector<std::string>& segs, const char* infile, const SampleSheet& sheet,
                  const td_run_report& r, std::string& out);
// ... with --join-barcodes: a column's architecture, segment strings and file name are those of sheet.files[t] in archs / segs / infile
bool samples_text_join(const td_run_opts* o, const std::vector<const td_arch*>& archs, const std::vector<std::vector<std::string>>& segs,
                       const char* const* infile, const SampleSheet& sheet, const td_run_report& r, std::string& out);
std::string molecules_text(const td_run_opts* o, const td_arch* a, const char* infile, const char* mate_infile, int dust, bool use_ref,
                           const SampleSheet& sheet, const td_run_report& r);

}   // namespace tdrun

struct td_run_plan_t {
	std::vector<int> source;                 // per input file
	std::vector<std::vector<std::string>> segs;   // ... its segments when no data is needed to know them
	tdrun::ArchFile arch_file;
	bool all_known = false;                  // no file waits for the arch file's choice
	tdrun::RunRoles roles;                   // valid when all_known
	std::vector<std::string> warnings;
	int dust = 0;
	bool use_ref = false;
	bool dedup = false;
	bool collapse = false;
	bool dedup_collapsed = false;
	int mate_bases = 0;                      // --mate-bases: 0 = off
	bool mate_filter = false;                // --mate-filter
	std::string ref_file;                    // -ref, for the plan's "mate:" line
	std::string samples_line;                // --samples: the plan's "samples:" line
	std::string quality_line;                // --min-base-quality: the plan's "quality:" line
};
