// td_run_plan.cpp -- the decisions of a whole run that need no data and no device (include/tagdust_run.h): the checks of the
// reference's main() (src/main.c:103-125), the arch file's candidates (src/test_architectures.c:72-133), the sample sheet, and
// which file plays which part once every architecture is known (hmm_controller_multiple(), src/barcode_hmm.c:105-159).
// Plain C++ over td_model.cpp (td_arch_parse) and td_fastq.cpp (the output files' names).
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>

#include "td_run_internal.h"
#include "td_io_internal.h"

namespace {

// byg_end (misc.c:160-205): the index behind the first occurrence of pattern in text, 0 when there is none
size_t find_end(const std::string& text, const std::string& pattern)
{
	const size_t p = text.find(pattern);
	return p == std::string::npos ? 0 : p + pattern.size();
}

// One line of an arch file (test_architectures.c:72-111): a line that contains "tagdust"; options -1 .. -9 and, as the reference
// spells the tenth, "-:" ((char)(9 + 49)); the value is the word behind the first occurrence of the option's two characters.  A
// line without -1 is no architecture.
bool arch_line_segments(const std::string& line, std::vector<std::string>& segs)
{
	segs.clear();
	if (!find_end(line, "tagdust")) return false;
	std::vector<std::string> found(TD_RUN_MAX_SEGMENTS);
	int last = -1;
	for (int c = 0; c < TD_RUN_MAX_SEGMENTS; c++) {
		const std::string opt = { '-', (char)(c + 49) };
		size_t at = find_end(line, opt);
		if (!at) { if (!c) return false; continue; }
		while (at < line.size() && isspace((unsigned char)line[at])) at++;
		size_t e = at;
		while (e < line.size() && !isspace((unsigned char)line[e])) e++;
		found[(size_t)c] = line.substr(at, e - at);
		last = c;
	}
	for (int c = 0; c <= last; c++) segs.push_back(found[(size_t)c]);   // (an empty one is a skipped segment: parse_arch says so)
	return true;
}

std::vector<std::string> cmdline_segments(const td_run_opts* o)
{
	int last = -1;
	for (int k = 0; k < TD_RUN_MAX_SEGMENTS; k++) if (o->segments[k]) last = k;
	std::vector<std::string> s;
	for (int k = 0; k <= last; k++) s.push_back(o->segments[k] ? o->segments[k] : "");
	return s;
}

}   // namespace

namespace tdrun {

std::string segments_text(const std::vector<std::string>& segs)
{
	std::string s;
	for (size_t k = 0; k < segs.size(); k++) {
		if (segs[k].empty()) continue;
		if (!s.empty()) s += ' ';
		s += '-' + std::to_string(k + 1) + ' ' + segs[k];
	}
	return s;
}

bool parse_arch(const std::vector<std::string>& segs, ArchPtr& out, std::string& why)
{
	if (segs.empty()) { why = "ERROR: No read architecture found."; return false; }
	for (size_t k = 0; k < segs.size(); k++) {
		const std::string& s = segs[k];
		if (s.empty()) { why = "ERROR: a hmm building lock was skipped??"; return false; }
		if (!strchr("RGOPSFB", s[0])) { why = std::string("Segment type :") + s[0] + " not recognized."; return false; }
		if (s.size() < 2 || s[1] != ':') { why = "Some problem with parsing an HMM segment: " + s + "."; return false; }
		if (s[0] != 'R') {
			size_t len = std::string::npos, start = 2;
			for (size_t p = 2; p <= s.size(); p++)
				if (p == s.size() || s[p] == ',') {
					if (len != std::string::npos && p - start != len) { why = "ERROR: the sequences in the same segment have to have the same length."; return false; }
					len = p - start; start = p + 1;
				}
			if (len == 0 || len == std::string::npos) { why = "Some problem with parsing an HMM segment: " + s + "."; return false; }
		}
	}
	std::vector<const char*> p;
	for (auto& s : segs) p.push_back(s.c_str());
	td_arch* a = nullptr;
	if (td_arch_parse(p.data(), (int32_t)p.size(), &a) != TD_OK) { why = "Some problem with parsing an HMM segment: " + segments_text(segs) + "."; return false; }
	out.reset(a);
	return true;
}

bool read_arch_file(const char* path, ArchFile& af, std::string& why)
{
	FILE* f = fopen(path, "r");
	if (!f) { why = std::string("Failed to open file:") + path; return false; }
	char* line = nullptr;
	size_t cap = 0;
	while (getline(&line, &cap, f) > 0) {
		std::vector<std::string> segs;
		if (!arch_line_segments(line, segs)) continue;
		af.lines.push_back(line);
		af.segs.push_back(segs);
		if (af.lines.size() == 100) {   // MAX_NUM_ARCH, test_architectures.c:18, :128-133
			why = "Error - your architechture file has too many architectures. Currently only 100 allowed.";
			free(line); fclose(f);
			return false;
		}
	}
	free(line);
	fclose(f);
	if (af.lines.empty()) { why = std::string("Error - could not find any architectures in file: ") + path; return false; }
	for (size_t i = 0; i < af.lines.size(); i++)
		for (size_t j = i + 1; j < af.lines.size(); j++)
			if (af.lines[i] == af.lines[j]) { why = std::string("ERROR: two architectures in ") + path + " are the same:" + af.lines[i]; return false; }
	return true;
}

// the rows of a sheet whose column t is segment sh.segs[t] of col_arch[t]; infile != NULL: --join-barcodes, the messages name the
// column's file (sh.files[t], infile[sh.files[t]]) beside its segment
static int read_sheet_rows(const char* path, const std::vector<const td_arch*>& col_arch, const char* const* infile, SampleSheet& sh)
{
	const int m = (int)sh.segs.size();
	FILE* f = fopen(path, "r");
	if (!f) return run_fail("--samples: cannot open the sample sheet %s.", path);
	char buf[4096];
	int line = 0;
	std::vector<int> at_line;
	int rc = TD_OK;
	while (rc == TD_OK && fgets(buf, sizeof buf, f)) {
		line++;
		std::vector<std::string> w;
		for (char* tok = strtok(buf, " \t\r\n"); tok; tok = strtok(nullptr, " \t\r\n")) w.push_back(tok);
		if (w.empty() || w[0][0] == '#') continue;
		if ((int)w.size() != m + 1) {
			rc = run_fail("--samples: %s line %d: %d columns, need %d (the name and one barcode per barcode segment%s).", path, line, (int)w.size(), m + 1,
			              infile ? " of every barcode file, files first" : "");
			break;
		}
		if (sh.n() == TD_SAMPLES_MAX) { rc = run_fail("--samples: %s line %d: more than %d samples.", path, line, TD_SAMPLES_MAX); break; }
		const std::string& name = w[0];
		bool ok = !name.empty() && name.size() <= TD_SAMPLES_MAX_NAME;
		for (const char ch : name) ok = ok && ((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '.' || ch == '_' || ch == '-');
		if (!ok) { rc = run_fail("--samples: %s line %d: the name '%s' is not 1..%d characters of [A-Za-z0-9._-].", path, line, name.c_str(), TD_SAMPLES_MAX_NAME); break; }
		std::vector<int32_t> row;
		for (int t = 0; t < m && rc == TD_OK; t++) {
			const int seg = sh.segs[(size_t)t];
			const td_arch* a = col_arch[(size_t)t];
			int found = -1;
			for (int q = 0; q < a->n_seq[seg] - 1; q++) if (w[(size_t)t + 1] == a->seqs[seg][q]) found = q;   // (the last one is the all-N wildcard)
			if (found < 0 && !infile) rc = run_fail("--samples: %s line %d: '%s' is not a barcode of segment %d.", path, line, w[(size_t)t + 1].c_str(), seg + 1);
			else if (found < 0)
				rc = run_fail("--samples: %s line %d: '%s' (column %d) is not a barcode of segment %d of file %d (%s).", path, line, w[(size_t)t + 1].c_str(), t + 1,
				              seg + 1, sh.files[(size_t)t], infile[sh.files[(size_t)t]]);
			row.push_back(found);
		}
		if (rc != TD_OK) break;
		for (int s = 0; s < sh.n() && rc == TD_OK; s++) {
			if (sh.names[(size_t)s] == name) rc = run_fail("--samples: %s line %d: the name '%s' is taken by line %d.", path, line, name.c_str(), at_line[(size_t)s]);
			else if (std::equal(row.begin(), row.end(), sh.tuples.begin() + (size_t)s * m))
				rc = run_fail("--samples: %s line %d: the barcodes repeat those of line %d.", path, line, at_line[(size_t)s]);
		}
		if (rc != TD_OK) break;
		sh.names.push_back(name);
		sh.tuples.insert(sh.tuples.end(), row.begin(), row.end());
		at_line.push_back(line);
	}
	fclose(f);
	if (rc != TD_OK) return rc;
	if (sh.n() == 0) return run_fail("--samples: %s lists no sample.", path);
	return TD_OK;
}

int read_sample_sheet(const char* path, const td_arch* a, SampleSheet& sh)
{
	sh = SampleSheet();
	for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'B') sh.segs.push_back(j);
	const int m = (int)sh.segs.size();
	if (m > TD_SAMPLES_MAX_SEGMENTS) return run_fail("--samples: the architecture has %d barcode segments (at most %d).", m, TD_SAMPLES_MAX_SEGMENTS);
	return read_sheet_rows(path, std::vector<const td_arch*>((size_t)m, a), nullptr, sh);
}

int read_sample_sheet_join(const char* path, const std::vector<const td_arch*>& archs, const std::vector<int>& bar_files, const char* const* infile,
                           SampleSheet& sh)
{
	sh = SampleSheet();
	std::vector<const td_arch*> col_arch;
	for (const int k : bar_files)
		for (int j = 0; j < archs[(size_t)k]->n_segments; j++)
			if (archs[(size_t)k]->type[j] == 'B') { sh.segs.push_back(j); sh.files.push_back(k); col_arch.push_back(archs[(size_t)k]); }
	return read_sheet_rows(path, col_arch, infile, sh);
}

int decide_roles(const td_run_opts* o, const std::vector<const td_arch*>& archs, RunRoles& r)
{
	r = RunRoles();
	// the decoded files: those with an architecture other than R:N.  --mate-bases and --min-base-quality each need exactly one
	int n_decoded = 0, decoded = 0;
	for (size_t k = 0; k < archs.size(); k++) if (!is_read_only(archs[k]) && n_decoded++ == 0) decoded = (int)k;
	if (o->mate_bases) {
		if (n_decoded != 1)
			return run_fail("--mate-bases: exactly one input file may have an architecture other than R:N (%d have): barcode and fingerprint of a "
			                "molecule come from one decoded file, every other file gives reads.", n_decoded);
		r.mol_file = decoded;
		r.mate_file = decoded == 0 ? 1 : 0;      // the first file in call order other than the decoded one
	}
	for (size_t k = 0; k < archs.size(); k++) {
		if (has_barcode(archs[k])) {
			if (o->join_barcodes) r.bar_files.push_back((int)k);   // --join-barcodes: every barcode file, the first holds the sheet
			if (r.bar_file >= 0 && !o->join_barcodes)
				return run_fail("Barcodes seem to be in both architectures... %s", o->samples_file ? "(--samples: barcodes spread over several input files are not "
				                "joined; the controller's rule of one barcode file stays, and a sheet lists the barcode segments of that one file.)" : "");
			if (r.bar_file < 0) r.bar_file = (int)k;
		}
		r.num_out_reads += read_segments(archs[k]);
	}
	std::vector<const char*> in_names;     // (td_run_output_files_describe decides without input files: a file is then named by "-")
	for (size_t k = 0; k < archs.size(); k++) in_names.push_back((int)k < o->n_infiles && o->infile ? o->infile[k] : "-");
	if (o->join_barcodes) {
		if (!o->samples_file) return run_fail("--join-barcodes needs --samples: the sheet names the barcodes of every file that are joined.");
		int columns = 0;
		for (const int k : r.bar_files) {
			r.first_column.push_back(columns);
			for (int j = 0; j < archs[(size_t)k]->n_segments; j++)
				if (archs[(size_t)k]->type[j] == 'B') { columns++; r.column_hmms.push_back(archs[(size_t)k]->n_seq[j]); }
		}
		if (r.bar_files.size() == 1)
			return run_fail("--join-barcodes: only one input file (%s) has barcode segments: there is nothing to join, drop the option (--samples alone "
			                "assigns by all barcode segments of one file).", in_names[(size_t)r.bar_files[0]]);
		if (!r.bar_files.empty() && columns > TD_SAMPLES_MAX_SEGMENTS)
			return run_fail("--join-barcodes: the barcode files have %d barcode segments together (at most %d).", columns, TD_SAMPLES_MAX_SEGMENTS);
	}
	if (r.num_out_reads == 0) return run_fail("No read segment in any architecture: there would be no output file.");
	// print_all() names its files after the barcode file's architecture, else the last file's (td_stream_run_multi; one file: td_writer_open)
	// (--samples is resolved here, where the architectures are known, so that it works with -arch)
	if (o->samples_file) {
		if (r.bar_file < 0) return run_fail("--samples: no input file's architecture has a barcode segment.");
		if (o->join_barcodes) {
			if (read_sample_sheet_join(o->samples_file, archs, r.bar_files, in_names.data(), r.sheet) != TD_OK) return TD_FAIL;
			r.join_line = "join: files ";
			for (size_t q = 0; q < r.bar_files.size(); q++) r.join_line += (q ? "," : "") + std::to_string(r.bar_files[q]);
			r.join_line += "; columns";
			for (size_t t = 0; t < r.sheet.segs.size(); t++)
				r.join_line += std::string(t ? ", " : " ") + std::to_string(t + 1) + " = segment " + std::to_string(r.sheet.segs[t] + 1) + " of file " + std::to_string(r.sheet.files[t]);
			r.join_line += "; file " + std::to_string(r.bar_file) + " holds the sheet, a read whose partner in another barcode file is not extracted goes to _un\n";
		} else if (read_sample_sheet(o->samples_file, archs[(size_t)r.bar_file], r.sheet) != TD_OK) return TD_FAIL;
		td_writer_file_names_samples(o->outfile, r.sheet.names, r.num_out_reads, r.out_files, nullptr);
		r.out_files.push_back(samples_file_name(o));
	} else {
		td_writer_file_names_n(o->outfile, archs[(size_t)(r.bar_file >= 0 ? r.bar_file : (int)archs.size() - 1)], r.num_out_reads, r.out_files, nullptr);
	}
	if (o->unknown_barcodes > 0) {
		if (r.bar_file < 0) return run_fail("--unknown-barcodes: no input file's architecture has a barcode segment.");
		r.out_files.push_back(unknown_file_name(o));
	}
	if (o->molecules) {
		if (archs.size() == 1 && is_read_only(archs[0])) return run_fail("--molecules: the architecture is a single read segment: there is no model whose labels mark a barcode or a fingerprint.");
		if (o->collapse_umis && !has_fingerprint(archs[(size_t)r.mol_file]))
			return run_fail("--collapse-umis: the architecture has no fingerprint (F) segment: there is no UMI whose neighbours could be collapsed.");
		r.out_files.push_back(molecules_file_name(o));
	}
	if (o->min_base_quality) {   // the base-quality filter judges the one decoded file's barcode / UMI bases
		if (n_decoded == 0) return run_fail("--min-base-quality: the architecture is a single read segment: there is no model whose labels mark a barcode or a fingerprint.");
		if (n_decoded > 1)
			return run_fail("--min-base-quality: exactly one input file may have an architecture other than R:N (%d have): one file's verdicts are the run's.", n_decoded);
		const bool b = (o->quality_segments & TD_QUAL_SEG_B) && has_barcode(archs[(size_t)decoded]), f = (o->quality_segments & TD_QUAL_SEG_F) && has_fingerprint(archs[(size_t)decoded]);
		if (!b && !f) return run_fail("--min-base-quality: the architecture has no segment of the types --quality-segments names: there is no base to judge.");
		r.qual_file = decoded;
	}
	if (r.bar_file >= 0 && !o->force)   // check_for_existing_demultiplexed_files_multiple, io.c:633-691 (made for the barcode file only)
		for (auto& n : r.out_files)
			if (file_exists(n)) return run_fail("Error: some output files already exists. (%s; --force overwrites)", n.c_str());
	return TD_OK;
}

int mate_filter_files(const td_run_opts* o, int dust, bool use_ref, const RunRoles& r)
{
	if (!o->mate_filter || o->n_infiles < 3 || (dust == 0 && !use_ref)) return TD_OK;
	int third = 0;
	while (third == r.mol_file || third == r.mate_file) third++;
	return run_fail("--mate-filter with DUST or -ref takes exactly two input files (%d given): the outcome of %s would be joined behind the count, "
	                "where a failing read takes a molecule's one kept read out of the files: run with -dust 0 and without -ref, or without that file.",
	                o->n_infiles, o->infile[third]);
}

}   // namespace tdrun

using namespace tdrun;

extern "C" void td_run_plan_free(td_run_plan_t* p) { delete p; }

extern "C" int td_run_plan(const td_run_opts* o, td_run_plan_t** out)
{
	if (!o || !out) return run_fail("td_run_plan: bad arguments");
	*out = nullptr;
	std::unique_ptr<td_run_plan_t> p(new td_run_plan_t());
	const std::vector<std::string> cmd = cmdline_segments(o);
	// main.c:103-125
	if (cmd.empty() && !o->arch_file) return run_fail("ERROR: No read architecture found.");
	std::string why;
	if (!cmd.empty()) { ArchPtr a; if (!parse_arch(cmd, a, why)) return run_fail("ERROR: Something wrong with the read architecture. %s", why.c_str()); }
	if (o->n_infiles == 0) return run_fail("ERROR: No input file found.");
	if (!o->outfile) return run_fail("ERROR: You need to specify an output file prefix using the -o / -out option.");
	if (o->arch_file && !file_exists(o->arch_file)) return run_fail("ERROR: Arch file:%s does not exists.", o->arch_file);
	if (o->join_barcodes) {
		if (!o->samples_file) return run_fail("--join-barcodes needs --samples: the sheet names the barcodes of every file that are joined.");
		if (o->n_devices > 1)
			return run_fail("--join-barcodes needs exactly one device (%d given): a batch's barcode calls travel from one file's context to another's.", o->n_devices);
		if (o->unknown_barcodes > 0)
			return run_fail("--join-barcodes cannot be combined with --unknown-barcodes: the census spells one file's last barcode segment, not the joined tuple.");
		if (o->matchstart != -1 || o->matchend != -1)
			return run_fail("--join-barcodes cannot be combined with -start / -end: labels behind a window do not mark the barcodes.");
	}
	if (o->unknown_barcodes > 0 && (o->matchstart != -1 || o->matchend != -1))
		return run_fail("--unknown-barcodes cannot be combined with -start / -end: labels behind a window do not spell the barcode.");
	if (o->samples_file && (o->matchstart != -1 || o->matchend != -1))
		return run_fail("--samples cannot be combined with -start / -end: labels behind a window do not mark the barcodes.");
	if (o->samples_file && !file_exists(o->samples_file)) return run_fail("--samples: the sample sheet %s does not exist.", o->samples_file);
	if (o->min_base_quality && (o->matchstart != -1 || o->matchend != -1))
		return run_fail("--min-base-quality cannot be combined with -start / -end: labels behind a window do not mark the bases.");
	if (o->min_base_quality && o->n_devices > 1)
		return run_fail("--min-base-quality needs exactly one device (%d given): a batch's quality lines travel with its reads to one context.", o->n_devices);
	if (o->mate_bases) {
		if (o->n_infiles < 2)
			return run_fail("--mate-bases needs two or more input files (%d given): the mate is the record of a second file.", o->n_infiles);
		if (o->molecules_prefix + o->mate_bases > TD_MOL_MAX_PREFIX)
			return run_fail("--molecules-prefix %d and --mate-bases %d are %d bases together: at most %d fit the key's one 64-bit word.", o->molecules_prefix,
			                o->mate_bases, o->molecules_prefix + o->mate_bases, TD_MOL_MAX_PREFIX);
		if (o->n_devices > 1)
			return run_fail("--mate-bases needs exactly one device (%d given): the mate batch travels with its reads to the one context that counts them.", o->n_devices);
		if (o->dedup_collapsed)
			return run_fail("--mate-bases cannot be combined with --dedup-collapsed: the survey reads one file.");
	}
	if (o->mate_filter && !o->mate_bases)
		return run_fail("--mate-filter needs --mate-bases: it judges the mate that --mate-bases joins to its read.");
	if (o->molecules && !o->mate_bases && o->n_infiles != 1)
		return run_fail("--molecules needs exactly one input file (%d given): a read and its fingerprint in different files are not joined.", o->n_infiles);
	if (o->molecules && (o->matchstart != -1 || o->matchend != -1))
		return run_fail("--molecules cannot be combined with -start / -end: labels behind a window do not mark the read's bases.");
	if (o->dedup && !o->molecules) return run_fail("--dedup needs --molecules: the duplicates are those of the molecule count.");
	if (o->dedup && o->n_devices > 1)
		return run_fail("--dedup needs exactly one device (%d given): each device has its own table, and a molecule split over two devices would survive twice.", o->n_devices);
	if (o->dedup_collapsed && !(o->dedup && o->collapse_umis))
		return run_fail("--dedup-collapsed needs --dedup and --collapse-umis: it is the second pass that makes the one follow the other.");
	if (o->dedup_collapsed)
		for (int k = 0; k < o->n_infiles; k++)
			if (!strcmp(o->infile[k], "-")) return run_fail("--dedup-collapsed cannot read the input from stdin (-): the input is read twice.");
	p->dedup = o->dedup != 0;
	p->collapse = o->collapse_umis != 0;
	p->dedup_collapsed = o->dedup_collapsed != 0;
	for (int k = 0; k < o->n_infiles; k++)
		if (strcmp(o->infile[k], "-") != 0 && !file_exists(o->infile[k])) return run_fail("ERROR: Input file:%s does not exists.", o->infile[k]);
	// interface.c:419-450: two or more R segments in the command line's architecture switch DUST and -ref off
	p->dust = o->dust;
	p->use_ref = o->reference_fasta != nullptr;
	int n_r = 0;
	for (auto& s : cmd) n_r += !s.empty() && s[0] == 'R';
	if (n_r >= 2 && (p->use_ref || p->dust)) {
		p->warnings.push_back("WARNING: cannot dust or filter sequences by comparison to a known sequence if multiple reads are present in one input seqeunce.");
		p->dust = 0;
		p->use_ref = false;
	}
	p->mate_bases = o->mate_bases;
	p->mate_filter = o->mate_filter != 0;
	if (p->use_ref) p->ref_file = o->reference_fasta;
	if (o->mate_bases && !o->mate_filter && (p->dust != 0 || p->use_ref))
		return run_fail("--mate-bases: the mate is not decoded and its outcome is not joined to the count, so a mate that DUST or the -ref filter "
		                "rejects would take a molecule's one kept read out of the files: run with -dust 0 and without -ref.");
	if (p->use_ref && !file_exists(o->reference_fasta)) return run_fail("ERROR: Reference file:%s does not exists.", o->reference_fasta);
	if (o->arch_file && !read_arch_file(o->arch_file, p->arch_file, why)) return run_fail("%s", why.c_str());
	// barcode_hmm.c:105-129
	p->all_known = true;
	std::vector<ArchPtr> archs;
	for (int k = 0; k < o->n_infiles; k++) {
		std::vector<std::string> segs;
		int src;
		if (k == 0 && !cmd.empty()) { src = SRC_CMDLINE; segs = cmd; }
		else if (o->arch_file) {
			src = SRC_ARCH_FILE;
			if (p->arch_file.segs.size() == 1) segs = p->arch_file.segs[0];   // (one candidate: nothing to choose)
			else p->all_known = false;
		} else { src = SRC_DEFAULT; segs = { "R:N" }; }
		p->source.push_back(src);
		p->segs.push_back(segs);
		if (!segs.empty()) {
			ArchPtr a;
			if (!parse_arch(segs, a, why)) return run_fail("ERROR: Something wrong with the read architecture. %s", why.c_str());
			archs.push_back(std::move(a));
		}
	}
	std::vector<const td_arch*> view;
	for (auto& a : archs) view.push_back(a.get());
	const RunRoles& r = p->roles;
	if (p->all_known && decide_roles(o, view, p->roles) != TD_OK) return TD_FAIL;
	if (o->samples_file) {
		p->samples_line = std::string("samples: ") + o->samples_file + ": ";
		if (!p->all_known) p->samples_line += "resolved once the arch file's choice is made";
		else {
			p->samples_line += std::to_string(r.sheet.n()) + " samples by segment";
			for (size_t t = 0; t < r.sheet.segs.size(); t++) p->samples_line += (t ? ", " : (r.sheet.segs.size() > 1 ? "s " : " ")) + std::to_string(r.sheet.segs[t] + 1);
			if (!o->join_barcodes) p->samples_line += " of file " + std::to_string(r.bar_file);
			else p->samples_line += " of the joined files";
			p->samples_line += "; a read whose barcodes are incomplete or name no sample goes to _un";
		}
		p->samples_line += "\n";
	}
	if (o->min_base_quality)
		p->quality_line = "quality: an extracted read with more than " + std::to_string(o->max_low_bases) + " bases below Q" + std::to_string(o->min_base_quality) +
		                  " (offset " + std::to_string(o->quality_offset) + ") in its " +
		                  (o->quality_segments == TD_QUAL_SEG_B ? "barcode" : (o->quality_segments == TD_QUAL_SEG_F ? "fingerprint" : "barcode or fingerprint")) +
		                  " segments goes to _un and is neither assigned, counted nor kept by --dedup\n";
	if (p->all_known && mate_filter_files(o, p->dust, p->use_ref, r) != TD_OK) return TD_FAIL;
	*out = p.release();
	return TD_OK;
}

extern "C" int64_t td_run_plan_describe(const td_run_plan_t* p, char* buf, int64_t cap)
{
	if (!p) return 0;
	std::string s;
	for (auto& w : p->warnings) s += "warning: " + w + "\n";
	for (size_t k = 0; k < p->source.size(); k++) {
		s += "file " + std::to_string(k) + " architecture: ";
		if (p->source[k] == SRC_CMDLINE) s += "command line: " + segments_text(p->segs[k]);
		else if (p->source[k] == SRC_DEFAULT) s += "default: " + segments_text(p->segs[k]);
		else if (!p->segs[k].empty()) s += "arch file (one candidate): " + segments_text(p->segs[k]);
		else s += "arch file: best of " + std::to_string(p->arch_file.segs.size()) + " candidates";
		s += "\n";
	}
	for (size_t k = 0; k < p->arch_file.segs.size(); k++) s += "arch file candidate " + std::to_string(k) + ": " + segments_text(p->arch_file.segs[k]) + "\n";
	s += "dust: " + std::to_string(p->dust) + "\n";
	s += std::string("ref: ") + (p->use_ref ? "on" : "off") + "\n";
	if (p->dedup) s += "dedup: one read per molecule is written (barcode, fingerprint and the start of the read)\n";
	if (p->collapse) s += "collapse: fingerprints one mismatch apart are counted as one molecule (directional rule; the count and --dedup stay exact)\n";
	if (p->dedup_collapsed)
		s += "dedup-collapsed: the input is read twice, a survey and then the run: one read per collapsed molecule is written, the first that carries the root's barcode, fingerprint and start\n";
	if (p->mate_bases) {
		s += "mate: " + std::to_string(p->mate_bases) + " bases of the mate join the molecule key behind the read's own prefix; ";
		if (!p->mate_filter) s += "the mate's own outcome takes no part";
		else s += "mate filter on: the mate is judged with dust " + std::to_string(p->dust) + " and -ref " + (p->use_ref ? p->ref_file : std::string("none")) +
		          ", and its outcome is joined to the read's in front of the count";
		if (p->all_known) s += " (file " + std::to_string(p->roles.mol_file) + " is decoded, file " + std::to_string(p->roles.mate_file) + " is its mate)";
		s += "\n";
	}
	s += p->samples_line;
	if (p->all_known) s += p->roles.join_line;
	s += p->quality_line;
	if (p->all_known) {
		s += "barcode file: " + (p->roles.bar_file >= 0 ? std::to_string(p->roles.bar_file) : std::string("none")) + "\n";
		s += "output reads: " + std::to_string(p->roles.num_out_reads) + "\n";
		for (auto& n : p->roles.out_files) s += "output file: " + n + "\n";
	} else {
		s += "output files: named once the arch file's choice is made\n";
	}
	return copy_out(s, buf, cap);
}

extern "C" int64_t td_run_output_files_describe(const td_run_opts* o, const char* const* architectures, int32_t n_files, char* buf, int64_t cap)
{
	if (!o || !o->outfile || !architectures || n_files < 1) { run_fail("td_run_output_files_describe: bad arguments"); return -1; }
	std::vector<ArchPtr> archs((size_t)n_files);
	std::vector<const td_arch*> view;
	std::string why;
	for (int k = 0; k < n_files; k++) {
		std::vector<std::string> segs;
		if (!architectures[k] || !arch_line_segments(std::string("tagdust ") + architectures[k] + "\n", segs) || !parse_arch(segs, archs[(size_t)k], why)) {
			run_fail("td_run_output_files_describe: file %d: %s", k, why.empty() ? "no architecture" : why.c_str());
			return -1;
		}
		view.push_back(archs[(size_t)k].get());
	}
	RunRoles r;
	if (decide_roles(o, view, r) != TD_OK) return -1;
	std::string s;
	for (auto& n : r.out_files) s += n + "\n";
	return copy_out(s, buf, cap);
}

extern "C" int64_t td_run_arch_file_describe(const char* path, char* buf, int64_t cap)
{
	ArchFile af;
	std::string why;
	if (!path || !read_arch_file(path, af, why)) { run_fail("%s", path ? why.c_str() : "td_run_arch_file_describe: NULL path"); return -1; }
	std::string s;
	for (auto& c : af.segs) s += segments_text(c) + "\n";
	return copy_out(s, buf, cap);
}
