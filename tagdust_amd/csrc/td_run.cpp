// td_run.cpp -- the whole-run driver (include/tagdust_run.h): what the reference's main() (src/main.c:95-217), interface()
// (src/interface.c:49-480), hmm_controller_multiple() (src/barcode_hmm.c:51-460), test_architectures()
// (src/test_architectures.c:20-289) and free_param() (src/interface.c:709-726) do, on this library's own entry points.
// Host code; the device work is behind td_sequence_stats_device, td_compare_architectures, td_estimate_threshold and the
// streaming pipelines.
#include <ctype.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tagdust_run.h"
#include "../../include/tagdust_multi.h"
#include "td_io_internal.h"

namespace {

thread_local std::string g_run_error;

int run_fail(const char* fmt, ...)
{
	char buf[1024];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	g_run_error = buf;
	return TD_FAIL;
}

double now_s()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec + (double)ts.tv_nsec * 1e-9;
}

char* dup_str(const char* s) { return s ? strdup(s) : nullptr; }
bool file_exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0; }   // misc.c:file_exists

int64_t copy_out(const std::string& s, char* buf, int64_t cap)
{
	if (buf && cap > 0) {
		const int64_t n = std::min<int64_t>((int64_t)s.size(), cap - 1);
		memcpy(buf, s.data(), (size_t)n);
		buf[n] = 0;
	}
	return (int64_t)s.size();
}

// ---- architectures ----
struct ArchDeleter { void operator()(td_arch* a) const { td_arch_free(a); } };
typedef std::unique_ptr<td_arch, ArchDeleter> ArchPtr;

// segments as "-1 B:ACGT -2 R:N" (pretty_print_selected_architecture's form, without "Using: ")
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

// QC_read_structure (interface.c:759-829) as far as it can fail, and td_arch_parse's own checks: no segment skipped, one length per segment
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

bool is_read_only(const td_arch* a) { return a->n_segments == 1 && a->type[0] == 'R'; }
bool has_fingerprint(const td_arch* a) { for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'F') return true; return false; }
bool has_barcode(const td_arch* a) { for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'B') return true; return false; }
int read_segments(const td_arch* a) { int n = 0; for (int j = 0; j < a->n_segments; j++) n += a->type[j] == 'R'; return n; }

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

struct ArchFile {
	std::vector<std::string> lines;                    // the candidates' lines as read (duplicates are an error)
	std::vector<std::vector<std::string>> segs;
};

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

// ---- options ----
struct OptSpec { const char* name; int arg; int id; };
enum { O_SEG = 1 /* .. 10 */, O_ARCH = 20, O_OUT, O_THREADS, O_Q, O_E, O_I, O_MINLEN, O_DUST, O_REF, O_FE, O_START, O_END, O_SEED,
       O_HELP, O_VERSION, O_DEVICES, O_RTEST, O_HOST_THREADS, O_BATCH_READS, O_SYNC_COMPILE, O_STATS_ON_HOST, O_FORCE, O_DRY_RUN,
       O_UNKNOWN, O_UNKNOWN_SLOTS, O_FINGER_SEQ, O_MOLECULES, O_MOLECULES_PREFIX, O_MOLECULES_SLOTS, O_DEDUP, O_COLLAPSE,
       O_DEDUP_COLLAPSED, O_MATE_BASES, O_MATE_FILTER, O_SAMPLES, O_MIN_BASE_QUALITY, O_MAX_LOW_BASES, O_QUALITY_SEGMENTS, O_QUALITY_OFFSET,
       O_UNSUPPORTED = 100 };
const OptSpec kOpts[] = {
	{ "1", 1, O_SEG + 0 }, { "2", 1, O_SEG + 1 }, { "3", 1, O_SEG + 2 }, { "4", 1, O_SEG + 3 }, { "5", 1, O_SEG + 4 }, { "6", 1, O_SEG + 5 },
	{ "7", 1, O_SEG + 6 }, { "8", 1, O_SEG + 7 }, { "9", 1, O_SEG + 8 }, { "10", 1, O_SEG + 9 },
	{ "arch", 1, O_ARCH }, { "o", 1, O_OUT }, { "out", 1, O_OUT }, { "t", 1, O_THREADS },
	{ "Q", 1, O_Q }, { "q", 1, O_Q }, { "threshold", 1, O_Q }, { "e", 1, O_E }, { "i", 1, O_I },
	{ "minlen", 1, O_MINLEN }, { "dust", 1, O_DUST }, { "ref", 1, O_REF }, { "fe", 1, O_FE },
	{ "start", 1, O_START }, { "end", 1, O_END }, { "seed", 1, O_SEED },
	{ "h", 0, O_HELP }, { "help", 0, O_HELP }, { "v", 0, O_VERSION }, { "version", 0, O_VERSION },
	// parsed by the reference, not implemented here
	{ "show_finger_seq", 0, O_UNSUPPORTED }, { "train", 1, O_UNSUPPORTED }, { "exact5", 1, O_UNSUPPORTED }, { "join", 0, O_UNSUPPORTED },
	{ "split", 0, O_UNSUPPORTED }, { "name", 1, O_UNSUPPORTED }, { "format", 1, O_UNSUPPORTED }, { "f", 1, O_UNSUPPORTED },
	{ "filter", 1, O_UNSUPPORTED }, { "a", 1, O_UNSUPPORTED }, { "l", 1, O_UNSUPPORTED }, { "L", 1, O_UNSUPPORTED }, { "log", 1, O_UNSUPPORTED },
	{ "p", 1, O_UNSUPPORTED }, { "simulation", 1, O_UNSUPPORTED }, { "numbarcode", 1, O_UNSUPPORTED },
	{ "sim_barlen", 1, O_UNSUPPORTED }, { "sim_barnum", 1, O_UNSUPPORTED }, { "sim_5seq", 1, O_UNSUPPORTED }, { "sim_3seq", 1, O_UNSUPPORTED },
	{ "sim_readlen", 1, O_UNSUPPORTED }, { "sim_readlen_mod", 1, O_UNSUPPORTED }, { "sim_error_rate", 1, O_UNSUPPORTED },
	{ "sim_InDel_frac", 1, O_UNSUPPORTED }, { "sim_numseq", 1, O_UNSUPPORTED }, { "sim_random_frac", 1, O_UNSUPPORTED },
	{ "sim_endloss", 1, O_UNSUPPORTED },
};
// this library's own: long names, two dashes
const OptSpec kOwnOpts[] = {
	{ "devices", 1, O_DEVICES }, { "rtest", 0, O_RTEST }, { "host-threads", 1, O_HOST_THREADS }, { "batch-reads", 1, O_BATCH_READS },
	{ "sync-compile", 0, O_SYNC_COMPILE }, { "stats-on-host", 0, O_STATS_ON_HOST }, { "force", 0, O_FORCE }, { "dry-run", 0, O_DRY_RUN },
	{ "unknown-barcodes", 1, O_UNKNOWN }, { "unknown-barcodes-slots", 1, O_UNKNOWN_SLOTS },
	{ "fingerprint-seq", 0, O_FINGER_SEQ }, { "molecules", 0, O_MOLECULES }, { "molecules-prefix", 1, O_MOLECULES_PREFIX },
	{ "molecules-slots", 1, O_MOLECULES_SLOTS }, { "dedup", 0, O_DEDUP }, { "collapse-umis", 0, O_COLLAPSE },
	{ "dedup-collapsed", 0, O_DEDUP_COLLAPSED }, { "mate-bases", 1, O_MATE_BASES }, { "mate-filter", 0, O_MATE_FILTER },
	{ "samples", 1, O_SAMPLES }, { "min-base-quality", 1, O_MIN_BASE_QUALITY }, { "max-low-bases", 1, O_MAX_LOW_BASES },
	{ "quality-segments", 1, O_QUALITY_SEGMENTS }, { "quality-offset", 1, O_QUALITY_OFFSET },
};

bool parse_devices(const char* s, td_run_opts* o, std::string& why)
{
	o->n_devices = 0;
	const char* p = s;
	while (*p) {
		char* end = nullptr;
		const long v = strtol(p, &end, 10);
		if (end == p || v < 0 || (*end && *end != ',')) { why = std::string("--devices: cannot read the device list \"") + s + "\" (want e.g. 0,1)"; return false; }
		if (o->n_devices == TD_RUN_MAX_DEVICES) { why = "--devices: more than 16 devices"; return false; }
		o->devices[o->n_devices++] = (int32_t)v;
		p = *end ? end + 1 : end;
		if (end[0] == ',' && !end[1]) { why = std::string("--devices: cannot read the device list \"") + s + "\""; return false; }
	}
	if (o->n_devices == 0) { why = "--devices: empty device list"; return false; }
	return true;
}

}   // namespace

extern "C" const char* td_run_last_error(void) { return g_run_error.c_str(); }

extern "C" td_run_opts* td_run_opts_new(void)
{
	td_run_opts* o = (td_run_opts*)calloc(1, sizeof(td_run_opts));
	if (!o) return nullptr;
	o->num_threads = 8;                 // interface.c:70
	o->confidence_threshold = 0.0f;     // :91
	o->sequencer_error_rate = 0.05f;    // :87
	o->indel_frequency = 0.1f;          // :88
	o->minlen = 16;                     // :82
	o->dust = 100;                      // :85
	o->filter_error = 2;                // :99
	o->matchstart = -1; o->matchend = -1;   // :80-81
	o->seed = 0;                        // :124
	o->n_devices = 1; o->devices[0] = 0;
	o->unknown_slots_log2 = 20;
	o->molecules_prefix = TD_MOL_DEFAULT_PREFIX;
	o->molecules_slots_log2 = TD_MOL_DEFAULT_LOG2_SLOTS;
	o->quality_segments = TD_QUAL_SEG_B | TD_QUAL_SEG_F;
	o->quality_offset = 33;
	return o;
}

extern "C" void td_run_opts_free(td_run_opts* o)
{
	if (!o) return;
	for (int k = 0; k < TD_RUN_MAX_SEGMENTS; k++) free(o->segments[k]);
	free(o->arch_file); free(o->outfile); free(o->reference_fasta); free(o->samples_file);
	for (int k = 0; k < o->n_infiles; k++) free(o->infile[k]);
	free(o->infile);
	for (int k = 0; k < o->argc; k++) free(o->argv[k]);
	free(o->argv);
	free(o);
}

extern "C" const char* td_run_version(void) { return "tagdust-hip 2.33 (TagDust 2.33 on libtagdust_hip, gfx950)\n"; }

extern "C" const char* td_run_usage(void)
{
	return "\nUsage:   tagdust-hip [options] <file> [<file> ...] -o <output prefix>\n\n"
	       "Options (as the reference's tagdust; one or two leading dashes):\n"
	       "\t-1 .. -10   STR   the HMM building blocks of the read architecture, e.g. -1 B:ACGT,TTGA -2 R:N\n"
	       "\t-arch       STR   file with candidate architectures, one tagdust command per line\n"
	       "\t-o / -out   STR   output file prefix\n"
	       "\t-Q          FLT   confidence threshold [calibrated]\n"
	       "\t-e          FLT   expected sequencer error rate [0.05]\n"
	       "\t-i          FLT   indel frequency [0.1]\n"
	       "\t-start      INT   start of search area [1]\n"
	       "\t-end        INT   end of search area [length of sequence]\n"
	       "\t-minlen     INT   minimal accepted read length [16]\n"
	       "\t-ref        STR   reference fasta file to be compared against\n"
	       "\t-fe         INT   number of errors allowed when comparing to reference [2]\n"
	       "\t-dust       INT   remove low complexity sequences [100]\n"
	       "\t-t          INT   number of threads of the reference run to reproduce [8]\n"
	       "\t-seed       INT   seed of the threshold calibration [time based]\n"
	       "\t-h / -help, -v / -version\n"
	       "Own options:\n"
	       "\t--devices 0,1     HIP devices to run on [0]\n"
	       "\t--rtest           the constants of the reference's -DRTEST builds (1000-record batches, 4000 calibration reads)\n"
	       "\t--host-threads N  host threads of the parse and write stages\n"
	       "\t--batch-reads N   records per batch\n"
	       "\t--sync-compile    compile the model kernel before decoding (default: decode while it compiles)\n"
	       "\t--stats-on-host   sequence statistics on the host\n"
	       "\t--force           overwrite existing output files\n"
	       "\t--dry-run         print the decisions of the run and stop\n"
	       "\t--unknown-barcodes K        the K most frequent barcode spellings of the reads that were not extracted,\n"
	       "\t                            into <output prefix>_unknown_barcodes.txt\n"
	       "\t--unknown-barcodes-slots N  slots of the counting table on every device, as a power of two [20]\n"
	       "\t--fingerprint-seq           fingerprints as bases in the read names, \";FP:ACGT\" (what the reference's -show_finger_seq\n"
	       "\t                            writes; that spelling itself is not accepted)\n"
	       "\t--molecules                 reads, molecules, duplication rate and duplication levels per barcode, counted by\n"
	       "\t                            barcode, fingerprint and start of the read, into <output prefix>_molecules.txt\n"
	       "\t--molecules-prefix P        bases of the read that belong to a molecule's identity, 1..32 [20]\n"
	       "\t--molecules-slots N         slots of the counting table on every device, as a power of two, 4..30 [26]\n"
	       "\t--dedup                     write one read per molecule: an extracted read that is not the first of its molecule in\n"
	       "\t                            the input goes to no output file (implies --molecules; one input file, one device)\n"
	       "\t--collapse-umis             count fingerprints one mismatch apart as one molecule where the counts say the rarer one is\n"
	       "\t                            a misread of the other: two more columns in <output prefix>_molecules.txt (implies\n"
	       "\t                            --molecules; needs an F segment; --dedup still matches exactly)\n"
	       "\t--dedup-collapsed           write one read per collapsed molecule: the input file is read twice, first to count, then to\n"
	       "\t                            write the first read that carries each collapsed molecule's own barcode, fingerprint and start\n"
	       "\t                            (implies --dedup, --collapse-umis and --molecules; a file, not stdin)\n"
	       "\t--mate-bases M              two or more input files: the first M bases of the read's mate, the record of the first other\n"
	       "\t                            file, belong to a molecule's identity behind the read's own --molecules-prefix bases, 1..31,\n"
	       "\t                            both at most 32 together (implies --molecules; one file with an architecture other than R:N,\n"
	       "\t                            one device, -dust 0, no -ref)\n"
	       "\t--mate-filter               with --mate-bases and two input files: DUST and the -ref filter judge the mate as well, and a\n"
	       "\t                            read whose mate fails is neither counted nor kept by --dedup (lifts -dust 0 / no -ref)\n"
	       "\t--samples FILE              combinatorial barcodes: FILE lists one sample per line, the name and one barcode per B segment;\n"
	       "\t                            a read is written to <output prefix>_BC_<name>.fq by ALL its barcodes, to _un when they are\n"
	       "\t                            incomplete or name no sample; the counts go to <output prefix>_samples.txt\n"
	       "\t--min-base-quality Q        drop an extracted read with low-quality barcode or UMI bases: more than --max-low-bases of them\n"
	       "\t                            below Q, 1..93; it goes to _un and is neither counted nor kept by --dedup (FASTQ input, one\n"
	       "\t                            device, one decoded file; not with -start / -end)\n"
	       "\t--max-low-bases K           low-quality barcode / UMI bases a read may have [0]\n"
	       "\t--quality-segments B|F|BF   judge the bases of the barcode segments, of the fingerprint segments, or of both [BF]\n"
	       "\t--quality-offset 33|64      what a quality character's code is counted from [33]\n\n";
}

extern "C" int td_run_parse_args(int argc, const char* const* argv, td_run_opts** out, char* err, size_t errcap)
{
	auto bad = [&](const std::string& m) {
		if (err && errcap) snprintf(err, errcap, "%s", m.c_str());
		g_run_error = m;
		return TD_FAIL;
	};
	if (!out || argc < 1 || !argv) return bad("td_run_parse_args: bad arguments");
	*out = nullptr;
	td_run_opts* o = td_run_opts_new();
	if (!o) return bad("td_run_parse_args: out of memory");
	std::unique_ptr<td_run_opts, void (*)(td_run_opts*)> guard(o, td_run_opts_free);
	o->argv = (char**)calloc((size_t)argc, sizeof(char*));
	for (int k = 0; k < argc; k++) o->argv[k] = dup_str(argv[k]);
	o->argc = argc;
	std::vector<std::string> files;
	bool given_quality_detail = false;   // --max-low-bases / --quality-segments / --quality-offset: they say how --min-base-quality judges
	for (int k = 1; k < argc; k++) {
		const std::string a = argv[k];
		if (a.size() < 2 || a[0] != '-') { files.push_back(a); continue; }   // an input file ("-" = stdin)
		const bool two = a[1] == '-';
		const std::string name = a.substr(two ? 2 : 1);
		const OptSpec* sp = nullptr;
		for (const OptSpec& q : kOpts) if (name == q.name) sp = &q;
		if (!sp && two) for (const OptSpec& q : kOwnOpts) if (name == q.name) sp = &q;
		if (!sp) return bad("unknown option " + a);
		if (sp->id == O_UNSUPPORTED) return bad("option " + a + " of the reference is not implemented by this program");
		const char* v = nullptr;
		if (sp->arg) {
			if (k + 1 >= argc) return bad("option " + a + " requires an argument");
			v = argv[++k];
		}
		std::string why;
		if (sp->id >= O_SEG && sp->id < O_SEG + TD_RUN_MAX_SEGMENTS) {
			free(o->segments[sp->id - O_SEG]);
			o->segments[sp->id - O_SEG] = dup_str(v);
			continue;
		}
		switch (sp->id) {
		case O_ARCH: free(o->arch_file); o->arch_file = dup_str(v); break;
		case O_OUT: free(o->outfile); o->outfile = dup_str(v); break;
		case O_THREADS: o->num_threads = atoi(v); break;
		case O_Q: o->confidence_threshold = (float)atof(v); break;
		case O_E: o->sequencer_error_rate = (float)atof(v); break;
		case O_I: o->indel_frequency = (float)atof(v); break;
		case O_MINLEN: o->minlen = atoi(v); break;
		case O_DUST: o->dust = atoi(v); break;
		case O_REF: free(o->reference_fasta); o->reference_fasta = dup_str(v); break;
		case O_FE: o->filter_error = atoi(v); break;
		case O_START: o->matchstart = atoi(v) - 1; break;     // interface.c:286
		case O_END: o->matchend = atoi(v); break;
		case O_SEED: o->seed = (uint32_t)atoi(v); break;
		case O_HELP: o->help = 1; break;
		case O_VERSION: o->version = 1; break;
		case O_DEVICES: if (!parse_devices(v, o, why)) return bad(why); break;
		case O_RTEST: o->flavour = 1; break;
		case O_HOST_THREADS: o->host_threads = atoi(v); break;
		case O_BATCH_READS: o->batch_reads = atoi(v); break;
		case O_SYNC_COMPILE: o->sync_compile = 1; break;
		case O_STATS_ON_HOST: o->stats_on_host = 1; break;
		case O_FORCE: o->force = 1; break;
		case O_DRY_RUN: o->dry_run = 1; break;
		case O_UNKNOWN: o->unknown_barcodes = atoi(v); if (o->unknown_barcodes < 1) return bad("--unknown-barcodes: need a number of lines K >= 1"); break;
		case O_UNKNOWN_SLOTS: o->unknown_slots_log2 = atoi(v); break;
		case O_FINGER_SEQ: o->fingerprint_seq = 1; break;
		case O_MOLECULES: o->molecules = 1; break;
		case O_MOLECULES_PREFIX: o->molecules_prefix = atoi(v); break;
		case O_MOLECULES_SLOTS: o->molecules_slots_log2 = atoi(v); break;
		case O_DEDUP: o->dedup = 1; break;
		case O_COLLAPSE: o->collapse_umis = 1; break;
		case O_DEDUP_COLLAPSED: o->dedup_collapsed = 1; break;
		case O_MATE_BASES:
			o->mate_bases = atoi(v);
			if (o->mate_bases < 1 || o->mate_bases > TD_MOL_MAX_PREFIX - 1) return bad("--mate-bases: need 1..31 bases of the mate");
			break;
		case O_MATE_FILTER: o->mate_filter = 1; break;
		case O_SAMPLES: free(o->samples_file); o->samples_file = dup_str(v); break;
		case O_MIN_BASE_QUALITY:
			o->min_base_quality = atoi(v);
			if (o->min_base_quality < 1 || o->min_base_quality > 93) return bad("--min-base-quality: need a quality Q of 1..93");
			break;
		case O_MAX_LOW_BASES:
			o->max_low_bases = atoi(v);
			if (o->max_low_bases < 0 || (v[0] < '0' || v[0] > '9')) return bad("--max-low-bases: need a number of bases K >= 0");
			given_quality_detail = true;
			break;
		case O_QUALITY_SEGMENTS:
			if (!strcmp(v, "B")) o->quality_segments = TD_QUAL_SEG_B;
			else if (!strcmp(v, "F")) o->quality_segments = TD_QUAL_SEG_F;
			else if (!strcmp(v, "BF") || !strcmp(v, "FB")) o->quality_segments = TD_QUAL_SEG_B | TD_QUAL_SEG_F;
			else return bad("--quality-segments: need B, F or BF");
			given_quality_detail = true;
			break;
		case O_QUALITY_OFFSET:
			o->quality_offset = atoi(v);
			if (o->quality_offset != 33 && o->quality_offset != 64) return bad("--quality-offset: need 33 or 64");
			given_quality_detail = true;
			break;
		default: return bad("unknown option " + a);
		}
	}
	if (o->dedup_collapsed) { o->dedup = 1; o->collapse_umis = 1; }   // the second pass of the two together
	if (o->dedup) o->molecules = 1;   // the duplicates are those of the molecule count
	if (o->collapse_umis) o->molecules = 1;   // ... and so are the molecules that are collapsed
	if (o->mate_bases) o->molecules = 1;      // ... and the mate joins the molecule count's key
	if (given_quality_detail && !o->min_base_quality)
		return bad("--max-low-bases / --quality-segments / --quality-offset need --min-base-quality: they say how it judges");
	if (o->num_threads < 1) return bad("option -t: need at least one thread");
	if (o->host_threads < 0 || o->batch_reads < 0) return bad("--host-threads / --batch-reads: negative value");
	if (o->unknown_slots_log2 < 4 || o->unknown_slots_log2 > 26) return bad("--unknown-barcodes-slots: need 4..26 (the table has 2^N slots)");
	if (o->molecules_prefix < 1 || o->molecules_prefix > TD_MOL_MAX_PREFIX) return bad("--molecules-prefix: need 1..32 bases");
	if (o->molecules_slots_log2 < 4 || o->molecules_slots_log2 > 30) return bad("--molecules-slots: need 4..30 (the table has 2^N slots)");
	if ((int)files.size() > TD_RUN_MAX_FILES) return bad("more than 8 input files");
	o->infile = (char**)calloc(files.size() ? files.size() : 1, sizeof(char*));
	for (auto& f : files) o->infile[o->n_infiles++] = dup_str(f.c_str());
	*out = guard.release();
	return TD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// the plan
// ---------------------------------------------------------------------------------------------------------
enum { SRC_CMDLINE = 0, SRC_ARCH_FILE = 1, SRC_DEFAULT = 2 };

struct td_run_plan_t {
	std::vector<int> source;                 // per input file
	std::vector<std::vector<std::string>> segs;   // ... its segments when no data is needed to know them
	ArchFile arch_file;
	bool all_known = false;                  // no file waits for the arch file's choice
	int bar_file = -1, num_out_reads = 0;
	std::vector<std::string> out_files;
	std::vector<std::string> warnings;
	int dust = 0;
	bool use_ref = false;
	bool dedup = false;
	bool collapse = false;
	bool dedup_collapsed = false;
	int mate_bases = 0;                      // --mate-bases: 0 = off
	bool mate_filter = false;                // --mate-filter
	std::string ref_file;                    // -ref, for the plan's "mate:" line
	int mol_file = 0, mate_file = -1;        // ... the one decoded file and its mate, once every architecture is known
	std::string samples_line;                // --samples: the plan's "samples:" line
	std::string quality_line;                // --min-base-quality: the plan's "quality:" line
};

namespace {

std::vector<std::string> cmdline_segments(const td_run_opts* o)
{
	int last = -1;
	for (int k = 0; k < TD_RUN_MAX_SEGMENTS; k++) if (o->segments[k]) last = k;
	std::vector<std::string> s;
	for (int k = 0; k <= last; k++) s.push_back(o->segments[k] ? o->segments[k] : "");
	return s;
}

// --mate-filter with DUST or -ref: the outcome of one mate is joined on the device, a third file's is not (mol / mate: decide_outputs')
int mate_filter_files(const td_run_opts* o, int dust, bool use_ref, int mol, int mate)
{
	if (!o->mate_filter || o->n_infiles < 3 || (dust == 0 && !use_ref)) return TD_OK;
	int third = 0;
	while (third == mol || third == mate) third++;
	return run_fail("--mate-filter with DUST or -ref takes exactly two input files (%d given): the outcome of %s would be joined behind the count, "
	                "where a failing read takes a molecule's one kept read out of the files: run with -dust 0 and without -ref, or without that file.",
	                o->n_infiles, o->infile[third]);
}

// --samples FILE (tagdust_samples.h): one sample per line -- the name, then one barcode spelling per 'B' segment as the architecture
// lists them, separated by white space; '#' lines and blank lines are skipped
struct SampleSheet {
	std::vector<int> segs;                 // the 'B' segments of the architecture, in order
	std::vector<std::string> names;
	std::vector<const char*> name_ptrs;    // (as td_samples_enable takes them)
	std::vector<int32_t> tuples;           // [names.size() * segs.size()]
	int n() const { return (int)names.size(); }
};

// TD_FAIL with a message that names the line.  The sheet's own rules (rows and names pairwise different, the name's characters) are
// checked here too, so that the plan refuses what td_samples_enable would.
int read_sample_sheet(const char* path, const td_arch* a, SampleSheet& sh)
{
	sh = SampleSheet();
	for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'B') sh.segs.push_back(j);
	const int m = (int)sh.segs.size();
	if (m > TD_SAMPLES_MAX_SEGMENTS) return run_fail("--samples: the architecture has %d barcode segments (at most %d).", m, TD_SAMPLES_MAX_SEGMENTS);
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
		if ((int)w.size() != m + 1) { rc = run_fail("--samples: %s line %d: %d columns, need %d (the name and one barcode per barcode segment).", path, line, (int)w.size(), m + 1); break; }
		if (sh.n() == TD_SAMPLES_MAX) { rc = run_fail("--samples: %s line %d: more than %d samples.", path, line, TD_SAMPLES_MAX); break; }
		const std::string& name = w[0];
		bool ok = !name.empty() && name.size() <= TD_SAMPLES_MAX_NAME;
		for (const char ch : name) ok = ok && ((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '.' || ch == '_' || ch == '-');
		if (!ok) { rc = run_fail("--samples: %s line %d: the name '%s' is not 1..%d characters of [A-Za-z0-9._-].", path, line, name.c_str(), TD_SAMPLES_MAX_NAME); break; }
		std::vector<int32_t> row;
		for (int t = 0; t < m && rc == TD_OK; t++) {
			const int seg = sh.segs[(size_t)t];
			int found = -1;
			for (int q = 0; q < a->n_seq[seg] - 1; q++) if (w[(size_t)t + 1] == a->seqs[seg][q]) found = q;   // (the last one is the all-N wildcard)
			if (found < 0) rc = run_fail("--samples: %s line %d: '%s' is not a barcode of segment %d.", path, line, w[(size_t)t + 1].c_str(), seg + 1);
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
	for (const std::string& s : sh.names) sh.name_ptrs.push_back(s.c_str());
	return TD_OK;
}

std::string samples_file_name(const td_run_opts* o) { return std::string(o->outfile) + "_samples.txt"; }
std::string unknown_file_name(const td_run_opts* o) { return std::string(o->outfile) + "_unknown_barcodes.txt"; }
std::string molecules_file_name(const td_run_opts* o) { return std::string(o->outfile) + "_molecules.txt"; }

// what the controller decides once every file's architecture is known (barcode_hmm.c:130-159): TD_FAIL with the reference's message
// (mol_file: the file whose contexts count molecules -- file 0, or with --mate-bases the one file that is decoded; mate_file: its mate)
// (sheet: --samples resolved against the barcode file's architecture -- here, where the architectures are known, so that it works with -arch)
int decide_outputs(const td_run_opts* o, const std::vector<const td_arch*>& archs, int& bar_file, int& num_out_reads, std::vector<std::string>& names,
                   int* mol_file = nullptr, int* mate_file = nullptr, SampleSheet* sheet = nullptr)
{
	bar_file = -1; num_out_reads = 0;
	int mol = 0, mate = -1;
	if (o->mate_bases) {
		int n_decoded = 0;
		for (size_t k = 0; k < archs.size(); k++) if (!is_read_only(archs[k]) && n_decoded++ == 0) mol = (int)k;
		if (n_decoded != 1)
			return run_fail("--mate-bases: exactly one input file may have an architecture other than R:N (%d have): barcode and fingerprint of a "
			                "molecule come from one decoded file, every other file gives reads.", n_decoded);
		mate = mol == 0 ? 1 : 0;                 // the first file in call order other than the decoded one
	}
	if (mol_file) *mol_file = mol;
	if (mate_file) *mate_file = mate;
	for (size_t k = 0; k < archs.size(); k++) {
		if (has_barcode(archs[k])) {
			if (bar_file >= 0)
				return run_fail("Barcodes seem to be in both architectures... %s", o->samples_file ? "(--samples: barcodes spread over several input files are not "
				                "joined; the controller's rule of one barcode file stays, and a sheet lists the barcode segments of that one file.)" : "");
			bar_file = (int)k;
		}
		num_out_reads += read_segments(archs[k]);
	}
	if (num_out_reads == 0) return run_fail("No read segment in any architecture: there would be no output file.");
	// print_all() names its files after the barcode file's architecture, else the last file's (td_stream_run_multi; one file: td_writer_open)
	SampleSheet local;
	SampleSheet& sh = sheet ? *sheet : local;
	sh = SampleSheet();
	if (o->samples_file) {
		if (bar_file < 0) return run_fail("--samples: no input file's architecture has a barcode segment.");
		if (read_sample_sheet(o->samples_file, archs[(size_t)bar_file], sh) != TD_OK) return TD_FAIL;
		td_writer_file_names_samples(o->outfile, sh.names, num_out_reads, names, nullptr);
		names.push_back(samples_file_name(o));
	} else {
		td_writer_file_names_n(o->outfile, archs[(size_t)(bar_file >= 0 ? bar_file : (int)archs.size() - 1)], num_out_reads, names, nullptr);
	}
	if (o->unknown_barcodes > 0) {
		if (bar_file < 0) return run_fail("--unknown-barcodes: no input file's architecture has a barcode segment.");
		names.push_back(unknown_file_name(o));
	}
	if (o->molecules) {
		if (archs.size() == 1 && is_read_only(archs[0])) return run_fail("--molecules: the architecture is a single read segment: there is no model whose labels mark a barcode or a fingerprint.");
		if (o->collapse_umis && !has_fingerprint(archs[(size_t)mol]))
			return run_fail("--collapse-umis: the architecture has no fingerprint (F) segment: there is no UMI whose neighbours could be collapsed.");
		names.push_back(molecules_file_name(o));
	}
	if (o->min_base_quality) {   // the base-quality filter judges the one decoded file's barcode / UMI bases
		int n_decoded = 0, dec = 0;
		for (size_t k = 0; k < archs.size(); k++) if (!is_read_only(archs[k]) && n_decoded++ == 0) dec = (int)k;
		if (n_decoded == 0) return run_fail("--min-base-quality: the architecture is a single read segment: there is no model whose labels mark a barcode or a fingerprint.");
		if (n_decoded > 1)
			return run_fail("--min-base-quality: exactly one input file may have an architecture other than R:N (%d have): one file's verdicts are the run's.", n_decoded);
		const bool b = (o->quality_segments & TD_QUAL_SEG_B) && has_barcode(archs[(size_t)dec]), f = (o->quality_segments & TD_QUAL_SEG_F) && has_fingerprint(archs[(size_t)dec]);
		if (!b && !f) return run_fail("--min-base-quality: the architecture has no segment of the types --quality-segments names: there is no base to judge.");
	}
	if (bar_file >= 0 && !o->force)   // check_for_existing_demultiplexed_files_multiple, io.c:633-691 (made for the barcode file only)
		for (auto& n : names)
			if (file_exists(n)) return run_fail("Error: some output files already exists. (%s; --force overwrites)", n.c_str());
	return TD_OK;
}

}   // namespace

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
	SampleSheet sheet;
	if (p->all_known && decide_outputs(o, view, p->bar_file, p->num_out_reads, p->out_files, &p->mol_file, &p->mate_file, &sheet) != TD_OK) return TD_FAIL;
	if (o->samples_file) {
		p->samples_line = std::string("samples: ") + o->samples_file + ": ";
		if (!p->all_known) p->samples_line += "resolved once the arch file's choice is made";
		else {
			p->samples_line += std::to_string(sheet.n()) + " samples by segment";
			for (size_t t = 0; t < sheet.segs.size(); t++) p->samples_line += (t ? ", " : (sheet.segs.size() > 1 ? "s " : " ")) + std::to_string(sheet.segs[t] + 1);
			p->samples_line += " of file " + std::to_string(p->bar_file) + "; a read whose barcodes are incomplete or name no sample goes to _un";
		}
		p->samples_line += "\n";
	}
	if (o->min_base_quality)
		p->quality_line = "quality: an extracted read with more than " + std::to_string(o->max_low_bases) + " bases below Q" + std::to_string(o->min_base_quality) +
		                  " (offset " + std::to_string(o->quality_offset) + ") in its " +
		                  (o->quality_segments == TD_QUAL_SEG_B ? "barcode" : (o->quality_segments == TD_QUAL_SEG_F ? "fingerprint" : "barcode or fingerprint")) +
		                  " segments goes to _un and is neither assigned, counted nor kept by --dedup\n";
	if (p->all_known && mate_filter_files(o, p->dust, p->use_ref, p->mol_file, p->mate_file) != TD_OK) return TD_FAIL;
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
		if (p->all_known) s += " (file " + std::to_string(p->mol_file) + " is decoded, file " + std::to_string(p->mate_file) + " is its mate)";
		s += "\n";
	}
	s += p->samples_line;
	s += p->quality_line;
	if (p->all_known) {
		s += "barcode file: " + (p->bar_file >= 0 ? std::to_string(p->bar_file) : std::string("none")) + "\n";
		s += "output reads: " + std::to_string(p->num_out_reads) + "\n";
		for (auto& n : p->out_files) s += "output file: " + n + "\n";
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
	int bar_file = -1, num_out_reads = 0;
	std::vector<std::string> names;
	if (decide_outputs(o, view, bar_file, num_out_reads, names) != TD_OK) return -1;
	std::string s;
	for (auto& n : names) s += n + "\n";
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

// ---------------------------------------------------------------------------------------------------------
// the log
// ---------------------------------------------------------------------------------------------------------
namespace {

// append_message(), misc.c:285-335: "[YYYY-MM-DD HH:MM:SS]\t" in front of every message; the messages end in '\n' themselves
struct Log {
	std::string text;
	bool echo = false;
	void add(const std::string& msg)
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
	void addf(const char* fmt, ...)
	{
		char buf[2048];
		va_list ap;
		va_start(ap, fmt);
		vsnprintf(buf, sizeof buf, fmt, ap);
		va_end(ap);
		add(buf);
	}
	// free_param(), interface.c:715-726
	void write(const char* outfile) const
	{
		if (!outfile) return;
		const std::string name = std::string(outfile) + "_logfile.txt";
		if (FILE* f = fopen(name.c_str(), "w")) { fprintf(f, "%s\n", text.c_str()); fclose(f); }
	}
};

// the messages of barcode_hmm.c:387-430
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

}   // namespace

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

// ---------------------------------------------------------------------------------------------------------
// the run
// ---------------------------------------------------------------------------------------------------------
namespace {

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
	int mol_file = 0, mate_file = -1;     // the file whose contexts count molecules; with --mate-bases its mate, else -1
	SampleSheet sheet;                    // --samples, resolved against the barcode file's architecture (no sample without the option)
	bool device_counts = false;           // rep->counts are a context's own tally (td_counts_get), not the combined records'
	int qual_file = -1;                   // --min-base-quality: the one decoded file, whose context judges (-1 without the option)

	int head_limit() const { return o->flavour ? 1001000 : 1000001; }   // io.c:125-188 with num_query 1000 / 1 000 001

	int fail(const char* fmt, ...)
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
	int unknown_barcodes(int bar_file);
	int molecules();
	int samples(int bar_file);
	int quality();

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
	std::vector<std::string> out_files;
	int bar_file = -1, num_out_reads = 0;
	{
		std::vector<const td_arch*> view;
		for (auto& f : files) view.push_back(f.arch.get());
		if (decide_outputs(o, view, bar_file, num_out_reads, out_files, &mol_file, &mate_file, &sheet) != TD_OK ||
		    mate_filter_files(o, dust, use_ref, mol_file, mate_file) != TD_OK) { log.add(g_run_error + "\n"); return TD_FAIL; }
	}

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
			if (o->unknown_barcodes > 0 && k == bar_file &&
			    td_census_enable(c, -1, TD_CENSUS_DEFAULT_MASK, o->unknown_slots_log2) != TD_OK) return fail("%s", td_last_error(c));
			// --samples: the contexts of the barcode file assign every extracted read by all its barcodes, in front of census and count
			if (sheet.n() > 0 && k == bar_file &&
			    td_samples_enable(c, sheet.tuples.data(), sheet.name_ptrs.data(), sheet.n(), 16) != TD_OK) return fail("%s", td_last_error(c));
			// --min-base-quality: the context of the one decoded file drops extracted reads with low-quality barcode / UMI bases, in front
			// of samples, census and count (the streaming run names every batch's quality lines)
			if (o->min_base_quality && tables) {
				if (td_qual_enable(c, o->min_base_quality, o->quality_offset, o->max_low_bases, o->quality_segments) != TD_OK) return fail("%s", td_last_error(c));
				qual_file = k;
			}
			// --molecules: the contexts of the one input file (with --mate-bases: of the one decoded file) count its extracted reads per
			// barcode, fingerprint and start of the read
			if (k != mol_file) continue;
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

	if (qual_file >= 0 && quality() != TD_OK) return TD_FAIL;
	if (sheet.n() > 0 && samples(bar_file) != TD_OK) return TD_FAIL;
	if (o->unknown_barcodes > 0 && unknown_barcodes(bar_file) != TD_OK) return TD_FAIL;
	if (o->molecules && molecules() != TD_OK) return TD_FAIL;

	// 6. the summary, barcode_hmm.c:387-430
	for (auto& m : summary_messages(o, rep)) log.add(m);
	return TD_OK;
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

// --unknown-barcodes: every device's census of the barcode file, merged (nothing of it enters the log), and <out>_unknown_barcodes.txt
int Run::unknown_barcodes(int bar_file)
{
	FileState& f = files[(size_t)bar_file];
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

	const td_arch* a = f.arch.get();
	int seg = -1;
	for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'B') seg = j;
	const std::string name = unknown_file_name(o);
	FILE* out = fopen(name.c_str(), "w");
	if (!out) return fail("Failed to open file:%s", name.c_str());
	fprintf(out, "# unknown barcodes: what the reads that were not extracted spell in segment %d (%s) of %s\n", seg + 1, f.segs[(size_t)seg].c_str(), o->infile[bar_file]);
	fprintf(out, "# eligible reads\t%lld\n# counted\t%lld\n# distinct sequences\t%lld\n# no base in the segment\t%lld\n# more than %d bases\t%lld\n# with N\t%lld\n",
	        (long long)sum.eligible, (long long)sum.counted, (long long)sum.distinct, (long long)sum.skipped_empty, TD_CENSUS_MAX_WORD,
	        (long long)sum.skipped_long, (long long)sum.skipped_n);
	if (sum.overflow > 0)
		fprintf(out, "# the counting table was too small: %lld reads were not counted (the counts below are exact; --unknown-barcodes-slots %d or more)\n",
		        (long long)sum.overflow, o->unknown_slots_log2 + 1);
	fprintf(out, "# count\tsequence\tnearest\tdistance\n");
	const int n_listed = a->n_seq[seg] - 1;   // (the last one is the all-N wildcard)
	for (int64_t i = 0; i < n_acc && i < o->unknown_barcodes; i++) {
		char word[32];
		if (td_census_key_text(acc[i].key, word) != TD_OK) { fclose(out); return fail("%s", td_last_error(nullptr)); }
		int best = -1, best_d = 0;
		for (int q = 0; q < n_listed; q++) {
			const int d = edit_distance(word, a->seqs[seg][q]);
			if (best < 0 || d < best_d) { best = q; best_d = d; }   // (ties go to the lower index)
		}
		fprintf(out, "%lld\t%s\t%s\t%d\n", (long long)acc[i].count, word, best >= 0 ? a->seqs[seg][best] : "-", best >= 0 ? best_d : -1);
	}
	fclose(out);
	return TD_OK;
}

// --min-base-quality: the totals of the decoded file's context (one device); behind the summary's counts in the log
int Run::quality()
{
	td_ctx* c = files[(size_t)qual_file].raw[0];
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
int Run::samples(int bar_file)
{
	FileState& f = files[(size_t)bar_file];
	td_census_entry* acc = nullptr;
	int64_t n_acc = 0;
	td_samples_totals sum{};
	std::vector<td_samples_totals> per;
	if (merged_entries(f, td_samples_get, acc, n_acc, per) != TD_OK) return TD_FAIL;
	for (const td_samples_totals& t : per) {
		sum.eligible += t.eligible; sum.assigned += t.assigned; sum.unlisted += t.unlisted; sum.incomplete += t.incomplete; sum.overflow += t.overflow;
	}
	rep->samples = acc; rep->n_sample_keys = n_acc; rep->samples_totals = sum; rep->n_samples = sheet.n();
	// a context's own tally is the decode kernel's: the reads that lost their extraction here move to "barcode / UMI not found"
	if (device_counts) {
		rep->counts[TD_EXTRACT_SUCCESS] -= sum.unlisted + sum.incomplete;
		rep->counts[TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND] += sum.unlisted + sum.incomplete;
	}
	const td_arch* a = f.arch.get();
	const int m = (int)sheet.segs.size();
	const std::string name = samples_file_name(o);
	FILE* out = fopen(name.c_str(), "w");
	if (!out) return fail("Failed to open file:%s", name.c_str());
	fprintf(out, "# samples: the extracted reads of %s by all their barcodes\n# sheet\t%s\n# samples\t%d\n# segments", o->infile[bar_file], o->samples_file, sheet.n());
	for (int t = 0; t < m; t++) fprintf(out, "\t%d (%s)", sheet.segs[(size_t)t] + 1, f.segs[(size_t)sheet.segs[(size_t)t]].c_str());
	fprintf(out, "\n# extracted reads\t%lld\n# assigned\t%lld\n# not in the sheet\t%lld\n# incomplete\t%lld\n# not counted\t%lld\n", (long long)sum.eligible,
	        (long long)sum.assigned, (long long)sum.unlisted, (long long)sum.incomplete, (long long)sum.overflow);
	if (sum.overflow > 0) fprintf(out, "# the counting table was too small: the counts below are exact, %lld reads are in none of them\n", (long long)sum.overflow);
	fprintf(out, "# sample");
	for (int t = 0; t < m; t++) fprintf(out, "\tbarcode %d", t + 1);
	fprintf(out, "\treads\tshare\n");
	std::vector<char> listed((size_t)std::max<int64_t>(n_acc, 1), 0);
	for (int s = 0; s < sheet.n(); s++) {
		const uint64_t key = td_samples_key(sheet.tuples.data() + (size_t)s * m, m);
		int64_t reads = 0;
		for (int64_t i = 0; i < n_acc; i++) if (acc[i].key == key) { reads = acc[i].count; listed[(size_t)i] = 1; }
		fprintf(out, "%s", sheet.names[(size_t)s].c_str());
		for (int t = 0; t < m; t++) fprintf(out, "\t%s", a->seqs[sheet.segs[(size_t)t]][sheet.tuples[(size_t)s * m + t]]);
		fprintf(out, "\t%lld\t%0.4f\n", (long long)reads, sum.eligible > 0 ? (double)reads / (double)sum.eligible : 0.0);
	}
	fprintf(out, "# combinations not in the sheet\n");
	for (int64_t i = 0; i < n_acc; i++) {   // (td_samples_get's order: count descending, then key ascending)
		if (listed[(size_t)i]) continue;
		int32_t calls[TD_SAMPLES_MAX_SEGMENTS], km = 0;
		if (td_samples_key_calls(acc[i].key, calls, &km) != TD_OK || km != m) { fclose(out); return fail("--samples: 0x%llx is no key of %d segments", (unsigned long long)acc[i].key, m); }
		for (int t = 0; t < m; t++) {
			const int seg = sheet.segs[(size_t)t];
			fprintf(out, "%s%s", t ? "\t" : "", calls[t] < 0 || calls[t] >= a->n_seq[seg] ? "-" : a->seqs[seg][calls[t]]);   // (the decoy's own spelling is its N's)
		}
		fprintf(out, "\t%lld\t%0.4f\n", (long long)acc[i].count, sum.eligible > 0 ? (double)acc[i].count / (double)sum.eligible : 0.0);
	}
	fclose(out);
	return TD_OK;
}

// --molecules: one device's own summary, or every device's entries merged and summarised on the host (nothing of it enters the
// log), and <out>_molecules.txt
int Run::molecules()
{
	FileState& f = files[(size_t)mol_file];
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
	td_mol_row* crows = nullptr;
	if (o->collapse_umis) {
		crows = (td_mol_row*)calloc(TD_NUM_BARCODE_BINS, sizeof(td_mol_row));
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

	const td_arch* a = f.arch.get();
	int seg = -1;
	for (int j = 0; j < a->n_segments; j++) if (a->type[j] == 'B') seg = j;
	const std::string name = molecules_file_name(o);
	FILE* out = fopen(name.c_str(), "w");
	if (!out) return fail("Failed to open file:%s", name.c_str());
	fprintf(out, "# molecules: the extracted reads of %s by barcode, fingerprint and the first bases of the read\n", o->infile[mol_file]);
	fprintf(out, "# prefix bases\t%d\n", o->molecules_prefix);
	if (o->mate_bases) fprintf(out, "# mate bases\t%d\n# mate file\t%s\n", o->mate_bases, o->infile[mate_file]);
	if (o->mate_filter) fprintf(out, "# mate filter\tdust %d, -ref %s\n", dust, use_ref ? o->reference_fasta : "none");
	fprintf(out, "# extracted reads\t%lld\n# counted\t%lld\n# molecules\t%lld\n# no read base\t%lld\n# N in the prefix\t%lld\n",
	        (long long)sum.eligible, (long long)sum.counted, (long long)sum.molecules, (long long)sum.skipped_empty, (long long)sum.skipped_n);
	if (sum.overflow > 0)
		fprintf(out, "# the counting table was too small: %lld reads were not counted (the counts below are exact; --molecules-slots %d or more)\n",
		        (long long)sum.overflow, o->molecules_slots_log2 + 1);
	if (o->dedup_collapsed) fprintf(out, "# dedup\tcollapsed molecules\n");
	if (o->dedup)
		fprintf(out, "# written\t%lld\n# duplicates removed\t%lld\n", (long long)rep->dedup_totals.kept, (long long)rep->dedup_totals.duplicates);
	if (crows)
		fprintf(out, "# UMI collapse\tfingerprints one mismatch apart, directional rule\n# molecules after collapse\t%lld\n# absorbed\t%lld\n",
		        (long long)rep->collapse_totals.molecules_after, (long long)rep->collapse_totals.absorbed);
	fprintf(out, "# barcode\treads\tmolecules\tduplication\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10+%s\n", crows ? "\tcollapsed\tduplication_collapsed" : "");
	// (collapsed: the molecules of the row after the collapse, with --collapse-umis)
	auto line = [&](const char* label, const td_mol_row& r, int64_t collapsed) {
		fprintf(out, "%s\t%lld\t%lld\t%0.4f", label, (long long)r.reads, (long long)r.molecules,
		        r.reads > 0 ? 1.0 - (double)r.molecules / (double)r.reads : 0.0);
		for (int q = 0; q < TD_MOL_LEVELS; q++) fprintf(out, "\t%lld", (long long)r.levels[q]);
		if (crows) fprintf(out, "\t%lld\t%0.4f", (long long)collapsed, r.reads > 0 ? 1.0 - (double)collapsed / (double)r.reads : 0.0);
		fprintf(out, "\n");
	};
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
	fclose(out);
	return TD_OK;
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
			    (sheet.n() > 0 && td_samples_reset(c) != TD_OK) || (o->min_base_quality && td_qual_reset(c) != TD_OK))
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
		sf[(size_t)k].ctx = o->mate_bases && k != mol_file ? nullptr : files[(size_t)k].raw.data();
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
