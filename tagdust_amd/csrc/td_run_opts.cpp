// td_run_opts.cpp -- the options of the whole-run driver (include/tagdust_run.h): what the reference's interface()
// (src/interface.c:49-480) and free_param() (src/interface.c:709-726) do for struct parameters -- the option table, the defaults,
// the usage text, td_run_parse_args -- and the message of a failed call.  Plain C++: no device, no other unit of the library.
#include <stdio.h>
#include <stdlib.h>

#include "td_run_internal.h"

namespace tdrun {

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

}   // namespace tdrun

using namespace tdrun;

namespace {

struct OptSpec { const char* name; int arg; int id; };
enum { O_SEG = 1 /* .. 10 */, O_ARCH = 20, O_OUT, O_THREADS, O_Q, O_E, O_I, O_MINLEN, O_DUST, O_REF, O_FE, O_START, O_END, O_SEED,
       O_HELP, O_VERSION, O_DEVICES, O_RTEST, O_HOST_THREADS, O_BATCH_READS, O_SYNC_COMPILE, O_STATS_ON_HOST, O_FORCE, O_DRY_RUN,
       O_UNKNOWN, O_UNKNOWN_SLOTS, O_FINGER_SEQ, O_MOLECULES, O_MOLECULES_PREFIX, O_MOLECULES_SLOTS, O_DEDUP, O_COLLAPSE,
       O_DEDUP_COLLAPSED, O_MATE_BASES, O_MATE_FILTER, O_SAMPLES, O_MIN_BASE_QUALITY, O_MAX_LOW_BASES, O_QUALITY_SEGMENTS, O_QUALITY_OFFSET,
       O_JOIN_BARCODES,
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
	{ "join-barcodes", 0, O_JOIN_BARCODES },
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
	       "\t--join-barcodes             with --samples: the barcodes of a sample lie in several input files (dual-index runs, I1.fq and\n"
	       "\t                            I2.fq): the sheet's barcode columns are the B segments of all files, files first in call order,\n"
	       "\t                            at most four; a read whose partner in another barcode file is not extracted goes to _un (one\n"
	       "\t                            device; not with --unknown-barcodes, --molecules, --min-base-quality or -start / -end)\n"
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
		case O_JOIN_BARCODES: o->join_barcodes = 1; break;
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
