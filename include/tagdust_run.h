/*
 * tagdust_run.h -- a whole TagDust2 run on this library alone: files in, demultiplexed files out (part of libtagdust_hip.so,
 * plain C; the `tagdust-hip` executable is a main() of a few lines over it).  What the reference does in
 *
 *   main()                      src/main.c:95-217        (the checks, "Start Run")
 *   interface()                 src/interface.c:49-480   (options, defaults, banner and cmd: line, the multiread rule)
 *   hmm_controller_multiple()   src/barcode_hmm.c:51-460 (architectures per file, statistics, thresholds, models, the run, the log)
 *   test_architectures()        src/test_architectures.c:20-289 (the -arch file)
 *   free_param()                src/interface.c:709-726  (<out>_logfile.txt)
 *
 * composed from td_arch_parse, td_compare_architectures, td_sequence_stats_device, td_estimate_threshold, td_model_build,
 * td_set_artifacts and the streaming pipelines td_stream_run / td_stream_run_multi.  The output files equal the reference
 * binary's byte for byte.  Every entry point returns TD_OK / TD_FAIL and never calls exit(); the message of a failed call of this
 * header is in td_run_last_error() (per thread) and, for td_run_execute, in the report.
 */
#ifndef TAGDUST_RUN_H
#define TAGDUST_RUN_H

#include <stddef.h>
#include <stdint.h>
#include "tagdust_hip.h"
#include "tagdust_io.h"
#include "tagdust_census.h"
#include "tagdust_molecules.h"
#include "tagdust_samples.h"
#include "tagdust_quality.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_RUN_MAX_SEGMENTS 10   /* options -1 .. -10 */
#define TD_RUN_MAX_FILES    8    /* input files of one run (td_stream_run_multi's limit) */
#define TD_RUN_MAX_DEVICES  16

/* struct parameters (src/interface.h:90-160) as far as a `tagdust` run uses it; defaults as interface.c:66-129 */
typedef struct td_run_opts {
	char*    segments[TD_RUN_MAX_SEGMENTS];  /* -1 .. -10: "B:ACGT,TTGA", "R:N", ...; NULL = not given */
	char*    arch_file;              /* -arch */
	char*    outfile;                /* -o / -out */
	int32_t  num_threads;            /* -t                     [8]  (thread ranges of the -ref filter and of the -arch score sums) */
	float    confidence_threshold;   /* -Q / -q / -threshold   [0 = calibrate]; a given value switches calibration off and every
	                                    file then runs with threshold 0 (barcode_hmm.c:102, :190-200, :314) */
	float    sequencer_error_rate;   /* -e                     [0.05]; calibration forces 0.05 (calibrateQ.c:65, :117) */
	float    indel_frequency;        /* -i                     [0.1] */
	int32_t  minlen;                 /* -minlen                [16] */
	int32_t  dust;                   /* -dust                  [100], 0 = off */
	char*    reference_fasta;        /* -ref */
	int32_t  filter_error;           /* -fe                    [2] */
	int32_t  matchstart, matchend;   /* -start (stored as atoi - 1, interface.c:286), -end   [-1, -1] */
	uint32_t seed;                   /* -seed                  [0 = time based, calibrateQ.c:27-31] */
	int32_t  n_infiles;
	char**   infile;
	/* this library's own */
	int32_t  n_devices;              /* --devices 0,1          [1] */
	int32_t  devices[TD_RUN_MAX_DEVICES];   /*                 [{0}] */
	int32_t  flavour;                /* --rtest: 0 = the release build's constants (batches of 1 000 001 records, 400 000 calibration
	                                    reads on the C library's rand()); 1 = those of the -DRTEST builds (1000 / 4000 / the private
	                                    generator, misc.c:878-887) */
	int32_t  host_threads;           /* --host-threads         [0 = td_stream_opts picks] */
	int32_t  batch_reads;            /* --batch-reads          [0 = td_stream_opts picks; 1000 in the RTEST flavour] */
	int32_t  sync_compile;           /* --sync-compile: 1 = compile the model kernel before decoding; 0 = option "async_compile" */
	int32_t  stats_on_host;          /* --stats-on-host: 1 = td_sequence_stats_limit instead of td_sequence_stats_device */
	int32_t  force;                  /* --force: overwrite existing output files */
	int32_t  dry_run;                /* --dry-run: print the plan and stop */
	int32_t  help, version;          /* -h / -help, -v / -version */
	int32_t  echo_log;               /* every log message also goes to stderr as it is made, as the reference does (the executable sets it) */
	int32_t  argc;                   /* the command line as given, for the log's "cmd:" line */
	char**   argv;
	int32_t  unknown_barcodes;       /* --unknown-barcodes K   [0 = off]: the K most frequent barcode spellings of the reads that were not
	                                    extracted (tagdust_census.h, the default outcomes) go to <out>_unknown_barcodes.txt */
	int32_t  unknown_slots_log2;     /* --unknown-barcodes-slots N   [20]: the census table of every device has 2^N slots */
	int32_t  fingerprint_seq;        /* --fingerprint-seq: ";FP:ACGT" instead of ";FP:27" in the read names, byte for byte what the
	                                    reference's -show_finger_seq writes (td_fingerprint_text) */
	int32_t  molecules;              /* --molecules: reads, molecules, duplication rate and duplication levels per barcode
	                                    (tagdust_molecules.h) go to <out>_molecules.txt; one input file only */
	int32_t  molecules_prefix;       /* --molecules-prefix P   [20]: read bases that tell molecules apart beside barcode and fingerprint, 1..32 */
	int32_t  molecules_slots_log2;   /* --molecules-slots N    [26]: the counting table of every device has 2^N slots, 4..30 */
	int32_t  dedup;                  /* --dedup: one read per molecule is written (tagdust_molecules.h, td_mol_dedup_enable): an extracted
	                                    read that is not the first of its molecule goes to no file.  Implies --molecules (the parser sets
	                                    it); one input file, one device */
	int32_t  collapse_umis;          /* --collapse-umis: fingerprints one mismatch apart are counted as one molecule (tagdust_molecules.h,
	                                    td_mol_collapse_enable).  Implies --molecules (the parser sets it); refused without an F segment */
	int32_t  dedup_collapsed;        /* --dedup-collapsed: one read per COLLAPSED molecule is written (tagdust_molecules.h, td_mol_dedup_freeze):
	                                    the input file is read twice -- td_stream_survey, the freeze, td_stream_run.  Implies --dedup,
	                                    --collapse-umis and --molecules (the parser sets them); refused wherever they are and for the input "-" */
	int32_t  mate_bases;             /* --mate-bases M         [0 = off]: with two or more input files, the first M bases (1..31) of the read's
	                                    mate -- the record of the first file in call order other than the decoded one -- join the molecule
	                                    key behind the read's own prefix (tagdust_molecules.h, td_mol_mate_enable).  Implies --molecules
	                                    (the parser sets it) and lifts its one-input-file rule; refused with one input file, when
	                                    molecules_prefix + M > 32, with an effective DUST other than 0 or a -ref filter (the mate's own outcome
	                                    is not joined), with more than one device, with --dedup-collapsed (the survey reads one file), and
	                                    unless exactly one file has an architecture other than R:N */
	int32_t  mate_filter;            /* --mate-filter: with --mate-bases, the mate is judged as the reference judges an R:N file -- this run's
	                                    DUST and -ref filter -- and its outcome joined to its read's in front of the count (tagdust_molecules.h,
	                                    td_mol_mate_filter_enable): a read whose mate fails is neither counted nor kept by --dedup.  Lifts
	                                    --mate-bases' refusal of DUST and -ref for two input files; refused without --mate-bases, and with
	                                    three or more files unless DUST is 0 and there is no -ref (a third file's outcome is not joined).
	                                    The one-device, one-decoded-file and no --dedup-collapsed rules of --mate-bases stay */
	char*    samples_file;           /* --samples FILE         [NULL = off]: combinatorial barcodes (tagdust_samples.h).  FILE holds one sample
	                                    per line: the name, then one barcode spelling per 'B' segment of the barcode file's architecture as
	                                    that lists them, separated by white space; '#' lines and blank lines are skipped.  It is resolved once
	                                    the architectures are known (so it works with -arch); a spelling that its segment does not list, a
	                                    wrong column count, a repeated row or name is an error that names the line.  The output files are
	                                    <out>_BC_<name>[_READ<k>].fq in sheet order, then _un; <out>_samples.txt reports the samples and the
	                                    combinations no sample has; <out>_molecules.txt labels its rows with the sample names.  Refused with
	                                    -start / -end and when no input file's architecture has a 'B' segment; barcodes spread over several
	                                    input files are joined only with --join-barcodes (else the controller's rule of one barcode file stays) */
	int32_t  min_base_quality;       /* --min-base-quality Q   [0 = off]: the base-quality filter (tagdust_quality.h, td_qual_enable): an
	                                    extracted read with more than max_low_bases barcode / UMI bases below Q (1..93) goes to the _un file
	                                    and is neither assigned, counted nor kept by --dedup.  Adds a "quality:" line to the plan and one line
	                                    behind the summary's counts to the log.  Refused with -start / -end, with more than one device, with
	                                    more than one decoded file (--mate-bases' layout, barcode and UMI in read 1 and R:N files beside
	                                    it, is in), for a read-only architecture and for FASTA input (the run fails at the first record
	                                    without a quality line) */
	int32_t  max_low_bases;          /* --max-low-bases K      [0] */
	int32_t  quality_segments;       /* --quality-segments B|F|BF   [BF = TD_QUAL_SEG_B | TD_QUAL_SEG_F]: the segments whose bases are judged */
	int32_t  quality_offset;         /* --quality-offset 33|64 [33] */
	int32_t  join_barcodes;          /* --join-barcodes        [0]: with --samples, the barcodes of a sample lie in several input files
	                                    (tagdust_samples.h, the join across input files).  The barcode files are those whose architecture
	                                    has a 'B' segment, in call order; the sheet's barcode columns are their 'B' segments, files first.
	                                    The first barcode file's contexts hold the sheet, every other one's export their calls.  Adds a
	                                    "join:" line to the plan; <out>_samples.txt names the file of each column and has a "# partner
	                                    failed" line.  Refused without --samples, with more than one device, with --unknown-barcodes, with
	                                    -start / -end, when the barcode files have more than four 'B' segments together and when only one
	                                    file has barcodes; --molecules, --mate-bases and --min-base-quality are refused for two decoded
	                                    files by their own rules */
} td_run_opts;

td_run_opts* td_run_opts_new(void);            /* the defaults */
void td_run_opts_free(td_run_opts* opts);
const char* td_run_last_error(void);

/* The reference's option table (interface.c:133-183) with one or two leading dashes, no abbreviations; an argument that is no
 * option (or is "-") is an input file, wherever it stands.  An option the reference parses but this library does not implement
 * (-show_finger_seq, -train, -exact5, -join, -split, -name / -format, -f / -filter, -a, -l / -log, -p, -simulation, -numbarcode,
 * every -sim_*) fails with a message that names it, as does anything unknown: nothing is silently ignored.  argv[0] is the program name. */
int td_run_parse_args(int argc, const char* const* argv, td_run_opts** out, char* err, size_t errcap);
/* the usage text / the version line the executable prints */
const char* td_run_usage(void);
const char* td_run_version(void);

/* ---- the decisions of a run that need no data and no GPU ----
 * main.c:103-125 (an architecture or an arch file, -o, the files exist), per file where its architecture comes from
 * (barcode_hmm.c:105-129: file 0 the command line's segments when there are any, else the arch file's best candidate, else R:N),
 * "barcodes in more than one file" (:141-146), the number of output reads and the output files' names (td_writer_open's), the
 * existing-output check (io.c:633-691: made when a file holds a barcode, like the reference's; skipped with `force`; with
 * --unknown-barcodes <out>_unknown_barcodes.txt is one of the output files, and the option is refused with -start / -end; with
 * --molecules <out>_molecules.txt is one, and the option is refused with -start / -end, with several input files -- the read and
 * its UMI then sit in different files' contexts -- and for a read-only architecture, which has no model; --dedup implies
 * --molecules, is refused wherever that is and with more than one device -- each has its own table, a molecule split over two
 * would survive twice -- and adds two lines, "# written" and "# duplicates removed", to <out>_molecules.txt and nothing to the
 * log, the _un file or the counts; --collapse-umis implies --molecules, is refused wherever that is and for an architecture without
 * an F segment, may be given with --dedup, which still matches exactly, and adds three lines -- "# UMI collapse", "# molecules
 * after collapse", "# absorbed" -- and two columns behind "10+", "collapsed" and "duplication_collapsed", to <out>_molecules.txt;
 * --dedup-collapsed implies --dedup, --collapse-umis and --molecules, is refused wherever they are and for the input "-" -- stdin
 * cannot be read twice --, gives "# written" and "# duplicates removed" the replay's numbers and adds one line, "# dedup", in front
 * of them, while every other output of the run reports the second pass alone; --mate-bases, see td_run_opts, adds a "mate:" line
 * to the plan and two lines, "# mate bases" and "# mate file", behind "# prefix bases" to <out>_molecules.txt, and the run gives the
 * files other than the decoded one no contexts, so their reads are uploaded once, as mates, by the decoded file's context;
 * --mate-filter, see td_run_opts, says in that "mate:" line that the filter is on and with what -- dust and the -ref file or none --
 * and adds one line, "# mate filter", behind "# mate file"), the
 * multiread rule (interface.c:441-450: DUST and -ref off, with a warning, when the command line's architecture has two or more
 * R segments).  What depends on the arch file's choice is decided again by td_run_execute once the choice is made. */
typedef struct td_run_plan_t td_run_plan_t;   /* (the function below has the plain name) */
int  td_run_plan(const td_run_opts* opts, td_run_plan_t** out);
void td_run_plan_free(td_run_plan_t* plan);
/* the plan as text, one line per decision ("key: value"); returns the length, copies at most cap - 1 bytes + NUL */
int64_t td_run_plan_describe(const td_run_plan_t* plan, char* buf, int64_t cap);
/* What the run decides once every file's architecture is known (td_run_execute does, after the arch file's choice): the output
 * files for these per-file architectures ("-1 B:ACGT,TTGA -2 R:N" each), one name per line, named after the barcode file's
 * architecture with one set per read segment of the whole run.  -1 (td_run_last_error) for barcodes in two files, no read
 * segment at all, or -- without opts->force -- an output file that exists. */
int64_t td_run_output_files_describe(const td_run_opts* opts, const char* const* architectures, int32_t n_files, char* buf, int64_t cap);
/* test_architectures.c:72-111 on its own: the candidates of an arch file, one "-1 X -2 Y ..." line each (as "Using:" prints them) */
int64_t td_run_arch_file_describe(const char* arch_file, char* buf, int64_t cap);

/* ---- the run ---- */
typedef struct td_run_report {
	char     error[1024];                     /* empty on success */
	int64_t  counts[TD_NUM_COUNTERS];         /* the controller's counting over the combined records (barcode_hmm.c:354-384) */
	int32_t  n_artifacts;                     /* -ref sequences */
	int64_t* artifact_hits;                   /* [n_artifacts] reference_fasta->mer_hash */
	char**   artifact_names;                  /* [n_artifacts] reference_fasta->sn */
	int32_t  n_files;
	float    thresholds[TD_RUN_MAX_FILES];    /* param->confidence_thresholds */
	float    selected_threshold;              /* what the log's "selected threshold" line shows: the last file's */
	char*    architectures[TD_RUN_MAX_FILES]; /* "-1 B:ACGT,TTGA -2 R:N" */
	td_stream_stats stream;
	double   arch_s, stats_s, calibration_s, compile_wait_s, stream_s;   /* seconds: -arch selection, statistics, calibration,
	                                              td_model_upload (the compile, unless it runs in the background), streaming */
	int32_t  stats_on_device;                 /* 1: the statistics were counted on the device */
	char*    log;                             /* the text of <out>_logfile.txt */
	int64_t  n_unknown;                       /* --unknown-barcodes: distinct spellings over all devices (0 without the option) */
	td_census_entry* unknown;                 /* [n_unknown] by count descending, then key ascending */
	td_census_totals unknown_totals;          /* summed over the devices */
	td_mol_row* molecules;                    /* --molecules: [TD_NUM_BARCODE_BINS] one row per barcode bin (NULL without the option):
	                                             one device's own summary (td_mol_get), or td_mol_summarise of the devices' merged entries */
	td_mol_totals molecules_totals;           /* summed over the devices; molecules = distinct keys after the merge */
	int32_t  dedup;                           /* 1: the run removed duplicates (--dedup) */
	td_mol_dedup_totals dedup_totals;         /* --dedup: extracted reads written, duplicates removed, reads that could not be judged */
	int32_t  collapse;                        /* 1: the run collapsed neighbouring UMIs (--collapse-umis) */
	td_mol_collapse_totals collapse_totals;   /* --collapse-umis: molecules before and after, absorbed, the longest chain */
	td_mol_row* molecules_collapsed;          /* --collapse-umis: [TD_NUM_BARCODE_BINS] the rows from the collapsed counts (NULL without the
	                                             option): td_mol_collapse_get's, or td_mol_summarise of td_mol_collapse_host over the devices' td_mol_origins */
	int32_t  dedup_collapsed;                 /* 1: the duplicates removed are those of the collapsed molecules (--dedup-collapsed) */
	double   survey_s;                        /* --dedup-collapsed: seconds of the first pass, td_stream_survey and the freeze (inside stream_s) */
	int32_t  n_samples;                       /* --samples: rows of the sheet (0 without the option) */
	int64_t  n_sample_keys;                   /* ... distinct barcode combinations over all devices */
	td_census_entry* samples;                 /* [n_sample_keys] td_samples_get's entries, merged with td_census_merge */
	td_samples_totals samples_totals;         /* summed over the devices.  With one file on one device `counts` are the context's own tally
	                                             (td_counts_get), and the reads that lost their extraction here are moved from slot
	                                             TD_EXTRACT_SUCCESS to slot TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND; the barcode bins stay the decode kernel's */
	int32_t  quality;                         /* 1: the run dropped reads by base quality (--min-base-quality) */
	td_qual_totals quality_totals;            /* ... td_qual_get's totals of the decoded file's context.  With one file on one device the reads
	                                             it failed are moved from slot TD_EXTRACT_SUCCESS to slot TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND
	                                             of `counts`, as the samples rewrite's are: the log's "extracted" agrees with the files */
	int64_t  partner_failed;                  /* --join-barcodes: reads extracted in the first barcode file whose partner in another was not */
} td_run_report;
/* In the controller's order: architectures per file, statistics over each file's head, thresholds, models, the run, the log.
 * A failure before the first batch leaves no output files behind; one during the run leaves them as they are and says so.  The
 * log written so far goes to <out>_logfile.txt either way.  report may be NULL; free its members with td_run_report_clear. */
int  td_run_execute(const td_run_opts* opts, td_run_report* report);
void td_run_report_clear(td_run_report* report);
/* The controller's summary block (barcode_hmm.c:387-430) from a report: "Done.", the input files, the counts, "%0.1f%%\textracted",
 * one "count\tname" line per artifact sequence that was hit -- the messages as they enter the log, without their time stamps,
 * each ending in '\n'.  Returns the length, copies at most cap - 1 bytes + NUL. */
int64_t td_run_format_summary(const td_run_opts* opts, const td_run_report* report, char* buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif
