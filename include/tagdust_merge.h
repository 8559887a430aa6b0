/*
 * tagdust_merge.h -- merging of overlapping paired-end reads (part of libtagdust_hip.so, plain C; the `tagdust-merge`
 * executable is a main() of a few lines over it).  What the reference's `merge` program does in
 *
 *   merge()           src/merge.c:59-216    (lock-step batches of both files, equal counts, the first 1000 names)
 *   do_merging()      src/merge.c:298-340   (read 2 reverse-complemented, its qualities reversed, one record per pair)
 *   overlap_reads()   src/merge.c:399-688   (per-base error profiles, every ungapped offset scored, the consensus)
 *
 * with the output of `merge -t 1` as the contract: records in input order, byte for byte.
 *
 * Arithmetic.  Everything in overlap_reads() is plain IEEE float in a fixed order except pow() and log(), the C library's
 * double routines.  Both have tiny domains here, so the host evaluates them into tables (td_merge_tables_build) and neither the
 * host path nor the kernel calls them per cell: the score of a cell is T[(q_f, x_f)][(q_r, x_r)], gathered and added.
 *
 * Where the reference has no defined behaviour this library does this:
 *   - no candidate offset qualifies (a read not longer than min_overlap), or every candidate scores -inf (best_d stays -1 and
 *     the reference reads seq[-1]): the pair writes no record, status TD_MERGE_NO_CANDIDATE, counted in n_too_short;
 *   - a base code 5 ('.', past rev_nuc_code[]), FASTA input (no qualities), another number of input files than two: TD_FAIL.
 *
 * Every entry point returns TD_OK / TD_FAIL and never calls exit(); the message of a failed call is in td_merge_last_error()
 * (per thread).
 */
#ifndef TAGDUST_MERGE_H
#define TAGDUST_MERGE_H

#include <stddef.h>
#include <stdint.h>
#include "tagdust_hip.h"
#include "tagdust_io.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_MERGE_TABLE_AUTO   0   /* T in LDS when it fits the budget, else in global memory */
#define TD_MERGE_TABLE_LDS    1   /* T in LDS; the call fails when it does not fit */
#define TD_MERGE_TABLE_GLOBAL 2   /* T in global memory */

typedef struct td_merge_opts {
	int32_t min_overlap;      /* -minlen                 [16]: a candidate needs more than this many bases left in both reads */
	float   threshold;        /* -Q / -q / -threshold    [0]: a record is written when id / aligned >= threshold */
	int32_t n_threads;        /* -t: host threads (td_merge_host, and the parse / format stages of td_merge_stream); 0 = pick */
	int32_t batch_pairs;      /* --batch-pairs: pairs per batch of td_merge_stream; 0 = 2^18 */
	int32_t device;           /* --device; -1 = the host path (--host) */
	int32_t table_placement;  /* TD_MERGE_TABLE_*: where the kernel keeps T */
} td_merge_opts;
void td_merge_opts_default(td_merge_opts* opts);
const char* td_merge_last_error(void);

/* ---- the host tables: pow() and log() of the C library, once per distinct argument ----
 * q: the distinct quality characters among `qual` (n bytes), in ascending order, renumbered 0 .. nq-1.
 * profile[2 q]     = (float)(1.0 - pow(10.0, -((int)char - 33) / 10.0))             the called base   (merge.c:428, :442)
 * profile[2 q + 1] = (float)((1.0 - (float)score) / 3.0)                            the other three   (merge.c:444)
 * T[(5 q_f + x_f) * dim + (5 q_r + x_r)] = prob2scaledprob(sum), sum = 0.0f + f[0]*r[0] + f[1]*r[1] + f[2]*r[2] + f[3]*r[3] in
 * float, f / r the profile of base code x (0.25 four times for x = 4); (float)log((double)sum), -inf for sum == 0
 * (merge.c:492-497, misc.c:85-92).  dim = 5 nq. */
typedef struct td_merge_tables {
	int32_t nq, dim;
	uint8_t qchar[256];       /* [nq] the characters */
	int16_t qindex[256];      /* character -> q, -1 for one that does not occur */
	float*  profile;          /* [2 nq] */
	float*  T;                /* [dim * dim] */
} td_merge_tables;
int  td_merge_tables_build(const uint8_t* qual, int64_t n, td_merge_tables** out);
void td_merge_tables_free(td_merge_tables* t);

/* ---- one batch ---- */
#define TD_MERGE_WRITTEN       0   /* a record (out_len > 0) */
#define TD_MERGE_BELOW         1   /* id / aligned < threshold: out_len = 0 */
#define TD_MERGE_NO_CANDIDATE  2   /* no candidate (see above): out_len = 0, best_d = -1, id = aligned = 0 */
typedef struct td_merge_record {
	int32_t best_d;           /* the winning candidate: d < len_f: read 1 from d against read 2 from 0; else read 2 from d - len_f */
	int32_t out_len;          /* characters of the merged read; 0 = nothing is written */
	int32_t id, aligned;      /* equal positions / positions of the aligned part */
	int32_t status;           /* TD_MERGE_* */
} td_merge_record;
typedef struct td_merge_result {
	int64_t n_pairs;
	td_merge_record* rec;     /* [n_pairs] */
	int64_t* out_off;         /* [n_pairs + 1]: pair p's text is seq / qual [out_off[p], out_off[p] + rec[p].out_len) */
	char*    seq;             /* merged sequences, letters */
	char*    qual;            /* merged qualities */
	int64_t  n_written, n_below, n_too_short;
	int32_t  table_in_lds;    /* td_merge_device: 1 = the kernel kept T in LDS */
	int32_t  n_on_host;       /* td_merge_device: pairs with a read longer than the kernel's staging room (512 bases), done by the host path */
	float    kernel_ms;       /* td_merge_device: the kernel, from HIP events */
} td_merge_result;
/* r1 / r2: the two files' batches as td_reads_parse gives them (base codes, offsets, quality bytes in place in `text`); read 2 as
 * it stands in its file -- the reverse complement and the reversal are part of the call.
 * td_merge_host: a restatement of overlap_reads() over the tables, opts->n_threads threads over the pairs, results in input order.
 * td_merge_device: the same from the kernel on opts->device (csrc/td_merge.hip). */
int  td_merge_host(const td_reads* r1, const td_reads* r2, const td_merge_opts* opts, td_merge_result** out);
int  td_merge_device(const td_reads* r1, const td_reads* r2, const td_merge_opts* opts, td_merge_result** out);
void td_merge_result_free(td_merge_result* res);

/* ---- two files of any size ----
 * in1 / in2: plain, .gz or .bz2 FASTQ, read in lock-step batches of opts->batch_pairs pairs by the streaming pipeline's readers
 * (tagdust_io.h); the record counts must be equal and the first 1000 names must name the same reads (merge.c:164-193).  The
 * device (or, with opts->device == -1, td_merge_host) runs on the calling thread, formatting and the append on a writer thread.
 * out_path: the records "@<name of read 1>\n<seq>\n+\n<qual>\n" in input order, whatever batch_pairs is; "-" = stdout. */
typedef struct td_merge_stats {
	int64_t n_pairs, n_written, n_below, n_too_short, n_batches, bytes_in, bytes_out;
	double  wall_s, read_s, parse_s, tables_s, merge_s, kernel_s, write_s;
} td_merge_stats;
int td_merge_stream(const char* in1, const char* in2, const char* out_path, const td_merge_opts* opts, td_merge_stats* stats);

/* ---- the command line of `tagdust-merge` ----
 * The reference's -t, -minlen, -Q / -q / -threshold (one or two leading dashes) and two input files; this library's --out,
 * --device, --host, --batch-pairs, -h / -help.  Anything else fails with a message that names it.  argv[0] is the program name. */
typedef struct td_merge_args {
	td_merge_opts opts;
	const char* in1;          /* point into argv */
	const char* in2;
	const char* out_path;     /* "-" unless --out */
	int32_t help;
} td_merge_args;
int td_merge_parse_args(int argc, const char* const* argv, td_merge_args* out, char* err, size_t errcap);
const char* td_merge_usage(void);

#ifdef __cplusplus
}
#endif
#endif
