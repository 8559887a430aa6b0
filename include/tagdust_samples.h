/*
 * tagdust_samples.h -- combinatorial barcodes: a read's sample is named by ALL 'B' segments of its architecture, not by one of them
 * (part of libtagdust_hip.so, plain C).  The reference decodes every 'B' segment and then reports the last one's call
 * (extract_reads, src/barcode_hmm.c:3216-3225) in files named after the first one's (print_all, src/io.c:859-915); dual and
 * combinatorial indexing -- an 8 x 12 plate, inline barcode plus index, split-pool rounds -- puts the sample in the tuple.
 *
 * Chosen segments: all 'B' segments of the uploaded model in model order, j_1 < .. < j_m, 1 <= m <= TD_SAMPLES_MAX_SEGMENTS.
 *
 * Sheet: n_samples (1..TD_SAMPLES_MAX) rows of m HMM indices, tuples[s * m + t] = b_t with 0 <= b_t < n_hmm[j_t] - 1 (the last HMM
 * of a 'B' segment is its all-N decoy and cannot be listed); rows pairwise different.  Every sample has a name of 1..64 characters
 * of [A-Za-z0-9._-], pairwise different; a NULL name (or names == NULL) means "S<s+1>".
 *
 * The call of a read for chosen segment t is (model.label[labels[p + 1]] >> 16) & 0x7FFF of the LAST position p in 0..len-1 whose
 * label's segment (model.label[..] & 0xFFFF) is j_t, -1 when no position has one: the reference's own rule for `bar`, per segment.
 *
 * A read is eligible when its final read_type equals TD_EXTRACT_SUCCESS (final: what the decode left, after the mate join where
 * that is on).  Every eligible read is in exactly one class:
 *     incomplete   some call is -1 or the decoy       read_type = TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND, barcode unchanged
 *     assigned     the calls equal row s              read_type unchanged, barcode = (j_m << 16) | s
 *     unlisted     complete calls that equal no row   read_type = TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND, barcode unchanged
 * No other field of td_read_result changes, nor the labels or the rewritten sequence; reads that are not eligible are untouched.
 * The rewrite stands in front of the census and the molecule count of the same batch: both see one sample per read.
 *
 * The combination count: every eligible read is counted under
 *     key = (uint64) m << 56 | sum over t of (call_t + 1) << (8 * t)
 * -- a missing call contributes 0, the decoy n_hmm[j_t]; a key is never 0 -- in a device table of 2^log2_slots keys.  A key that
 * finds no slot within its probe window adds its reads to `overflow`, on every attempt alike, so a reported count is exact; the
 * rewrite never depends on the table.  Always
 *     eligible == assigned + unlisted + incomplete      and      the sum of all counts == eligible - overflow.
 */
#ifndef TAGDUST_SAMPLES_H
#define TAGDUST_SAMPLES_H

#include <stdint.h>
#include "tagdust_hip.h"
#include "tagdust_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_SAMPLES_MAX          255
#define TD_SAMPLES_MAX_SEGMENTS 4
#define TD_SAMPLES_MAX_NAME     64

typedef struct td_samples_totals { int64_t eligible, assigned, unlisted, incomplete, overflow; } td_samples_totals;

/* Switches sample assignment of this context on (off by default); log2_slots in 4..26.  TD_FAIL with a message when no model is
 * uploaded, the model has no 'B' segment or more than four, the sheet is bad (the message names the row), a -start/-end window is
 * set, or td_submit tickets are outstanding.  While it is on every TD_MODE_GET_LABEL batch (td_run and td_submit alike) is
 * rewritten and counted, no other mode; td_set_window fails; a batch staged under another state of the switch is refused by
 * td_run (upload it again); a later td_model_upload switches it off.  td_counts_get stays the decode kernel's own tally. */
int td_samples_enable (td_ctx* ctx, const int32_t* tuples, const char* const* names, int32_t n_samples, int32_t log2_slots);
int td_samples_disable(td_ctx* ctx);                /* frees table and sheet */
int td_samples_reset  (td_ctx* ctx);                /* zero table and tallies; the sheet stays */
/* Waits for the context's queued work.  *n = the number of distinct keys; at most cap entries are copied, in td_census_get's
 * order (count descending, then key ascending), so that td_census_merge adds the results of two devices.  entries may be NULL
 * when cap is 0; totals may be NULL. */
int td_samples_get    (td_ctx* ctx, td_census_entry* entries, int64_t cap, int64_t* n, td_samples_totals* totals);
/* the name of sample s ("S<s+1>" where none was given); NULL when sample assignment is off or s is out of range */
const char* td_samples_name(td_ctx* ctx, int32_t s);
/* calls[m] (-1 = missing; the decoy is n_hmm[j_t] - 1 like any call) -> key, 0 for calls that are no key; and back */
uint64_t td_samples_key(const int32_t* calls, int32_t m);
int td_samples_key_calls(uint64_t key, int32_t calls[TD_SAMPLES_MAX_SEGMENTS], int32_t* m);
/* The same definition from host arrays, no GPU: for hosts without one and as the yardstick of the device path.  offs as for
 * td_batch_upload, res and labels as td_batch_download leaves them (the labels of read i at offs[i] + i, len + 1 bytes); res is
 * rewritten in place.  Never overflows.  *entries is freed with td_census_free; the message of a failure is td_last_error(NULL)'s. */
int td_samples_host   (const td_model_desc* model, const int32_t* tuples, int32_t n_samples, const int64_t* offs, int64_t n_reads,
                       td_read_result* res, const int8_t* labels, td_census_entry** entries, int64_t* n, td_samples_totals* totals);

/*
 * The join across input files (dual-index runs: I1.fq and I2.fq carry one barcode each).  The files whose model has a 'B' segment
 * are the barcode files, in call order; their 'B' segments are the COLUMNS t = 0..m-1 of the sheet, files first, then model order
 * within a file, 2 <= m <= TD_SAMPLES_MAX_SEGMENTS.  The first barcode file is the PRIMARY: its contexts hold the sheet and assign.
 * Every other barcode file is an EXPORTER: its contexts hand over one word per read of a batch, in the caller's order,
 *     0xFFFFFFFF                                   the read's final read_type != TD_EXTRACT_SUCCESS ("partner failed")
 *     byte first_column + u = call_u + 1           else, for the exporter's own u-th 'B' segment (0: no position; the decoy n_hmm)
 * -- the call by the rule above; all other bytes 0.  Words of several exporters combine by bitwise OR (all ones absorbs).
 *
 * In a primary context a read whose own final read_type is TD_EXTRACT_SUCCESS and whose partner word is 0xFFFFFFFF is not
 * eligible: nothing of it changes, nothing is counted, it is tallied as partner_failed.  Otherwise it is eligible and its calls
 * word is its own (bytes first_column..first_column + m_own - 1) OR the partner word; classes, rewrite, key and count are those
 * above with m = the number of columns, the decoy of column t being column_hmms[t], and barcode = (j_last_own << 16) | s.  Always
 *     eligible == assigned + unlisted + incomplete     and     reads that are SUCCESS in the primary == eligible + partner_failed.
 * A partner word of 0 contributes nothing.  Limits: one device; at most four columns in all; no window, and in a whole run no
 * --unknown-barcodes, --molecules or quality filter with the join yet.
 */
typedef struct td_samples_join_totals { td_samples_totals t; int64_t partner_failed; } td_samples_join_totals;

/* Exporter side.  Needs an uploaded model with 1..4 - first_column 'B' segments, no window, no outstanding tickets; not together
 * with td_samples_enable or the join on one context.  While it is on, every TD_MODE_GET_LABEL batch leaves its words in the array
 * td_samples_export_next named for it (n_reads words, page-locked or pageable; valid after td_run / td_wait): name it in front of
 * td_batch_upload / td_submit.  A batch without a named array, or one named for another number of reads, is refused with a
 * message and the context stays usable. */
int td_samples_export_enable (td_ctx* ctx, int32_t first_column);
int td_samples_export_disable(td_ctx* ctx);
int td_samples_export_next   (td_ctx* ctx, uint32_t* words, int64_t n_reads);
/* Primary side.  As td_samples_enable, with a sheet of m_total columns: column_hmms[m_total] holds every column's n_hmm, the
 * context's own columns (first_column..) are held against its model.  td_samples_join_next names the partner words of the next
 * TD_MODE_GET_LABEL batch (read when the batch is staged); the rules are td_samples_export_next's.  td_samples_disable,
 * td_samples_reset and td_samples_name serve the join too; td_samples_get reports it without partner_failed. */
int td_samples_join_enable(td_ctx* ctx, const int32_t* tuples, const char* const* names, int32_t n_samples, int32_t log2_slots,
                           int32_t m_total, int32_t first_column, const int32_t* column_hmms);
int td_samples_join_next  (td_ctx* ctx, const uint32_t* words, int64_t n_reads);
int td_samples_join_get   (td_ctx* ctx, td_census_entry* entries, int64_t cap, int64_t* n, td_samples_join_totals* totals);
/* td_get_option: "samples_export" (1 while the context exports), "samples_join" (the joined sheet's n_samples, 0 = off),
 * "samples_export_kernel_us" and "samples_join_kernel_us", the kernels' times of the last batch; "batch_sorted", 1 when the device
 * order of the batch td_run decoded last differs from the caller's (reads of several lengths: both sides of the join then carry
 * their words between the two orders) -- its meaning holds for td_batch_upload / td_run; with td_submit tickets in flight it speaks
 * of whichever batch was submitted or waited for last. */
/* The same definitions from host arrays, no GPU (arguments as td_samples_host's). */
int td_samples_export_host(const td_model_desc* model, int32_t first_column, const int64_t* offs, int64_t n_reads,
                           const td_read_result* res, const int8_t* labels, uint32_t* words);
int td_samples_join_host  (const td_model_desc* model, const int32_t* tuples, int32_t n_samples, int32_t m_total, int32_t first_column,
                           const int32_t* column_hmms, const uint32_t* words, const int64_t* offs, int64_t n_reads, td_read_result* res,
                           const int8_t* labels, td_census_entry** entries, int64_t* n, td_samples_join_totals* totals);

#ifdef __cplusplus
}
#endif
#endif
