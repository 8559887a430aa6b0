/*
 * tagdust_census.h -- what stood where the barcode should have been: a census of the barcode spellings of a run's reads, counted
 * on the device behind every TD_MODE_GET_LABEL batch of a context (part of libtagdust_hip.so, plain C).  The reference has no
 * counterpart; bcl2fastq and its successors print "top unknown barcodes" for the same reason.
 *
 * The observed word of a read for segment j is the bases seq[p], in read order, at every position p in 0..len-1 with
 * (model.label[labels[p + 1]] & 0xFFFF) == j -- the mapping extract_reads uses (src/barcode_hmm.c:3205-3208).  A read is eligible
 * when bit (read_type & 0xFF) of outcome_mask is set, read_type being the final outcome (after the -ref filter and DUST).  An
 * eligible read is tallied instead of counted when its word is empty (skipped_empty), else longer than 28 bases (skipped_long),
 * else holds a base that is not A, C, G or T (skipped_n) -- in this order, so every eligible read is in exactly one class.
 * Otherwise its key is (uint64) length << 56 | bases, two bits per base (A, C, G, T = 0..3), the first base the most significant.
 * A key is never 0.
 *
 * The device table holds 2^log2_slots keys; a key that finds no slot within its probe window adds its reads to `overflow`, on
 * every attempt alike (nothing is ever removed), so a reported count is always exact.  Always
 *     eligible == counted + skipped_empty + skipped_long + skipped_n + overflow      and      counted == the sum of all counts.
 */
#ifndef TAGDUST_CENSUS_H
#define TAGDUST_CENSUS_H

#include <stdint.h>
#include "tagdust_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_CENSUS_MAX_WORD 28
#define TD_CENSUS_DEFAULT_MASK ((1u << TD_EXTRACT_FAIL_ARCHITECTURE_MISMATCH) | (1u << TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND))

typedef struct td_census_entry  { uint64_t key; int64_t count; } td_census_entry;
typedef struct td_census_totals { int64_t eligible, counted, skipped_empty, skipped_long, skipped_n, overflow, distinct; } td_census_totals;

/* Switches the census of this context on (off by default): segment = a 'B' segment of the uploaded model, -1 = the last one (the
 * one whose barcode extract_reads reports); outcome_mask = any non-empty subset of bits 0..7; log2_slots in 4..26.  TD_FAIL with a
 * message when no model is uploaded, the model has no 'B' segment, the segment is not one, a -start/-end window is set, or
 * td_submit tickets are outstanding.  While it is on every TD_MODE_GET_LABEL batch (td_run and td_submit alike) adds to it, no other
 * mode and not td_arch_scores; td_set_window fails; a later td_model_upload switches it off. */
int td_census_enable (td_ctx* ctx, int32_t segment, uint32_t outcome_mask, int32_t log2_slots);
int td_census_disable(td_ctx* ctx);                 /* frees the table */
int td_census_reset  (td_ctx* ctx);                 /* zero table and tallies; td_counts_reset does not touch it */
/* Waits for the context's queued work.  *n = the number of distinct keys; at most cap entries are copied, sorted by count
 * descending, then key ascending.  entries may be NULL when cap is 0; totals may be NULL. */
int td_census_get    (td_ctx* ctx, td_census_entry* entries, int64_t cap, int64_t* n, td_census_totals* totals);
/* the same result from host arrays, no GPU: for hosts without one and as the yardstick of the device path.  codes are base codes
 * 0..4, offs as for td_batch_upload, res and labels as td_batch_download leaves them (the labels of read i at offs[i] + i,
 * len + 1 bytes).  Never overflows.  *entries is freed with td_census_free; the message of a failure is td_last_error(NULL)'s. */
int td_census_host   (const td_model_desc* model, int32_t segment, uint32_t outcome_mask, const uint8_t* codes, const int64_t* offs,
                      int64_t n_reads, const td_read_result* res, const int8_t* labels,
                      td_census_entry** entries, int64_t* n, td_census_totals* totals);
/* the sum of two results (either may be empty), in the order of td_census_get */
int td_census_merge  (const td_census_entry* a, int64_t na, const td_census_entry* b, int64_t nb, td_census_entry** out, int64_t* n);
int td_census_key_text(uint64_t key, char buf[32]);   /* "ACGTTG"; TD_FAIL for a value that is no key */
void td_census_free(td_census_entry* entries);

#ifdef __cplusplus
}
#endif
#endif
