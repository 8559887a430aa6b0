/*
 * tagdust_quality.h -- drop reads with low-quality barcode or UMI bases, judged on the device (part of libtagdust_hip.so, plain C).
 * The barcode call and the fingerprint are matched exactly, so a sequencing error in either makes a new sample or a new molecule;
 * the base qualities are the sequencer's own evidence for such errors.  The reference has nothing of the kind: this text is the
 * definition, held by the device path (td_quality.hip) and by td_qual_host alike.
 *
 * Parameters: min_quality Q in 1..93; offset 33 or 64; max_low K >= 0; segments, a non-empty subset of TD_QUAL_SEG_B | TD_QUAL_SEG_F.
 * thr = offset + Q.
 *
 * Low:     base p of read i is low when (uint8_t) qual[offs[i] + p] < thr.
 * Judged:  base p is judged when seg_type[model.label[labels[p + 1]] & 0xFFFF] is 'B' or 'F' as chosen -- the mapping extract_reads
 *          uses (src/barcode_hmm.c:3172), the one the census and the molecule count cite.
 * Count:   n_low = the number of positions in 0..len-1 that are both judged and low.
 *
 * A read is eligible when its read_type equals TD_EXTRACT_SUCCESS: the whole word, as decoded, after its own -ref / DUST and after
 * the mate join where that is on.  An eligible read with n_low > K gets read_type = TD_EXTRACT_FAIL_LOW_BASE_QUALITY (8,
 * tagdust_hip.h); barcode, fingerprint, scores, labels and seq_out stay as decoded.  Reads that are not eligible are untouched.
 *
 * Everything that reads a batch's outcomes behind its decode sees the verdict: td_read_result; sample assignment (its eligibility
 * is SUCCESS, so a failed read is neither assigned nor counted there); the census (its mask has bits 0..7, so outcome 8 is never
 * eligible: a dropped read had a listed barcode and is no "unknown barcode"); the molecule count, dedup and the replay of a frozen
 * context; the writers (any non-zero outcome goes to the _un file).  td_counts_get stays the decode kernel's own tally.
 *
 * Tallies: eligible, passed, failed, and low_bases = the sum of n_low over the eligible reads.  Always eligible == passed + failed.
 *
 * The result is a function of the reads, their qualities and the parameters alone: not of the batching, of td_run versus td_submit,
 * of the tickets in flight, of length classes or of the kernel variant.
 *
 * Limits: the mate's qualities are not judged; one device; refused under a -start/-end window (labels behind a window do not mark
 * the bases); FASTA records have nothing to judge -- the library call cannot know, the streaming run refuses them.
 */
#ifndef TAGDUST_QUALITY_H
#define TAGDUST_QUALITY_H

#include <stdint.h>
#include "tagdust_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_QUAL_SEG_B 1
#define TD_QUAL_SEG_F 2

typedef struct td_qual_params { int32_t min_quality, offset, max_low, segments; } td_qual_params;
typedef struct td_qual_totals { int64_t eligible, passed, failed, low_bases; } td_qual_totals;

/* One bit per base: bit (g & 31) of words[g >> 5] = (qual[g] < thr) for g < n, every bit at or beyond n is zero.  words has
 * (n + 31) / 32 + 1 entries: the last one is always zero (the device reads the word behind a base's own).  thr in 0..256.  A flat
 * pass over the bytes, no per-read logic. */
int td_qual_pack(const uint8_t* qual, int64_t n, int32_t thr, uint32_t* words);

/* The definition from host arrays, no GPU: for hosts without one and as the yardstick of the device path.  offs as for
 * td_batch_upload, res and labels as td_batch_download leaves them (the labels of read i at offs[i] + i, len + 1 bytes), read i's
 * quality bytes at qual + offs[i]; res is rewritten in place.  TD_FAIL with td_last_error(NULL)'s message for a model without a
 * segment of a chosen type or parameters out of range. */
int td_qual_host(const td_model_desc* model, const td_qual_params* params, const int64_t* offs, int64_t n_reads, td_read_result* res,
                 const int8_t* labels, const uint8_t* qual, td_qual_totals* totals);

/* Switches the filter of this context on (off by default).  TD_FAIL with a message when no model is uploaded, the model has no
 * segment of a chosen type, the parameters are out of range, a -start/-end window is set, or td_submit tickets are outstanding.
 * While it is on every TD_MODE_GET_LABEL batch (td_run and td_submit alike) is judged, no other mode; td_set_window fails; a later
 * td_model_upload switches it off.  Option "quality_filter" of td_get_option is 1 while it is on, "quality_kernel_us" the judge
 * kernel's time of the last batch. */
int td_qual_enable (td_ctx* ctx, int32_t min_quality, int32_t offset, int32_t max_low, int32_t segments);
int td_qual_disable(td_ctx* ctx);
int td_qual_reset  (td_ctx* ctx);                         /* the tallies to zero */
int td_qual_get    (td_ctx* ctx, td_qual_totals* totals); /* waits for the context's queued work */
/* Names the quality bytes of the next batch staged for TD_MODE_GET_LABEL: read i's bytes are at qual + offs[i], with the batch's
 * own offs.  td_submit takes them when its mode is TD_MODE_GET_LABEL, td_batch_upload when n_reads is the batch's.  The bytes are
 * packed during staging: qual may be reused as soon as the staging call returns.  While the filter is on, a TD_MODE_GET_LABEL batch
 * without named qualities, qualities named for another n_reads, and a resident batch staged under another state of the switch or
 * other parameters are TD_FAIL with a message that says what to do: nothing is decoded and the context stays usable. */
int td_qual_next   (td_ctx* ctx, const uint8_t* qual, int64_t n_reads);

#ifdef __cplusplus
}
#endif
#endif
