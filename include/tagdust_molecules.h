/*
 * tagdust_molecules.h -- how many molecules did each barcode yield: the extracted reads of a run counted per (barcode, fingerprint,
 * start of the read), on the device behind every TD_MODE_GET_LABEL batch of a context (part of libtagdust_hip.so, plain C).  The
 * reference extracts the fingerprint (UMI) and prints it; it counts nothing with it.
 *
 * A read is eligible when its final outcome (read_type & 0xFF, after the -ref filter and DUST) is TD_EXTRACT_SUCCESS.  Its read
 * bases are the bases seq[p], in read order, at the positions p in 0..len-1 whose label belongs to an 'R' segment:
 * model.seg_type[model.label[labels[p + 1]] & 0xFFFF] == 'R', the mapping extract_reads uses (src/barcode_hmm.c:3205-3208).  Its
 * prefix is the first n = min(number of read bases, P) of them, P = prefix_bases; w holds the prefix, two bits per base (A, C, G,
 * T = 0..3), the first base the most significant of the 2n bits.  An eligible read is in exactly one of three classes, checked
 * in this order: skipped_empty when n == 0; skipped_n when a prefix base is not A, C, G or T; otherwise it is counted under
 *
 *     mix(k): k ^= k >> 30; k *= 0xBF58476D1CE4E5B9; k ^= k >> 27; k *= 0x94D049BB133111EB; k ^= k >> 31        (uint64_t)
 *     a   = mix(((uint64_t)(uint32_t)fingerprint << 8) | n)
 *     low = mix(w ^ a) & 0x00FFFFFFFFFFFFFF;   if (low == 0) low = 1
 *     bin = barcode == -1 ? 0 : barcode & 0xFF          (the writer's file index, the bin of td_counts_get)
 *     key = (uint64_t)bin << 56 | low                    (never 0)
 *
 * with the record's own fingerprint and barcode (td_read_result; the fingerprint is -1 without an 'F' segment).  So two reads are
 * the same molecule when they have the same barcode, the same fingerprint and the same first P read bases.  The match is exact: a
 * sequencing error in the prefix or in the UMI makes a new molecule (the count itself collapses no neighbouring UMIs; the collapse
 * below does, on top of it).  Two limits:
 *   - within one barcode two molecules whose 56-bit `low` collide are counted as one.  Among m molecules of a barcode about
 *     m^2 / 2 * 2^-56 pairs do: 0.0007 for m = 10^7 -- one run in 1400 counts one molecule too few;
 *   - the reference's fingerprint is an int of (bases << 8 | length): a UMI of more than 12 bases has lost its leading bases in
 *     it, and such UMIs that differ only there are one fingerprint.
 *
 * The table is the census's (tagdust_census.h): 2^log2_slots slots of 16 bytes (a key and a count); a key that finds no slot
 * within its probe window adds its reads to `overflow`, on every attempt alike, so a reported count is always exact.  Always
 *     eligible == counted + skipped_empty + skipped_n + overflow      and      counted == the sum of all counts.
 * The default of 2^26 slots (1 GiB) holds the 2^24 molecules of a large run at a quarter full, where no probe comes near the window.
 *
 * Dedup (td_mol_dedup_enable) -- one read per molecule -- extends the count and uses its eligibility, prefix and key unchanged.
 * The reference has nothing of the kind; this is the definition, held by the device path and by td_mol_dedup_host alike:
 *   - every read of a context has an ordinal: the number of reads submitted to the context in TD_MODE_GET_LABEL since dedup was
 *     enabled or last reset (td_mol_reset), plus the read's index in its batch in the caller's order (not the device's
 *     length-sorted order);
 *   - a counted read is a duplicate when the table holds its key with a smaller first ordinal than its own, the first ordinal of a
 *     key being the minimum over all counted reads seen so far with that key;
 *   - eligible reads that are not counted (skipped_empty, skipped_n, overflow) cannot be judged: they are kept, and tallied as
 *     `unjudged`;
 *   - a duplicate's outcome becomes TD_EXTRACT_DUPLICATE (tagdust_hip.h; not an outcome of the reference); its barcode,
 *     fingerprint, scores, labels and seq_out stay as decoded, and the writers write it to no file.  td_counts_get, the census and
 *     the count itself see the outcome as decoded.
 * Always
 *     eligible == kept + duplicates      and      kept == molecules + skipped_empty + skipped_n + overflow,
 * molecules being the keys that entered the table since the reset.  The result is a function of the context's sequence of reads
 * alone: not of how it was cut into batches, of td_run or td_submit, of the tickets in flight or of the kernel variant.  Limits:
 * the 56-bit collision above (two molecules that collide lose one read); and which keys overflow in a nearly full table depends on
 * the claim order within a batch, as it does for the count.  Dedup matches exactly, with or without the collapse below (the frozen
 * state further down, DESIGN.md section 17, is the second pass that does not); a molecule split over two contexts survives in both
 * (each has its own table).
 *
 * Collapse (td_mol_collapse_enable) -- UMIs one mismatch apart counted as one molecule -- reads the count's table and changes
 * nothing in it.  The reference has nothing of the kind; this is the definition, held bit for bit by the device path and by
 * td_mol_collapse_host:
 *   - origin.  A key is a hash, so beside every key the table keeps what it was made of: the counted read's prefix word w, its
 *     record's fingerprint and its prefix length n (td_mol_origin), the arguments of td_mol_key beside the barcode bin, which is
 *     the key's top byte.  All reads of a key have the same origin, but for the 56-bit collision above: then it is that of any
 *     one of the colliding molecules;
 *   - neighbours.  L = fingerprint & 0xFF, m = min(L, 12), the bases an int fingerprint still holds.  The neighbours of molecule
 *     u are the 3 * m keys
 *         td_mol_key(bin(u), fingerprint ^ (d << (8 + 2 * i)), w, n)      i in 0..m-1, d in 1..3     (xor on the uint32 pattern)
 *     that the table holds: the same barcode bin, the same prefix, a UMI at Hamming distance exactly one.  A key that overflowed
 *     is in nobody's neighbourhood; a molecule with fingerprint -1 (no 'F' segment) has no neighbours;
 *   - parent (the directional rule of UMI-tools, made deterministic).  v qualifies as a parent of u when
 *     count(v) >= 2 * count(u) - 1 and (count(v), key(v)) comes strictly before (count(u), key(u)) in the order of td_census_get
 *     (count descending, then key ascending).  The parent of u is the qualifying neighbour that comes first in that order;
 *     without one u is a root.  Two neighbours qualify for each other only when both have count 1, and then the key decides: the
 *     relation is a forest, and every step up is strictly earlier in a total order, so the walk to a root ends;
 *   - collapse.  Every molecule is counted under its root: collapsed(root) = the sum of the counts of the root's tree.  Always
 *         molecules_after + absorbed == molecules_before      and      the sum of collapsed == counted,
 *     and the reads of a barcode bin are unchanged (a parent is in its child's bin).  longest_chain is the largest number of
 *     steps from a molecule to its root.
 * The result is a function of the set of (key, count, origin) alone: not of slot positions, batching, tickets in flight or kernel
 * variant.  Limits: distance one only; the UMI only (an error in the prefix still makes a new molecule); the leading bases of a
 * UMI of more than 12 are not in the fingerprint and take no part; the tree can differ from UMI-tools' breadth-first clusters, in
 * which the largest root claims a shared descendant -- here the child chooses; dedup is not changed by it (unless the context is
 * frozen: below, and DESIGN.md section 17).
 *
 * Survey, freeze, replay (td_mol_dedup_freeze) -- one read per COLLAPSED molecule.  Which read of a tree survives is only known once
 * the counts are final, so it takes a second pass over the same reads.  The reference has nothing of the kind; this is the
 * definition, held by the device path and by td_mol_dedup_collapsed_host alike.  A context with count, dedup and collapse on is in
 * one of two states:
 *   - survey: everything above, unchanged -- the count, the origins, the first ordinals, the exact marks;
 *   - frozen, entered by td_mol_dedup_freeze: it waits for the context's queued work, runs the collapse as td_mol_collapse_get does,
 *     computes for every molecule u   keeper(u) = first(root(u)),   the first ordinal of the ROOT'S OWN KEY -- not the minimum over
 *     the tree --, zeroes dedup's three tallies and sets the ordinal counter to 0.
 * While frozen a TD_MODE_GET_LABEL batch changes nothing in the table: keys, counts, origins, first ordinals and the count's totals
 * (eligible .. molecules) stay as the survey left them, and td_mol_get, td_mol_entries, td_mol_origins, td_mol_collapse_get and
 * td_mol_collapse_entries return the survey's results as often as they are asked.  A read's ordinal is the number of reads
 * submitted since the freeze plus its index in its batch in the caller's order, the rule of the survey.  The batch is replayed:
 *   - an eligible read whose key the table holds is a duplicate (TD_EXTRACT_DUPLICATE, every other field as decoded) when
 *     keeper(its key) != its ordinal, and kept otherwise;
 *   - an eligible read with no key in the table -- skipped_empty, skipped_n, a key that overflowed in the survey, a key never
 *     surveyed -- is kept and tallied `unjudged`;
 *   - td_mol_dedup_get returns the replay's tallies.
 * td_mol_dedup_freeze called again recomputes the keepers and restarts the ordinals.  td_mol_reset ends the frozen state with an
 * empty table; so do td_mol_disable, td_mol_dedup_disable, td_mol_collapse_disable and a new model.  When the same reads are
 * replayed in the same order:
 *   - the one written read of a tree is the first read of the input that carries the root's barcode, fingerprint and prefix, so
 *     every written judged read spells an entry of td_mol_collapse_entries and its ";FP:" is the UMI the table reports;
 *   - eligible(survey) == kept + duplicates      and      kept == molecules_after + skipped_empty + skipped_n + overflow.
 * The result is a function of the surveyed sequence of reads and the replayed sequence of reads alone: not of either pass's
 * batching, of td_run or td_submit, of the tickets in flight, of length classes or of the kernel variant.  Limits: those of dedup
 * and of the collapse; the input is decoded twice; replaying other reads, or the same in another order, is defined (the rule
 * above) but keeps no longer one read per molecule.
 *
 * Mate mode (td_mol_mate_enable) -- the first bases of a read's MATE, a read of a second file, as part of the key.  UMI protocols put
 * barcode and UMI into read 1 and the cDNA into read 2 (Drop-seq, CEL-seq, inDrop, the CASAVA three-read layout): the file that is
 * decoded has few or no read bases of its own, and without the mate every read is skipped_empty or all molecules of a barcode and UMI
 * share one key.  The reference has nothing of the kind; this is the definition, held by the device path and by the *_mated host
 * functions alike.  A context with the count on may be put into mate mode with M = mate_bases, M >= 1 and P + M <= 32.  While it is
 * on, every TD_MODE_GET_LABEL batch of n reads comes with a mate batch: codes (bytes 0..3 = A, C, G, T; any other value is N) and
 * offs[n + 1]; mate i belongs to read i of the batch in the caller's order.  For an eligible read (eligibility is unchanged):
 *   - the own prefix is as above: n1 = min(read bases, P), word w1;
 *   - the mate prefix is n2 = min(len(mate i), M), word w2, two bits per base, the first base the most significant;
 *   - n = n1 + n2 and w = (w1 << 2 * n2) | w2;
 *   - the read is skipped_empty when n == 0, skipped_n when any of those n bases is not A, C, G or T, and otherwise counted under
 *     td_mol_key(barcode, fingerprint, w, n) with origin {w, fingerprint, n}.
 * Dedup (ordinals, first, mark), the collapse (a neighbour keeps w and n), freeze and replay, the identities and td_mol_summarise
 * follow from that key unchanged.  With mate mode off every result is bit for bit what it is without this paragraph.  Limits:
 *   - the split between n1 and n2 is not in the key: two reads whose own read segments are shorter than P by different amounts can
 *     share a word (own ACG + mate T.. and own AC + mate GT..);
 *   - the mate's own outcome takes no part: the mate is not decoded, filtered or DUSTed here, only its first M bases are read.  A
 *     run that joins files (tagdust_run.h, --mate-bases) therefore refuses a -ref filter and DUST -- unless the mate filter is on.
 *
 * Mate filter (td_mol_mate_filter_enable) -- the mate's outcome joined to its read's, the reference's combination of a record over its
 * files (HMMER3_MAX, src/barcode_hmm.c:344-350) moved in front of the count.  It applies to a context in mate mode.  While it is on,
 * the mate batch of every TD_MODE_GET_LABEL batch is judged, and the verdict is joined to its read before anything reads the outcomes:
 *   - mate type.  t2[i] is what TD_MODE_RNA_DUST leaves in read_type for mate i when the mates are taken as a batch of their own,
 *     given as codes, under this context's settings as they stand when the batch is staged (td_batch_upload, td_submit): `dust` of
 *     td_set_params; the artifacts, filter_error and n_threads of td_set_artifacts; the thread ranges of td_set_batch_window.  That is
 *     do_rna_dust (src/barcode_hmm.c:2370-2395): 0, then match_to_reference sets (1-based sequence << 8) | 5, then DUST sets 6
 *     whatever the type was.  Mate i is a left-over read of its thread range exactly when read i is: run_rna_dust (:2059-2068) and
 *     run_pHMM (:1911-1922) split the same n the same way;
 *   - join.  read_type[i] = max(read_type[i] as decoded, t2[i]), both signed ints, whole words.  read_type[i] as decoded includes
 *     the read's own -ref and DUST.  Barcode, fingerprint, scores, labels and seq_out stay as decoded;
 *   - the joined outcome is what everything sees that reads a batch's outcomes behind its decode: td_read_result, the -ref hit count
 *     (td_artifact_hits_get; the reference counts hits from the combined type, :378-382), the census, the count's eligibility,
 *     dedup's first ordinals and marks, the replay of a frozen context, the writers;
 *   - td_counts_get does not: it is the decode kernel's own tally and stays as decoded.
 * The host definition needs no function of its own: the four *_mated host functions, run over the same records with read_type
 * replaced by the joined value, are the yardstick of the device path.  With dust == 0 and no artifacts every t2 is 0, and every
 * result is bit for bit what it is with the filter off.  Limits: one mate -- a third file's outcome is not joined; one device.
 */
#ifndef TAGDUST_MOLECULES_H
#define TAGDUST_MOLECULES_H

#include <stdint.h>
#include "tagdust_hip.h"
#include "tagdust_census.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TD_MOL_MAX_PREFIX          32
#define TD_MOL_DEFAULT_PREFIX      20
#define TD_MOL_DEFAULT_LOG2_SLOTS  26
#define TD_MOL_LEVELS              10

typedef struct td_mol_totals { int64_t eligible, counted, skipped_empty, skipped_n, overflow, molecules; } td_mol_totals;
/* one barcode bin: reads counted, distinct molecules, and levels[min(count, 10) - 1] = molecules seen `count` times (the last
 * level: 10 times or more) */
typedef struct td_mol_row { int64_t reads, molecules, levels[TD_MOL_LEVELS]; } td_mol_row;

/* Switches the molecule count of this context on (off by default): prefix_bases in 1..32, log2_slots in 4..30 (0 = the default).
 * TD_FAIL with a message when no model is uploaded, a -start/-end window is set, or td_submit tickets are outstanding.  While it
 * is on every TD_MODE_GET_LABEL batch (td_run and td_submit alike) adds to it, no other mode and not td_arch_scores;
 * td_set_window fails; a later td_model_upload switches it off.  It may be on together with the census, each with its own table. */
int td_mol_enable (td_ctx* ctx, int32_t prefix_bases, int32_t log2_slots);
int td_mol_disable(td_ctx* ctx);                    /* frees the table */
int td_mol_reset  (td_ctx* ctx);                    /* zero table and tallies (dedup's first ordinals, ordinal counter and tallies
                                                       with them); td_counts_reset does not touch it */
/* Waits for the context's queued work.  The raw (key, count) pairs, compacted on the device: *n = the number of molecules; at
 * most cap entries are copied, sorted as td_census_get sorts (count descending, then key ascending).  This is what is merged
 * across devices: td_census_merge adds two such results.  entries may be NULL when cap is 0; totals may be NULL. */
int td_mol_entries(td_ctx* ctx, td_census_entry* entries, int64_t cap, int64_t* n, td_mol_totals* totals);
/* the summary per barcode bin, computed on the device by a sweep over the table; totals may be NULL */
int td_mol_get    (td_ctx* ctx, td_mol_row rows[TD_NUM_BARCODE_BINS], td_mol_totals* totals);
/* the same rows from entries, on the host: after merging several devices, and the yardstick of td_mol_get */
int td_mol_summarise(const td_census_entry* entries, int64_t n, td_mol_row rows[TD_NUM_BARCODE_BINS]);
/* the same entries from host arrays, no GPU: for hosts without one and as the yardstick of the device path.  Arguments as
 * td_census_host takes them.  Never overflows.  *entries is freed with td_census_free; the message of a failure is
 * td_last_error(NULL)'s. */
int td_mol_host   (const td_model_desc* model, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                   const td_read_result* res, const int8_t* labels, td_census_entry** entries, int64_t* n, td_mol_totals* totals);
/* Mate mode, see above.  One mate batch: codes and offs[n_reads + 1] as a batch's own input, and M. */
typedef struct td_mol_mate { const uint8_t* codes; const int64_t* offs; int32_t bases; } td_mol_mate;
/* td_mol_mate_enable: TD_FAIL with a message unless the count is on, no td_submit tickets are outstanding and 1 <= mate_bases <=
 * 32 - prefix_bases; it starts from an empty table (it does what td_mol_reset does), so a table never mixes keys of two kinds.
 * td_mol_mate_disable empties the table as well; td_mol_disable, and with it a new model, switches mate mode off. */
int td_mol_mate_enable (td_ctx* ctx, int32_t mate_bases);
int td_mol_mate_disable(td_ctx* ctx);
/* Names the mate batch of the next batch that is staged for TD_MODE_GET_LABEL: td_submit takes it when its mode is
 * TD_MODE_GET_LABEL (no other mode needs or consumes one); td_batch_upload, which does not know the mode yet, takes it when its
 * n_reads is the batch's, and it then serves every td_run of that resident batch.  The staging copies the mate with the batch's own
 * input on the same upload stream -- page-locked memory straight, anything else through pinned staging --, so codes and offs must
 * stay valid and unchanged as long as the batch's own input must.  A TD_MODE_GET_LABEL td_run or td_submit in mate mode without a
 * mate for its batch, or with one of another n_reads, is TD_FAIL with a message: nothing is counted, the named mate is dropped and
 * the context stays usable.  A call names one batch: a second call before the staging replaces the first.
 * td_get_option: "mate_bases" (0 = off) and "mate_kernel_us", the mate kernel's time of the last staged mate batch. */
int td_mol_mate_next   (td_ctx* ctx, const uint8_t* codes, const int64_t* offs, int64_t n_reads);
/* The mate filter, see above.  Both are TD_FAIL with a message unless mate mode is on and no td_submit tickets are outstanding; both
 * start from an empty table (they do what td_mol_reset does), so a table never holds counts made under two eligibility rules.  A
 * batch is judged as it is staged: one that is resident across the switch has to be uploaded again (td_run says so).
 * td_mol_mate_disable, td_mol_disable and a new model switch the filter off as well.
 * td_get_option: "mate_filter" (0 / 1); "mate_filter_kernel_us" and "mate_join_kernel_us", the filter kernel's time of the last staged
 * mate batch and the join kernel's of the last decoded batch (TD_FAIL while the filter is off or before the first such launch; with
 * dust == 0 and no artifacts neither kernel is launched). */
int td_mol_mate_filter_enable (td_ctx* ctx);
int td_mol_mate_filter_disable(td_ctx* ctx);
/* t2 of the batch resident in the context (td_batch_upload / td_run path), in the caller's order: *n = its number of reads, at most
 * cap types are copied.  Waits for the context's queued work.  TD_FAIL with a message while the filter is off or when the resident
 * batch was staged without its mates. */
int td_mol_mate_types  (td_ctx* ctx, int32_t* types, int64_t cap, int64_t* n);
/* The four host definitions over reads with the mate joined into the key: the arguments of td_mol_host, td_mol_host_origins,
 * td_mol_dedup_host and td_mol_dedup_collapsed_host plus the mate batch behind labels.  mate == NULL is the unmated function (those
 * four are this call).  TD_FAIL with a message when mate->bases < 1 or prefix_bases + mate->bases > 32. */
int td_mol_host_mated   (const td_model_desc* model, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                         const td_read_result* res, const int8_t* labels, const td_mol_mate* mate, td_census_entry** entries, int64_t* n,
                         td_mol_totals* totals);
/* Dedup, see above.  td_mol_dedup_enable: TD_FAIL with a message unless the count is on (td_mol_enable first) and no td_submit
 * tickets are outstanding; it allocates 8 more bytes per slot and starts from an empty table (it does what td_mol_reset does).
 * td_mol_disable, and with it a new model, switches it off as well. */
typedef struct td_mol_dedup_totals { int64_t kept, duplicates, unjudged; } td_mol_dedup_totals;
int td_mol_dedup_enable (td_ctx* ctx);
int td_mol_dedup_disable(td_ctx* ctx);              /* frees the first ordinals; table and count stay as they are */
int td_mol_dedup_get    (td_ctx* ctx, td_mol_dedup_totals* totals);   /* waits for the context's queued work */
/* the same decision from host arrays, no GPU, the reads in the given order (read i has ordinal i): is_duplicate[i] = 1 for a
 * duplicate, else 0.  For hosts without a GPU and as the yardstick of the device path.  Arguments as td_mol_host takes them.
 * Never overflows.  totals may be NULL. */
int td_mol_dedup_host   (const td_model_desc* model, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                         const td_read_result* res, const int8_t* labels, uint8_t* is_duplicate, td_mol_dedup_totals* totals);
int td_mol_dedup_host_mated(const td_model_desc* model, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                            const td_read_result* res, const int8_t* labels, const td_mol_mate* mate, uint8_t* is_duplicate,
                            td_mol_dedup_totals* totals);
/* Collapse, see above.  td_mol_collapse_enable: TD_FAIL with a message unless the count is on, the model has an 'F' segment and no
 * td_submit tickets are outstanding; it allocates 16 more bytes per slot (the origins) and starts from an empty table, so every key
 * in the table has its origin.  td_mol_disable, and with it a new model, switches it off as well; td_mol_reset clears the origins. */
typedef struct td_mol_origin { uint64_t w; int32_t fingerprint; int32_t n; } td_mol_origin;   /* 16 bytes */
typedef struct td_mol_collapse_totals { int64_t molecules_before, molecules_after, absorbed, longest_chain; } td_mol_collapse_totals;
int td_mol_collapse_enable (td_ctx* ctx);
int td_mol_collapse_disable(td_ctx* ctx);           /* frees the origins and what the collapse itself allocated; table and count stay */
/* td_mol_entries with the origin of every entry in a parallel array, in the same order (collapse on) */
int td_mol_origins         (td_ctx* ctx, td_census_entry* entries, td_mol_origin* origins, int64_t cap, int64_t* n, td_mol_totals* totals);
/* Both wait for the context's queued work and run the collapse on the device; keys, counts and origins stay untouched, so both may
 * be called in the middle of a run and again later.  td_mol_collapse_get: the rows of td_mol_get made from the collapsed counts
 * (molecules = roots, levels from collapsed).  td_mol_collapse_entries: the roots with collapsed as their count, in the order of
 * td_census_get, with their origins; *n = the number of roots, at most cap are copied.  totals may be NULL. */
int td_mol_collapse_get    (td_ctx* ctx, td_mol_row rows[TD_NUM_BARCODE_BINS], td_mol_collapse_totals* totals);
int td_mol_collapse_entries(td_ctx* ctx, td_census_entry* entries, td_mol_origin* origins, int64_t cap, int64_t* n, td_mol_collapse_totals* totals);
/* td_mol_host plus the origin of every entry (*origins is freed with free) */
int td_mol_host_origins    (const td_model_desc* model, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                            const td_read_result* res, const int8_t* labels, td_census_entry** entries, td_mol_origin** origins, int64_t* n,
                            td_mol_totals* totals);
int td_mol_host_origins_mated(const td_model_desc* model, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                              const td_read_result* res, const int8_t* labels, const td_mol_mate* mate, td_census_entry** entries,
                              td_mol_origin** origins, int64_t* n, td_mol_totals* totals);
/* The collapse on the host, no GPU: what td_mol_collapse_entries returns, from entries and their origins.  A key may be given more
 * than once: its counts are added first, so the td_mol_origins results of several devices, concatenated, are a valid input -- the
 * multi-device path, and the yardstick of the device.  *out_entries is freed with td_census_free, *out_origins with free. */
int td_mol_collapse_host   (const td_census_entry* entries, const td_mol_origin* origins, int64_t n,
                            td_census_entry** out_entries, td_mol_origin** out_origins, int64_t* out_n, td_mol_collapse_totals* totals);
/* The frozen state, see above.  td_mol_dedup_freeze: TD_FAIL with a message when the count, dedup or the collapse is off or td_submit
 * tickets are outstanding.  The first call allocates 8 more bytes per slot (the keepers); whatever frees dedup's or the collapse's
 * arrays frees them.  totals (may be NULL): the collapse's, as td_mol_collapse_get gives them. */
int td_mol_dedup_freeze    (td_ctx* ctx, td_mol_collapse_totals* totals);
/* the same decision from host arrays, no GPU: the given sequence is surveyed and the same sequence replayed, read i has ordinal i;
 * is_duplicate[i] = 1 for a duplicate, else 0.  For hosts without a GPU and as the yardstick of the device path.  Arguments as
 * td_mol_dedup_host takes them.  Never overflows.  totals and collapse_totals may be NULL. */
int td_mol_dedup_collapsed_host(const td_model_desc* model, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs,
                                int64_t n_reads, const td_read_result* res, const int8_t* labels, uint8_t* is_duplicate,
                                td_mol_dedup_totals* totals, td_mol_collapse_totals* collapse_totals);
int td_mol_dedup_collapsed_host_mated(const td_model_desc* model, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs,
                                      int64_t n_reads, const td_read_result* res, const int8_t* labels, const td_mol_mate* mate,
                                      uint8_t* is_duplicate, td_mol_dedup_totals* totals, td_mol_collapse_totals* collapse_totals);
/* the key of a counted read: its record's barcode and fingerprint, its prefix word w of n bases (1..32) */
uint64_t td_mol_key(int32_t barcode, int32_t fingerprint, uint64_t w, int32_t n);
int32_t  td_mol_key_bin(uint64_t key);              /* the barcode bin a key belongs to */

#ifdef __cplusplus
}
#endif
#endif
