// td_samples.h -- sample assignment by all 'B' segments (include/tagdust_samples.h) inside a context: its state, and what td_api.hip
// and td_batch.hip call.  The kernel and every td_samples_* entry point that takes a context are in td_samples.hip; the definition
// both sides compile is td_samples_def.h.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "td_keytable.h"
#include "td_samples_def.h"

struct TdSlot;

// tallies of the device table, 64 bits each, in the order of td_samples_totals; behind them the distinct keys and the compaction's cursor
// (the join's partner_failed behind them: td_samples_get's order stays)
enum { SMP_ELIGIBLE = 0, SMP_ASSIGNED, SMP_UNLISTED, SMP_INCOMPLETE, SMP_OVERFLOW, SMP_DISTINCT, SMP_CURSOR, SMP_PARTNER_FAILED_TALLY, SMP_TALLY_WORDS };

// The words of the next batch, named by td_samples_export_next (out) or td_samples_join_next (in): taken when the batch is staged
struct TdSamplesNamed {
	bool named = false;
	uint32_t* out = nullptr; const uint32_t* in = nullptr;
	int64_t reads = 0;
};

struct TdSamplesState {
	bool on = false;
	bool join = false;                // switched on by td_samples_join_enable: every batch comes with its partner words
	int32_t gen = 0;                  // counts the enables: a batch remembers the one it was staged under (TdStaged::samples_gen)
	TdSamplePlan plan{};
	TdSamplePlan* d_plan = nullptr;   // ... and its copy on the device
	std::vector<std::string> names;
	TdCountTable table;               // td_keytable.h, SMP_TALLY_WORDS tallies
	TdSamplesNamed next;              // (join)
};

// the exporter side of the join: no sheet, no table -- a plan for its tc, two events around the kernel
struct TdSamplesExportState {
	bool on = false;
	int32_t gen = 0;                  // counts the enables, as TdSamplesState::gen (TdStaged::export_gen)
	int32_t H = 0;
	TdSamplePlan* d_plan = nullptr;
	KtEventPair ev;
	TdSamplesNamed next;
};

struct TdSamplesArgs {
	TdTileView tile;                         // td_keytable.h
	const int32_t* __restrict__ lens;        // [n_tiles*64]
	int32_t* __restrict__ out_type;          // [n_tiles*64]  final outcomes of the decode launch, rewritten
	int32_t* __restrict__ out_barcode;       // [n_tiles*64]  ... and its barcodes
	const TdSamplePlan* __restrict__ plan;
	int64_t n_reads;
	int32_t n_tiles, H;
	TdKeyTable table;
	unsigned long long* __restrict__ tallies;
	// the join: the batch's partner words in the CALLER's order, and the caller's index of every device position (NULL: the same)
	const uint32_t* __restrict__ partner;    // [n_reads]
	const int32_t* __restrict__ read_at;     // [n_reads]
};

struct TdSamplesExportArgs {
	TdTileView tile;
	const int32_t* __restrict__ lens;        // [n_tiles*64]
	const int32_t* __restrict__ out_type;    // [n_tiles*64]  final outcomes of the decode launch
	const TdSamplePlan* __restrict__ plan;
	uint32_t* __restrict__ words;            // [n_reads]  the export words, in the CALLER's order
	const int32_t* __restrict__ read_at;     // [n_reads]  the caller's index of every device position (NULL: the same)
	int64_t n_reads;
	int32_t n_tiles, H;
};

// the rewrite and count of one decoded slot, queued on its compute stream (td_batch.hip's launch_end while samples are on)
KT_HIDDEN int samples_slot(td_ctx* c, TdSlot& s, int32_t* out_type, int32_t* out_barcode, const int8_t* labels);
// ... and at its place in a context that exports: the words of one decoded slot into the slot's d_smp_w
KT_HIDDEN int samples_export_slot(td_ctx* c, TdSlot& s, const int32_t* out_type, const int8_t* labels);
// td_submit, in front of staging: this batch of n reads has its words named (the join's partner words / the export's array)
KT_HIDDEN int samples_words_check(td_ctx* c, int64_t n, const char* who);
// slot_stage: the named words taken for this batch -- a join's copied to the device on `up`, an export's destination remembered
KT_HIDDEN int samples_words_stage(td_ctx* c, TdSlot& s, int64_t n, hipStream_t up);
// the export words of a slot that has run: queued device -> pinned host on `down` / copied out to the named array
KT_HIDDEN int samples_export_issue_copy(td_ctx* c, TdSlot& s, hipStream_t down);
KT_HIDDEN void samples_export_copy_out(TdSlot& s);
KT_HIDDEN int samples_export_last_kernel_us(td_ctx* c, int32_t* us);
KT_HIDDEN void samples_export_release(td_ctx* c);
// option "samples_kernel_us" of td_get_option: the kernel's time of the last batch (waits for it)
KT_HIDDEN int samples_last_kernel_us(td_ctx* c, int32_t* us);
// table, plan and names freed, samples off (the caller has made sure nothing of it is queued any more)
KT_HIDDEN void samples_release(td_ctx* c);
