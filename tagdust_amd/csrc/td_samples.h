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
enum { SMP_ELIGIBLE = 0, SMP_ASSIGNED, SMP_UNLISTED, SMP_INCOMPLETE, SMP_OVERFLOW, SMP_DISTINCT, SMP_CURSOR, SMP_TALLY_WORDS };

struct TdSamplesState {
	bool on = false;
	int32_t gen = 0;                  // counts the enables: a batch remembers the one it was staged under (TdStaged::samples_gen)
	TdSamplePlan plan{};
	TdSamplePlan* d_plan = nullptr;   // ... and its copy on the device
	std::vector<std::string> names;
	TdCountTable table;               // td_keytable.h, SMP_TALLY_WORDS tallies
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
};

// the rewrite and count of one decoded slot, queued on its compute stream (td_batch.hip's launch_end while samples are on)
KT_HIDDEN int samples_slot(td_ctx* c, TdSlot& s, int32_t* out_type, int32_t* out_barcode, const int8_t* labels);
// option "samples_kernel_us" of td_get_option: the kernel's time of the last batch (waits for it)
KT_HIDDEN int samples_last_kernel_us(td_ctx* c, int32_t* us);
// table, plan and names freed, samples off (the caller has made sure nothing of it is queued any more)
KT_HIDDEN void samples_release(td_ctx* c);
