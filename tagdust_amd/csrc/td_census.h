// td_census.h -- the census of barcode spellings (include/tagdust_census.h) inside a context: its state, and what td_api.hip and td_batch.hip
// call.  The kernel and every td_census_* entry point that takes a context are in td_census.hip.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "td_keytable.h"

struct td_ctx;
struct TdSlot;

// tallies of the device table, 64 bits each, in the order of td_census_totals; behind them the compaction's cursor
enum { TDC_ELIGIBLE = 0, TDC_COUNTED, TDC_EMPTY, TDC_LONG, TDC_N, TDC_OVERFLOW, TDC_DISTINCT, TDC_CURSOR, TDC_TALLY_WORDS };

struct TdCensusState {
	bool on = false;
	int32_t segment = -1;       // the 'B' segment whose spellings are counted
	uint32_t mask = 0;          // outcomes (low byte of read_type) that are eligible
	// model.label's segments never decrease with the HMM index: a path (labels only move to a higher HMM, td_model_upload checks the
	// transition matrix) that has left the segment does not come back, and a scan may stop there
	bool ordered = false;
	TdCountTable table;         // td_keytable.h, TDC_TALLY_WORDS tallies
};

struct TdCensusArgs {
	TdTileView tile;                       // td_keytable.h
	const int32_t*  __restrict__ lens;     // [n_tiles*64]
	const int32_t*  __restrict__ out_type; // [n_tiles*64]  final outcomes of the decode launch
	const int32_t*  __restrict__ label;    // [H] model.label
	int64_t n_reads;
	int32_t n_tiles, H;
	int32_t segment, ordered;
	uint32_t mask;
	TdKeyTable table;                      // td_keytable.h
	unsigned long long* __restrict__ tallies;
};

// the count of one decoded slot, queued on its compute stream (td_batch.hip calls it behind the decode launch while the census is on)
__attribute__((visibility("hidden"))) int census_count_slot(td_ctx* c, TdSlot& s, const int32_t* out_type, const int8_t* labels);
// option "census_kernel_us" of td_get_option: the count kernel's time of the last counted batch (waits for it)
__attribute__((visibility("hidden"))) int census_last_kernel_us(td_ctx* c, int32_t* us);
// table and label copy freed, census off (the caller has made sure nothing of it is queued any more)
__attribute__((visibility("hidden"))) void census_release(td_ctx* c);
