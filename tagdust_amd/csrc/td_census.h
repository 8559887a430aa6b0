// td_census.h -- the census of barcode spellings (include/tagdust_census.h) inside a context: its state, and what td_api.hip
// calls.  The kernels and every td_census_* entry point are in td_census.hip.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "td_keytable.h"

struct td_ctx;
struct TdSlot;

// tallies of the device table, 64 bits each, in the order of td_census_totals; behind them the compaction's cursor
enum { TDC_ELIGIBLE = 0, TDC_COUNTED, TDC_EMPTY, TDC_LONG, TDC_N, TDC_OVERFLOW, TDC_DISTINCT, TDC_CURSOR, TDC_TALLY_WORDS };

struct TdCensusState {
	bool on = false;
	int32_t segment = -1;       // the 'B' segment whose spellings are counted
	uint32_t mask = 0;          // outcomes (low byte of read_type) that are eligible
	int32_t log2_slots = 0;
	int32_t H = 0;
	// model.label's segments never decrease with the HMM index: a path (labels only move to a higher HMM, td_model_upload checks the
	// transition matrix) that has left the segment does not come back, and a scan may stop there
	bool ordered = false;
	int32_t* d_label = nullptr;               // [H] model.label, the census's own copy
	unsigned long long* d_keys = nullptr;     // [2^log2_slots], 0 = empty
	unsigned long long* d_counts = nullptr;   // [2^log2_slots]
	unsigned long long* d_tallies = nullptr;  // [TDC_TALLY_WORDS]
	hipEvent_t ev_c0 = nullptr, ev_c1 = nullptr;   // around the last count launch (option "census_kernel_us")
};

struct TdCensusArgs {
	const uint32_t* __restrict__ packed;   // [n_tiles][nw2 + nw1][64]  2-bit words then N-mask words
	const int32_t*  __restrict__ lens;     // [n_tiles*64]
	const int32_t*  __restrict__ out_type; // [n_tiles*64]  final outcomes of the decode launch
	const int8_t*   __restrict__ labels;   // [n_tiles][lmax + 1][64]
	const int32_t*  __restrict__ label;    // [H] model.label
	int64_t n_reads;
	int32_t n_tiles, lmax, nw2, nw1, H;
	int32_t segment, ordered;
	uint32_t mask;
	TdKeyTable table;                      // td_keytable.h
	unsigned long long* __restrict__ tallies;
};

__attribute__((visibility("hidden"))) hipError_t td_census_launch_count(const TdCensusArgs& a, hipStream_t stream);
// the count of one decoded slot, queued on its compute stream (td_api.hip calls it behind the decode launch while the census is on)
__attribute__((visibility("hidden"))) int census_count_slot(td_ctx* c, TdSlot& s, const int32_t* out_type, const int8_t* labels);
// option "census_kernel_us" of td_get_option: the count kernel's time of the last counted batch (waits for it)
__attribute__((visibility("hidden"))) int census_last_kernel_us(td_ctx* c, int32_t* us);
// table and label copy freed, census off (the caller has made sure nothing of it is queued any more)
__attribute__((visibility("hidden"))) void census_release(td_ctx* c);
// host helpers of every result made of td_census_entry (td_molecules.hip uses them too): the order of td_census_get; a malloc'd copy
// for td_census_free (NULL: out of memory); keys (any order, repeated) -> entries in that order
__attribute__((visibility("hidden"))) bool census_entry_before(const td_census_entry& x, const td_census_entry& y);
__attribute__((visibility("hidden"))) td_census_entry* census_copy_entries(const std::vector<td_census_entry>& v);
__attribute__((visibility("hidden"))) void census_tally_keys(std::vector<uint64_t>& keys, std::vector<td_census_entry>& out);
