// td_mate_filter.h -- arguments of the mate filter's two kernels (td_mate_filter.hip; td_mol_mate_filter_enable,
// include/tagdust_molecules.h).  Library-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct TdMateFilterArgs {
	// the mate batch as uploaded, in the caller's order: codes (0..3 = A, C, G, T, anything else N) and offs[n_reads + 1] from 0.
	// raw is dword-aligned and allocated up to offs[n_reads] rounded up to a multiple of 4.
	const uint8_t* raw;
	const int64_t* offs;
	int64_t n_reads;
	int32_t dust;             // param->dust, 0 = off
	// -ref artifact filter as TdRnaDustArgs has it; art_n == 0: off
	const uint32_t* art_pk;
	const int32_t*  art_seq;
	int32_t art_n, art_fe;
	// the thread ranges of match_to_reference: td_set_artifacts' n_threads and td_set_batch_window's first_read / total
	int32_t art_threads;
	int64_t win_first, win_total;
	int32_t* mate_type;       // [n_reads] what TD_MODE_RNA_DUST leaves in read_type for mate i
};

hipError_t td_launch_mate_filter(const TdMateFilterArgs& a, hipStream_t stream);
// out_type[k] = max(out_type[k], mate_type[read_at ? read_at[k] : k]) for the n_reads reads of a decoded batch in device order
hipError_t td_launch_mate_join(int32_t* out_type, const int32_t* mate_type, const int32_t* read_at, int64_t n_reads, hipStream_t stream);
