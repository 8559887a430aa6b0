// td_rnadust.h -- arguments of the run_rna_dust kernel (td_rnadust.hip, TD_MODE_RNA_DUST).  Library-internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct TdRnaDustArgs {
	// the staged batch (td_stage.hip): device order k = tile * 64 + lane
	const uint32_t* packed;   // [n_tiles][nw2 + nw1][64]  2-bit words, then N-mask words
	const int32_t*  lens;     // [n_tiles * 64]
	int32_t n_tiles, nw2, nw1;
	// the raw bytes in the caller's order: DUST reads the code of an N-masked base from them ('.' is 5, and 5 & 3 = 1)
	const uint8_t* raw;
	const int64_t* offs;
	const int32_t* read_at;   // [n] or nullptr (identity)
	int64_t n_reads;
	int32_t is_ascii;
	int32_t dust;             // param->dust, 0 = off
	// -ref artifact filter; art_n == 0: off
	const uint32_t* art_pk;   // every sequence's text ('X' byte included) as 2-bit codes, 16 per dword, from a dword boundary
	const int32_t*  art_seq;  // [art_n][2]: (first dword in art_pk, characters)
	const uint8_t*  art_left; // [n_tiles * 64] 1 = left-over read of its thread range (bpm_check_error path)
	int32_t art_n, art_fe;
	// outputs, device order (the decode kernels' SoA block: td_stage_finish reads it)
	float*   out_f;
	float*   out_b;
	float*   out_r;
	float*   out_bar;
	float*   out_q;
	int32_t* out_type;
	int32_t* out_barcode;
	int32_t* out_finger;
	uint32_t* out_keep;       // [n_tiles][nw1][64]: all ones (nothing is removed from a read that is not decoded)
	unsigned long long* counters;
};

hipError_t td_launch_rna_dust(const TdRnaDustArgs& a, hipStream_t stream);
