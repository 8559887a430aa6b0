// td_rnadust.hip -- run_rna_dust() on the device (TD_MODE_RNA_DUST): what the controller runs instead of the HMM for a file
// whose architecture is one read segment (src/barcode_hmm.c:313-325).  do_rna_dust (:2370-2395) sets read_type =
// EXTRACT_SUCCESS, runs match_to_reference (:2478-2583) with -ref, then dust_sequences (:2407-2467) with -dust, which
// overwrites read_type with LOW_COMPLEXITY whatever it was.  The read is the read as it was read: nothing is removed.
//
// One read per lane over the length-sorted tiles of the staging (td_stage.hip), one wave per tile.  The arithmetic -- the artifact
// filter's Myers columns, mask builds and best-hit rules, DUST's triplet score -- is td_rnadust_inner.h's, shared with the mate
// filter (td_mate_filter.hip); this unit says where a lane's bases come from: the packed 2-bit words and N masks of its tile.
#include <hip/hip_runtime.h>

#include "td_device.h"
#include "td_rnadust.h"
#include "td_rnadust_inner.h"

#define RD_BLOCK 256
#define RD_WAVES (RD_BLOCK / TD_WAVE)
#define RD_OUTCOME_SLOTS 8

__global__ __launch_bounds__(RD_BLOCK) void td_rna_dust_kernel(const TdRnaDustArgs a)
{
	// per wave: the match masks of both strands, [strand][code][lane] (4 KiB); DUST's triplet counters reuse the space
	__shared__ rd_u64 s_eq[RD_WAVES][2][4][TD_WAVE];
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int wv = threadIdx.x >> 6;
	const int tile = blockIdx.x * RD_WAVES + wv;
	if (tile >= a.n_tiles) return;                    // (whole waves; no workgroup barrier below)
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	const bool real = k < a.n_reads;
	const int len = a.lens[k];                        // 0 for the padding lanes of the last tile
	int tmax = len;
	for (int o = 32; o >= 1; o >>= 1) { const int t2 = __shfl_xor(tmax, o); tmax = t2 > tmax ? t2 : tmax; }
	const uint32_t* pk = a.packed + (int64_t)tile * (a.nw2 + a.nw1) * TD_WAVE + lane;
	// base at position p < len: 2-bit code (0 for N) and N flag
	auto code2 = [&](int p) -> int { return (int)((pk[(p >> 4) * TD_WAVE] >> (2 * (p & 15))) & 3u); };
	auto is_n = [&](int p) -> bool { return ((pk[(a.nw2 + (p >> 5)) * TD_WAVE] >> (p & 31)) & 1u) != 0u; };
	rd_u64* eqf = &s_eq[wv][0][0][lane];
	rd_u64* eqr = &s_eq[wv][1][0][lane];

	int read_type = RD_SUCCESS;
	// ---- match_to_reference, src/barcode_hmm.c:2478-2583 ----
	if (a.art_n > 0) {
		const bool left = real && a.art_left[k] != 0;
		const int found = rd_match(a, len, tmax, real, left, code2, is_n, code2, is_n, eqf, eqr);
		if (found > 0) read_type = (found << 8) | RD_ARTIFACT;
	}

	// ---- dust_sequences, :2407-2467, on the read as it was read (rna_dust_low, td_stream.cpp) ----
	if (a.dust && len >= 1) {
		uint8_t* cnt = (uint8_t*)&s_eq[wv][0][0][0] + lane;      // [key][lane] bytes
		const uint8_t* src = nullptr;
		if (real) { const int64_t i = a.read_at ? (int64_t)a.read_at[k] : k; src = a.raw + a.offs[i]; }
		// the reference's code & 3: an N-masked base is read back from the raw bytes ('.' = 5 -> 1, other non-ACGT -> 0)
		auto dcode = [&](int p) -> uint32_t {
			if (p >= len) return 0u;                               // (the reference's sequences end in a 0 byte)
			if (!is_n(p)) return (uint32_t)code2(p);
			const uint32_t ch = src ? (uint32_t)src[p] : 4u;
			return a.is_ascii ? (ch == '.' ? 1u : 0u) : (ch & 3u);
		};
		if (rd_dust_low(len, a.dust, cnt, dcode)) read_type = RD_LOW_COMPLEXITY;
	}

	// ---- the record read_fasta_fastq leaves (io.c:1698-1702) with this read_type; nothing removed ----
	a.out_f[k] = 0.0f; a.out_b[k] = 0.0f; a.out_r[k] = 0.0f; a.out_bar[k] = 0.0f; a.out_q[k] = -1.0f;
	a.out_type[k] = read_type; a.out_barcode[k] = -1; a.out_finger[k] = -1;
	uint32_t* kw = a.out_keep + (int64_t)tile * a.nw1 * TD_WAVE + lane;
	for (int w = 0; w < a.nw1; w++) kw[w * TD_WAVE] = 0xFFFFFFFFu;
	// counters like TD_MODE_GET_LABEL: one atomic per wave and distinct outcome (no barcode bins: there is no barcode)
	const int key1 = (real && len >= 1) ? (read_type & (RD_OUTCOME_SLOTS - 1)) : -1;
	unsigned long long todo = __builtin_amdgcn_ballot_w64(key1 >= 0);
	while (todo) {
		const int leader = __builtin_ctzll(todo);
		const int kv = __builtin_amdgcn_readlane(key1, leader);
		const unsigned long long same = __builtin_amdgcn_ballot_w64(key1 == kv);
		if (lane == leader) atomicAdd(&a.counters[kv], (unsigned long long)__builtin_popcountll(same));
		todo &= ~same;
	}
}

hipError_t td_launch_rna_dust(const TdRnaDustArgs& a, hipStream_t stream)
{
	if (a.n_tiles <= 0) return hipSuccess;
	const unsigned blocks = (unsigned)((a.n_tiles + RD_WAVES - 1) / RD_WAVES);
	hipLaunchKernelGGL(td_rna_dust_kernel, dim3(blocks), dim3(RD_BLOCK), 0, stream, a);
	return hipGetLastError();
}
