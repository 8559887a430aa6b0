// td_rnadust.hip -- run_rna_dust() on the device (TD_MODE_RNA_DUST): what the controller runs instead of the HMM for a file
// whose architecture is one read segment (src/barcode_hmm.c:313-325).  do_rna_dust (:2370-2395) sets read_type =
// EXTRACT_SUCCESS, runs match_to_reference (:2478-2583) with -ref, then dust_sequences (:2407-2467) with -dust, which
// overwrites read_type with LOW_COMPLEXITY whatever it was.  The read is the read as it was read: nothing is removed.
//
// One read per lane over the length-sorted tiles of the staging (td_stage.hip), one wave per tile.  The artifact filter is the
// same computation as td_artifact.inc (reads in fours: bmp_single, src/misc.c:718-765; the left-over reads of a thread range:
// bpm_check_error, :581-640), arranged for this kernel's inner loop:
//   - the text comes as 2-bit codes, 16 per dword (td_set_artifacts packs them), one wave-uniform load per 16 characters;
//   - a lane's four match masks per strand sit in LDS, and the text character picks one with a wave-uniform offset: one
//     address add and two LDS reads per character instead of a branch tree;
//   - the forward and the reverse-complement strand run side by side in one pass over the text;
//   - a wave whose reads all have 63 or more bases (the usual case) takes the score from a fixed bit.
// DUST is rna_dust_low of td_stream.cpp: the first 64 bases, triplet counts, double arithmetic, the (c - 3) divisor.
#include <hip/hip_runtime.h>

#include "td_device.h"
#include "td_rnadust.h"

typedef unsigned long long rd_u64;

#define RD_BLOCK 256
#define RD_WAVES (RD_BLOCK / TD_WAVE)

// extraction outcomes, include/tagdust_hip.h
#define RD_SUCCESS 0
#define RD_ARTIFACT 5
#define RD_LOW_COMPLEXITY 6
#define RD_OUTCOME_SLOTS 8

// One column of Myers' recurrence with the score bit at `sh` (bmp_single, misc.c:718-765; signed running score).
// kTop: every lane of the wave has a 63-character pattern, so the score bit is bit 62.
template <bool kTop>
__device__ __forceinline__ void rd_step(rd_u64 eq, rd_u64& VP, rd_u64& VN, int& d, int& k, int sh)
{
	rd_u64 X = eq | VN;
	const rd_u64 D0 = ((VP + (X & VP)) ^ VP) | X;
	const rd_u64 HN = VP & D0;
	const rd_u64 HP = VN | ~(VP | D0);
	X = HP << 1;
	VN = X & D0;
	VP = (HN << 1) | ~(X | D0);
	if (kTop) d += (int)(((uint32_t)(HP >> 32) >> 30) & 1u) - (int)(((uint32_t)(HN >> 32) >> 30) & 1u);
	else d += (int)((HP >> sh) & 1ull) - (int)((HN >> sh) & 1ull);
	k = d < k ? d : k;
}

// bpm_check_error's column (misc.c:581-640): the running score is unsigned 64-bit, the bit taken modulo 64
__device__ __forceinline__ void rd_step_chk(rd_u64 eq, rd_u64& VP, rd_u64& VN, rd_u64& d, rd_u64& k, int sh)
{
	rd_u64 X = eq | VN;
	const rd_u64 D0 = ((VP + (X & VP)) ^ VP) | X;
	const rd_u64 HN = VP & D0;
	const rd_u64 HP = VN | ~(VP | D0);
	X = HP << 1;
	VN = X & D0;
	VP = (HN << 1) | ~(X | D0);
	d += (HP >> sh) & 1ull;
	d -= (HN >> sh) & 1ull;
	k = d < k ? d : k;
}

// The text of one artifact sequence, 16 characters per wave-uniform dword; f(tc) is called once per character, in order.
template <class F>
__device__ __forceinline__ void rd_scan_text(const uint32_t* __restrict__ tw, int n, F&& f)
{
	for (int q = 0; q < n; q += 16) {
		const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)tw[q >> 4]);
		if (n - q >= 16) {
#pragma unroll
			for (int i = 0; i < 16; i++) f((int)((w >> (2 * i)) & 3u));
		} else {
			for (int i = 0; i < n - q; i++) f((int)((w >> (2 * i)) & 3u));
		}
	}
}

// Reads in fours: best (sequence, strand) by the smallest error count, forward before reverse, the first sequence on ties.
// eqf / eqr: this lane's four match masks per strand in LDS (mask of text code c at index c * 64).
template <bool kTop>
__device__ int rd_best(const TdRnaDustArgs& a, const rd_u64* eqf, const rd_u64* eqr, int m, int& errors_out)
{
	const int mp = m > 0 ? m : 1;
	const int sh = mp - 1;
	const rd_u64 ones = (mp >= 64) ? ~0ull : ((1ull << mp) - 1ull);
	int errors = 100000, id = 0;
	for (int j = 0; j < a.art_n; j++) {
		const int p0 = a.art_seq[2 * j], n = a.art_seq[2 * j + 1];
		rd_u64 VPf = ones, VNf = 0ull, VPr = ones, VNr = 0ull;
		int df = mp, kf = mp, dr = mp, kr = mp;
		rd_scan_text(a.art_pk + p0, n, [&](int tc) {
			const rd_u64 ef = eqf[tc * TD_WAVE], er = eqr[tc * TD_WAVE];
			rd_step<kTop>(ef, VPf, VNf, df, kf, sh);
			rd_step<kTop>(er, VPr, VNr, dr, kr, sh);
		});
		// validate_bpm_sse (misc.c:776-795): an empty query scores the text length
		const int ef = m > 0 ? kf : n, er = m > 0 ? kr : n;
		if (ef < errors) { errors = ef; id = j + 1; }
		if (er < errors) { errors = er; id = j + 1; }
	}
	errors_out = errors;
	return id;
}

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
		// reads in fours: the pattern is the read's first 63 bases; its reverse complement the last 63, complemented
		// (rev_nuc_code, N -> 4 & 3 = 0)
		const int m = len > 63 ? 63 : len;
		{
			rd_u64 F0 = 0ull, F1 = 0ull, F2 = 0ull, F3 = 0ull, R0 = 0ull, R1 = 0ull, R2 = 0ull, R3 = 0ull;
			const int mm = tmax > 63 ? 63 : tmax;
			for (int c = 0; c < mm; c++) {
				if (c < m) {
					const rd_u64 bit = 1ull << c;
					const int s = code2(c);                             // (N is 0 in the 2-bit words)
					F0 |= s == 0 ? bit : 0ull; F1 |= s == 1 ? bit : 0ull; F2 |= s == 2 ? bit : 0ull; F3 |= s == 3 ? bit : 0ull;
					const int p = len - 1 - c;
					const int r = is_n(p) ? 0 : 3 - code2(p);
					R0 |= r == 0 ? bit : 0ull; R1 |= r == 1 ? bit : 0ull; R2 |= r == 2 ? bit : 0ull; R3 |= r == 3 ? bit : 0ull;
				}
			}
			eqf[0] = F0; eqf[TD_WAVE] = F1; eqf[2 * TD_WAVE] = F2; eqf[3 * TD_WAVE] = F3;
			eqr[0] = R0; eqr[TD_WAVE] = R1; eqr[2 * TD_WAVE] = R2; eqr[3 * TD_WAVE] = R3;
		}
		// (padding lanes count as full patterns: their scores are not used)
		const bool top = __builtin_amdgcn_readfirstlane((int)(__ballot(real && m != 63) == 0ull)) != 0;
		int errors = 0;
		const int id = top ? rd_best<true>(a, eqf, eqr, m, errors) : rd_best<false>(a, eqf, eqr, m, errors);
		int found = (!left && errors <= a.art_fe) ? id : 0;
		// left-over reads: first hit, forward strand before reverse complement; masks of the whole read with the shifts of the
		// reference's build taken modulo 64, all-ones VP, the pattern length capped at 31 after the masks were built, the
		// running score started from the uncapped length
		if (__builtin_amdgcn_readfirstlane((int)(__ballot(left) != 0ull))) {
			rd_u64 F0 = 0ull, F1 = 0ull, F2 = 0ull, F3 = 0ull, R0 = 0ull, R1 = 0ull, R2 = 0ull, R3 = 0ull;
			for (int c = 0; c < tmax; c++) {
				if (c < len) {
					const rd_u64 bit = 1ull << (c & 63);
					const int s = code2(c);
					F0 |= s == 0 ? bit : 0ull; F1 |= s == 1 ? bit : 0ull; F2 |= s == 2 ? bit : 0ull; F3 |= s == 3 ? bit : 0ull;
					const int p = len - 1 - c;
					const int r = is_n(p) ? 0 : 3 - code2(p);
					R0 |= r == 0 ? bit : 0ull; R1 |= r == 1 ? bit : 0ull; R2 |= r == 2 ? bit : 0ull; R3 |= r == 3 ? bit : 0ull;
				}
			}
			eqf[0] = F0; eqf[TD_WAVE] = F1; eqf[2 * TD_WAVE] = F2; eqf[3 * TD_WAVE] = F3;
			eqr[0] = R0; eqr[TD_WAVE] = R1; eqr[2 * TD_WAVE] = R2; eqr[3 * TD_WAVE] = R3;
			const int new_len = len > 31 ? 31 : len;              // (a raw read has no spacer byte: every base is usable)
			const int sh = (new_len - 1) & 63;
			int hit = 0;
			for (int j = 0; j < a.art_n; j++) {
				const int p0 = a.art_seq[2 * j], n = a.art_seq[2 * j + 1];
				rd_u64 VPf = ~0ull, VNf = 0ull, VPr = ~0ull, VNr = 0ull;
				rd_u64 df = (rd_u64)(unsigned)len, kf = (rd_u64)(unsigned)new_len, dr = df, kr = kf;
				rd_scan_text(a.art_pk + p0, n, [&](int tc) {
					rd_step_chk(eqf[tc * TD_WAVE], VPf, VNf, df, kf, sh);
					rd_step_chk(eqr[tc * TD_WAVE], VPr, VNr, dr, kr, sh);
				});
				if (hit == 0 && (int)kf <= a.art_fe) hit = j + 1;
				if (hit == 0 && (int)kr <= a.art_fe) hit = j + 1;
			}
			if (left) found = hit;
		}
		if (found > 0) read_type = (found << 8) | RD_ARTIFACT;
	}

	// ---- dust_sequences, :2407-2467, on the read as it was read (rna_dust_low, td_stream.cpp) ----
	if (a.dust && len >= 1) {
		uint8_t* cnt = (uint8_t*)&s_eq[wv][0][0][0] + lane;      // [key][lane] bytes
		for (int q = 0; q < 64; q++) cnt[q * TD_WAVE] = 0;
		const uint8_t* src = nullptr;
		if (real) { const int64_t i = a.read_at ? (int64_t)a.read_at[k] : k; src = a.raw + a.offs[i]; }
		// the reference's code & 3: an N-masked base is read back from the raw bytes ('.' = 5 -> 1, other non-ACGT -> 0)
		auto dcode = [&](int p) -> uint32_t {
			if (p >= len) return 0u;                               // (the reference's sequences end in a 0 byte)
			if (!is_n(p)) return (uint32_t)code2(p);
			const uint32_t ch = src ? (uint32_t)src[p] : 4u;
			return a.is_ascii ? (ch == '.' ? 1u : 0u) : (ch & 3u);
		};
		uint32_t key = (dcode(0) << 2) | dcode(1);
		const int n = len > 64 ? 64 : len;
		int c = 2;
		for (int j = 2; j < 64; j++) {
			if (j < n) {
				key = ((key << 2) | dcode(j)) & 0x3Fu;
				cnt[key * TD_WAVE]++;
				c++;
			}
		}
		uint32_t pairs = 0;                                        // sum of t (t - 1) / 2: exact, as the reference's doubles are
		for (int q = 0; q < 64; q++) { const uint32_t t = cnt[q * TD_WAVE]; pairs += t * (t - 1u) / 2u; }
		double s = (double)pairs;
		s = s / (double)(c - 3) * 10.0;
		if (s > (double)a.dust) read_type = RD_LOW_COMPLEXITY;
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
