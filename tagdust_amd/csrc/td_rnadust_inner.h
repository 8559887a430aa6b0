// td_rnadust_inner.h -- the arithmetic of run_rna_dust on the device, one text for the two kernels that judge a read without
// decoding it: td_rna_dust_kernel (td_rnadust.hip, a batch of its own from packed tiles) and td_mate_filter_kernel
// (td_mate_filter.hip, the mates of a TD_MODE_GET_LABEL batch from their raw codes).  Device code only; library-internal.
//
// Everything here is parametrised over how a lane reaches its bases:
//   code2(p)  the 2-bit code of base p < len, 0 for an N;
//   is_n(p)   base p is not A, C, G or T;
//   dcode(p)  DUST's code of base p, the reference's `code & 3` of the byte as it was read (0 behind the read's end).
// The artifact filter is the same computation as td_artifact.inc (reads in fours: bmp_single, src/misc.c:718-765; the left-over
// reads of a thread range: bpm_check_error, :581-640), arranged for these kernels' inner loop:
//   - the text comes as 2-bit codes, 16 per dword (td_set_artifacts packs them), one wave-uniform load per 16 characters;
//   - a lane's four match masks per strand sit in LDS, and the text character picks one with a wave-uniform offset: one
//     address add and two LDS reads per character instead of a branch tree;
//   - the forward and the reverse-complement strand run side by side in one pass over the text;
//   - a wave whose reads all have 63 or more bases (the usual case) takes the score from a fixed bit.
// DUST is rna_dust_low of td_stream.cpp: the first 64 bases, triplet counts, double arithmetic, the (c - 3) divisor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "td_device.h"

typedef unsigned long long rd_u64;

// extraction outcomes, include/tagdust_hip.h
#define RD_SUCCESS 0
#define RD_ARTIFACT 5
#define RD_LOW_COMPLEXITY 6

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
// a: the kernel's arguments, of which art_n, art_seq and art_pk are read (TdRnaDustArgs names them).
template <bool kTop, class Args>
__device__ int rd_best(const Args& a, const rd_u64* eqf, const rd_u64* eqr, int m, int& errors_out)
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

// A lane's match masks of both strands into LDS: pattern bit c (taken modulo 64) is base c forward and the complement of base
// len - 1 - c reverse (rev_nuc_code, N -> 4 & 3 = 0), for c < min(len, cap); `bound` is the wave's largest such count.
template <class C2, class IsN>
__device__ __forceinline__ void rd_build_masks(int len, int cap, int bound, C2&& code2, IsN&& is_n, rd_u64* eqf, rd_u64* eqr)
{
	rd_u64 F0 = 0ull, F1 = 0ull, F2 = 0ull, F3 = 0ull, R0 = 0ull, R1 = 0ull, R2 = 0ull, R3 = 0ull;
	for (int c = 0; c < bound; c++) {
		if (c < cap) {
			const rd_u64 bit = 1ull << (c & 63);
			const int s = code2(c);                             // (N is 0 in the 2-bit codes)
			F0 |= s == 0 ? bit : 0ull; F1 |= s == 1 ? bit : 0ull; F2 |= s == 2 ? bit : 0ull; F3 |= s == 3 ? bit : 0ull;
			const int p = len - 1 - c;
			const int r = is_n(p) ? 0 : 3 - code2(p);
			R0 |= r == 0 ? bit : 0ull; R1 |= r == 1 ? bit : 0ull; R2 |= r == 2 ? bit : 0ull; R3 |= r == 3 ? bit : 0ull;
		}
	}
	eqf[0] = F0; eqf[TD_WAVE] = F1; eqf[2 * TD_WAVE] = F2; eqf[3 * TD_WAVE] = F3;
	eqr[0] = R0; eqr[TD_WAVE] = R1; eqr[2 * TD_WAVE] = R2; eqr[3 * TD_WAVE] = R3;
}

// match_to_reference, src/barcode_hmm.c:2478-2583, for the lane's read: the 1-based sequence it matches, 0 for none.  Whole waves:
// every lane of the wave calls this (padding lanes with len 0, real false).  tmax: the wave's longest read.  left: the read is a
// left-over read of its thread range.  code2 / is_n serve the reads in fours (positions 0..62 and len-63..len-1 are asked for),
// wcode2 / wis_n the left-over pass, which asks for every position of every lane's read -- only a left-over lane's answers count.
template <class Args, class C2, class IsN, class WC2, class WIsN>
__device__ __forceinline__ int rd_match(const Args& a, int len, int tmax, bool real, bool left, C2&& code2, IsN&& is_n, WC2&& wcode2,
                                        WIsN&& wis_n, rd_u64* eqf, rd_u64* eqr)
{
	// reads in fours: the pattern is the read's first 63 bases; its reverse complement the last 63, complemented
	const int m = len > 63 ? 63 : len;
	rd_build_masks(len, m, tmax > 63 ? 63 : tmax, code2, is_n, eqf, eqr);
	// (padding lanes count as full patterns: their scores are not used)
	const bool top = __builtin_amdgcn_readfirstlane((int)(__ballot(real && m != 63) == 0ull)) != 0;
	int errors = 0;
	const int id = top ? rd_best<true>(a, eqf, eqr, m, errors) : rd_best<false>(a, eqf, eqr, m, errors);
	int found = (!left && errors <= a.art_fe) ? id : 0;
	// left-over reads: first hit, forward strand before reverse complement; masks of the whole read with the shifts of the
	// reference's build taken modulo 64, all-ones VP, the pattern length capped at 31 after the masks were built, the
	// running score started from the uncapped length
	if (__builtin_amdgcn_readfirstlane((int)(__ballot(left) != 0ull))) {
		rd_build_masks(len, len, tmax, wcode2, wis_n, eqf, eqr);
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
	return found;
}

// dust_sequences, :2407-2467, on the read as it was read (rna_dust_low, td_stream.cpp), len >= 1: true = low complexity.
// cnt: the lane's 64 triplet counters, bytes at a stride of TD_WAVE.
template <class DC>
__device__ __forceinline__ bool rd_dust_low(int len, int dust, uint8_t* cnt, DC&& dcode)
{
	for (int q = 0; q < 64; q++) cnt[q * TD_WAVE] = 0;
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
	return s > (double)dust;
}
