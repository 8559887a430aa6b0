// td_mate_filter.hip -- the mate filter (td_mol_mate_filter_enable, include/tagdust_molecules.h): run_rna_dust over the MATES of a
// TD_MODE_GET_LABEL batch, and the join of its verdict into the batch's outcomes.  The reference takes the maximum outcome of a
// record over its files (src/barcode_hmm.c:344-350) on the host behind everything; here that step stands on the device in front
// of whatever reads a batch's outcomes, so that the count, dedup and the writers see one outcome per pair.
//
// td_mate_filter_kernel: one mate per lane in the caller's order, a wave takes 64 consecutive mates; waves stay whole (padding
// lanes have length 0).  The arithmetic is td_rnadust_inner.h's, the text td_rna_dust_kernel runs; this unit says where a lane's
// bases come from.  A mate's bytes lie at a stride of one read length from its neighbour's, where single-byte loads cost ten
// times their bytes' worth -- but the 64 mates of a wave are one contiguous span of d_mate_raw.  The wave
// loads that span with coalesced dword loads into LDS in pieces of MF_PIECE_BYTES, and while a piece is there every lane takes
// from it what it needs of its own mate: the first 64 bases and the last 63, as 2-bit codes and N flags in six 64-bit registers.
// Masks and triplet counts are then built from registers.  Only the left-over reads of a thread range (at most 3 per range) need
// every base of a read: those lanes read global bytes.  A dword load never leaves the allocation: the span's last dword ends at
// offs[n] rounded up to 4, which mol_mate_stage allocates.
// LDS per workgroup of 4 waves: 16 KiB match masks (DUST's counters reuse them) + 16 KiB pieces = 32 KiB.  No scratch.
//
// td_mate_join_kernel: out_type[k] = max(out_type[k], mate_type[caller's index of k]), whole signed words (HMMER3_MAX).
#include <hip/hip_runtime.h>

#include "td_device.h"
#include "td_mate_filter.h"
#include "td_rnadust_inner.h"

#define MF_BLOCK 256
#define MF_WAVES (MF_BLOCK / TD_WAVE)
#define MF_PIECE_BYTES 4096
#define MF_PIECE_LOADS (MF_PIECE_BYTES / 4 / TD_WAVE)   // dword loads per lane and piece

// the wave's LDS writes are visible to its own later reads, and the other way round (one wave: no s_barrier)
__device__ __forceinline__ void mf_wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a 64-bit value every lane of the wave holds alike, said so to the compiler (the piece loop is the wave's, not a lane's)
__device__ __forceinline__ int64_t mf_uniform(int64_t v)
{
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
	return (int64_t)(((uint64_t)hi << 32) | lo);
}

// 64 bases of a window in registers: byte b of window position q (the code is b & 3 also for an N: DUST reads that back)
struct MfWindow { rd_u64 c0 = 0ull, c1 = 0ull, n = 0ull; };
__device__ __forceinline__ void mf_put(MfWindow& w, int q, uint32_t b)
{
	const rd_u64 c = (rd_u64)(b & 3u) << (2 * (q & 31));
	if (q < 32) w.c0 |= c; else w.c1 |= c;
	w.n |= (rd_u64)(b > 3u ? 1u : 0u) << q;
}
// (values, not references: a select between two registers, never between two addresses)
__device__ __forceinline__ uint32_t mf_bits(rd_u64 c0, rd_u64 c1, int q) { const rd_u64 w = q < 32 ? c0 : c1; return (uint32_t)((w >> (2 * (q & 31))) & 3ull); }

__global__ __launch_bounds__(MF_BLOCK) void td_mate_filter_kernel(const TdMateFilterArgs a)
{
	// per wave: the match masks of both strands, [strand][code][lane] (4 KiB; DUST's triplet counters reuse the space), and a piece
	__shared__ rd_u64 s_eq[MF_WAVES][2][4][TD_WAVE];
	__shared__ uint32_t s_piece[MF_WAVES][MF_PIECE_BYTES / 4];
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int wv = threadIdx.x >> 6;
	const int64_t i0 = ((int64_t)blockIdx.x * MF_WAVES + wv) * TD_WAVE;
	if (i0 >= a.n_reads) return;                      // (whole waves; no workgroup barrier below)
	const int64_t i = i0 + lane;
	const bool real = i < a.n_reads;
	const int64_t i1 = i0 + TD_WAVE < a.n_reads ? i0 + TD_WAVE : a.n_reads;
	const int64_t span0 = mf_uniform(a.offs[i0]), span1 = mf_uniform(a.offs[i1]);   // the wave's mates are raw[span0, span1)
	const int64_t o = real ? a.offs[i] : span1;
	const int len = real ? (int)(a.offs[i + 1] - o) : 0;
	int tmax = len;
	for (int s = 32; s >= 1; s >>= 1) { const int t2 = __shfl_xor(tmax, s); tmax = t2 > tmax ? t2 : tmax; }

	// ---- the lane's first 64 bases and its last 63 (positions ts..len-1), out of the wave's span piece by piece ----
	const int nf = len > 64 ? 64 : len;
	const int ts = len > 63 ? len - 63 : 0;
	MfWindow head, tail;
	uint32_t* sp = s_piece[wv];
	const uint8_t* sb = (const uint8_t*)sp;
	for (int64_t pb = span0 & ~3ll; pb < span1; pb += MF_PIECE_BYTES) {
#pragma unroll
		for (int d = 0; d < MF_PIECE_LOADS; d++) {
			const int idx = d * TD_WAVE + lane;
			const int64_t at = pb + 4 * (int64_t)idx;
			if (at < span1) sp[idx] = *(const uint32_t*)(a.raw + at);   // (its last bytes may lie behind span1, inside the padding)
		}
		mf_wave_sync();
		const int64_t pe = pb + MF_PIECE_BYTES < span1 ? pb + MF_PIECE_BYTES : span1;
		{
			const int64_t w0 = o, w1 = o + nf;               // the window in raw; [lo, hi) is what of it this piece holds
			const int64_t lo = w0 > pb ? w0 : pb, hi = w1 < pe ? w1 : pe;
			for (int64_t p = lo; p < hi; p++) mf_put(head, (int)(p - w0), sb[p - pb]);
		}
		{
			const int64_t w0 = o + ts, w1 = o + len;
			const int64_t lo = w0 > pb ? w0 : pb, hi = w1 < pe ? w1 : pe;
			for (int64_t p = lo; p < hi; p++) mf_put(tail, (int)(p - w0), sb[p - pb]);
		}
		mf_wave_sync();
	}
	// base at position p of the mate, p < 64 or p >= ts: DUST's code, the N flag, the 2-bit code (0 for N)
	const rd_u64 hc0 = head.c0, hc1 = head.c1, hn = head.n, tc0 = tail.c0, tc1 = tail.c1, tn = tail.n;
	auto bits = [=](int p) -> uint32_t { const bool h = p < 64; return mf_bits(h ? hc0 : tc0, h ? hc1 : tc1, h ? p : p - ts); };
	auto is_n = [=](int p) -> bool { const bool h = p < 64; return (((h ? hn : tn) >> (h ? p : p - ts)) & 1ull) != 0ull; };
	auto code2 = [&](int p) -> int { return is_n(p) ? 0 : (int)bits(p); };
	rd_u64* eqf = &s_eq[wv][0][0][lane];
	rd_u64* eqr = &s_eq[wv][1][0][lane];

	int read_type = RD_SUCCESS;
	// ---- match_to_reference, src/barcode_hmm.c:2478-2583 ----
	if (a.art_n > 0) {
		// the closed form of td_art_left_kernel (td_stage.hip): mate i is a left-over read of its thread range exactly when read i is
		bool left = false;
		if (real && a.art_threads > 0) {
			const int64_t g = a.win_first + i;
			const int64_t n = a.win_total > 0 ? a.win_total : a.n_reads, T = a.art_threads, interval = n / T;
			int64_t t = interval > 0 ? g / interval : T - 1;
			if (t > T - 1) t = T - 1;
			const int64_t start = t * interval, end = (t == T - 1) ? n : (t + 1) * interval;
			left = g >= start + (end - start) / 4 * 4;
		}
		// a left-over lane takes every base of its mate from global memory (the other lanes' answers are not used)
		const uint8_t* src = a.raw + o;
		auto wcode2 = [&](int p) -> int { if (!left) return 0; const uint32_t b = src[p]; return b > 3u ? 0 : (int)b; };
		auto wis_n = [&](int p) -> bool { return left && src[p] > 3u; };
		const int found = rd_match(a, len, tmax, real, left, code2, is_n, wcode2, wis_n, eqf, eqr);
		if (found > 0) read_type = (found << 8) | RD_ARTIFACT;
	}

	// ---- dust_sequences, :2407-2467: the first 64 bases, an N read back as code & 3 ----
	if (a.dust && len >= 1) {
		uint8_t* cnt = (uint8_t*)&s_eq[wv][0][0][0] + lane;      // [key][lane] bytes
		auto dcode = [&](int p) -> uint32_t { return p >= len ? 0u : bits(p); };   // (p < 64 here)
		if (rd_dust_low(len, a.dust, cnt, dcode)) read_type = RD_LOW_COMPLEXITY;
	}
	if (real) a.mate_type[i] = read_type;
}

hipError_t td_launch_mate_filter(const TdMateFilterArgs& a, hipStream_t stream)
{
	if (a.n_reads <= 0) return hipSuccess;
	const int64_t waves = (a.n_reads + TD_WAVE - 1) / TD_WAVE;
	hipLaunchKernelGGL(td_mate_filter_kernel, dim3((unsigned)((waves + MF_WAVES - 1) / MF_WAVES)), dim3(MF_BLOCK), 0, stream, a);
	return hipGetLastError();
}

__global__ __launch_bounds__(MF_BLOCK) void td_mate_join_kernel(int32_t* __restrict__ out_type, const int32_t* __restrict__ mate_type,
                                                                 const int32_t* __restrict__ read_at, int64_t n_reads)
{
	const int64_t k = (int64_t)blockIdx.x * MF_BLOCK + threadIdx.x;
	if (k >= n_reads) return;
	const int32_t t2 = mate_type[read_at ? (int64_t)read_at[k] : k];
	const int32_t t = out_type[k];
	out_type[k] = t2 > t ? t2 : t;
}

hipError_t td_launch_mate_join(int32_t* out_type, const int32_t* mate_type, const int32_t* read_at, int64_t n_reads, hipStream_t stream)
{
	if (n_reads <= 0) return hipSuccess;
	hipLaunchKernelGGL(td_mate_join_kernel, dim3((unsigned)((n_reads + MF_BLOCK - 1) / MF_BLOCK)), dim3(MF_BLOCK), 0, stream, out_type, mate_type,
	                   read_at, n_reads);
	return hipGetLastError();
}
