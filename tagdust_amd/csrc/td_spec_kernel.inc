// td_spec_kernel.inc -- MODEL-SPECIALISED decode kernel for gfx950 (MI355X), hand-written HIP.
//
// Compiled at td_model_upload() time with hiprtc, behind a generated "model section" that states the
// read-architecture HMM as constexpr tables (kCols, kNHmm, ...).  Every segment / HMM / column loop below is
// fully unrolled over those tables, so
//   * every transition / emission / entry parameter is an instruction literal (no parameter loads at all),
//   * every term gated by a -inf parameter disappears at compile time (logsum(x, -inf) == x exactly),
//   * emission lookups collapse to the few distinct values a column really has (2 selects for a barcode column).
// Same mapping as the generic kernel (td_kernels.hip): ONE READ PER LANE, wave-uniform control flow, no
// cross-lane arithmetic -- the reference's (+) chains are folded in the reference's order.  On top of that,
// kGroup[j] HMMs of a segment are swept together per position pass: independent dependency chains in one
// instruction stream (ILP hides the LDS latency of the logsum look-ups) and fewer silent-row round trips.
//
// Reference: backward() src/barcode_hmm.c:3439-3640, forward_max_posterior_decoding() :4128-4525,
// Q value do_label_thread :2320-2338, extract_reads()/make_extracted_read() :3172-3356,
// dust_sequences() :2407-2467, logsum() src/misc.c:72-78.
//
// Expects from the model section: TD_S, TD_H, TD_C, TD_REQ_FINGER, TD_NPRED, struct GCol, kCols[TD_C], kNHmm[], kNCol[],
// kColOff[], kHmmOff[], kSkip[], kGroup[], kGroupF[], kPureLast[], kRt[], kBase[TD_C], kHi[], kLo[], kNv[], kDropM[], kBwOff[TD_H] (stored half-columns -- 4 B per lane -- per position before HMM h), kBg[5], kRStay,
// kRExit, kHinfo[TD_H], kPredOff[TD_H+1], kPredIdx[].

#ifndef TDS_BLOCK
#define TDS_BLOCK 512
#endif
#ifndef TDS_MIN_WAVES
#define TDS_MIN_WAVES 4
#endif
#define TDS_REG_H 32   // label DP row / total_prob in registers up to this many HMMs, in the workspace beyond
#define TDS_WPB (TDS_BLOCK / TD_WAVE)
#define NEG_INF (-__builtin_inff())
#define DEV __device__ __forceinline__

#define MODE_GET_LABEL 1
#define MODE_ARCH_COMP 5
#define OUT_SUCCESS 0
#define OUT_ARCH_MISMATCH 1
#define OUT_TOO_SHORT 2
#define OUT_BAR_FINGER_NOT_FOUND 3
#define OUT_MATCHES_ARTIFACTS 5
#define OUT_LOW_COMPLEXITY 6
#define N_OUTCOME_SLOTS 8
// Diagnostic counters (TDS_PROFILE, TDS_PRUNE_STATS, TDS_ENDSTATS) live in a tail of 64 words behind the 8 outcome + 256
// per-barcode counters the ABI reports (td_counts_get, the RCCL all-reduce): td_diag_get reads it.  Slot numbers 192..255
// are historical (the words once shared the per-barcode bins 192..255).
#define TDS_DIAG(k) (N_OUTCOME_SLOTS + 256 + ((k) - 192))

#ifndef TDS_LSUM_OOB
#define TDS_LSUM_OOB 1
#endif
#if TDS_LSUM_OOB
// logsum table in LDS, padded with zeros to 66 560 B (a whole number of LDS allocation granules, so that the table is
// the workgroup's entire allocation).  A look-up past the end is out of range for the LDS unit, which returns 0.
#define TDS_TABLE_N 16640
#else
// logsum table in LDS; slot [TD_LOGSUM_LIVE] holds 0 so that "return max" needs no select
#define TDS_TABLE_N (TD_LOGSUM_LIVE + 4)
#endif
// g_T must stay the ONLY __shared__ object of this translation unit: the clamp-free lsum() below relies on the table
// being the workgroup's whole LDS allocation, starting at LDS address 0 (td_spec_selfcheck verifies the behaviour it
// relies on every time a compiled kernel is loaded).
__shared__ float g_T[TDS_TABLE_N];

// logsum, src/misc.c:72-78.
DEV float lsum(float a, float b)
{
#if TDS_LSUM_OOB
	// 6 VALU + 1 ds_read_b32: sub, mul with |.| source modifier, cvt, and, max, add.  max - min == |a - b| bit for bit
	// (negation is exact).  The reference's "return max" for d >= 15.7 needs no clamp here: indices 15700..16639 hit the
	// zero padding, anything larger (d = +inf -> INT_MAX, address 0x7ffffffc) is out of LDS range and reads as 0, and
	// d = NaN (both operands -inf) converts to index 0, -inf + ln 2 = -inf.  The host only selects the clamp-free logsum
	// when the model's parameters and the batch's longest read bound every finite score difference far below 1e6
	// (td_api.hip, spec_lsum_range_ok).
	// (byte address = trunc(4000 |a - b|) with its two low bits cleared: 4000 x = 4 * (1000 x) exactly in floating point, so
	// that is 4 * trunc(1000 |a - b|) -- an AND of the fast issue class instead of a shift of the slow one, and a conversion
	// that saturates where a shift would wrap at index 2^30; -1 % on config 3)
	const float t = __builtin_fabsf(a - b) * 4000.0f;
	int idx;
	asm("v_cvt_i32_f32 %0, %1" : "=v"(idx) : "v"(t));
	const float tv = *(const float*)((const char*)g_T + ((unsigned)idx & ~3u));
	return fmaxf(a, b) + tv;
#else
	// 8 VALU + 1 ds_read_b32.  d = max-min; d >= 15.7f, d = +inf (min = -inf) and d = NaN (both -inf) all clamp
	// to 15.7f -> index 15700 -> + 0.0f, i.e. the reference's "return max"; below that (int)(d*1000.0f) <= 15699.
	// (measured on MI355X: max - min is 5 % faster than fabsf(a - b) as a source modifier on the clamp)
	const float mx = fmaxf(a, b);
	const float dc = fminf(mx - fminf(a, b), 15.7f);
	return mx + g_T[(int)(dc * 1000.0f)];
#endif
}

// A log-space value that may be *statically* known to be -inf (log 0).  After full unrolling `z` is a compile-time fact,
// so every fold whose accumulator or term is known-empty disappears: lsum(-inf, x) == x and lsum(x, -inf) == x bit for bit
// (max = x, |x - -inf| = inf -> table slot 0.0; x = -inf gives -inf either way).  This prunes the terms behind dead
// (-inf) model parameters *and* the first fold of every chain that starts from a dead entry probability, a dead delete
// state or an empty accumulator -- about a quarter of the forward pass's logsums.
struct SV { float v; bool z; };
DEV SV sv(float v) { SV r; r.v = v; r.z = false; return r; }
DEV SV sv_none() { SV r; r.v = NEG_INF; r.z = true; return r; }
#define LIVE(v) ((v) != NEG_INF)
DEV SV addc(const SV a, const float c) { SV r; r.z = a.z || !LIVE(c); r.v = r.z ? NEG_INF : a.v + c; return r; } // c: model constant
DEV SV addv(const SV a, const float x) { SV r; r.z = a.z; r.v = a.z ? NEG_INF : a.v + x; return r; }             // x: run-time value
DEV SV subv(const SV a, const float x) { SV r; r.z = a.z; r.v = a.z ? NEG_INF : a.v - x; return r; }
DEV SV lsum(const SV a, const SV b) { if (a.z) return b; if (b.z) return a; return sv(lsum(a.v, b.v)); }

// Two independent folds at once: both table look-ups are issued before either result is used, so a wave keeps two LDS
// round trips in flight instead of one (the compiler, left alone, serialises the chains under the register budget).
DEV void lsum2(SV& a0, const SV b0, SV& a1, const SV b1)
{
#if TDS_LSUM_OOB
	if (!a0.z && !b0.z && !a1.z && !b1.z) {
		const float t0 = __builtin_fabsf(a0.v - b0.v) * 4000.0f, t1 = __builtin_fabsf(a1.v - b1.v) * 4000.0f;
		int i0, i1;
		asm("v_cvt_i32_f32 %0, %1" : "=v"(i0) : "v"(t0));
		asm("v_cvt_i32_f32 %0, %1" : "=v"(i1) : "v"(t1));
		const float m0 = fmaxf(a0.v, b0.v), m1 = fmaxf(a1.v, b1.v);
		const float v0 = *(const float*)((const char*)g_T + ((unsigned)i0 & ~3u));
		const float v1 = *(const float*)((const char*)g_T + ((unsigned)i1 & ~3u));
		__builtin_amdgcn_sched_barrier(0);
		a0 = sv(m0 + v0);
		a1 = sv(m1 + v1);
		return;
	}
#endif
	a0 = lsum(a0, b0);
	a1 = lsum(a1, b1);
}

// ---------------------------------------------------------------------------------------------------------
// Interval arithmetic over the reference's operators, for the restarted sweeps (see "Restarted sweeps" below).
// An SI is a pair of floats that ENCLOSES the float the reference computes: lo <= value <= hi.  Float addition and the
// conversion chain of logsum's table index are monotone, the table decreases with its index, so
//   logsum(a, b) = max(a, b) + T[k(|a - b|)]   lies in   [max(a.lo, b.lo) + T[k(dmax)],  max(a.hi, b.hi) + T[k(dmin)]]
// with dmin / dmax the smallest / largest |a - b| over the two intervals.  The table form of logsum is NOT monotone in its
// operands (at an index boundary the result drops by up to 5e-4 while an operand rises by an ulp), which is why a pair of
// plain runs cannot bracket anything and the enclosure is formed per operation.  On degenerate intervals (lo == hi in both
// operands) both ends equal lsum(a, b) bit for bit: dmin = dmax = |a - b| (x - y and y - x are exact negatives; both -inf
// gives NaN -> index 0 -> -inf + ln 2 = -inf, like the plain form).
// ---------------------------------------------------------------------------------------------------------
struct SI { float lo, hi; bool z; };
DEV SI si(float lo, float hi) { SI r; r.lo = lo; r.hi = hi; r.z = false; return r; }
DEV SI si(float v) { return si(v, v); }
DEV SI si_none() { SI r; r.lo = NEG_INF; r.hi = NEG_INF; r.z = true; return r; }
DEV SI addc(const SI a, const float c) { SI r; r.z = a.z || !LIVE(c); r.lo = r.z ? NEG_INF : a.lo + c; r.hi = r.z ? NEG_INF : a.hi + c; return r; }
DEV SI addv(const SI a, const float x) { SI r; r.z = a.z; r.lo = a.z ? NEG_INF : a.lo + x; r.hi = a.z ? NEG_INF : a.hi + x; return r; }
// T[k(d)] for a difference d >= 0 (+inf: 0; NaN: T[0]) -- the table term of lsum() above, same instructions
DEV float lsum_term(const float d)
{
#if TDS_LSUM_OOB
	const float t = d * 4000.0f;
	int idx;
	asm("v_cvt_i32_f32 %0, %1" : "=v"(idx) : "v"(t));
	return *(const float*)((const char*)g_T + ((unsigned)idx & ~3u));
#else
	// (the clamped form: NaN -> fminf gives 15.7 -> T[15700] = 0, and -inf + 0 = -inf as well)
	return g_T[(int)(fminf(d, 15.7f) * 1000.0f)];
#endif
}
DEV SI lsum(const SI a, const SI b)
{
	if (a.z) return b;
	if (b.z) return a;
	const float dmin = fmaxf(fmaxf(a.lo - b.hi, b.lo - a.hi), 0.0f);   // 0 when the intervals overlap (fmaxf drops a NaN operand)
	const float dmax = fmaxf(a.hi - b.lo, b.hi - a.lo);
	return si(fmaxf(a.lo, b.lo) + lsum_term(dmax), fmaxf(a.hi, b.hi) + lsum_term(dmin));
}
DEV bool same(const SI a) { return a.lo == a.hi || (!(a.lo > NEG_INF) && !(a.hi > NEG_INF)); }

// Spilled backward rows: written once, read once, 20+ GB apart -- with the non-temporal hint (plain accesses measured 3 %
// slower; the hint on the posterior and silent rows as well changed nothing).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
DEV void st4(uint8_t* p, int lane, float a, float b, float c, float d)
{
	const f32x4 v = { a, b, c, d };
	__builtin_nontemporal_store(v, (f32x4*)p + lane);
}
DEV void st2(uint8_t* p, int lane, float a, float b)
{
	const f32x2 v = { a, b };
	__builtin_nontemporal_store(v, (f32x2*)p + lane);
}
DEV void st1(uint8_t* p, int lane, float a) { __builtin_nontemporal_store(a, (float*)p + lane); }
DEV float ld1(const uint8_t* p, int lane) { return __builtin_nontemporal_load((const float*)p + lane); }
DEV f32x4 ld4(const uint8_t* p, int lane) { return __builtin_nontemporal_load((const f32x4*)p + lane); }
DEV f32x2 ld2(const uint8_t* p, int lane) { return __builtin_nontemporal_load((const f32x2*)p + lane); }
// float number k of a lane's stride-byte record at p
DEV float ldk(const uint8_t* p, int lane, int stride, int k) { return __builtin_nontemporal_load((const float*)(p + lane * stride) + k); }
// Entry i of a host table that no kernel writes (the pruning bounds), i the same in every lane: a scalar load.  A vector load the
// wave waits for at once would also wait for every row requested ahead of it (the counter is in-order) -- it would undo the
// request rings of the sweeps.
DEV float uload(const float* tab, int i)
{
	typedef const __attribute__((address_space(4))) float* ctab;
	return ((ctab)(unsigned long long)tab)[__builtin_amdgcn_readfirstlane(i)];
}

struct BaseMask { bool m0, m1, m2, m3, m4; };
DEV BaseMask mk_mask(int x) { BaseMask k; k.m0 = x == 0; k.m1 = x == 1; k.m2 = x == 2; k.m3 = x == 3; k.m4 = x == 4; return k; }

// emission value for a per-lane base code given 5 compile-time constants: start from the value most of A,C,G,T
// share and patch the others in (masks are mutually exclusive).  Everything but the selects folds away.
DEV float emit(const float e0, const float e1, const float e2, const float e3, const float e4, const BaseMask& k)
{
	const int c0 = (e1 == e0) + (e2 == e0) + (e3 == e0);
	const int c1 = (e0 == e1) + (e2 == e1) + (e3 == e1);
	const int c2 = (e0 == e2) + (e1 == e2) + (e3 == e2);
	const int c3 = (e0 == e3) + (e1 == e3) + (e2 == e3);
	float lo = e0;
	int best = c0;
	if (c1 > best) { lo = e1; best = c1; }
	if (c2 > best) { lo = e2; best = c2; }
	if (c3 > best) { lo = e3; best = c3; }
	float r = lo;
	if (e0 != lo) r = k.m0 ? e0 : r;
	if (e1 != lo) r = k.m1 ? e1 : r;
	if (e2 != lo) r = k.m2 ? e2 : r;
	if (e3 != lo) r = k.m3 ? e3 : r;
	if (e4 != lo) r = k.m4 ? e4 : r;
	return r;
}
#define EMIT_M(col, k) emit(kCols[col].eM[0], kCols[col].eM[1], kCols[col].eM[2], kCols[col].eM[3], kCols[col].eM[4], k)
#define EMIT_I(col, k) emit(kCols[col].eI[0], kCols[col].eI[1], kCols[col].eI[2], kCols[col].eI[3], kCols[col].eI[4], k)
// Run-time HMM loop (segments with many HMMs, e.g. 96 barcodes): the HMMs [0, kRt[J]) of such a segment share every
// transition / entry / insert-emission parameter with HMM 0 and differ only in the base each match column expects, so
// one loop body (parameters = HMM 0's literals, base codes from kBase[]) serves them all instead of kRt[J] unrolled copies.
DEV float emit_rt(const int b, const float hi, const float lo, const float nv, const BaseMask& k, const int x)
{
	const float r = (x == b) ? hi : lo;
	return k.m4 ? nv : r;
}

// Diagnostic (TD_SPEC_PROFILE=1): per-phase wave clock sums in the diagnostic slots 240..251.  Phase k's share =
// slot[240+k] / sum.
#ifndef TDS_PROFILE
#define TDS_PROFILE 0
#endif
#define TDS_PHASE(k) do { if (TDS_PROFILE) { const long long t_ = (long long)__builtin_readcyclecounter(); \
	if (lane == 0) atomicAdd(&ka.counters[TDS_DIAG(240 + (k))], (unsigned long long)(t_ - tprof)); tprof = t_; } } while (0)

#ifndef TDS_WINDOW
#define TDS_WINDOW 0
#endif
// Posterior rows that are zero for every read of the tile (most barcode labels beyond the first positions, the adapter
// label before the last ones) are neither stored by the forward sweep nor loaded by the label DP: one bit per label and
// position (per wave) records which rows exist.  Only on the register path of the label DP.
constexpr bool kMaskDP = TD_H - kFirstN <= TDS_REG_H;

struct Wv {
	uint32_t* pmask;   // [TD_H][nwm] posterior-row bits
	int nwm;           // words per label = ceil(lmax / 32)
	uint8_t* slot;
	int lane, len, lmax, tmax, tmin;
	float* bm;      // running maximum of the first segment's label sums, per position (kFirstN > 0)
	uint8_t* ba;    // and the label that holds it
	// position pruning of the leading segments (kPruneSegs > 0), all wave-uniform:
	int cut;            // forward sweep: segments j < kPruneSegs are swept over positions 1..cut only (tmax: no pruning)
	int cutS;           // backward sweep: their rows are spilled for positions 1..cutS only (cut < cutS, or both tmax)
	const float* wa;    // check thresholds of the first unpruned segment, per position (host tables, td_jit.hip)
	const float* wb;
	// ... and of the trailing segments (kSfxFirst < TD_S):
	int sstop;          // forward sweep: segments j >= kSfxFirst fold no posteriors at positions i < sstop (1: everywhere)
	int sstopS;         // backward sweep: those segments are swept (and spilled) for positions i >= sstopS only (sstopS <= sstop)
	const float* wc;    // check thresholds of the read segment in front of them, per bases to go
	const float* wd;
	mutable int bad;    // per lane: checks that failed (bit 0: wa, 1: wb, 2: total_prob, 3: wc, 4: wd, 5: a restarted sweep did not close); the tile is then decoded again without pruning
	// restarted sweeps (TDS_RESTART): the leading segments' backward sweep takes over at cutS + J * (W + 1), the trailing
	// segments' forward sweep at sstop - (S - 1 - J) * (W + 1); the W positions before that are bridged in interval arithmetic
	bool rb_on, rf_on;
	float* rs;          // [2 * TD_C][64] hand-over rows (M, I) per column
	float* hb;          // [lmax + 2][64] staircase bridges: upper end of every row of the segment being bridged, by position (this lane's read)
	int rWf;            // ... and a forward bridge of the trailing segments (starts at TDS_RESTART_WF)
	int rW;             // positions a backward bridge is given (starts at TDS_RESTART_W; a wave whose bridges do not close widens it)
	const float* bwt;   // host bound tables (td_spec_prune_tables): backward values of the leading segments by bases to go,
	const float* fbs;   // forward values of the trailing segments by position
	unsigned long long* stats;   // the counter block (TDS_PRUNE_STATS)
	long long* tprof;            // TDS_PROFILE: the wave's phase clock (per-segment shares with TDS_PROFILE=2: slots 208 + J backward, 216 + J forward)
	const float* ptab;  // all host tables (stride pstride): 8 + j = impulse response of leading segment j, 12 + t of trailing segment kSfxFirst + t
	int pstride;
	const float* qr;    // silent_backward row in front of the first unpruned segment (swept densely: exact everywhere)
	const float* pr;    // silent_forward row the last read segment leaves (likewise)
};

// ---------------------------------------------------------------------------------------------------------
// Position pruning (kPruneSegs = number of leading segments it applies to, 0 = off; kSfxFirst = first trailing segment it
// applies to, TD_S = off).
//
// The segments in front of the first read segment (barcodes, spacers, UMIs, linkers) can only sit near the start of a
// read: a state of such a segment at position i needs i - (its columns) insertions, ~8 nats each, so far into the read
// its forward value is so small that (1) every posterior it takes part in narrows to exactly +0.0f
// (scaledprob2prob below -103.98, post_prob()), (2) every logsum that folds a value derived from it into the read
// segment's chain returns the other operand unchanged (the reference's logsum returns max(a, b) for |a - b| >= 15.7,
// src/misc.c:72-78).  Past such a position the forward sweep of those segments changes nothing the reference outputs --
// and the backward rows that only the forward sweep reads need not be spilled there.
//
// Nothing is assumed: the host states an upper bound on every forward value of those segments at position i that
// holds for ANY read (FB[i]: the same recurrence with every emission at its maximum and a slack per logsum for the table
// quantisation, td_spec_prune_tables) and on every backward value with m bases to go (BWB[m]); after the backward sweep,
// when b_score is known, the wave picks the smallest cut with FB[i] + BWB[len - i] - b < -103.98 - ln(terms) - margin for
// all i > cut and all of its 64 reads (fold of <= 2*columns terms, each below the bound).  total_prob of a multi-HMM
// segment drops terms below that bound, which is exact while the accumulated value is at least 15.7 above them (checked
// per lane).  The first unpruned segment -- a read segment: one column whose match state is unreachable, entered through
// its insert state -- runs past the cut with its entry term P[i-1] + sI (and skip term) at -inf (logsum(x, -inf) == x bit for
// bit) and checks per lane and position that the chain term it was folded with is >= 15.7 above the term's upper bound (wa[], wb[]).  Any failed
// check, a read without a valid path, or a spill cut that turns out too short makes the wave decode the tile again
// with cut = tmax: results are bit-identical by construction, pruning only ever removes work that cannot matter.
//
// The mirror image at the 3' end: the segments behind the last read segment (an adapter) can only sit at a read's end, far
// from it their BACKWARD values are tiny.  Their backward sweep stops at a position sstop (nothing downstream of it exists:
// the sweep runs towards the start of the read), the read segment in front of them runs below it with its exit term
// P_next[i+1] + ISKIP at -inf and the matching check (wc[], wd[]), and their forward sweep -- whose values are ordinary
// numbers and whose chain stays exact -- folds no posteriors and loads no spilled rows below sstop.  b_score is exact as soon
// as the read segment's checks hold (induction from the end of the read), so the stop is verified with it after the backward
// sweep; before it, it is guessed from the random-model score like the spill cut.  Only when every trailing segment has a
// single HMM.  Bound tables for both ends: td_spec_prune_tables (td_jit.hip), checked against the oracle's DP matrices in
// tests/test_prune.py.
// ---------------------------------------------------------------------------------------------------------
#ifndef TDS_LATE_CS
#define TDS_LATE_CS 1   // the last segment's silent_forward row is folded from the tile's shortest read on only (0: everywhere)
#endif
#ifndef TDS_PF_DIST
#define TDS_PF_DIST 4   // positions a light group of the sweeps requests its rows ahead (1: one position, as the heavy groups)
#endif
#ifndef TDS_PF_COLS
#define TDS_PF_COLS 2   // a group is light up to this many columns (HMMs x columns); 6 takes in config 3's spacer and costs +20 % in spills
#endif
#ifndef TDS_LDP
#define TDS_LDP 2   // positions the label DP / traceback request their rows ahead (a divisor of 32)
#endif
#ifndef TDS_LDT
#define TDS_LDT 4   // positions the traceback requests its path words ahead (a slot is PWL words: 4 costs 16 registers on config 3; round 4: 2 -> 4 is -3 % on config 3, 8 and 16 give less)
#endif
#ifndef TDS_SCAN_B
#define TDS_SCAN_B 8    // table entries the scans between the sweeps request together (one round trip per block; 16 measured 2 % slower on config 3: the registers)
#endif
#ifndef TDS_PRUNE_TT
#define TDS_PRUNE_TT (-88.0f)
#endif
#ifndef TDS_PRUNE_MARGIN
#define TDS_PRUNE_MARGIN 1   // positions the spill cut lies beyond the guessed cut
#endif
#ifndef TDS_PRUNE_BGAP
#define TDS_PRUNE_BGAP 5.0f  // the spill cut is taken for a backward score this far below the random-model score (round 4: 30 and a margin
                             // of 2 left ten positions between the spill cut and the cut the tile then needed on config 3, 41 against 31; 5 and 1
                             // leave six, and 0 / 0 is too short for every wave's first tile -- a wave whose guess fails adds 40 for its next tiles)
#endif
#ifndef TDS_PRUNE_STATS
#define TDS_PRUNE_STATS 0    // diagnostic: counter slots 194.. = restarted sweeps: forward bridges' interval steps, forward bridges, backward bridges' interval steps, backward bridges, tiles with a forward restart, tiles failing on a bridge in the forward sweep; 206, 207 = tiles with a backward restart, of those failing; 224.. = trailing: decisions, sum of required stops, fall-backs, sum of stops used; 228.. lanes failing wa / wb / total_prob; 232.. = leading: cut decisions, sum of required cuts, spill-too-short, failed checks, tiles, sum of cuts used, dense tiles, sum of spill cuts
#endif

constexpr int cmin(int a, int b) { return a < b ? a : b; }
// request distance of a group of the sweeps with `cols` columns in all (see bwd_group)
constexpr int pf_dist(int cols, bool rt) { return (!rt && cols <= TDS_PF_COLS) ? TDS_PF_DIST : 1; }
// A request ring of PD slots is walked in blocks of PD positions with the slot index a compile-time constant.  Whole blocks run
// as straight code: were each position guarded on its own, the copies of the step would be joined by branches, the slots would
// change registers from copy to copy, and the moves between them would wait for the very loads just issued.  The last, partial
// block follows once, position by position.   step(IC<slot>, position)
template <int D> struct IC { static constexpr int v = D; };
// label (= HMM) h belongs to a pruned leading segment: past the pruning cut it has no posterior row
constexpr bool label_leading(int h)
{
	for (int j = 0; j < kPruneSegs; j++) if (h >= kHmmOff[j] && h < kHmmOff[j] + kNHmm[j]) return true;
	return false;
}
template <int PD, int D, typename F>
DEV void ring_block(F& step, const int base)
{
	if constexpr (D < PD) { step(IC<D>{}, base + D); ring_block<PD, D + 1>(step, base); }
}
template <int PD, int D, typename F>
DEV void ring_rest(F& step, const int base, const int iend)
{
	if constexpr (D < PD - 1) { if (base + D <= iend) { step(IC<D>{}, base + D); ring_rest<PD, D + 1>(step, base, iend); } }
}

// ---------------------------------------------------------------------------------------------------------
// One backward step of one HMM: (M, I)_backward of every column at position i from the values at i+1.
// barcode_hmm.c:3518-3586 without the silent-state folds.
//   Mn, In: rows of position i+1;  Pn = P_backward_next[i+1];  kc / c: base x_{i+1};  kx / xi: base x_i
// ---------------------------------------------------------------------------------------------------------
template <int J, bool RT>
DEV void bwd_row(const int fa, const float (&Mn)[kNCol[J]], const float (&In)[kNCol[J]], const float Pn,
                 const BaseMask& kc, const int c, const BaseMask& kx, const int xi, SV (&Mc)[kNCol[J]], SV (&Ic)[kNCol[J]])
{
#define EM(gcol, mask, xval) (RT ? emit_rt(kBase[colr + (gcol)], kHi[J], kLo[J], kNv[J], mask, xval) : EMIT_M(col0 + (gcol), mask))
	constexpr int NC = kNCol[J];
	constexpr int K = NC - 1;
	const int col0 = kColOff[J] + (RT ? 0 : fa) * NC;   // parameters (HMM 0 stands for all in a run-time loop)
	const int colr = kColOff[J] + fa * NC;               // this HMM's own columns (base codes)
	(void)colr;
	SV Dp = sv_none();
	{   // last column, :3518-3543
		const int q = col0 + K;
		const SV M = addc(sv(Pn), kCols[q].t[7]);
		SV I = addc(sv(Pn), kCols[q].t[8]);
		I = lsum(I, addv(addc(sv(Mn[K]), kCols[q].t[4]), EM(K, kc, c)));
		I = lsum(I, addv(addc(sv(In[K]), kCols[q].t[3]), EMIT_I(q, kc)));
		Mc[K] = M; Ic[K] = I;
	}
#pragma unroll
	for (int g = K - 1; g >= 0; --g) { // :3544-3586
		const int q = col0 + g;
		const float epc = EM(g + 1, kc, c);
		const float eic = EMIT_I(q, kc);
		// the M- and the I-chain of a column are independent: their folds are issued in pairs, each chain in its own order
		SV M = addc(addv(sv(Mn[g + 1]), epc), kCols[q].t[0]);
		SV I = addv(addc(sv(In[g]), kCols[q].t[3]), eic);
		lsum2(M, addc(sv(Pn), kCols[q].t[7]), I, addc(sv(Pn), kCols[q].t[8]));
		lsum2(M, addc(addv(sv(In[g]), eic), kCols[q].t[1]), I, addv(addc(sv(Mn[g + 1]), kCols[q].t[4]), epc));
		SV D = addc(Dp, kCols[q].t[5]);
		lsum2(M, addc(Dp, kCols[q].t[2]), D, addc(addv(Mc[g + 1], EM(g + 1, kx, xi)), kCols[q].t[6]));
		Mc[g] = M; Ic[g] = I; Dp = D;
	}
#undef EM
}

// Columns GT .. GB of bwd_row() (GT == K: from the last column on; else Mc[GT + 1] -- this position's row of the column above --
// and Dp = D_backward[GT + 1][i] come in).  Dp leaves as D_backward[GB][i].  The same statements in the same order: a sweep that
// shares the trailing columns of several HMMs (below) computes them once with <K, K - SH> and each HMM's own with <K - SH - 1, 0>.
template <int J, bool RT, int GT, int GB>
DEV void bwd_cols(const int fa, const float (&Mn)[kNCol[J]], const float (&In)[kNCol[J]], const float Pn,
                  const BaseMask& kc, const int c, const BaseMask& kx, const int xi, SV (&Mc)[kNCol[J]], SV (&Ic)[kNCol[J]], SV& Dp)
{
#define EM(gcol, mask, xval) (RT ? emit_rt(kBase[colr + (gcol)], kHi[J], kLo[J], kNv[J], mask, xval) : EMIT_M(col0 + (gcol), mask))
	constexpr int NC = kNCol[J];
	constexpr int K = NC - 1;
	const int col0 = kColOff[J] + (RT ? 0 : fa) * NC;
	const int colr = kColOff[J] + fa * NC;
	(void)colr;
	if constexpr (GT == K) {   // last column, :3518-3543
		const int q = col0 + K;
		const SV M = addc(sv(Pn), kCols[q].t[7]);
		SV I = addc(sv(Pn), kCols[q].t[8]);
		I = lsum(I, addv(addc(sv(Mn[K]), kCols[q].t[4]), EM(K, kc, c)));
		I = lsum(I, addv(addc(sv(In[K]), kCols[q].t[3]), EMIT_I(q, kc)));
		Mc[K] = M; Ic[K] = I;
		Dp = sv_none();
	}
#pragma unroll
	for (int g = (GT == K ? K - 1 : GT); g >= GB; --g) { // :3544-3586
		const int q = col0 + g;
		const float epc = EM(g + 1, kc, c);
		const float eic = EMIT_I(q, kc);
		SV M = addc(addv(sv(Mn[g + 1]), epc), kCols[q].t[0]);
		SV I = addv(addc(sv(In[g]), kCols[q].t[3]), eic);
		lsum2(M, addc(sv(Pn), kCols[q].t[7]), I, addc(sv(Pn), kCols[q].t[8]));
		lsum2(M, addc(addv(sv(In[g]), eic), kCols[q].t[1]), I, addv(addc(sv(Mn[g + 1]), kCols[q].t[4]), epc));
		SV D = addc(Dp, kCols[q].t[5]);
		lsum2(M, addc(Dp, kCols[q].t[2]), D, addc(addv(Mc[g + 1], EM(g + 1, kx, xi)), kCols[q].t[6]));
		Mc[g] = M; Ic[g] = I; Dp = D;
	}
#undef EM
}

// ---------------------------------------------------------------------------------------------------------
// Restarted sweeps (TDS_RESTART).
//
// The backward values of the leading segments (barcodes, spacers, UMIs, linkers) are only *used* near the start of a read:
// by the forward sweep up to the pruning cut, and through the chain down to position 1 (b_score).  They are ordinary numbers
// everywhere, though, and position i is computed from position i + 1, so the dense sweep starts at the end of the read --
// 110 of 150 positions of config 3, a fifth of all logsums, only to arrive.  What carries a value of such an HMM from
// position i + 1 to position i?  The match chain leaves the HMM within its few columns; beyond that only the insert
// self-loops do (II + e_I, about -8.3 nats a step), every other term comes from the next segment's silent row, which is
// known exactly (the segments behind are swept densely or were restarted further out).  So a row's dependence on the rows
// n positions further on fades like e^(-8.3 n): after a few positions it is below the resolution of the table operator --
// the sweep can start ANYWHERE with ANY rows and arrives at the same floats.  Proving that for a given read is what the
// interval type is for: the sweep is started W positions early with the interval [-inf, host upper bound] in every row and
// run in interval arithmetic (SI), which encloses the reference's floats at every step; once lo == hi in every row the
// enclosure IS the reference's value, bit for bit, and the plain sweep takes over from there (the staircase bridges below
// run the intervals column by column).  Rows that have not
// closed after W positions fail the tile (w.bad bit 5): it is decoded again densely, like after any other failed check.
// Mirror image at the 3' end: the forward values of the trailing segments (the adapter) are only used from `sstop` on; their
// forward sweep starts W positions before it from [-inf, bound].  tests/test_prune.py forces both failure routes.
//
// Where the intervals start decides everything: from the absolute host bounds (bwb / fbs: any read, every emission at its
// maximum) the upper ends sit ~90 nats too high and need 16-27 positions to come down at 6.9 nats a position.  They start
// instead from bounds RELATIVE to a row the kernel knows exactly -- the silent row in front of the first unpruned segment, which
// is swept densely: a backward value is a sum over the position at which the path reaches that row, and the host states an
// impulse response gq_J[k] >= the weight of getting there after k more bases, for any read (td_jit.hip; tests/test_prune.py
// holds max_k (gq[k] + row[t + 1 + k]) + log(terms) against the oracle's matrices: a start below a true value would close on a
// wrong number).  With that the backward bridges of config 5 close after 12.9 positions on average (a 6-column match chain
// carries the excess undamped, then ~7 more), none later than 16.
//
// State of the measurement (round 3, DESIGN.md section 4): exact -- outputs identical on every test and on 2^20-read batches --
// and ON for models with 48 or more leading columns (td_spec_restart): config 5 (97 barcode HMMs, their bridges in the run-time
// HMM loop) 30.3 -> 27.0 ms per 2^18 reads, config 3 (nine barcode HMMs and a spacer) 19.1 -> 18.6 ms per 2^20.  OFF for config
// 2's eight 4-column HMMs: a bridge runs one HMM at a time, a single dependent chain without the interleaving the grouped
// sweeps live on, and there it costs more than the dense positions it replaces.  The forward restart of the trailing segments
// (TDS_RESTART_FWD) was off as well in round 3: a 13-column adapter needed ~27 positions of all-interval arithmetic to close.
// ---------------------------------------------------------------------------------------------------------
#ifndef TDS_RESTART
#define TDS_RESTART 0
#endif
#ifndef TDS_RESTART_W
#define TDS_RESTART_W 20   // positions a restarted sweep is given to close (config 5: 12.9 on average, none beyond 16; config 3: 12.3)
#endif
#ifndef TDS_RESTART_FWD
#define TDS_RESTART_FWD 1  // the trailing segments' forward sweep as well (round 4: on, as a staircase -- a 13-column adapter closes in 37 positions of a 44-position window; the all-interval bridge of round 3 needed 27 positions of all-interval arithmetic and lost)
#endif

// ---------------------------------------------------------------------------------------------------------
// Staircase bridges (round 4): the same certificate at a third of the cost of round 3's bridges, which treated every row of
// the HMM alike -- all 2 * columns rows intervals until the last one had closed (removed; see git history).  But the
// recurrence has structure: column g at position i reads column g + 1 (at i + 1 and at i), the silent row behind the segment,
// and ONE value of its own -- I_backward[g][i + 1], the insert self-loop (barcode_hmm.c:3544-3586: M_backward and
// D_backward of a column never read that column's own row).  So exactness spreads from the last column (which reads the silent
// row only) to the first, one column at a time, and at any position the columns fall into three classes:
//   * g >  gc: exact at position i + 1 -- computed in the reference's plain arithmetic, one table look-up per fold;
//   * g == gc: the "candidate": column gc + 1 is exact, its own rows are intervals that start as [-inf, bound] and enclose the
//              reference's floats (SI); as soon as both have closed in every lane the column is exact and gc - 1 takes over;
//   * g <  gc: not computed at all -- nothing that is computed reads them.
// Only one column per position pays for interval arithmetic, the columns above it cost what a dense position costs and the
// ones below cost nothing: config 3's barcode HMMs (five live columns, three positions per column to close) take ~270 logsum
// evaluations' worth per bridge instead of ~820, config 5's likewise.  The certificate is the one above, row by row: a
// candidate starts from an upper end that holds for every state of the segment at that position (bwd_stair_bounds: the
// relative bound, td_jit.hip "impulse responses"), and it is only ever declared exact when lo == hi bit for bit.
// A wave whose bridges do not close inside their window widens the window before it gives the restarts up (w.rW).
// ---------------------------------------------------------------------------------------------------------
#ifndef TDS_RESTART_WMAX
#define TDS_RESTART_WMAX 44   // widest bridge window a wave tries before it goes on without restarts
#endif
DEV SI to_si(const SV a) { return a.z ? si_none() : si(a.v); }

// Upper ends for the rows of positions p_lo + 1 .. p_hi + 1 of leading segment J (any state; this lane's read), into w.hb:
// max_k (gq_J[k] + Q[t + 1 + k]) + log(number of k) + 0.02 (td_jit.hip, "impulse responses"), at most the absolute bound.
template <int J>
DEV void bwd_stair_bounds(const Wv& w, const int p_lo, const int p_hi)
{
	const float* gq = w.ptab + (int64_t)(8 + J) * w.pstride;
	for (int t = p_hi + 1; t > p_lo; --t) {
		float hi = NEG_INF;
		for (int k0 = 0; t + 1 + k0 <= w.tmax + 1; k0 += TDS_SCAN_B) {
			float q[TDS_SCAN_B];
#pragma unroll
			for (int u = 0; u < TDS_SCAN_B; u++) {
				const int pos = t + 1 + k0 + u;
				q[u] = w.qr[(pos <= w.tmax + 1 ? pos : w.tmax + 1) * TD_WAVE + w.lane];
			}
			__builtin_amdgcn_sched_barrier(0);   // (the scheduler would otherwise pair each load with its use again)
#pragma unroll
			for (int u = 0; u < TDS_SCAN_B; u++) {
				const int pos = t + 1 + k0 + u;
				const float g = uload(gq, k0 + u);
				if (pos <= w.len + 1) hi = fmaxf(hi, g + q[u]);
			}
		}
		const bool live = w.len >= t;      // a read that ends before t has the -inf rows the dense sweep starts from there
		hi = hi + (__logf((float)(live ? w.len - t + 1 : 1)) + 0.02f);
		hi = fminf(hi, w.bwt[live ? w.len - t : 0]);
		w.hb[t * TD_WAVE + w.lane] = live ? hi : NEG_INF;
	}
}

// Upper bound on a chain of table logsums over n live terms whose largest is mx: the reference's logsum exceeds log(e^a + e^b) by
// less than 1e-3 (table indexed with the truncated difference, src/misc.c:72-78), so a chain of n - 1 of them stays below
// max + log(n) + (n - 1) * 1e-3; the relative part covers the float rounding of the additions that formed the terms (monotone,
// like the table conversion: a bound on the operands bounds the result).
DEV void ub_term(float& mx, int& n, const SV t) { if (!t.z) { mx = n ? fmaxf(mx, t.v) : t.v; n++; } }
DEV float ub_done(const float mx, const int n)
{
	if (n == 0) return NEG_INF;
	if (n == 1) return mx;
	const float lnn = (n == 2) ? 0.69320f : (n == 3) ? 1.09870f : 1.38640f;
	return mx + ((lnn + 1.0e-3f * (float)(n - 1)) + fminf(fabsf(mx), 1.0e30f) * 4.0e-7f);
}

// One position of one HMM whose columns above GC are exact (GC compile-time; -1: every column is).  barcode_hmm.c:3518-3586, the
// terms and their order as in bwd_row().  The rows of position i + 1 come in as intervals (Mlo / Mhi, Ilo / Ihi)
// and are replaced by those of position i; by column:
//   g > GC                    exact: lo == hi, the reference's plain arithmetic on lo;
//   GC >= g > GC - TDS_STAIR_WN    the window: interval arithmetic, enclosing the reference's floats (lo may still be -inf);
//   g <= GC - TDS_STAIR_WN         below the window: lo = -inf, hi an UPPER BOUND that follows the row down cheaply (max instead of
//                             logsum, the read's own emissions) -- the contamination from the unknown rows above the bridge fades
//                             through the insert self-loop at a few nats a position in every column at once, so a column enters
//                             the window within a few nats of the truth instead of at the any-read bound ~20 nats above it.
// Why a window and not one column: an interval has to shrink from ~1 nat to below the float spacing, at a factor e^-3 .. e^-8 a
// position (in the middle of a read a mismatch costs 4.2 nats, an insertion 8.3: the self-loop is never negligible) -- three to
// four positions per column if they ran one after the other, but the shrinking of column g - 1 can run beside that of column g.
// Two columns in the window close as fast as all of them (tools/stair_emu.py, the reference's own table on the CPU: 10.8 against
// 10.5 positions per read for six columns, 14.8 with a window of one).
#ifndef TDS_STAIR_WN
#define TDS_STAIR_WN 2
#endif
#ifndef TDS_STAIR_STATIC_COLS
#define TDS_STAIR_STATIC_COLS 8   // segments of up to this many columns get one straight instantiation per candidate column (config 5: -2 %)
#endif
// GC >= -1: the candidate column as a compile-time constant (one instantiation per value: straight code, short segments);
// GC == -2: the class of every column is decided at run time from `gcr` (wave-uniform branches around the three bodies: one
// instantiation whatever the number of columns -- the code of a 13- or 30-column segment would otherwise grow with its square).
template <int J, bool RT, int GC>
DEV void stair_step(const int gcr, const int fa, float (&Mlo)[kNCol[J]], float (&Mhi)[kNCol[J]], float (&Ilo)[kNCol[J]], float (&Ihi)[kNCol[J]],
                    const float Pn, const BaseMask& kc, const int c, const BaseMask& kx, const int xi)
{
#define EM(gcol, mask, xval) (RT ? emit_rt(kBase[colr + (gcol)], kHi[J], kLo[J], kNv[J], mask, xval) : EMIT_M(col0 + (gcol), mask))
	constexpr int NC = kNCol[J];
	constexpr int K = NC - 1;
	const int gcv = (GC == -2) ? gcr : GC;
	const int GW = gcv - TDS_STAIR_WN;   // columns g <= GW are below the window
	const int col0 = kColOff[J] + (RT ? 0 : fa) * NC;
	const int colr = kColOff[J] + fa * NC;
	(void)colr;
	SI Mc[NC], Ic[NC];   // rows of position i (exact columns: lo == hi; below the window: only hi means anything)
	SI Dp = si_none();   // D_backward[g + 1][i], likewise
	{   // last column, :3518-3543
		const int q = col0 + K;
		const SV M = addc(sv(Pn), kCols[q].t[7]);
		Mc[K] = to_si(M);
		if (K > gcv) {
			SV I = addc(sv(Pn), kCols[q].t[8]);
			I = lsum(I, addv(addc(sv(Mlo[K]), kCols[q].t[4]), EM(K, kc, c)));
			I = lsum(I, addv(addc(sv(Ilo[K]), kCols[q].t[3]), EMIT_I(q, kc)));
			Ic[K] = to_si(I);
		} else {
			SI I = addc(si(Pn), kCols[q].t[8]);
			I = lsum(I, addv(addc(si(Mlo[K], Mhi[K]), kCols[q].t[4]), EM(K, kc, c)));
			I = lsum(I, addv(addc(si(Ilo[K], Ihi[K]), kCols[q].t[3]), EMIT_I(q, kc)));
			Ic[K] = I;
		}
	}
#pragma unroll
	for (int g = K - 1; g >= 0; --g) { // :3544-3586
		const int q = col0 + g;
		const float epc = EM(g + 1, kc, c);
		const float eic = EMIT_I(q, kc);
		if (g > gcv) {
			SV M = addc(addv(sv(Mlo[g + 1]), epc), kCols[q].t[0]);
			SV I = addv(addc(sv(Ilo[g]), kCols[q].t[3]), eic);
			lsum2(M, addc(sv(Pn), kCols[q].t[7]), I, addc(sv(Pn), kCols[q].t[8]));
			lsum2(M, addc(addv(sv(Ilo[g]), eic), kCols[q].t[1]), I, addv(addc(sv(Mlo[g + 1]), kCols[q].t[4]), epc));
			SV Dx; Dx.z = Dp.z; Dx.v = Dp.lo;
			SV Mn1; Mn1.z = Mc[g + 1].z; Mn1.v = Mc[g + 1].lo;
			SV D = addc(Dx, kCols[q].t[5]);
			lsum2(M, addc(Dx, kCols[q].t[2]), D, addc(addv(Mn1, EM(g + 1, kx, xi)), kCols[q].t[6]));
			Mc[g] = to_si(M); Ic[g] = to_si(I); Dp = to_si(D);
		} else if (g > GW) {
			// in the window: the same terms in the same order over intervals (exact operands are degenerate intervals)
			const SI Mn1 = si(Mlo[g + 1], Mhi[g + 1]), In0 = si(Ilo[g], Ihi[g]);
			SI M = addc(addv(Mn1, epc), kCols[q].t[0]);
			SI I = addv(addc(In0, kCols[q].t[3]), eic);
			M = lsum(M, addc(si(Pn), kCols[q].t[7]));
			I = lsum(I, addc(si(Pn), kCols[q].t[8]));
			M = lsum(M, addc(addv(In0, eic), kCols[q].t[1]));
			I = lsum(I, addv(addc(Mn1, kCols[q].t[4]), epc));
			SI D = addc(Dp, kCols[q].t[5]);
			M = lsum(M, addc(Dp, kCols[q].t[2]));
			D = lsum(D, addc(addv(Mc[g + 1], EM(g + 1, kx, xi)), kCols[q].t[6]));
			Mc[g] = M; Ic[g] = I; Dp = D;
		} else {
			// below the window: upper bounds only
			SV Mup; Mup.z = false; Mup.v = Mhi[g + 1];       // M_backward[g + 1][i + 1]
			SV Iup; Iup.z = false; Iup.v = Ihi[g];           // I_backward[g][i + 1]
			SV Dup; Dup.z = Dp.z; Dup.v = Dp.hi;             // D_backward[g + 1][i]
			SV Mcu; Mcu.z = Mc[g + 1].z; Mcu.v = Mc[g + 1].hi;   // M_backward[g + 1][i]
			float mm = NEG_INF, mi = NEG_INF, md = NEG_INF;
			int nm = 0, ni = 0, nd = 0;
			ub_term(mm, nm, addc(addv(Mup, epc), kCols[q].t[0]));
			ub_term(mm, nm, addc(sv(Pn), kCols[q].t[7]));
			ub_term(mm, nm, addc(addv(Iup, eic), kCols[q].t[1]));
			ub_term(mm, nm, addc(Dup, kCols[q].t[2]));
			ub_term(mi, ni, addv(addc(Iup, kCols[q].t[3]), eic));
			ub_term(mi, ni, addc(sv(Pn), kCols[q].t[8]));
			ub_term(mi, ni, addv(addc(Mup, kCols[q].t[4]), epc));
			ub_term(md, nd, addc(Dup, kCols[q].t[5]));
			ub_term(md, nd, addc(addv(Mcu, EM(g + 1, kx, xi)), kCols[q].t[6]));
			Mc[g] = nm ? si(NEG_INF, ub_done(mm, nm)) : si_none();
			Ic[g] = ni ? si(NEG_INF, ub_done(mi, ni)) : si_none();
			Dp = nd ? si(NEG_INF, ub_done(md, nd)) : si_none();
		}
	}
#pragma unroll
	for (int g = 0; g < NC; g++) {
		Mlo[g] = Mc[g].z ? NEG_INF : Mc[g].lo; Mhi[g] = Mc[g].z ? NEG_INF : Mc[g].hi;
		Ilo[g] = Ic[g].z ? NEG_INF : Ic[g].lo; Ihi[g] = Ic[g].z ? NEG_INF : Ic[g].hi;
	}
#undef EM
}

template <int J, bool RT, int GC>
DEV void stair_dispatch(const int gc, const int fa, float (&Mlo)[kNCol[J]], float (&Mhi)[kNCol[J]], float (&Ilo)[kNCol[J]], float (&Ihi)[kNCol[J]],
                        const float Pn, const BaseMask& kc, const int c, const BaseMask& kx, const int xi)
{
	if constexpr (kNCol[J] > TDS_STAIR_STATIC_COLS) {
		stair_step<J, RT, -2>(gc, fa, Mlo, Mhi, Ilo, Ihi, Pn, kc, c, kx, xi);
	} else if constexpr (GC >= -1) {
		if (gc == GC) stair_step<J, RT, GC>(gc, fa, Mlo, Mhi, Ilo, Ihi, Pn, kc, c, kx, xi);
		else stair_dispatch<J, RT, GC - 1>(gc, fa, Mlo, Mhi, Ilo, Ihi, Pn, kc, c, kx, xi);
	}
}

// Bridge for one HMM of a leading segment: positions p_hi .. p_lo + 1; the rows of position p_lo + 1 go to w.rs.
template <int J, bool RT>
DEV void bwd_stair(const Wv& w, const uint8_t* __restrict__ codes, const float* __restrict__ P, const int fa, const int p_hi, const int p_lo)
{
	constexpr int NC = kNCol[J];
	constexpr int K = NC - 1;
	constexpr bool p_init = (J == TD_S - 1);
#define PBW(pos) (p_init ? (((pos) == w.len + 1) ? 0.0f : NEG_INF) : P[(pos) * TD_WAVE + w.lane])
	// every row of position p_hi + 1 is unknown, the last column's included (the silent row behind the segment exists up to
	// position p_hi + 1 only), and at most h: the first column to close is the last one, with its first step
	const float h = w.hb[(p_hi + 1) * TD_WAVE + w.lane];
	float Mlo[NC], Mhi[NC], Ilo[NC], Ihi[NC];
#pragma unroll
	for (int g = 0; g < NC; g++) { Mlo[g] = NEG_INF; Ilo[g] = NEG_INF; Mhi[g] = h; Ihi[g] = h; }
	int gc = K;              // (wave-uniform) the columns above gc are exact at position i + 1
	int c = codes[(p_hi + 1) * TD_WAVE + w.lane];
	float Pn = PBW(p_hi + 1);
	// (what the next position needs is requested a whole position ahead: a bridge is one dependent chain, and a load it waits for
	// at once costs it a round trip per position)
	int xi_n = codes[p_hi * TD_WAVE + w.lane];
	float Pi_n = PBW(p_hi);
	int i = p_hi;
	int closed_at = -1;      // steps the staircase took (statistics)
	auto close_check = [&](const int steps_done) __attribute__((always_inline)) {   // has column gc closed (in every lane)?
		if (gc >= 0) {
			bool cl = true;
#pragma unroll
			for (int g = 0; g < NC; g++) if (g == gc) cl = same(si(Mlo[g], Mhi[g])) && same(si(Ilo[g], Ihi[g]));
			if (__builtin_amdgcn_ballot_w64(!cl) == 0) { gc--; if (gc < 0) closed_at = steps_done; }
		}
	};
	for (; i > p_lo; --i) {
		const int xi = xi_n;
		const float Pi = Pi_n;
		{
			const int ip = (i - 1 >= 1) ? i - 1 : 1;
			xi_n = codes[ip * TD_WAVE + w.lane];
			Pi_n = PBW(ip);
		}
		close_check(p_hi - i); close_check(p_hi - i);
		if (i <= w.len) stair_dispatch<J, RT, K>(gc, fa, Mlo, Mhi, Ilo, Ihi, Pn, mk_mask(c), c, mk_mask(xi), xi);
		c = xi;
		Pn = Pi;
	}
	close_check(p_hi - p_lo); close_check(p_hi - p_lo);
	if (gc >= 0) w.bad |= 32;
	if (TDS_PRUNE_STATS && w.lane == 0) {
		const int st = closed_at >= 0 ? closed_at : p_hi - p_lo;
		atomicAdd(&w.stats[TDS_DIAG(196)], (unsigned long long)st); atomicAdd(&w.stats[TDS_DIAG(197)], 1ull);
		atomicMax(&w.stats[TDS_DIAG(193)], (unsigned long long)st);
	}
	float* rs = w.rs + (int64_t)(kColOff[J] + fa * NC) * 2 * TD_WAVE + w.lane;
#pragma unroll
	for (int g = 0; g < NC; g++) { rs[(2 * g) * TD_WAVE] = Mlo[g]; rs[(2 * g + 1) * TD_WAVE] = Ilo[g]; }
#undef PBW
}

template <int J, int F>
DEV void bwd_stair_rest(const Wv& w, const uint8_t* __restrict__ codes, const float* __restrict__ P, const int p_hi, const int p_lo)
{
	if constexpr (F < kNHmm[J]) {
		bwd_stair<J, false>(w, codes, P, F, p_hi, p_lo);
		bwd_stair_rest<J, F + 1>(w, codes, P, p_hi, p_lo);
	}
}

// One position of bwd_group's sweep as a macro, so that the sweep can run it in two loops (with and without the spill) as straight
// code: SPILL_ = the rows of this position are stored, WANT_CS_ = the silent row is folded.  (Comments: see the history of this
// file or the prose in bwd_group -- a macro body cannot carry them.)  Carried state: c, Pn, Mn, In and the request ring
// xi_q / Pi_q / cs_q (slot d_ holds position i and is refilled with position i - PD).
//   * below sstopS the silent row a segment leaves into was not computed (trailing pruned segments): its terms enter the folds
//     as -inf and the folds they would have gone through are checked against the host bounds (wc / wd);
//   * the loads of position i-PD are issued before position i is computed (software pipeline);
//   * silent-state folds column-descending, M term then I term (:3537-3541, :3578-3583), skip term once per HMM (:3600);
//   * spill: 8 B per column and lane, two columns per 16-byte store plus an 8-byte tail; column K-1 of a kDropM segment keeps
//     only its I_backward.
#define TDS_BWD_BOUNDS(d, pos) { const int k_ = w.len - (pos); wc_q[d] = w.wc[k_ >= 1 ? k_ - 1 : 0]; if (skip_live) wd_q[d] = w.wd[k_ >= 0 ? k_ : 0]; }
#define TDS_BWD_STEP(SPILL_, WANT_CS_) \
		const int xi = xi_q[d_]; \
		const bool tailb = sfx_nb && i < w.sstopS; \
		const float Pi = tailb ? NEG_INF : Pi_q[d_]; \
		if (tailb) Pn = NEG_INF; \
		SV cs; cs.v = cs_q[d_]; cs.z = RT ? false : first; \
		{ \
			const int ip = (i > PD) ? i - PD : 1; \
			xi_q[d_] = codes[ip * TD_WAVE + w.lane]; \
			Pi_q[d_] = p_init ? ((ip == w.len + 1) ? 0.0f : NEG_INF) : P[ip * TD_WAVE + w.lane]; \
			if (!first && (J > 0 || ip == 1)) cs_q[d_] = Cs[ip * TD_WAVE + w.lane]; \
			if (sfx_nb && ip < w.sstopS) { TDS_BWD_BOUNDS(d_, ip) } \
		} \
		const bool want_cs = (WANT_CS_) && !defer_cs; \
		if (i <= w.len) { \
			const BaseMask kc = mk_mask(c), kx = mk_mask(xi); \
_Pragma("unroll") \
			for (int f = 0; f < NF; f++) { \
				const int col0 = kColOff[J] + (RT ? 0 : FL(f)) * NC; \
				const int colr = kColOff[J] + FL(f) * NC; \
				(void)colr; \
				SV Mc[NC], Ic[NC]; \
				if (sfx_nb && tailb) { \
					const int q = col0 + K; \
					if (!((In[f][K] + kCols[q].t[3]) + EMIT_I(q, kc) >= wc_q[d_])) w.bad |= 8; \
				} \
				if constexpr (SHB == 0) { \
					bwd_row<J, RT>(FL(f), Mn[f], In[f], Pn, kc, c, kx, xi, Mc, Ic); \
				} else { \
					/* the HMMs of this group expect the same bases in their last SHB match columns: the rows of columns K - SHB .. K \
					   are the same floats in all of them -- computed with the first, taken over by the others */ \
					SV Dp_; \
					if (f == 0) { \
						bwd_cols<J, RT, K, K - SHB>(FL(f), Mn[f], In[f], Pn, kc, c, kx, xi, Mc, Ic, Dp_); \
_Pragma("unroll") \
						for (int g = K - SHB; g <= K; g++) { Msh[g] = Mc[g]; Ish[g] = Ic[g]; } \
						Dsh = Dp_; \
					} else { \
_Pragma("unroll") \
						for (int g = K - SHB; g <= K; g++) { Mc[g] = Msh[g]; Ic[g] = Ish[g]; } \
						Dp_ = Dsh; \
					} \
					bwd_cols<J, RT, K - SHB - 1, 0>(FL(f), Mn[f], In[f], Pn, kc, c, kx, xi, Mc, Ic, Dp_); \
				} \
				if (want_cs) { \
_Pragma("unroll") \
					for (int g = K; g >= 0; --g) { \
						const int q = col0 + g; \
						cs = lsum(cs, addv(addc(Mc[g], kCols[q].sM), EM(g, kx, xi))); \
						cs = lsum(cs, addv(addc(Ic[g], kCols[q].sI), EMIT_I(q, kx))); \
					} \
					if (sfx_nb && tailb && skip_live) { if (!(cs.v >= wd_q[d_])) w.bad |= 16; } \
					cs = lsum(cs, addc(sv(Pi), kSkip[J])); \
				} \
				if (SPILL_) { \
					uint8_t* bw = BW + ((int64_t)kBwOff[kHmmOff[J] + FL(f)] * w.lmax + (int64_t)(i - 1) * ROWH) * (TD_WAVE * 4); \
_Pragma("unroll") \
					for (int p = 0; p < NSF / 2; p++) \
						st4(bw + p * (TD_WAVE * 16), w.lane, Mc[2 * p].v, Ic[2 * p].v, Mc[2 * p + 1].v, Ic[2 * p + 1].v); \
					if (NSF & 1) st2(bw + (NSF / 2) * (TD_WAVE * 16), w.lane, Mc[NSF - 1].v, Ic[NSF - 1].v); \
					if (DM) st1(bw + NSF * (TD_WAVE * 8), w.lane, Ic[NS - 1].v); \
				} \
				if (defer_cs && i == 1) {   /* position 1's rows, for bwd_fold_first() */ \
					float* rs_ = w.rs + (int64_t)(kColOff[J] + FL(f) * NC) * 2 * TD_WAVE + w.lane; \
_Pragma("unroll") \
					for (int g = 0; g < NC; g++) { rs_[(2 * g) * TD_WAVE] = Mc[g].v; rs_[(2 * g + 1) * TD_WAVE] = Ic[g].v; } \
				} \
_Pragma("unroll") \
				for (int g = 0; g < NC; g++) { Mn[f][g] = Mc[g].v; In[f][g] = Ic[g].v; } \
			} \
			if (want_cs) Cs[i * TD_WAVE + w.lane] = cs.v; \
		} \
		c = xi; \
		Pn = Pi;

// ---------------------------------------------------------------------------------------------------------
// backward: NF HMMs (F0 .. F0+NF-1) of segment J in one sweep over the positions.  barcode_hmm.c:3505-3607
// ---------------------------------------------------------------------------------------------------------
// Trailing-column sharing (round 4, "trie" order): the rows of column g depend on the bases the columns g + 1 .. K expect, so HMMs
// that expect the same last bases have the same floats in their trailing columns.  A run-time-looped first segment (96 barcodes)
// is swept in SUFFIX order -- kTrieOrd: slot -> HMM -- in groups whose HMMs share their last SHB match columns (kTrieShare per
// group; the host forms the groups, td_jit.hip); those columns are computed once per group and position.  What makes the order
// free: a first segment's silent_backward row is read at position 1 only (b_score, :3610), so its folds -- whose order over the
// HMMs is fixed, :3537-3600 -- are deferred: every HMM leaves its rows of position 1 in w.rs and bwd_fold_first() folds them in
// HMM order afterwards.  Rows are still spilled per HMM (the forward sweep reads them in label order).
template <int J, int NF, bool RT, int SHB = 0>
DEV void bwd_group(const Wv& w, const uint8_t* __restrict__ codes, const float* __restrict__ P,
                   float* __restrict__ Cs, uint8_t* __restrict__ BW, const int f0)
{
	constexpr bool defer_cs = kTrieOn && (J == 0);    // (all groups of the segment, the unrolled ones behind the loop included)
	constexpr bool permuted = kTrieOn && (J == 0) && RT;
#define FL(f_) (permuted ? kTrieOrd[f0 + (f_)] : f0 + (f_))
	const bool first = (f0 == 0);
	SV Msh[kNCol[J]], Ish[kNCol[J]], Dsh = sv_none();   // the shared trailing columns' rows of this position (SHB > 0)
	(void)Msh; (void)Ish; (void)Dsh;
#define EM(gcol, mask, xval) (RT ? emit_rt(kBase[colr + (gcol)], kHi[J], kLo[J], kNv[J], mask, xval) : EMIT_M(col0 + (gcol), mask))
	constexpr int NC = kNCol[J];
	constexpr int K = NC - 1;
	constexpr int NS = NC - kPureLast[J]; // stored columns: a "pure" last column is Pn + const and is recomputed
	constexpr int DM = kDropM[J];         // 1: the last stored column (K-1) keeps only its I_backward
	constexpr int NSF = NS - DM;          // columns stored in full, 8 B per lane and position
	constexpr int ROWH = 2 * NS - DM;     // half-columns (4 B per lane) per HMM and position
	constexpr bool skip_live = LIVE(kSkip[J]);
	float Mn[NF][NC], In[NF][NC];
#pragma unroll
	for (int f = 0; f < NF; f++) {
#pragma unroll
		for (int g = 0; g < NC; g++) { Mn[f][g] = NEG_INF; In[f][g] = NEG_INF; }
	}
	if (TDS_RESTART && J < kPruneSegs && w.rb_on) {   // rows of position istart + 1, left by bwd_stair()
#pragma unroll
		for (int f = 0; f < NF; f++) {
			const float* rs = w.rs + (int64_t)(kColOff[J] + FL(f) * NC) * 2 * TD_WAVE + w.lane;
#pragma unroll
			for (int g = 0; g < NC; g++) { Mn[f][g] = rs[(2 * g) * TD_WAVE]; In[f][g] = rs[(2 * g + 1) * TD_WAVE]; }
		}
	}
	// Software pipeline: the loads of position i-1 are issued before position i is computed, so their latency
	// (and the in-order vmcnt behind this iteration's stores) never sits on the dependent chain.  Carried state is
	// updated by every lane: for a lane still above its read (i > len) x_i is 0 and P[len+1] is the initialised
	// entry, which is exactly what the first real step (i == len) must see.
	// The last segment's P is the initial previous_silent row (barcode_hmm.c:3476-3479: -inf, [len+1] = 0): its values are
	// known, so they are formed in registers instead of being written to and read from the workspace.
	constexpr bool p_init = (J == TD_S - 1);
#define PBW(pos) (p_init ? (((pos) == w.len + 1) ? 0.0f : NEG_INF) : P[(pos) * TD_WAVE + w.lane])
	// a leading segment whose far positions were bridged by bwd_stair() is swept from the hand-over position on
	const bool resumed = TDS_RESTART && (J < kPruneSegs) && w.rb_on;
	const int istart = resumed ? w.cutS + J * (w.rW + 1) : w.tmax;
	int c = resumed ? (int)codes[(istart + 1) * TD_WAVE + w.lane] : 0;   // x_{i+1} (0 past the end of the read)
	float Pn = PBW(istart + 1);                             // P[i+1]
	// A heavy group computes for longer than a memory round trip takes, so requesting position i-1 while position i is computed
	// hides it.  A light one (TDS_PF_COLS columns or fewer in all) does not: each of its positions would cost a whole round trip
	// to HBM (~1.5 us measured under load, several times its arithmetic), so it requests PD positions ahead, in a ring of PD
	// register slots addressed by the unrolled position index.
	constexpr int PD = pf_dist(NF * NC, RT);
	int xi_q[PD];
	float Pi_q[PD], cs_q[PD];
	float wc_q[PD], wd_q[PD];   // the host bounds the reduced form below sstopS is checked against (a lane's own entries)
	constexpr bool sfx_nb = (kSfxFirst < TD_S) && (J == kSfxFirst - 1);   // this segment leaves into the trailing segments
#pragma unroll
	for (int d = 0; d < PD; d++) {
		const int ip = (istart - d >= 1) ? istart - d : 1;
		xi_q[d] = codes[ip * TD_WAVE + w.lane];
		Pi_q[d] = PBW(ip);
		cs_q[d] = first ? NEG_INF : Cs[ip * TD_WAVE + w.lane];
		wc_q[d] = 0.0f; wd_q[d] = 0.0f;
		if (sfx_nb && ip < w.sstopS) { TDS_BWD_BOUNDS(d, ip) }
	}

	// trailing pruned segment: positions tmax .. sstopS; the read segment in front of them runs its reduced form below sstopS
	const int ilow = (J >= kSfxFirst) ? w.sstopS : 1;
	// One position of the group (TDS_BWD_STEP above).  The sweeps live off one long basic block per iteration that the
	// scheduler can interleave, so the positions whose rows are not spilled (past the spill cut of a pruned segment) run in a
	// loop of their own without the spill code instead of branching around it per HMM.  The first segment's silent row is only
	// folded where it is read, at position 1.  (The mirror image -- the last segment's silent_forward row is only read at each
	// read's last position -- was built too: its folds moved behind the column chain under one branch cost the forward sweep
	// more than they saved, 24.0 -> 26.8 ms.)
	if constexpr (PD > 1) {
		int base = istart;
		for (; base - (PD - 1) >= ilow; base -= PD) {   // whole blocks as straight code, then the partial one (see ring_block)
#pragma unroll
			for (int d_ = 0; d_ < PD; d_++) {
				const int i = base - d_;
				{ TDS_BWD_STEP((J >= kPruneSegs || i <= w.cutS || i == 1), ((J > 0) || i == 1)) }
			}
		}
#pragma unroll
		for (int d_ = 0; d_ < PD - 1; d_++) {
			const int i = base - d_;
			if (i >= ilow) { TDS_BWD_STEP((J >= kPruneSegs || i <= w.cutS || i == 1), ((J > 0) || i == 1)) }
		}
	} else {
		constexpr int d_ = 0;
		int i = istart;
		if (J < kPruneSegs) {
			for (; i > w.cutS && i >= 2 && i >= ilow; --i) { TDS_BWD_STEP(false, (J > 0)) }
		}
		for (; i >= ilow; --i) { TDS_BWD_STEP(true, ((J > 0) || i == 1)) }
	}
#undef EM
#undef PBW
#undef FL
}

// The deferred folds of a first segment swept in suffix order: silent_backward[1] (= b_score) from the rows of position 1 every HMM
// left in w.rs, HMM-ascending, column-descending, M term then I term, the skip term once per HMM -- barcode_hmm.c:3537-3541,
// :3578-3583, :3600 as TDS_BWD_STEP folds them.
template <int J, int F, bool RT>
DEV void fold_first_hmm(const Wv& w, const int fa, const int x1, const BaseMask& kx, const float Pi, SV& cs)
{
#define EM(gcol, mask, xval) (RT ? emit_rt(kBase[colr + (gcol)], kHi[J], kLo[J], kNv[J], mask, xval) : EMIT_M(col0 + (gcol), mask))
	constexpr int NC = kNCol[J];
	const int col0 = kColOff[J] + (RT ? 0 : fa) * NC;
	const int colr = kColOff[J] + fa * NC;
	(void)colr;
	const float* rs = w.rs + (int64_t)(kColOff[J] + fa * NC) * 2 * TD_WAVE + w.lane;
	float M[NC], I[NC];
#pragma unroll
	for (int g = 0; g < NC; g++) { M[g] = rs[(2 * g) * TD_WAVE]; I[g] = rs[(2 * g + 1) * TD_WAVE]; }
#pragma unroll
	for (int g = NC - 1; g >= 0; --g) {
		const int q = col0 + g;
		cs = lsum(cs, addv(addc(sv(M[g]), kCols[q].sM), EM(g, kx, x1)));
		cs = lsum(cs, addv(addc(sv(I[g]), kCols[q].sI), EMIT_I(q, kx)));
	}
	cs = lsum(cs, addc(sv(Pi), kSkip[J]));
#undef EM
}
template <int J, int F>
DEV void fold_first_rest(const Wv& w, const int x1, const BaseMask& kx, const float Pi, SV& cs)
{
	if constexpr (F < kNHmm[J]) {
		fold_first_hmm<J, F, false>(w, F, x1, kx, Pi, cs);
		fold_first_rest<J, F + 1>(w, x1, kx, Pi, cs);
	}
}
template <int J>
DEV void bwd_fold_first(const Wv& w, const uint8_t* __restrict__ codes, const float* __restrict__ P, float* __restrict__ Cs)
{
	if (w.len < 1) return;                          // (no position 1: b_score is not read)
	const int x1 = codes[1 * TD_WAVE + w.lane];
	const BaseMask kx = mk_mask(x1);
	constexpr bool p_init = (J == TD_S - 1);
	const float Pi = p_init ? ((1 == w.len + 1) ? 0.0f : NEG_INF) : P[1 * TD_WAVE + w.lane];
	SV cs; cs.v = NEG_INF; cs.z = false;            // (an empty accumulator: logsum(-inf, x) == x bit for bit)
	if constexpr (kRt[J] > 0) { for (int f = 0; f < kRt[J]; f++) fold_first_hmm<J, 0, true>(w, f, x1, kx, Pi, cs); }
	fold_first_rest<J, kRt[J]>(w, x1, kx, Pi, cs);
	Cs[1 * TD_WAVE + w.lane] = cs.v;
}

template <int J, int F0>
DEV void bwd_groups(const Wv& w, const uint8_t* __restrict__ codes, const float* __restrict__ P,
                    float* __restrict__ Cs, uint8_t* __restrict__ BW)
{
	if constexpr (TDS_RESTART && F0 == 0 && J < kPruneSegs) {
		if (w.rb_on) {   // bridge the positions between the end of the read and the hand-over, HMM by HMM
			const int p_lo = w.cutS + J * (w.rW + 1), p_hi = p_lo + w.rW;
			bwd_stair_bounds<J>(w, p_hi, p_hi);   // (the rows of position p_hi + 1)
			if constexpr (kRtB[J] > 0) { for (int f = 0; f < kRtB[J]; f++) bwd_stair<J, true>(w, codes, P, f, p_hi, p_lo); }
			bwd_stair_rest<J, kRtB[J]>(w, codes, P, p_hi, p_lo);
		}
	}
	if constexpr (F0 == 0 && kRt[J] > 0) {
		if constexpr (kTrieOn && J == 0) {
			// suffix order: the groups that share their last kTrieSH match columns first (kTrieNShare of them), the others behind
			for (int f0 = 0; f0 < kTrieNShare * kGroup[J]; f0 += kGroup[J]) bwd_group<J, kGroup[J], true, kTrieSH>(w, codes, P, Cs, BW, f0);
			for (int f0 = kTrieNShare * kGroup[J]; f0 < kRt[J]; f0 += kGroup[J]) bwd_group<J, kGroup[J], true>(w, codes, P, Cs, BW, f0);
		} else {
			for (int f0 = 0; f0 < kRt[J]; f0 += kGroup[J]) bwd_group<J, kGroup[J], true>(w, codes, P, Cs, BW, f0);
		}
		bwd_groups<J, kRt[J]>(w, codes, P, Cs, BW);
	} else if constexpr (F0 < kNHmm[J]) {
		constexpr int NF = cmin(kGroup[J], kNHmm[J] - F0);
		bwd_group<J, NF, false>(w, codes, P, Cs, BW, F0);
		bwd_groups<J, F0 + NF>(w, codes, P, Cs, BW);
	} else if constexpr (kTrieOn && J == 0) {
		bwd_fold_first<J>(w, codes, P, Cs);          // every HMM of the segment has left its rows of position 1
	}
}

template <int J>
DEV void bwd_segments(const Wv& w, const uint8_t* __restrict__ codes, float* __restrict__ SB, int rowlen,
                      uint8_t* __restrict__ BW)
{
	if constexpr (J >= 0) {
		bwd_groups<J, 0>(w, codes, SB + (int64_t)(J + 1) * rowlen, SB + (int64_t)J * rowlen, BW);
		if (TDS_PROFILE == 2 && J < 8) { const long long t_ = (long long)__builtin_readcyclecounter(); if (w.lane == 0) atomicAdd(&w.stats[TDS_DIAG(208 + J)], (unsigned long long)(t_ - *w.tprof)); *w.tprof = t_; }
		bwd_segments<J - 1>(w, codes, SB, rowlen, BW);
	}
}

// ---------------------------------------------------------------------------------------------------------
// forward + posterior accumulation.  barcode_hmm.c:4213-4344, :4431-4440
// ---------------------------------------------------------------------------------------------------------
DEV float post_prob(float lp)
{
	// scaledprob2prob (src/misc.c:98-105): (float) exp((double) lp).  For lp < -103.98 the double result is
	// below 2^-150 and narrows to +0.0f, so the exp is skipped there (and for -inf).
	float p = 0.0f;
	if (lp > -103.98f) p = (float)exp((double)lp);
	return p;
}

// ---------------------------------------------------------------------------------------------------------
// Forward staircase (round 4): the mirror image of bwd_stair for the single HMM of a trailing segment (the 3' adapter).  Its
// forward rows are only used from position sstop on; the sweep starts `w.rWf` positions before that from unknown rows.  Column g
// at position i reads column g - 1 (at i - 1 and at i), the silent row in front of the segment, and its own rows of position i - 1
// only through the insert state (I[g][i] takes I[g][i-1] and M[g][i-1]; M[g][i] and D[g][i] read column g - 1 alone,
// barcode_hmm.c:4271-4334) -- exactness spreads from column 0 upwards: columns below GC exact (plain arithmetic), a window of
// TDS_STAIR_WN columns in interval arithmetic, the columns above as upper bounds that follow their rows along.
// ---------------------------------------------------------------------------------------------------------
#ifndef TDS_STAIR_WNF
#define TDS_STAIR_WNF TDS_STAIR_WN   // columns in the forward staircase's interval window
#endif
#ifndef TDS_RESTART_WF
#define TDS_RESTART_WF 0    // positions a forward bridge is given; 0: three per column + 5
#endif
constexpr int fwd_window_all()
{
	int wmax = 1;
	if constexpr (kSfxFirst < TD_S) { for (int j = kSfxFirst; j < TD_S; j++) { const int wj = TDS_RESTART_WF > 0 ? TDS_RESTART_WF : 3 * kNCol[j] + 5; if (wj > wmax) wmax = wj; } }
	return wmax;
}

template <int J, int GC>   // GC == -2: classes decided at run time from gcr (see stair_step)
DEV void fstair_step(const int gcr, float (&Mlo)[kNCol[J]], float (&Mhi)[kNCol[J]], float (&Ilo)[kNCol[J]], float (&Ihi)[kNCol[J]], const float Pm, const BaseMask& kc)
{
	constexpr int NC = kNCol[J];
	constexpr int col0 = kColOff[J];
	const int gcv = (GC == -2) ? gcr : GC;
	const int GW = gcv + TDS_STAIR_WNF;  // columns g >= GW are above the window
	SI Mc[NC], Ic[NC];
	SI Dc = si_none();
#pragma unroll
	for (int g = 0; g < NC; ++g) {
		const int q = col0 + g, qp = q - 1;
		const float em = EMIT_M(q, kc), ei = EMIT_I(q, kc);
		if (g < gcv) {
			// exact: plain values
			SV M = addc(sv(Pm), kCols[q].sM);
			SV I = addc(sv(Pm), kCols[q].sI);
			SV Dx; Dx.z = Dc.z; Dx.v = Dc.lo;
			SV D = sv_none();
			if (g > 0) {
				SV Ml; Ml.z = false; Ml.v = Mlo[g - 1];
				SV Il; Il.z = false; Il.v = Ilo[g - 1];
				lsum2(M, addc(Ml, kCols[qp].t[0]), I, addc(sv(Ilo[g]), kCols[q].t[3]));
				lsum2(M, addc(Il, kCols[qp].t[4]), I, addc(sv(Mlo[g]), kCols[q].t[1]));
				SV Mcl; Mcl.z = Mc[g - 1].z; Mcl.v = Mc[g - 1].lo;
				D = addc(Mcl, kCols[qp].t[2]);
				lsum2(M, addc(Dx, kCols[qp].t[6]), D, addc(Dx, kCols[qp].t[5]));
			} else {
				I = lsum(I, addc(sv(Ilo[0]), kCols[q].t[3]));
				I = lsum(I, addc(sv(Mlo[0]), kCols[q].t[1]));
			}
			M = addv(M, em); I = addv(I, ei);
			Mc[g] = to_si(M); Ic[g] = to_si(I); Dc = to_si(D);
		} else if (g < GW) {
			SI M = addc(si(Pm), kCols[q].sM);
			SI I = addc(si(Pm), kCols[q].sI);
			SI D = si_none();
			const SI Io = si(Ilo[g], Ihi[g]), Mo = si(Mlo[g], Mhi[g]);
			if (g > 0) {
				const SI Ml = si(Mlo[g - 1], Mhi[g - 1]), Il = si(Ilo[g - 1], Ihi[g - 1]);
				M = lsum(M, addc(Ml, kCols[qp].t[0])); I = lsum(I, addc(Io, kCols[q].t[3]));
				M = lsum(M, addc(Il, kCols[qp].t[4])); I = lsum(I, addc(Mo, kCols[q].t[1]));
				D = addc(Mc[g - 1], kCols[qp].t[2]);
				M = lsum(M, addc(Dc, kCols[qp].t[6])); D = lsum(D, addc(Dc, kCols[qp].t[5]));
			} else {
				I = lsum(I, addc(Io, kCols[q].t[3]));
				I = lsum(I, addc(Mo, kCols[q].t[1]));
			}
			M = addv(M, em); I = addv(I, ei);
			Mc[g] = M; Ic[g] = I; Dc = D;
		} else {
			// above the window: upper bounds (g >= 1 here: column 0 is in the first window)
			SV Ml; Ml.z = false; Ml.v = Mhi[g - 1];
			SV Il; Il.z = false; Il.v = Ihi[g - 1];
			SV Io; Io.z = false; Io.v = Ihi[g];
			SV Mo; Mo.z = false; Mo.v = Mhi[g];
			SV Du; Du.z = Dc.z; Du.v = Dc.hi;
			SV Mcu; Mcu.z = Mc[g - 1].z; Mcu.v = Mc[g - 1].hi;
			float mm = NEG_INF, mi = NEG_INF, md = NEG_INF;
			int nm = 0, ni = 0, nd = 0;
			ub_term(mm, nm, addc(sv(Pm), kCols[q].sM));
			ub_term(mm, nm, addc(Ml, kCols[qp].t[0]));
			ub_term(mm, nm, addc(Il, kCols[qp].t[4]));
			ub_term(mm, nm, addc(Du, kCols[qp].t[6]));
			ub_term(mi, ni, addc(sv(Pm), kCols[q].sI));
			ub_term(mi, ni, addc(Io, kCols[q].t[3]));
			ub_term(mi, ni, addc(Mo, kCols[q].t[1]));
			ub_term(md, nd, addc(Mcu, kCols[qp].t[2]));
			ub_term(md, nd, addc(Du, kCols[qp].t[5]));
			// (the emission is added to the fold's result, :4287 / :4313: one more rounding, inside ub_done's relative slack)
			Mc[g] = nm ? si(NEG_INF, ub_done(mm, nm) + em) : si_none();
			Ic[g] = ni ? si(NEG_INF, ub_done(mi, ni) + ei) : si_none();
			Dc = nd ? si(NEG_INF, ub_done(md, nd)) : si_none();
		}
	}
#pragma unroll
	for (int g = 0; g < NC; g++) {
		Mlo[g] = Mc[g].z ? NEG_INF : Mc[g].lo; Mhi[g] = Mc[g].z ? NEG_INF : Mc[g].hi;
		Ilo[g] = Ic[g].z ? NEG_INF : Ic[g].lo; Ihi[g] = Ic[g].z ? NEG_INF : Ic[g].hi;
	}
}

template <int J, int GC>
DEV void fstair_dispatch(const int gc, float (&Mlo)[kNCol[J]], float (&Mhi)[kNCol[J]], float (&Ilo)[kNCol[J]], float (&Ihi)[kNCol[J]], const float Pm, const BaseMask& kc)
{
	if constexpr (kNCol[J] > TDS_STAIR_STATIC_COLS) {
		fstair_step<J, -2>(gc, Mlo, Mhi, Ilo, Ihi, Pm, kc);
	} else if constexpr (GC <= kNCol[J]) {
		if (gc == GC) fstair_step<J, GC>(gc, Mlo, Mhi, Ilo, Ihi, Pm, kc);
		else fstair_dispatch<J, GC + 1>(gc, Mlo, Mhi, Ilo, Ihi, Pm, kc);
	}
}

// Bridge for a trailing segment (one HMM): positions q_lo .. q_hi - 1 from unknown rows at q_lo - 1; the rows of position q_hi - 1
// go to w.rs.  Every read of the tile reaches q_hi (q_hi <= sstop <= the tile's shortest read).
template <int J>
DEV void fwd_stair(const Wv& w, const uint8_t* __restrict__ codes, const float* __restrict__ P, const int q_lo, const int q_hi)
{
	constexpr int NC = kNCol[J];
	// every row of position t = q_lo - 1 is at most max_k (gf_J[k] + PR[t - k]) + log(number of k), and at most the absolute bound
	float hi0 = NEG_INF;
	{
		const float* gf = w.ptab + (int64_t)(12 + J - kSfxFirst) * w.pstride;
		const int t = q_lo - 1;
		for (int k0 = 1; k0 <= t; k0 += 8) {
			float pr[8];
#pragma unroll
			for (int u = 0; u < 8; u++) { const int k = k0 + u; pr[u] = w.pr[((k <= t) ? t - k : 0) * TD_WAVE + w.lane]; }
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int u = 0; u < 8; u++) { const int k = k0 + u; if (k <= t) hi0 = fmaxf(hi0, uload(gf, k) + pr[u]); }
		}
		hi0 = fminf(hi0 + (__logf((float)(t > 1 ? t : 1)) + 0.02f), w.fbs[t]);
	}
	float Mlo[NC], Mhi[NC], Ilo[NC], Ihi[NC];
#pragma unroll
	for (int g = 0; g < NC; g++) { Mlo[g] = NEG_INF; Ilo[g] = NEG_INF; Mhi[g] = hi0; Ihi[g] = hi0; }
	int gc = 0;              // (wave-uniform) the columns below gc are exact at position i - 1
	int closed_at = -1;
	auto close_check = [&](const int steps_done) __attribute__((always_inline)) {
		if (gc < NC) {
			bool cl = true;
#pragma unroll
			for (int g = 0; g < NC; g++) if (g == gc) cl = same(si(Mlo[g], Mhi[g])) && same(si(Ilo[g], Ihi[g]));
			if (__builtin_amdgcn_ballot_w64(!cl) == 0) { gc++; if (gc == NC) closed_at = steps_done; }
		}
	};
	int c_n = codes[q_lo * TD_WAVE + w.lane];
	float Pm_n = P[(q_lo - 1) * TD_WAVE + w.lane];
	for (int i = q_lo; i < q_hi; ++i) {
		const int c = c_n;
		const float Pm = Pm_n;
		{   // (requested a position ahead: the bridge is one dependent chain)
			const int ip = (i + 1 < q_hi) ? i + 1 : i;
			c_n = codes[ip * TD_WAVE + w.lane];
			Pm_n = P[(ip - 1) * TD_WAVE + w.lane];
		}
		close_check(i - q_lo); close_check(i - q_lo);
		fstair_dispatch<J, 0>(gc, Mlo, Mhi, Ilo, Ihi, Pm, mk_mask(c));
	}
	close_check(q_hi - q_lo); close_check(q_hi - q_lo);
	if (gc < NC) w.bad |= 32;
	if (TDS_PRUNE_STATS && w.lane == 0) {
		const int st = closed_at >= 0 ? closed_at : q_hi - q_lo;
		atomicAdd(&w.stats[TDS_DIAG(194)], (unsigned long long)st); atomicAdd(&w.stats[TDS_DIAG(195)], 1ull);
		atomicMax(&w.stats[TDS_DIAG(192)], (unsigned long long)st);
	}
	float* rs = w.rs + (int64_t)kColOff[J] * 2 * TD_WAVE + w.lane;
#pragma unroll
	for (int g = 0; g < NC; g++) { rs[(2 * g) * TD_WAVE] = Mlo[g]; rs[(2 * g + 1) * TD_WAVE] = Ilo[g]; }
}

template <int J, int NF, bool RT>
DEV void fwd_group(const Wv& w, const uint8_t* __restrict__ codes, const float* __restrict__ P,
                   float* __restrict__ Cs, const float* __restrict__ PB, const uint8_t* __restrict__ BW,
                   float* __restrict__ DP, float* __restrict__ TOTAL, const float b, const int f0)
{
	const bool first = (f0 == 0);
#define EM(gcol, mask, xval) (RT ? emit_rt(kBase[colr + (gcol)], kHi[J], kLo[J], kNv[J], mask, xval) : EMIT_M(col0 + (gcol), mask))
	constexpr int NC = kNCol[J];
	constexpr int K = NC - 1;
	constexpr bool pure = kPureLast[J] != 0;
	constexpr int NS = NC - kPureLast[J];
	constexpr int DM = kDropM[J];         // 1: column K-1 was spilled without its M_backward
	constexpr int NSF = NS - DM;
	constexpr int ROWH = 2 * NS - DM;
	constexpr int NQ = NSF / 2;           // float4 loads per HMM and position
	constexpr int NT = NSF & 1;           // float2 tail
	constexpr bool skip_live = LIVE(kSkip[J]);
	float Mp[NF][NC], Ip[NF][NC], tot[NF];
#pragma unroll
	for (int f = 0; f < NF; f++) {
		tot[f] = NEG_INF;
#pragma unroll
		for (int g = 0; g < NC; g++) { Mp[f][g] = NEG_INF; Ip[f][g] = NEG_INF; }
	}
	if (TDS_RESTART && J >= kSfxFirst && w.rf_on) {   // rows of position i0 - 1, left by fwd_stair() (one HMM: NF == 1)
		const float* rs = w.rs + (int64_t)kColOff[J] * 2 * TD_WAVE + w.lane;
#pragma unroll
		for (int g = 0; g < NC; g++) { Mp[0][g] = rs[(2 * g) * TD_WAVE]; Ip[0][g] = rs[(2 * g + 1) * TD_WAVE]; }
	}
	// Base code and silent rows are fetched one position ahead (software pipeline as in bwd_group).  The spilled backward
	// rows of position i are requested at the top of iteration i and first used after the HMM's column chain (which does
	// not need them), so their latency hides behind that chain without a register double buffer (measured +3 % over
	// prefetching them a whole position ahead: fewer live registers, fewer spills).
	// The first segment's P is the initial previous_silent row (barcode_hmm.c:4191-4196: [0] = 0, -inf elsewhere): formed in
	// registers, never stored.
	constexpr bool p_init = (J == 0);
	// a trailing segment whose early positions were bridged by fwd_stair() is swept from the hand-over position on
	const bool resumed = TDS_RESTART && (J >= kSfxFirst) && w.rf_on;
	const int i0 = resumed ? w.sstop - (TD_S - 1 - J) * (w.rWf + 1) : 1;
	float Pm = p_init ? 0.0f : P[(i0 - 1) * TD_WAVE + w.lane]; // P[i-1], carried
	// request ring as in bwd_group: slot d holds what position i needs and is refilled with position i + PD.  With PD == 1 that
	// is "one position ahead" and the spilled backward rows are requested at the top of their own iteration (see above); a light
	// group has no column chain to hide them behind and requests them PD positions ahead with the rest.
	constexpr int PD = pf_dist(NF * NC, RT);
	const int pmax = (w.tmax >= 1) ? w.tmax : 1;
	int c_q[PD];
	float Pi_q[PD], cs_q[PD], pb_q[PD], bm_q[PD], ik_q[PD][NF];
	int ba_q[PD];
	float MB_q[PD][NF][NSF + 1], IB_q[PD][NF][NSF + 1];   // PD > 1: the spilled rows, float by float (one whose value is never used
	                                                       // then costs no load, and no register is overwritten under a pending one)
	// P_backward_next of the last segment is the initial previous_silent row of the backward pass: formed, not loaded
	constexpr bool pb_init = (J == TD_S - 1);
#define PBR(pos) (pb_init ? (((pos) == w.len + 1) ? 0.0f : NEG_INF) : PB[(pos) * TD_WAVE + w.lane])
#define BWROW(f_, pos_) (BW + ((int64_t)kBwOff[kHmmOff[J] + f0 + (f_)] * w.lmax + (int64_t)((pos_) - 1) * ROWH) * (TD_WAVE * 4))
	// what position p needs, into slot d (p clamped to the tile's positions: a slot past the end is filled but never used)
#define TDS_FWD_FILL(d, p_raw) { \
		const int p_ = ((p_raw) <= pmax) ? (p_raw) : pmax; \
		c_q[d] = codes[p_ * TD_WAVE + w.lane]; \
		Pi_q[d] = p_init ? NEG_INF : P[p_ * TD_WAVE + w.lane]; \
		if (!first) cs_q[d] = Cs[p_ * TD_WAVE + w.lane]; \
		if (pure) pb_q[d] = PBR(p_ + 1); \
		if (own_sum && !first) { bm_q[d] = w.bm[p_ * TD_WAVE + w.lane]; ba_q[d] = w.ba[p_ * TD_WAVE + w.lane]; } \
		const bool rows_ = !((J >= kSfxFirst) && p_ < w.sstop);   /* wave-uniform: below sstop the rows were not computed */ \
_Pragma("unroll") \
		for (int f = 0; f < NF; f++) { \
			if (DM && rows_) ik_q[d][f] = ld1(BWROW(f, p_) + NSF * (TD_WAVE * 8), w.lane); \
			if (PD > 1 && rows_) { \
_Pragma("unroll") \
				for (int q = 0; q < NQ; q++) { \
					MB_q[d][f][2 * q] = ldk(BWROW(f, p_) + q * (TD_WAVE * 16), w.lane, 16, 0); IB_q[d][f][2 * q] = ldk(BWROW(f, p_) + q * (TD_WAVE * 16), w.lane, 16, 1); \
					MB_q[d][f][2 * q + 1] = ldk(BWROW(f, p_) + q * (TD_WAVE * 16), w.lane, 16, 2); IB_q[d][f][2 * q + 1] = ldk(BWROW(f, p_) + q * (TD_WAVE * 16), w.lane, 16, 3); \
				} \
				if (NT) { MB_q[d][f][NSF - 1] = ldk(BWROW(f, p_) + NQ * (TD_WAVE * 16), w.lane, 8, 0); IB_q[d][f][NSF - 1] = ldk(BWROW(f, p_) + NQ * (TD_WAVE * 16), w.lane, 8, 1); } \
			} \
		} \
	}
	// Labels without predecessors (the first segment, kFirstN > 0): the label DP of such a label is the running sum of
	// its posteriors (:4447-4472 with an empty predecessor set: "stay" always wins), formed here instead of storing the
	// posteriors; later labels and the termination need only the first maximum over these sums, folded label-ascending
	// across the groups of the segment into one row (value + label).
	constexpr bool own_sum = (J == 0) && (kFirstN > 0);
	float lacc[NF];
	uint32_t mbits[NF];   // wave-uniform: posterior-row bits of the current block of 32 positions
#pragma unroll
	for (int f = 0; f < NF; f++) { lacc[f] = 0.0f; mbits[f] = 0u; }
	// I_backward of column K-1 (kDropM) travels in the ring too: the slot of position i serves the posterior fold of that position
	// and, one iteration earlier (as "the next position's"), the recomputation of M_backward[K-1]
#pragma unroll
	for (int d = 0; d < PD; d++) {
		cs_q[d] = NEG_INF; pb_q[d] = 0.0f; bm_q[d] = -1.0f; ba_q[d] = 0;
#pragma unroll
		for (int f = 0; f < NF; f++) ik_q[d][f] = NEG_INF;
		TDS_FWD_FILL(d, i0 + d)
	}

	// pruned segment: positions 1..cut; the first unpruned segment runs its reduced form ("tail") from cut + 1 on
	const int iend = (J < kPruneSegs && w.cut < w.tmax) ? w.cut : w.tmax;
	const int itail = (J == kPruneSegs && kPruneSegs > 0) ? w.cut + 1 : w.tmax + 1;
	(void)itail;
	if (i0 > 1 && kMaskDP && !own_sum) {   // posterior rows before the start: none exists
#pragma unroll
		for (int f = 0; f < NF; f++) {
			if (w.lane == 0) for (int wd = 0; wd < ((i0 - 1) >> 5); wd++) w.pmask[(kHmmOff[J] + f0 + f) * w.nwm + wd] = 0u;
			mbits[f] = 0u;
		}
	}
	auto step_cs = [&](auto dtag, auto cstag, const int i) __attribute__((always_inline)) {
		constexpr int d_ = decltype(dtag)::v;
		constexpr bool want_cs = decltype(cstag)::v != 0;   // 0: the silent row this segment leaves is not read at this position
		const int c = c_q[d_];
		const float Pi = Pi_q[d_];
		const float pb = pb_q[d_];
		SV cs; cs.v = cs_q[d_]; cs.z = RT ? false : first;   // the segment's first group starts from an empty accumulator
		float bm = bm_q[d_];
		int ba = ba_q[d_];
		f32x4 cb[NF][NQ + 1];
		f32x2 ct[NF];
		// trailing pruned segment below sstop: every posterior there is exactly zero, the backward rows were not even computed
		const bool sfx_skip = (J >= kSfxFirst) && i < w.sstop;   // wave-uniform
		float ik[NF];     // I_backward[K-1] at position i and (ik_n) at position i+1
#pragma unroll
		for (int f = 0; f < NF; f++) {
			if constexpr (PD == 1) {
				const uint8_t* bw = BW + ((int64_t)kBwOff[kHmmOff[J] + f0 + f] * w.lmax + (int64_t)(i - 1) * ROWH) * (TD_WAVE * 4);
				if (!sfx_skip) {
#pragma unroll
					for (int p = 0; p < NQ; p++) cb[f][p] = ld4(bw + p * (TD_WAVE * 16), w.lane);
					if (NT) ct[f] = ld2(bw + NQ * (TD_WAVE * 16), w.lane);
				}
			} else {
#pragma unroll
				for (int p = 0; p < NQ; p++) cb[f][p] = f32x4{ MB_q[d_][f][2 * p], IB_q[d_][f][2 * p], MB_q[d_][f][2 * p + 1], IB_q[d_][f][2 * p + 1] };
				if (NT) ct[f] = f32x2{ MB_q[d_][f][NSF - 1], IB_q[d_][f][NSF - 1] };
			}
			ik[f] = ik_q[d_][f];
		}
		TDS_FWD_FILL(d_, i + PD)
		// the next position's: slot d_ itself once refilled when PD == 1, the following slot otherwise
		const int dn_ = (d_ + 1) % PD;
		const int c_n = c_q[dn_];
		const float pb_n = pb_q[dn_];
		float ik_n[NF];
#pragma unroll
		for (int f = 0; f < NF; f++) ik_n[f] = ik_q[dn_][f];
		float lpost[NF];   // log posterior of label f0+f at this position; -inf in lanes whose read has ended
#pragma unroll
		for (int f = 0; f < NF; f++) lpost[f] = NEG_INF;
		// The first unpruned segment past the cut ("tail", see "Position pruning"): the silent row it is entered from was not
		// computed there.  Its terms enter the folds as -inf -- logsum(x, -inf) == x bit for bit -- and the folds they would
		// have gone through are checked against the host's bounds.
		const bool tail = (J == kPruneSegs && kPruneSegs > 0) && i >= itail;   // wave-uniform
		if (i <= w.len) {
			const SV PmS = sv(tail ? NEG_INF : Pm);
			const SV PiS = sv(tail ? NEG_INF : Pi);
			const BaseMask kc = mk_mask(c);
#pragma unroll
			for (int f = 0; f < NF; f++) {
				const int col0 = kColOff[J] + (RT ? 0 : (f0 + f)) * NC;
				const int colr = kColOff[J] + (f0 + f) * NC;
				(void)colr;
				const int h = kHmmOff[J] + f0 + f;
				SV Mc[NC], Ic[NC];
				SV Dc = sv_none();
				const float ei0 = EMIT_I(col0, kc);
				{   // column 0, :4220-4268 (posterior terms folded below)
					const int q = col0;
					const SV M = addv(addc(PmS, kCols[q].sM), EM(0, kc, c));
					SV I = addc(PmS, kCols[q].sI);
					if (tail && LIVE(kCols[q].sI)) {
						// P[i-1] + sI <= wa[i] - 15.75 for any read: folded with a term at least that far above it, the
						// reference's logsum returns that term
						if (!(Ip[f][0] + kCols[q].t[3] >= uload(w.wa, i))) w.bad |= 1;
					}
					I = lsum(I, addc(sv(Ip[f][0]), kCols[q].t[3]));
					I = lsum(I, addc(sv(Mp[f][0]), kCols[q].t[1]));
					I = addv(I, ei0);
					if (want_cs) { cs = lsum(cs, addc(M, kCols[q].t[7])); cs = lsum(cs, addc(I, kCols[q].t[8])); }
					Mc[0] = M; Ic[0] = I;
				}
#pragma unroll
				for (int g = 1; g <= K; ++g) { // :4271-4334
					const int q = col0 + g, qp = q - 1;
					// The M- and the I-chain of a column are independent: their folds are issued in pairs.  Each chain keeps
					// its own order (M: entry, M(g-1), I(g-1), D;  I: entry, I(g), M(g));  D pairs with M's last fold.
					SV M = addc(PmS, kCols[q].sM);
					SV I = addc(PmS, kCols[q].sI);
					lsum2(M, addc(sv(Mp[f][g - 1]), kCols[qp].t[0]), I, addc(sv(Ip[f][g]), kCols[q].t[3]));
					lsum2(M, addc(sv(Ip[f][g - 1]), kCols[qp].t[4]), I, addc(sv(Mp[f][g]), kCols[q].t[1]));
					SV D = addc(Mc[g - 1], kCols[qp].t[2]);
					lsum2(M, addc(Dc, kCols[qp].t[6]), D, addc(Dc, kCols[qp].t[5]));
					M = addv(M, EM(g, kc, c));
					I = addv(I, EMIT_I(q, kc));
					if (want_cs) { cs = lsum(cs, addc(M, kCols[q].t[7])); cs = lsum(cs, addc(I, kCols[q].t[8])); }
					Mc[g] = M; Ic[g] = I; Dc = D;
				}
				if (tail && skip_live) { if (!(cs.v >= uload(w.wb, i))) w.bad |= 2; }   // P[i] + skip <= wb[i] - 15.75
				if (want_cs) cs = lsum(cs, addc(PiS, kSkip[J])); // :4341
				if (!sfx_skip) {
				// posterior fold, in the reference's order (column ascending, M term then I term)
				float MB[NC], IB[NC];
#pragma unroll
				for (int p = 0; p < NQ; p++) {
					const f32x4 v = cb[f][p];
					MB[2 * p] = v.x; IB[2 * p] = v.y; MB[2 * p + 1] = v.z; IB[2 * p + 1] = v.w;
				}
				if (NT) { MB[NSF - 1] = ct[f].x; IB[NSF - 1] = ct[f].y; }
				if constexpr (DM != 0) {
					// M_backward[K-1][i], barcode_hmm.c:3546-3562 as bwd_row() folds it: from M_backward[K][i+1] (pure:
					// P[i+2] + MSKIP_K), P[i+1] and I_backward[K-1][i+1]; the delete term is dead (D_backward[K] = -inf).
					// A lane whose read ends at i starts from the -inf rows the backward sweep started from.
					constexpr int g = K - 1;
					const int q = col0 + g;
					const bool nxt = i < w.len;
					const int cx = (i < w.tmax) ? c_n : 0;              // x_{i+1}
					const BaseMask kn = mk_mask(cx);
					SV MnK = addc(sv(pb_n), kCols[col0 + K].t[7]);
					if (!MnK.z) MnK.v = nxt ? MnK.v : NEG_INF;
					const float InK = nxt ? ik_n[f] : NEG_INF;
					SV Mr = addc(addv(MnK, EM(K, kn, cx)), kCols[q].t[0]);
					Mr = lsum(Mr, addc(sv(pb), kCols[q].t[7]));
					Mr = lsum(Mr, addc(addv(sv(InK), EMIT_I(q, kn)), kCols[q].t[1]));
					MB[g] = Mr.v; IB[g] = ik[f];
				}
				if (pure) {
					MB[K] = pb + kCols[col0 + K].t[7];
					IB[K] = pb + kCols[col0 + K].t[8];
				}
				// total_prob is only read for segments with several HMMs (:4354-4429)
				constexpr bool want_tt = kNHmm[J] > 1;
				SV acc = sv_none(), tt = sv(tot[f]);
#pragma unroll
				for (int g = 0; g <= K; ++g) {
					const SV pm = subv(addv(Mc[g], MB[g]), b);
					if (want_tt && g == 0) tt = lsum(tt, pm);
					acc = lsum(acc, pm);
					if (want_tt && g == 0) tt = lsum(tt, subv(addv(addv(addc(PmS, kCols[col0].sI), ei0), IB[0]), b));
					acc = lsum(acc, subv(addv(Ic[g], IB[g]), b));
				}
				if (want_tt) tot[f] = tt.v;
				if (own_sum) {
					lacc[f] = post_prob(acc.v) + lacc[f];                        // dyn_prog[i][h] + dyn_prog[i-1][h]
					if (lacc[f] > bm) { bm = lacc[f]; ba = h; }                 // first maximum, labels ascending
				} else if (kMaskDP) {
					lpost[f] = acc.v;   // stored (or skipped) below, in uniform control flow
				} else {
					DP[((int64_t)(i - 1) * TD_H + h) * TD_WAVE + w.lane] = post_prob(acc.v);
				}
				}
#pragma unroll
				for (int g = 0; g < NC; g++) { Mp[f][g] = Mc[g].v; Ip[f][g] = Ic[g].v; }
			}
			if (want_cs) Cs[i * TD_WAVE + w.lane] = cs.v;
			if (own_sum) { w.bm[i * TD_WAVE + w.lane] = bm; w.ba[i * TD_WAVE + w.lane] = (uint8_t)ba; }
		}
		if (kMaskDP && !own_sum) {   // in uniform control flow: the bits are the same in every lane
#pragma unroll
			for (int f = 0; f < NF; f++) {
				// scaledprob2prob gives +0.0f below -103.98 (post_prob): a row that is zero in every lane is not stored
				const bool on = lpost[f] > -103.98f;
				const bool any_on = __builtin_amdgcn_ballot_w64(on) != 0;
				if (any_on) {
					float pp = 0.0f;
					if (on) pp = (float)exp((double)lpost[f]);
					if (i <= w.len) DP[((int64_t)(i - 1) * TD_H + kHmmOff[J] + f0 + f) * TD_WAVE + w.lane] = pp;
				}
				mbits[f] |= (any_on ? 1u : 0u) << ((i - 1) & 31);
				if ((((i - 1) & 31) == 31) || i == iend) {
					if (w.lane == 0) w.pmask[(kHmmOff[J] + f0 + f) * w.nwm + ((i - 1) >> 5)] = mbits[f];
					mbits[f] = 0u;
				}
			}
		}
		Pm = Pi;
	};
	{
		// The last segment's silent row is read in one place, f_score = its entry at each read's last base (:4349): below the tile's
		// shortest read nobody reads it, and its folds -- two per column and HMM for a 3' partial segment, a quarter of config 3's
		// adapter sweep -- are not evaluated.  As two loops over the same body (the folds compiled out of the first), not as a branch
		// inside one: a branch per position or per column cost more than the folds it saved (DESIGN.md section 4, round 3), the sweeps
		// live off one long basic block per position.
		constexpr bool cs_late = TDS_LATE_CS && (J == TD_S - 1) && !((J == kPruneSegs && kPruneSegs > 0) && skip_live);
		auto step = [&](auto dtag, const int i) __attribute__((always_inline)) { step_cs(dtag, IC<1>{}, i); };
		auto step_nocs = [&](auto dtag, const int i) __attribute__((always_inline)) { step_cs(dtag, IC<0>{}, i); };
		int base = i0;
		if constexpr (cs_late) {
			const int i_cs = (w.tmin < iend) ? w.tmin : iend;      // the first position whose entry somebody reads
			for (; base + PD - 1 < i_cs; base += PD) ring_block<PD, 0>(step_nocs, base);
		}
		for (; base + PD - 1 <= iend; base += PD) ring_block<PD, 0>(step, base);
		ring_rest<PD, 0>(step, base, iend);
	}
	if (J < kPruneSegs && iend < w.tmax) {
		// posterior rows past the cut: none exists (all exactly zero)
		if (kMaskDP && !own_sum && w.lane == 0) {
#pragma unroll
			for (int f = 0; f < NF; f++)
				for (int wd = ((iend - 1) >> 5) + 1; wd < w.nwm; wd++) w.pmask[(kHmmOff[J] + f0 + f) * w.nwm + wd] = 0u;
		}
		// total_prob: the terms past the cut are below -103.98 - ...; folding them in leaves a value at least 15.7 above unchanged
		if (kNHmm[J] > 1 && w.len > iend) {
#pragma unroll
			for (int f = 0; f < NF; f++) if (!(tot[f] >= TDS_PRUNE_TT)) w.bad |= 4;
		}
	}
	if (kNHmm[J] > 1) {
#pragma unroll
		for (int f = 0; f < NF; f++) TOTAL[(kHmmOff[J] + f0 + f) * TD_WAVE + w.lane] = tot[f];
	}
#undef EM
#undef PBR
#undef BWROW
#undef TDS_FWD_FILL
}

template <int J, int F0>
DEV void fwd_groups(const Wv& w, const uint8_t* __restrict__ codes, const float* __restrict__ P,
                    float* __restrict__ Cs, const float* __restrict__ PB, const uint8_t* __restrict__ BW,
                    float* __restrict__ DP, float* __restrict__ TOTAL, const float b)
{
	if constexpr (TDS_RESTART && F0 == 0 && J >= kSfxFirst) {
		if (w.rf_on) {
			const int q_hi = w.sstop - (TD_S - 1 - J) * (w.rWf + 1);
			fwd_stair<J>(w, codes, P, q_hi - w.rWf, q_hi);
		}
	}
	if constexpr (F0 == 0 && kRt[J] > 0) {
		for (int f0 = 0; f0 < kRt[J]; f0 += kGroupF[J]) fwd_group<J, kGroupF[J], true>(w, codes, P, Cs, PB, BW, DP, TOTAL, b, f0);
		fwd_groups<J, kRt[J]>(w, codes, P, Cs, PB, BW, DP, TOTAL, b);
	} else if constexpr (F0 < kNHmm[J]) {
		constexpr int NF = cmin(kGroupF[J], kNHmm[J] - F0);
		fwd_group<J, NF, false>(w, codes, P, Cs, PB, BW, DP, TOTAL, b, F0);
		fwd_groups<J, F0 + NF>(w, codes, P, Cs, PB, BW, DP, TOTAL, b);
	}
}

template <int J>
DEV void fwd_segments(const Wv& w, const uint8_t* __restrict__ codes, float* __restrict__ SF, const float* __restrict__ SB,
                      int rowlen, const uint8_t* __restrict__ BW, float* __restrict__ DP, float* __restrict__ TOTAL, const float b)
{
	if constexpr (J < TD_S) {
		fwd_groups<J, 0>(w, codes, SF + (int64_t)J * rowlen, SF + (int64_t)(J + 1) * rowlen, SB + (int64_t)(J + 1) * rowlen,
		                 BW, DP, TOTAL, b);
		if (TDS_PROFILE == 2 && J < 8) { const long long t_ = (long long)__builtin_readcyclecounter(); if (w.lane == 0) atomicAdd(&w.stats[TDS_DIAG(216 + J)], (unsigned long long)(t_ - *w.tprof)); *w.tprof = t_; }
		fwd_segments<J + 1>(w, codes, SF, SB, rowlen, BW, DP, TOTAL, b);
	}
}

// Path words (four path bytes each) whose labels all lack predecessors -- e.g. the labels of a leading barcode segment --
// always say "stay": such a word is neither stored by the label DP nor loaded by the traceback.
constexpr bool path_word_trivial(int k)
{
	for (int b = 0; b < 4; b++) {
		const int v = kFirstN + 4 * k + b;
		if (v < TD_H && (kPredFirst[v] != 0 || kPredOff2[v + 1] != kPredOff2[v])) return false;
	}
	return true;
}
constexpr uint32_t path_word_identity(int k)
{
	uint32_t w = 0;
	for (int b = 0; b < 4; b++) w |= (uint32_t)((kFirstN + 4 * k + b) & 0xFF) << (8 * b);
	return w;
}

// Position pruning: the last position at which a state of the pruned segments can still have a posterior term above the
// zero bound in any lane, fb[i] + bwb[len - i] > thr (thr = b - kPruneZ per lane); wave-uniform result, at least 1.
DEV int prune_scan(const float thr, const int len, const int tmax, const float* __restrict__ fbt, const float* __restrict__ bwt)
{
	int cl = 1;
	// (eight positions at a time: the table look-ups of a block are independent and issued together -- one round trip per block,
	// not per position; the tables have 24 spare entries behind lcap)
	for (int i0 = 2; i0 <= tmax; i0 += TDS_SCAN_B) {
		float g[TDS_SCAN_B];
#pragma unroll
		for (int k = 0; k < TDS_SCAN_B; k++) {
			const int i = i0 + k;
			const int mm = (i <= len) ? len - i : 0;
			g[k] = bwt[mm];
		}
		__builtin_amdgcn_sched_barrier(0);   // (the scheduler would otherwise pair each load with its use again)
#pragma unroll
		for (int k = 0; k < TDS_SCAN_B; k++) g[k] = uload(fbt, i0 + k) + g[k];
#pragma unroll
		for (int k = 0; k < TDS_SCAN_B; k++) {
			const int i = i0 + k;
			if (i <= len && i <= tmax && g[k] > thr) cl = i;
		}
	}
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) cl = max(cl, __shfl_xor(cl, o));
	return __builtin_amdgcn_readfirstlane(cl);
}

// max over the leading segments of the relative backward bound at position i: every backward value of theirs at i is at most
// max_k (gq_J[k] + Q[i + 1 + k]) + log(len - i + 1) + 0.02 (tests/test_prune.py::test_restart_bounds_dominate_reference_values)
DEV float leading_bwd_bound(const Wv& w, const int i)
{
	float hb = NEG_INF;
	for (int k0 = 0; i + 1 + k0 <= w.tmax + 1; k0 += TDS_SCAN_B) {
		float q[TDS_SCAN_B];
#pragma unroll
		for (int u = 0; u < TDS_SCAN_B; u++) {
			const int pos = i + 1 + k0 + u;
			q[u] = w.qr[(pos <= w.tmax + 1 ? pos : w.tmax + 1) * TD_WAVE + w.lane];
		}
		__builtin_amdgcn_sched_barrier(0);   // (the scheduler would otherwise pair each load with its use again)
#pragma unroll
		for (int u = 0; u < TDS_SCAN_B; u++) {
			const int k = k0 + u, pos = i + 1 + k;
			float g = uload(w.ptab + (int64_t)8 * w.pstride, k);
#pragma unroll
			for (int J = 1; J < 4; J++) if (J < kPruneSegs) g = fmaxf(g, uload(w.ptab + (int64_t)(8 + J) * w.pstride, k));
			if (pos <= w.len + 1) hb = fmaxf(hb, g + q[u]);
		}
	}
	return hb + (__logf((float)(w.len - i + 1)) + 0.02f);
}
// prune_scan's answer `cq` (last position with a possible posterior above the zero bound, absolute bounds) moved down under the
// smaller of the absolute and the relative backward bound; wave-uniform, at least 1
DEV int refine_cut(const Wv& w, int cq, const float thr, const float* __restrict__ fbt, const float* __restrict__ bwt)
{
	while (cq > 1) {
		bool viol = false;
		if (cq <= w.len) {
			const float bb = fminf(bwt[w.len - cq], leading_bwd_bound(w, cq));
			viol = uload(fbt, cq) + bb > thr;
		}
		if (__builtin_amdgcn_ballot_w64(viol) != 0) break;
		cq--;
	}
	return cq;
}

// The same for the trailing segments: the first position at which a state of theirs can have a posterior term above the zero
// bound in any lane (at most the shortest read's last position); wave-uniform, at least 1.
DEV int prune_scan_sfx(const float thr, const int len, const int tmax, const float* __restrict__ fbs, const float* __restrict__ bws)
{
	int st = (len >= 1) ? len : 0x7fffffff;
	for (int i0 = tmax; i0 >= 1; i0 -= TDS_SCAN_B) {
		float g[TDS_SCAN_B];
#pragma unroll
		for (int k = 0; k < TDS_SCAN_B; k++) {
			const int i = (i0 - k >= 1) ? i0 - k : 1;
			const int mm = (i <= len) ? len - i : 0;
			g[k] = bws[mm];
		}
		__builtin_amdgcn_sched_barrier(0);   // (the scheduler would otherwise pair each load with its use again)
#pragma unroll
		for (int k = 0; k < TDS_SCAN_B; k++) g[k] = uload(fbs, (i0 - k >= 1) ? i0 - k : 1) + g[k];
#pragma unroll
		for (int k = 0; k < TDS_SCAN_B; k++) {
			const int i = i0 - k;
			if (i >= 1 && i <= len && g[k] > thr) st = i;
		}
	}
#pragma unroll
	for (int o = 32; o >= 1; o >>= 1) st = min(st, __shfl_xor(st, o));
	st = __builtin_amdgcn_readfirstlane(st);
	return st > tmax ? 1 : st;
}

// ---------------------------------------------------------------------------------------------------------
// the kernel
// ---------------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(TDS_BLOCK, TDS_MIN_WAVES) void td_spec_kernel(const TdSpecArgs ka)
{
	for (int k = threadIdx.x; k < TDS_TABLE_N; k += TDS_BLOCK) g_T[k] = (k < TD_LOGSUM_LIVE) ? ka.logsum[k] : 0.0f;
	__syncthreads();

	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int slot = blockIdx.x * TDS_WPB + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	if (slot >= ka.n_slots) return;

	constexpr int S = TD_S, H = TD_H;
	// (length classes: the first n_big slots have the geometry of the batch's longest read, see TdSpecArgs)
	const bool big = slot < ka.n_big;
	const TdSpecLayout& lay = big ? ka.lay_big : ka.lay;
	const int lmax = big ? ka.lmax_big : ka.lmax;
	const int rowlen = (lmax + 2) * TD_WAVE;
	constexpr int PW = (TD_H + 3) / 4; // path words per position

	Wv w;
	w.slot = big ? ka.ws + (int64_t)slot * ka.lay_big.slot_bytes
	             : ka.ws + (int64_t)ka.n_big * ka.lay_big.slot_bytes + (int64_t)(slot - ka.n_big) * ka.lay.slot_bytes;
	w.lane = lane;
	w.lmax = lmax;
	w.pmask = (uint32_t*)(w.slot + lay.pmask);
	w.nwm = (lmax + 31) >> 5;
	w.bm = (float*)(w.slot + lay.bm);
	w.ba = w.slot + lay.ba;
	uint8_t* const codesF = w.slot + lay.codes;   // base codes of the whole reads, x_0..x_{tmaxF+1}
	float* SB = (float*)(w.slot + lay.sb);
	float* SF = (float*)(w.slot + lay.sf);
	uint8_t* BW = w.slot + lay.bw;
	float* DP = (float*)(w.slot + lay.dp);
	uint32_t* PATH = (uint32_t*)(w.slot + lay.path);
	float* TOTAL = (float*)(w.slot + lay.total);

#ifdef TDS_ENDSTATS
	// diagnostic: when do the waves start and finish?  (100 MHz wall clock; counter slots 200..205: min start, max start, min end,
	// max end, sum of ends, waves)
	const unsigned long long t_start = wall_clock64();
#endif
	long long tprof = TDS_PROFILE ? (long long)__builtin_readcyclecounter() : 0;
	(void)tprof;
	// position pruning: a wave whose tiles keep failing the checks stops trying
	int n_fallback = 0, n_tiles_done = 0;
	bool prune_on = true;
	bool restart_on = true;        // restarted sweeps: a wave whose bridges do not close (N-rich reads) goes on without them
	bool restart_fwd_on = true;    // ... and the forward ones of the trailing segments on their own
	int n_fwd_fail = 0;
	(void)restart_fwd_on; (void)n_fwd_fail;
	float bgap = TDS_PRUNE_BGAP;   // grows when a guess turns out too short: the wave's reads score lower than assumed
	(void)n_fallback; (void)n_tiles_done; (void)prune_on; (void)bgap; (void)restart_on;
	w.wa = ka.prune + 2 * (int64_t)ka.prune_stride;
	w.wb = ka.prune + 3 * (int64_t)ka.prune_stride;
	w.wc = ka.prune + 6 * (int64_t)ka.prune_stride;
	w.wd = ka.prune + 7 * (int64_t)ka.prune_stride;
	w.sstop = 1; w.sstopS = 1;
	w.cut = 0; w.cutS = 0; w.bad = 0;
	w.rb_on = false; w.rf_on = false;
	w.rs = (float*)(w.slot + lay.rs);
	w.hb = SB + (int64_t)TD_S * rowlen;   // (row S of the silent_backward block: previous_silent, formed in registers -- free)
	w.rW = TDS_RESTART_W;
	w.rWf = fwd_window_all();
	w.stats = ka.counters;
	w.tprof = &tprof;
	w.bwt = ka.prune + 1 * (int64_t)ka.prune_stride;
	w.fbs = ka.prune + 4 * (int64_t)ka.prune_stride;
	w.ptab = ka.prune; w.pstride = ka.prune_stride;
	w.qr = SB + (int64_t)(kPruneSegs < TD_S ? kPruneSegs : 0) * rowlen;
	w.pr = SF + (int64_t)(kSfxFirst < TD_S ? kSfxFirst : 0) * rowlen;
	// Tiles: the first one by slot number, the following ones from a shared counter (longest reads first: tiles are sorted by
	// length ascending).  The waves do not run at one speed -- on the boxes measured the waves of four of the eight XCDs take
	// ~10 % longer for the same tiles (tools/endstats.py) -- so a static share per wave leaves the fast ones idle at the end.
	auto next_tile = [&](void) -> int {
		int t = 0;
		if (lane == 0) t = atomicAdd(ka.tile_next, 1);
		return ka.n_tiles - 1 - ka.n_slots - __builtin_amdgcn_readfirstlane(t);
	};
	for (int tile = ka.n_tiles - 1 - slot; tile >= 0; tile = next_tile()) {
		const int64_t rid = (int64_t)tile * TD_WAVE + lane;
		// -start / -end (td_set_window): the DP phases see bases [woff, woff + len) of every read (do_label_thread /
		// do_probability_estimation decode seq + matchstart for matchend - matchstart bases, barcode_hmm.c:2290-2296), the
		// phases after them -- the rewrite, the artifact filter, DUST -- the whole read (make_extracted_read walks ri->len,
		// :3336).  `len`, `tmax`, `codes` are the window's; `lenF`, `tmaxF`, `codesF` the whole read's.
		const int lenF = ka.lens[rid];
#if TDS_WINDOW
		const int woff = ka.win_len > 0 ? ka.win_start : 0;   // wave-uniform
		int len = lenF;
		if (ka.win_len > 0) {
			const int e = lenF < woff + ka.win_len ? lenF : woff + ka.win_len;
			len = e > woff ? e - woff : 0;
		}
#else
		constexpr int woff = 0;       // (a context with a window set loads the kernel compiled with TDS_WINDOW)
		const int len = lenF;
#endif
		w.len = len;
		int tmax = len;
#pragma unroll
		for (int o = 32; o >= 1; o >>= 1) tmax = max(tmax, __shfl_xor(tmax, o));
		tmax = __builtin_amdgcn_readfirstlane(tmax);
		w.tmax = tmax;
		int tmin = len;
#pragma unroll
		for (int o = 32; o >= 1; o >>= 1) tmin = min(tmin, __shfl_xor(tmin, o));
		w.tmin = __builtin_amdgcn_readfirstlane(tmin);
#if TDS_WINDOW
		int tmaxF = lenF;
#pragma unroll
		for (int o = 32; o >= 1; o >>= 1) tmaxF = max(tmaxF, __shfl_xor(tmaxF, o));
		tmaxF = __builtin_amdgcn_readfirstlane(tmaxF);
#else
		const int tmaxF = tmax;
#endif
		uint8_t* const codes = codesF + woff * TD_WAVE;

		TDS_PHASE(11);
		float r_score = 0.0f;
		// ---- unpack 2-bit codes + N mask into x_0..x_{tmax+1} ----
		{
			const uint32_t* pk = ka.packed + (int64_t)tile * (ka.nw2 + ka.nw1) * TD_WAVE;
			codesF[lane] = 0;
			uint32_t w2 = 0, w1 = 0;
			// (the words of the next 16 / 32 positions are requested a block ahead: a block of positions takes longer than the trip)
			uint32_t w2n = (ka.nw2 > 0) ? pk[lane] : 0u, w1n = (ka.nw1 > 0) ? pk[ka.nw2 * TD_WAVE + lane] : 0u;
			for (int i = 1; i <= tmaxF + 1; i++) {
				const int k = i - 1;
				if ((k & 15) == 0) { w2 = w2n; w2n = ((k >> 4) + 1) < ka.nw2 ? pk[((k >> 4) + 1) * TD_WAVE + lane] : 0u; }
				if ((k & 31) == 0) { w1 = w1n; w1n = ((k >> 5) + 1) < ka.nw1 ? pk[(ka.nw2 + (k >> 5) + 1) * TD_WAVE + lane] : 0u; }
				uint32_t code = (w2 >> (2 * (k & 15))) & 3u;
				if ((w1 >> (k & 31)) & 1u) code = 4u;
				if (i > lenF) code = 0u;
				codesF[i * TD_WAVE + lane] = (uint8_t)code;
				// the random model's score (:4516-4523) over the window's bases, in their order, while the codes are in hand
				const int iw = i - woff;
				if (iw >= 1 && iw <= len) r_score = (r_score + emit(kBg[0], kBg[1], kBg[2], kBg[3], kBg[4], mk_mask((int)code))) + kRStay;
			}
		}

		TDS_PHASE(0);
		// Backward and forward sweep, with position pruning of the leading segments when the model has any (see "Position
		// pruning" above): the first pass spills / sweeps those segments up to a cut; when the cut cannot be shown to be
		// exact for every read of the tile the pass is repeated without pruning (`dense`).
		// ---- random model, :4516-4523 (first: the spill cut of the pruned segments is guessed from it) ----
		r_score += kRExit;   // (summed up by the unpack loop above)

		float b_score = NEG_INF, f_score = NEG_INF, b_use = 0.0f;
		bool dead = false, arch_done = false;
		bool dense = !((kPruneSegs > 0 || kSfxFirst < TD_S) && prune_on);
		// The backward sweep has to know how far to spill before b_score exists: the cut is taken for a score
		// TDS_PRUNE_BGAP below the read's score under the random model (a read that fits the architecture scores above
		// that, a random read a little below), plus a margin; a guess that turns out too short costs a second pass.
		int cut_guess = tmax;
		if (kPruneSegs > 0 && !dense)
			cut_guess = prune_scan((len >= 1 ? r_score : 0.0f) - bgap - kPruneZ, len, tmax, ka.prune, ka.prune + ka.prune_stride) + 1 + TDS_PRUNE_MARGIN;
		// the trailing segments the other way round: first position their backward sweep still has to reach
		int sfx_guess = 1;
		if (kSfxFirst < TD_S && !dense) {
			sfx_guess = prune_scan_sfx((len >= 1 ? r_score : 0.0f) - bgap - kPruneZ, len, tmax, ka.prune + 4 * (int64_t)ka.prune_stride,
			                           ka.prune + 5 * (int64_t)ka.prune_stride) - TDS_PRUNE_MARGIN;
			if (sfx_guess < 1) sfx_guess = 1;
		}
		for (;;) {
			// (a guess within a few positions of the read's end / start is not worth the risk of a second pass)
			w.cutS = (dense || cut_guess + 8 >= tmax) ? tmax : cut_guess;
			w.cut = tmax;
			w.sstopS = (dense || sfx_guess <= 8) ? 1 : sfx_guess;
			w.sstop = w.sstopS;
			w.bad = 0;
			// restarted sweeps: only when the bridges and the regular part behind them fit between the cut and the end of the tile's
			// longest read (otherwise the sweep simply starts at the end, as ever)
			w.rb_on = TDS_RESTART && restart_on && kPruneSegs > 0 && !dense && w.cutS < tmax && w.cutS + kPruneSegs * (w.rW + 1) + 1 <= tmax;
			w.rf_on = false;
			// ---- backward, barcode_hmm.c:3439-3640 ----
			{
				// (previous_silent -- -inf except [len+1] = 0 -- is formed in registers by the last segment's sweep)
				float run = 0.0f;
#pragma unroll
				for (int j = S - 1; j >= 0; j--) {
					run = run + kSkip[j];
					SB[(int64_t)j * rowlen + (len + 1) * TD_WAVE + lane] = run;
				}
				bwd_segments<S - 1>(w, codes, SB, rowlen, BW);
				b_score = (len >= 1) ? SB[1 * TD_WAVE + lane] : NEG_INF; // :3610
			}
			if (TDS_RESTART && w.rb_on) {
				const bool open = __builtin_amdgcn_ballot_w64((w.bad & 32) != 0) != 0;
				if (TDS_PRUNE_STATS && lane == 0) { atomicAdd(&ka.counters[TDS_DIAG(206)], 1ull); if (open) atomicAdd(&ka.counters[TDS_DIAG(207)], 1ull); }
				// a bridge did not close within its W positions: the tile again, pruned as before but swept from the end of the read --
				// and so the wave's following tiles (reads rich in N close late: 19.5 positions at 20 % N against 12.9)
				// (a staircase bridge that ran out of positions gets a wider window first -- for this tile and the wave's following ones)
				if (open) {
					if (w.rW + 8 <= TDS_RESTART_WMAX) w.rW += 8; else restart_on = false;
					continue;
				}
			}
			dead = !(b_score > NEG_INF);  // no valid path: the reference crashes (SURVEY.md Q11); here: mismatch, Q = 0
			b_use = dead ? 0.0f : b_score;
			const bool any_dead = __builtin_amdgcn_ballot_w64(dead && len >= 1) != 0;
			if (kSfxFirst < TD_S && !dense) {
				// the read segment's checks in the backward sweep, and -- now that b_score is known (it is exact once those checks
				// hold) -- the first position from which the trailing segments' posteriors can be non-zero: the rows must exist there
				const int sq = any_dead ? 1 : prune_scan_sfx(b_use - kPruneZ, len, tmax, ka.prune + 4 * (int64_t)ka.prune_stride, ka.prune + 5 * (int64_t)ka.prune_stride);
				if (TDS_PRUNE_STATS && lane == 0) { atomicAdd(&ka.counters[TDS_DIAG(224)], 1ull); atomicAdd(&ka.counters[TDS_DIAG(225)], (unsigned long long)sq); }
				if (__builtin_amdgcn_ballot_w64((w.bad & 24) != 0) != 0 || sq < w.sstopS) {
					if (TDS_PRUNE_STATS && lane == 0) atomicAdd(&ka.counters[TDS_DIAG(226)], 1ull);
					bgap += 40.0f;
					dense = true; n_fallback++; continue;
				}
				w.sstop = sq;
			}
			if (ka.mode == MODE_ARCH_COMP) { // do_arch_comparison, barcode_hmm.c:2111-2148: backward only
				ka.out_b[rid] = b_score;
				arch_done = true;
				break;
			}

			if (kPruneSegs > 0 && !dense) {
				// smallest cut that is exact for all 64 reads: the last position at which a state of the pruned segments can
				// still have a posterior term above the zero bound, fb[i] + bwb[len - i] - b > -kPruneZ, in any lane
				int cq = tmax;
				if (!any_dead) cq = prune_scan(b_use - kPruneZ, len, tmax, ka.prune, ka.prune + ka.prune_stride);
				// The backward bound in that test is absolute (any read, every emission at its maximum).  Now that the silent row in
				// front of the first unpruned segment exists -- it was swept densely -- the bound relative to it (the restarted sweeps'
				// impulse responses, td_jit.hip) is tighter by what this read loses behind the leading segments: the cut moves down
				// while no lane has a state that can still be above the zero bound under the smaller of the two.
				if (kPruneSegs <= 4 && !any_dead && cq + 1 < tmax) cq = refine_cut(w, cq, b_use - kPruneZ, ka.prune, ka.prune + ka.prune_stride);
				if (TDS_PRUNE_STATS && lane == 0) {
					atomicAdd(&ka.counters[TDS_DIAG(232)], 1ull);
					atomicAdd(&ka.counters[TDS_DIAG(233)], (unsigned long long)cq);
				}
				if (cq + 1 < tmax) {
					if (cq + 1 > w.cutS) {   // rows the forward sweep needs were not spilled
						if (TDS_PRUNE_STATS && lane == 0) atomicAdd(&ka.counters[TDS_DIAG(234)], 1ull);
						bgap += 40.0f;
						dense = true; n_fallback++; continue;
					}
					w.cut = cq;
				} else if (w.cutS < tmax) {
					dense = true; n_fallback++; continue;
				}
			}

			// the trailing segments' forward sweep starts W positions before the first position their values are used at
			w.rf_on = TDS_RESTART && TDS_RESTART_FWD && restart_fwd_on && kSfxFirst < TD_S && !dense && w.sstop - (TD_S - kSfxFirst) * (w.rWf + 1) >= 1;
			if (TDS_PRUNE_STATS && w.rf_on && lane == 0) atomicAdd(&ka.counters[TDS_DIAG(198)], 1ull);
			TDS_PHASE(1);
			// ---- forward + posteriors, :4155-4349 ----
			{
				// (previous_silent -- [0] = 0, -inf elsewhere -- is formed in registers by the first segment's sweep)
				float run = 0.0f;
#pragma unroll
				for (int j = 0; j < S; j++) {
					run = run + kSkip[j];
					SF[(int64_t)(j + 1) * rowlen + lane] = run;
				}
				fwd_segments<0>(w, codes, SF, SB, rowlen, BW, DP, TOTAL, b_use);
				if constexpr (TDS_RESTART && TDS_RESTART_FWD && kSfxFirst < TD_S) {
					if (w.rf_on && __builtin_amdgcn_ballot_w64((w.bad & 32) != 0) != 0) {
						// A forward bridge of the trailing segments did not close.  Nothing else depends on it: their forward sweep is
						// run again from position 1 (it rewrites every row and mask word it owns), the rest of the tile stands.  The
						// wave's next tiles get a wider window, and after two such failures none.
						if (TDS_PRUNE_STATS && lane == 0) atomicAdd(&ka.counters[TDS_DIAG(199)], 1ull);
						if (n_fwd_fail == 0 && w.rWf + 12 <= 96) w.rWf += 12; else restart_fwd_on = false;
						n_fwd_fail++;
						w.rf_on = false;
						w.bad &= ~32;
						fwd_segments<(kSfxFirst < TD_S ? kSfxFirst : 0)>(w, codes, SF, SB, rowlen, BW, DP, TOTAL, b_use);
					}
				}
				f_score = (len >= 1) ? SF[(int64_t)S * rowlen + len * TD_WAVE + lane] : NEG_INF; // :4349
			}
			if ((kPruneSegs > 0 || kSfxFirst < TD_S) && !dense && __builtin_amdgcn_ballot_w64(w.bad != 0) != 0) {
				if (TDS_PRUNE_STATS) {
					if (lane == 0) atomicAdd(&ka.counters[TDS_DIAG(235)], 1ull);
					for (int k = 0; k < 3; k++) if (w.bad & (1 << k)) atomicAdd(&ka.counters[TDS_DIAG(228 + k)], 1ull);
					if (lane == 0 && __builtin_amdgcn_ballot_w64((w.bad & 32) != 0) != 0) atomicAdd(&ka.counters[TDS_DIAG(199)], 1ull);
				}
				dense = true; n_fallback++; continue;
			}
			break;
		}
		if (arch_done) continue;
		if (kPruneSegs > 0 || kSfxFirst < TD_S) {
			// a model / data set on which the checks keep failing pays for two passes per tile: give up pruning in this wave
			n_tiles_done++;
			if (n_fallback * 4 > n_tiles_done + 4) prune_on = false;
			if (TDS_PRUNE_STATS && lane == 0) {
				atomicAdd(&ka.counters[TDS_DIAG(236)], 1ull);
				atomicAdd(&ka.counters[TDS_DIAG(237)], (unsigned long long)w.cut);
				atomicAdd(&ka.counters[TDS_DIAG(238)], (unsigned long long)(dense ? 1 : 0));
				atomicAdd(&ka.counters[TDS_DIAG(239)], (unsigned long long)w.cutS);
				atomicAdd(&ka.counters[TDS_DIAG(227)], (unsigned long long)w.sstop);
			}
		}

		TDS_PHASE(2);
		// ---- barcode confidence, :4354-4429 ----
		float bar_prob;
		if constexpr (H <= TDS_REG_H) {
			{
				float tv[H];   // (total_prob is only kept for segments with several HMMs)
	#pragma unroll
				for (int j = 0; j < S; j++) {
	#pragma unroll
					for (int f = 0; f < kNHmm[j]; f++) tv[kHmmOff[j] + f] = (kNHmm[j] > 1) ? TOTAL[(kHmmOff[j] + f) * TD_WAVE + lane] : 0.0f;
				}
	#pragma unroll
				for (int j = 0; j < S; j++) {
					if (kNHmm[j] > 1) {
						float n1 = NEG_INF;
	#pragma unroll
						for (int f = 0; f < kNHmm[j]; f++) n1 = lsum(n1, tv[kHmmOff[j] + f]);
	#pragma unroll
						for (int f = 0; f < kNHmm[j]; f++) tv[kHmmOff[j] + f] = tv[kHmmOff[j] + f] - n1;
					}
				}
				int gg = 1;
				float n0 = NEG_INF, n2 = 0.0f;
	#pragma unroll
				for (int j = 0; j < S; j++) {
					if (kNHmm[j] > 1) {
						gg = 0;
						float n1 = NEG_INF;
	#pragma unroll
						for (int f = 0; f < kNHmm[j]; f++) {
							const float t = tv[kHmmOff[j] + f];
							if (f != kNHmm[j] - 1) n0 = (t > n0) ? t : n0;
							n1 = lsum(n1, t);
						}
						n0 = n0 - n1; // not reset between segments, :4387
						n2 = n2 + n0;
					}
				}
				bar_prob = (gg || n2 > 0.0f) ? 0.0f : n2;
			}

		} else {
			// many HMMs: total_prob stays in the workspace
			int hc = 0;
#pragma unroll
			for (int j = 0; j < S; j++) {
				const int n = kNHmm[j];
				if (n > 1) {
					float n1 = NEG_INF;
					for (int f = 0; f < n; f++) n1 = lsum(n1, TOTAL[(hc + f) * TD_WAVE + lane]);
					for (int f = 0; f < n; f++) TOTAL[(hc + f) * TD_WAVE + lane] = TOTAL[(hc + f) * TD_WAVE + lane] - n1;
				}
				hc += n;
			}
			hc = 0;
			int gg = 1;
			float n0 = NEG_INF, n2 = 0.0f;
#pragma unroll
			for (int j = 0; j < S; j++) {
				const int n = kNHmm[j];
				if (n > 1) {
					gg = 0;
					float n1 = NEG_INF;
					for (int f = 0; f < n; f++) {
						const float t = TOTAL[(hc + f) * TD_WAVE + lane];
						if (f != n - 1) n0 = (t > n0) ? t : n0;
						n1 = lsum(n1, t);
					}
					n0 = n0 - n1;
					n2 = n2 + n0;
				}
				hc += n;
			}
			bar_prob = (gg || n2 > 0.0f) ? 0.0f : n2;
		}

		// ---- Q value, do_label_thread :2320-2338 ----
		float Q;
		{
			float pbest = lsum(f_score, r_score); // logsum(-inf, f_score) == f_score
			const double t = ((double)bar_prob + (double)f_score) - (double)pbest;
			const float tf = (float)t;
			const float e = (tf == NEG_INF) ? 0.0f : (float)exp((double)tf);
			pbest = (float)(1.0 - (double)e);
			if (pbest == 0.0f) Q = 40.0f;
			else if (pbest == 1.0f) Q = 0.0f;
			else Q = (float)(-10.0 * log10((double)pbest));
		}
		if (dead || len < 1) Q = 0.0f;

		// the first segment's running maximum past the pruning cut is the row at the cut (nothing was added to the sums)
#define BMROW(pos) ((kPruneSegs > 0 && (pos) > w.cut) ? w.cut : (pos))
		int read_type = 0, barcode = -1, fingerprint = -1;
		const int nw1 = ka.nw1;
		uint32_t* keep = ka.out_keep + (int64_t)tile * nw1 * TD_WAVE;

		if (ka.mode == MODE_GET_LABEL) {
			int8_t* labels = ka.out_labels + (int64_t)tile * (ka.out_lmax + 1) * TD_WAVE;
			// Labels 0 .. F1-1 (kFirstN, the predecessor-free first segment) were summed up by the forward sweep; the DP
			// below runs over the HL remaining labels and meets the first segment only through the running maximum of
			// its sums (bm / ba rows): as a predecessor candidate that comes before every other predecessor, at the
			// termination, and in the traceback (once the path is in the first segment it stays on that label).
			constexpr int F1 = kFirstN;
			constexpr int HL = H - F1;
			constexpr int PWL = (HL + 3) / 4;
			TDS_PHASE(3);   // bar_prob, random model, Q
			if constexpr (HL <= TDS_REG_H) {
				// ---- label DP, :4447-4472: running row in registers, updated from the highest label down ----
				float acc[HL];
	#pragma unroll
				for (int v = 0; v < HL; v++) acc[v] = 0.0f;
				// The posteriors were written a whole forward sweep ago and come from HBM, one dependent round trip per position if
				// requested one position ahead -- this phase is all latency.  They are requested TDS_LDP positions ahead, a block
				// at a time (every lane loads; rows past a lane's read are never used).
				constexpr int LD = TDS_LDP;
				// Every load of the loop is unconditional and every whole block of LD positions straight code: a load behind a branch
				// (a row whose mask bit is clear, a position past the end) would leave the number of loads in flight unknown to the
				// compiler, which then waits for all of them -- the requests ahead included -- at the first use.  So a row is loaded
				// whether its bit is set or not (what comes back for an unwritten row is dropped at use), except that the labels of the
				// pruned leading segments have no row at all past the cut: the loop runs in two parts, with and without their loads.
				float dq[LD][HL];
				uint32_t mq[LD];   // bit v: the row of label v in this slot was written (wave-uniform)
				uint32_t mw[HL];   // posterior-row bits of the block of 32 positions the requested position lies in (wave-uniform)
				auto mask_words = [&](const int word) __attribute__((always_inline)) {
					uint32_t t[HL];
#pragma unroll
					for (int v = 0; v < HL; v++) t[v] = w.pmask[(F1 + v) * w.nwm + word];   // all requested, then one wait
					__builtin_amdgcn_sched_barrier(0);   // (the scheduler would otherwise pair each load with its use again)
#pragma unroll
					for (int v = 0; v < HL; v++) mw[v] = (uint32_t)__builtin_amdgcn_readfirstlane((int)t[v]);
				};
#pragma unroll
				for (int v = 0; v < HL; v++) mw[v] = 0xFFFFFFFFu;
				if (kMaskDP && tmax >= 1) mask_words(0);
				const int rmax = (tmax >= 1) ? tmax - 1 : 0;   // last row of the tile
				// slot d <- the rows of position p (row p - 1)
				auto request = [&](auto dtag, auto leadtag, const int p) __attribute__((always_inline)) {
					constexpr int d = decltype(dtag)::v;
					constexpr bool with_lead = decltype(leadtag)::v != 0;
					const int nb = p - 1;
					if (kMaskDP && (nb & 31) == 0 && nb > 0 && nb < tmax) mask_words(nb >> 5);
					const int row = (nb < rmax) ? nb : rmax;
					const float* dpn = DP + ((int64_t)row * H + F1) * TD_WAVE + lane;
					uint32_t bits = 0;
#pragma unroll
					for (int v = 0; v < HL; v++) {
						if (with_lead || !label_leading(F1 + v)) {
							dq[d][v] = dpn[v * TD_WAVE];
							bits |= ((mw[v] >> (nb & 31)) & 1u) << v;
						} else {
							dq[d][v] = 0.0f;
						}
					}
					mq[d] = (nb < tmax) ? bits : 0u;
				};
#pragma unroll
				for (int d = 0; d < LD; d++) mq[d] = 0u;
				float bm_p = 0.0f;   // first-segment maximum at position i-1: all sums are 0 before the first position,
				int ba_p = 0;        // and the first of equals wins
				// its rows travel in the ring too (past the pruning cut the row is the one at the cut: BMROW)
				float bm_q[LD];
				int ba_q[LD];
				auto request_bm = [&](auto dtag, const int p) __attribute__((always_inline)) {
					constexpr int d = decltype(dtag)::v;
					if (F1 > 0) {
						const int pc = (p <= tmax) ? p : (tmax >= 1 ? tmax : 1);
						const int rb = BMROW(pc);
						bm_q[d] = w.bm[rb * TD_WAVE + lane]; ba_q[d] = w.ba[rb * TD_WAVE + lane];
					} else {
						bm_q[d] = 0.0f; ba_q[d] = 0;
					}
				};
				auto fill0 = [&](auto dtag, const int p) __attribute__((always_inline)) { request(dtag, IC<1>{}, p); request_bm(dtag, p); };
				ring_block<LD, 0>(fill0, 1);   // positions 1 .. LD
				auto dp_step = [&](auto dtag, auto leadtag, auto reqtag, const int i) __attribute__((always_inline)) {
					constexpr int d = decltype(dtag)::v;
					float dc[HL];
#pragma unroll
					for (int v = 0; v < HL; v++) dc[v] = dq[d][v];
					const uint32_t mc = mq[d];
					const float bm_c = bm_q[d];        // value at position i (for the next iteration)
					const int ba_c = ba_q[d];
					if (decltype(reqtag)::v) { request(dtag, leadtag, i + LD); request_bm(dtag, i + LD); }   // this slot's next occupant
					uint32_t pws[PWL > 0 ? PWL : 1];
#pragma unroll
					for (int k = 0; k < PWL; k++) pws[k] = 0u;
					if (i <= len) {
						uint32_t pw = 0;
	#pragma unroll
						for (int v = HL - 1; v >= 0; v--) {
							float m = -1.0f;
							int mv = 0;
							if (F1 > 0 && kPredFirst[F1 + v]) {                         // labels 0 .. F1-1 come first
								const bool gt = bm_p > m;
								m = gt ? bm_p : m;
								mv = gt ? ba_p : mv;
							}
	#pragma unroll
							for (int p = kPredOff2[F1 + v]; p < kPredOff2[F1 + v + 1]; p++) { // other predecessors u < v, ascending
								const int u = kPredIdx2[p] - F1;
								const bool gt = acc[u] > m;
								m = gt ? acc[u] : m;
								mv = gt ? u + F1 : mv;
							}
							const bool st = acc[v] >= m;    // staying in v wins ties (:4461-4464)
							m = st ? acc[v] : m;
							mv = st ? v + F1 : mv;
							acc[v] = (((mc >> v) & 1u) ? dc[v] : 0.0f) + m;
							pw |= (uint32_t)mv << (8 * (v & 3));
							if ((v & 3) == 0) { pws[v >> 2] = pw; pw = 0; }
						}
					}
					// (stored by every lane: a lane past its read never loads that row again)
					uint32_t* pathi = PATH + (int64_t)(i - 1) * PWL * TD_WAVE + lane;
#pragma unroll
					for (int k = 0; k < PWL; k++) if (!path_word_trivial(k)) pathi[k * TD_WAVE] = pws[k];
					bm_p = bm_c; ba_p = ba_c;
				};
				{
					auto step_a = [&](auto dtag, const int i) __attribute__((always_inline)) { dp_step(dtag, IC<1>{}, IC<1>{}, i); };
					auto step_b = [&](auto dtag, const int i) __attribute__((always_inline)) { dp_step(dtag, IC<0>{}, IC<1>{}, i); };
					auto step_r = [&](auto dtag, const int i) __attribute__((always_inline)) { dp_step(dtag, IC<0>{}, IC<0>{}, i); };
					int base = 1;
					// whole blocks whose first request (position base + LD) may still meet a row of the leading segments ...
					for (; base + LD - 1 <= tmax && (kPruneSegs == 0 || base + LD <= w.cut); base += LD) ring_block<LD, 0>(step_a, base);
					// ... and those past the cut
					for (; base + LD - 1 <= tmax; base += LD) ring_block<LD, 0>(step_b, base);
					ring_rest<LD, 0>(step_r, base, tmax);   // (what these positions need was requested by the last whole block)
				}
				TDS_PHASE(4);   // label DP
				{   // termination + traceback, :4494-4514
					float m = -1.0f;
					int move = 0;
					if (F1 > 0 && len >= 1) {
						const float bl = w.bm[BMROW(len) * TD_WAVE + lane];
						if (bl > m) { m = bl; move = w.ba[BMROW(len) * TD_WAVE + lane]; }
					}
	#pragma unroll
					for (int v = 0; v < HL; v++) {
						const bool gt = acc[v] > m;
						m = gt ? acc[v] : m;
						move = gt ? v + F1 : move;
					}
					if (len >= 1) labels[len * TD_WAVE + lane] = (int8_t)move;
					// The word a step needs depends on the previous step's move; all PWL words of the next positions are requested a
					// block of TDS_LDP steps ahead instead, so the chain of dependent steps never waits on memory.
					constexpr int LDT = TDS_LDT;   // the traceback's own request distance: a slot is PWL words, not a row of posteriors
					uint32_t wq[LDT][PWL > 0 ? PWL : 1];
					auto request_path = [&](auto dtag, const int r) __attribute__((always_inline)) {   // slot <- row r (clamped: unconditional, as above)
						constexpr int d = decltype(dtag)::v;
						const int rc = (r >= 0) ? r : 0;
#pragma unroll
						for (int k = 0; k < PWL; k++)
							wq[d][k] = path_word_trivial(k) ? path_word_identity(k) : PATH[((int64_t)rc * PWL + k) * TD_WAVE + lane];
					};
					// the walk goes down: slot d of a block starting at row `top` is row top - d (ring_block counts up, so it is
					// handed the negated row)
					auto tb_step = [&](auto dtag, auto reqtag, const int r) __attribute__((always_inline)) {
						constexpr int d = decltype(dtag)::v;
						uint32_t wc[PWL > 0 ? PWL : 1];
#pragma unroll
						for (int k = 0; k < PWL; k++) wc[k] = wq[d][k];
						if (decltype(reqtag)::v) request_path(dtag, r - LDT);   // this slot's next occupant
						const int i = r + 1;
						if (i <= len) {
							if (move >= F1) {          // a first-segment label has itself as its only way in
								const int ml = move - F1;
								uint32_t pwv = wc[0];
	#pragma unroll
								for (int k = 1; k < PWL; k++) pwv = ((ml >> 2) == k) ? wc[k] : pwv;
								move = (pwv >> (8 * (ml & 3))) & 0xFF;
							}
							labels[(i - 1) * TD_WAVE + lane] = (int8_t)move;
						}
					};
					if (tmax >= 1) {
						auto fillp = [&](auto dtag, const int nr) __attribute__((always_inline)) { request_path(dtag, -nr); };
						auto step_w = [&](auto dtag, const int nr) __attribute__((always_inline)) { tb_step(dtag, IC<1>{}, -nr); };
						auto step_r = [&](auto dtag, const int nr) __attribute__((always_inline)) { tb_step(dtag, IC<0>{}, -nr); };
						int nbase = -(tmax - 1);                 // rows tmax - 1, tmax - 2, ..: the steps at positions tmax, tmax - 1, ..
						ring_block<LDT, 0>(fillp, nbase);
						for (; nbase + LDT - 1 <= 0; nbase += LDT) ring_block<LDT, 0>(step_w, nbase);
						ring_rest<LDT, 0>(step_r, nbase, 0);
					}
				}

			} else {
				// ---- label DP for many labels: two rows in the workspace (previous / current position, so that the loads
				// of one label's step do not wait for the stores of another's), one path byte per (position, label) ----
				float* const ACCB = (float*)(w.slot + lay.acc);
				uint8_t* PATH8 = (uint8_t*)PATH;
				for (int v = 0; v < HL; v++) ACCB[v * TD_WAVE + lane] = 0.0f;
				float bm_p = 0.0f;
				int ba_p = 0;
				for (int i = 1; i <= tmax; i++) {
					if (i <= len) {
						const float* __restrict__ a0 = ACCB + (int64_t)((i - 1) & 1) * HL * TD_WAVE + lane;   // row of position i-1
						float* __restrict__ a1 = ACCB + (int64_t)(i & 1) * HL * TD_WAVE + lane;             // row of position i
						const float* __restrict__ dpi = DP + ((int64_t)(i - 1) * H + F1) * TD_WAVE + lane;
						uint8_t* __restrict__ pathi = PATH8 + (int64_t)(i - 1) * HL * TD_WAVE + lane;
						// Labels come in runs that share one predecessor set (kRunOff): the best predecessor is found once per
						// run, and both that scan and the run's own labels go eight at a time -- eight loads in flight, then
						// the arithmetic, then the stores -- instead of one memory round trip per label and operand.
						constexpr int CH = 8;
						for (int r = 0; r < kNRuns; r++) {
							const int v0 = kRunOff[r], v1 = kRunOff[r + 1];
							float m0 = -1.0f;
							int mv0 = 0;
							if (F1 > 0 && kPredFirst[F1 + v0]) {
								const bool gt = bm_p > m0;
								m0 = gt ? bm_p : m0;
								mv0 = gt ? ba_p : mv0;
							}
							const int p1 = kPredOff2[F1 + v0 + 1];
							for (int p = kPredOff2[F1 + v0]; p < p1; p += CH) {
								float au[CH];
								int uu[CH];
	#pragma unroll
								for (int k = 0; k < CH; k++) {
									uu[k] = (p + k < p1) ? kPredIdx2[p + k] - F1 : 0;
									au[k] = (p + k < p1) ? a0[uu[k] * TD_WAVE] : -2.0f;     // -2: never above the running maximum
								}
	#pragma unroll
								for (int k = 0; k < CH; k++) {
									const bool gt = au[k] > m0;
									m0 = gt ? au[k] : m0;
									mv0 = gt ? uu[k] + F1 : mv0;
								}
							}
							for (int v = v0; v < v1; v += CH) {
								float self[CH], dpv[CH];
	#pragma unroll
								for (int k = 0; k < CH; k++) {
									const bool in = v + k < v1;
									self[k] = in ? a0[(v + k) * TD_WAVE] : 0.0f;
									dpv[k] = in ? dpi[(v + k) * TD_WAVE] : 0.0f;
								}
	#pragma unroll
								for (int k = 0; k < CH; k++) {
									if (v + k < v1) {
										const bool st = self[k] >= m0;    // staying wins ties (:4461-4464)
										a1[(v + k) * TD_WAVE] = dpv[k] + (st ? self[k] : m0);
										pathi[(v + k) * TD_WAVE] = (uint8_t)(st ? v + k + F1 : mv0);
									}
								}
							}
						}
						if (F1 > 0) { bm_p = w.bm[BMROW(i) * TD_WAVE + lane]; ba_p = w.ba[BMROW(i) * TD_WAVE + lane]; }
					}
				}
				TDS_PHASE(4);   // label DP
				float m = -1.0f;
				int move = 0;
				if (F1 > 0 && len >= 1) {
					const float bl = w.bm[BMROW(len) * TD_WAVE + lane];
					if (bl > m) { m = bl; move = w.ba[BMROW(len) * TD_WAVE + lane]; }
				}
				{
					const float* fin = ACCB + (int64_t)(len & 1) * HL * TD_WAVE + lane;   // the row of each lane's last position
					for (int v = 0; v < HL; v++) {
						const float a = fin[v * TD_WAVE];
						const bool gt = a > m;
						m = gt ? a : m;
						move = gt ? v + F1 : move;
					}
				}
				if (len >= 1) labels[len * TD_WAVE + lane] = (int8_t)move;
				for (int i = tmax; i >= 1; i--) {
					if (i <= len) {
						if (move >= F1) move = PATH8[((int64_t)(i - 1) * HL + (move - F1)) * TD_WAVE + lane];
						labels[(i - 1) * TD_WAVE + lane] = (int8_t)move;
					}
				}
			}

			// with a window, ri->labels beyond it keeps the zeros read_fasta_fastq() put there (io.c:1755-1764)
			if (TDS_WINDOW && ka.win_len > 0) {
				for (int i = w.tmin + 1; i <= tmaxF; i++)
					if (i > len && i <= lenF) labels[i * TD_WAVE + lane] = 0;
			}
#if TDS_TEST_WRONG_RESULT == 2
			// test hook (see below): one interior label of every read of odd length becomes another valid label
			if (H > 1 && lenF >= 3 && (lenF & 1)) labels[1 * TD_WAVE + lane] = (int8_t)(labels[1 * TD_WAVE + lane] == 0 ? 1 : 0);
#endif
			// the label path as runs, for the compact egress: the wave reads back the column it has just written (L2-hot) -- labels
			// 0..lenF of a read whose window held a base, the one label 0 otherwise (what td_stage's finish kernel hands out)
			if (ka.out_runs) {
				uint32_t* runs = ka.out_runs + (int64_t)tile * ka.rle_cap * TD_WAVE + lane;
				// The runs gather in registers (the host's default capacity is S + 2 entries) and are stored once at the end: a store
				// behind the run logic's branches would make every later step of the scan wait for it.
				constexpr int RC = TD_S + 2;
				const bool in_regs = ka.rle_cap <= RC;   // (TD_RLE_CAP may ask for more: those go to memory as they end)
				uint32_t rr[RC];
#pragma unroll
				for (int j = 0; j < RC; j++) rr[j] = 0u;
				if (!in_regs) for (int j = 0; j < ka.rle_cap; j++) runs[j * TD_WAVE] = 0u;
				const int last = (lenF >= 1) ? lenF : 0;      // index of the read's last label
				int nr = 0, run = 0, cur = 0;
				auto put_run = [&]() __attribute__((always_inline)) {
					const uint32_t e = ((uint32_t)run << 8) | (uint32_t)(cur & 0xFF);
					if (in_regs) {
#pragma unroll
						for (int j = 0; j < RC; j++) rr[j] = (nr == j) ? e : rr[j];
					} else if (nr < ka.rle_cap) {
						runs[nr * TD_WAVE] = e;
					}
				};
				for (int p0 = 0; p0 <= tmaxF; p0 += 8) {   // eight labels requested together, then the (serial) run logic
					int vv[8];
#pragma unroll
					for (int k = 0; k < 8; k++) vv[k] = (lenF >= 1 && p0 + k <= lenF) ? (int)labels[(p0 + k) * TD_WAVE + lane] : 0;
					__builtin_amdgcn_sched_barrier(0);   // (the scheduler would otherwise pair each load with its use again)
#pragma unroll
					for (int k = 0; k < 8; k++) {
						const int p = p0 + k, v = vv[k];
						if (p <= last) {
							if (p == 0) { cur = v; run = 1; }
							else if (v == cur) run++;
							else {
								put_run();
								nr++; cur = v; run = 1;
							}
						}
					}
				}
				put_run();
				if (in_regs) {
#pragma unroll
					for (int j = 0; j < RC; j++) if (j < ka.rle_cap) runs[j * TD_WAVE] = rr[j];
				}
				if (nr >= ka.rle_cap) atomicOr(ka.rle_overflow, 1);
			}
			TDS_PHASE(5);   // traceback
			// ---- extract_reads, :3172-3313 ----
			bool extracted = false;
			for (int k = 0; k < nw1; k++) keep[k * TD_WAVE + lane] = 0xFFFFFFFFu;
			if (dead || len < 1 || !(ka.threshold <= Q)) {
				read_type = OUT_ARCH_MISMATCH;
			} else {
				uint32_t key = 0;
				int bar = -1, mem = -1, fingerlen = 0, s_pos = 0, has_bar = 0;
				bool too_short = false, in_read = false, stopped = false;
				uint32_t kw = 0;
				// the label of the next position is requested one step ahead; the per-label info word comes from a select
				// chain over the (few) labels rather than from a table in memory: two dependent memory round trips per
				// position are what this loop would otherwise consist of
				// make_extracted_read (:3336-3352) walks the whole read with labels[j+1] on position j: beyond a window those
				// labels are 0, i.e. HMM 0 of segment 0 -- kept only if that segment is a read segment
				constexpr bool tail_kept = (kHinfo[0] & 0xFF) == 'R';
				const int xmax = (TDS_WINDOW && ka.win_len > 0) ? tmaxF : tmax;
				for (int jx0 = 0; jx0 < xmax; jx0 += 8) {
				int labq[8];   // eight labels requested together
#pragma unroll
				for (int k = 0; k < 8; k++) labq[k] = (jx0 + k < xmax) ? (int)labels[(jx0 + k + 1) * TD_WAVE + lane] : 0;
				__builtin_amdgcn_sched_barrier(0);   // (the scheduler would otherwise pair each load with its use again)
#pragma unroll
				for (int k = 0; k < 8; k++) {
					const int jx = jx0 + k;
					if (jx < xmax) {
					const int lab = labq[k];
					if (jx < len) {
						uint32_t hi;
						if constexpr (H <= TDS_REG_H) {
							hi = kHinfo[0];
		#pragma unroll
							for (int v = 1; v < H; v++) hi = (lab == v) ? kHinfo[v] : hi;
						} else {
							hi = kHinfo[lab];
						}
						const int ty = hi & 0xFF;
						if (!stopped) {
							if (ty == 'F') {
								fingerlen++;
								key = (key << 2) | (uint32_t)(codes[(jx + 1) * TD_WAVE + lane] & 3);
							}
							if (ty == 'B') {
								has_bar = (hi >> 31) ? -1 : 1;
								bar = (hi >> 16) & 0x7FFF;
								mem = (hi >> 8) & 0xFF;
							}
							if (ty == 'R') {
								s_pos++;
								in_read = true;
							} else {
								if (in_read && s_pos < ka.minlen) { too_short = true; stopped = true; }
								in_read = false;
								s_pos = 0;
							}
						}
						if (ty == 'R') kw |= 1u << (jx & 31);
					} else if (TDS_WINDOW && jx < lenF && tail_kept) {
						kw |= 1u << (jx & 31);
					}
					if ((jx & 31) == 31 || jx == xmax - 1) { keep[(jx >> 5) * TD_WAVE + lane] = kw; kw = 0; }
					}
				}
				}
				if (in_read && s_pos < ka.minlen) too_short = true;
				constexpr int req = TD_REQ_FINGER;
				const int fp = (int)((key << 8) | (uint32_t)(req <= 255 ? req : 255));
				if (too_short) {
					read_type = OUT_TOO_SHORT;
				} else if (has_bar == -1) {
					read_type = OUT_BAR_FINGER_NOT_FOUND;
				} else if (has_bar && req) {
					if (fingerlen == req && bar != -1) { extracted = true; barcode = (mem << 16) | bar; fingerprint = fp; }
					else read_type = OUT_BAR_FINGER_NOT_FOUND;
				} else if (has_bar) {
					if (bar != -1) { extracted = true; barcode = (mem << 16) | bar; }
					else read_type = OUT_BAR_FINGER_NOT_FOUND;
				} else if (req) {
					if (fingerlen == req) { extracted = true; fingerprint = fp; }
					else read_type = OUT_BAR_FINGER_NOT_FOUND;
				} else {
					extracted = true;
				}
				if (extracted) read_type = OUT_SUCCESS;
			}
			if (!extracted) for (int k = 0; k < nw1; k++) keep[k * TD_WAVE + lane] = 0xFFFFFFFFu;

			TDS_PHASE(6);   // extraction
			// ---- match_to_reference, :2478-2583 (td_artifact.inc) ----
			if (ka.art_n > 0) {
				const uint8_t* cd = codesF;
				auto sq = [&](int kk) -> int {
					return ((keep[(kk >> 5) * TD_WAVE + lane] >> (kk & 31)) & 1u) ? (int)cd[(kk + 1) * TD_WAVE + lane] : 65;
				};
				const int id = td_art_match(sq, lenF, tmaxF, ka.art_left[rid] != 0, ka.art_text, ka.art_index, ka.art_n, ka.art_fe);
				if (id > 0 && read_type == OUT_SUCCESS) read_type = (id << 8) | OUT_MATCHES_ARTIFACTS;
			}

			TDS_PHASE(7);   // artifacts
			// ---- dust_sequences, :2407-2467, on the rewritten sequence ----
			// One wave-uniform pass over the first 64 positions with a per-lane state machine (skip the leading spacer
			// bytes, take two characters for the first key, then count triplets until a spacer byte or the 64th
			// character); the 64 triplet counters are 8-bit fields of 16 registers, updated through a select chain --
			// no memory round trip per position.
			if (ka.dust) {
				const uint32_t kw0 = keep[lane], kw1 = (nw1 > 1) ? keep[TD_WAVE + lane] : 0u;
				uint32_t cnt[16];
	#pragma unroll
				for (int k = 0; k < 16; k++) cnt[k] = 0u;
				const int n = lenF > 64 ? 64 : lenF;
				const int scan = tmaxF > 64 ? 64 : tmaxF;
				int state = 0, c0 = 0, key = 0, cc = 0;     // 0: skipping, 1: first character seen, 2: counting, 3: stopped
				for (int jx0 = 0; jx0 < scan; jx0 += 8) {
				int cq8[8];   // eight characters requested together (scan <= 64 <= the tile's rows)
	#pragma unroll
				for (int k = 0; k < 8; k++) cq8[k] = codesF[((jx0 + k < scan ? jx0 + k : scan - 1) + 1) * TD_WAVE + lane];
				__builtin_amdgcn_sched_barrier(0);
	#pragma unroll
				for (int k = 0; k < 8; k++) {
					const int jx = jx0 + k;
					if (jx < scan) {
					const int code = cq8[k];
					const bool kept = (((jx < 32) ? kw0 >> jx : kw1 >> (jx - 32)) & 1u) != 0u;
					const int ch = (jx < lenF) ? (kept ? code : 65) : 0;   // the reference's seq carries a 0 terminator
					if (state == 0) {
						if (ch != 65) { state = 1; c0 = jx; key = (ch & 3) << 2; }
					} else if (state == 1) {
						key |= ch & 3;
						cc = c0 + 2;
						state = 2;
					} else if (state == 2 && jx < n) {
						if (ch == 65) {
							state = 3;
						} else {
							key = (int)(((uint32_t)key << 2) | (uint32_t)(ch & 3));
							const uint32_t inc = 1u << (8 * (key & 3));
							const int wsel = (key & 63) >> 2;
	#pragma unroll
							for (int k2 = 0; k2 < 16; k2++) cnt[k2] += (wsel == k2) ? inc : 0u;
							cc++;
						}
					}
					}
				}
				}
				// leading spacer bytes all the way through the scanned part (or a first character at the very end): no
				// triplet is counted, s = 0 / (cc - 3) * 10 with cc = c0 + 2
				if (state == 0) { c0 = scan; while (c0 < lenF && !((keep[(c0 >> 5) * TD_WAVE + lane] >> (c0 & 31)) & 1u)) c0++; cc = c0 + 2; }
				if (state == 1) cc = c0 + 2;
				double sd = 0.0;
	#pragma unroll
				for (int k = 0; k < 64; k++) {
					const double tcount = (double)((cnt[k >> 2] >> (8 * (k & 3))) & 0xFFu);
					sd += tcount * (tcount - 1.0) / 2.0;
				}
				sd = sd / (double)(cc - 3) * 10.0;
				if (lenF >= 1 && sd > (double)ka.dust) read_type = OUT_LOW_COMPLEXITY;
			}
		}

		TDS_PHASE(8);   // DUST
#if TDS_TEST_WRONG_RESULT == 1
		// test hook: -DTDS_TEST_WRONG_RESULT=k through TD_SPEC_EXTRA_OPTS (part of the cache key, absent from every normal build) makes
		// the kernel compute wrong VALUES -- nothing is read or written that it would not read or write anyway -- so that the load-time
		// probe (td_api.hip) has something to reject: k = 1 flips the lowest mantissa bit of b_score in one lane of every tile, k = 2
		// (above) changes one label of every read of odd length.
		if (lane == 5) b_score = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, b_score) ^ 1u);
#endif
		ka.out_f[rid] = f_score;
		ka.out_b[rid] = b_score;
		ka.out_r[rid] = r_score;
		ka.out_bar[rid] = bar_prob;
		ka.out_q[rid] = Q;
		ka.out_type[rid] = read_type;
		ka.out_barcode[rid] = barcode;
		ka.out_finger[rid] = fingerprint;
		if (ka.mode == MODE_GET_LABEL) {
			// Outcome counters (the controller's serial counting, barcode_hmm.c:354-384): one atomic per wave and distinct value,
			// not one per read.  A million reads adding 1 to the same two or three words is a million atomics queued on one L2
			// channel -- they return nothing, so no phase of the wave clock shows them, but every memory operation of the
			// machine waits behind them: 4 ms of an 18.5 ms launch on config 3, 8.4 of 13.2 on config 2.
			const int key1 = (lenF >= 1) ? (read_type & (N_OUTCOME_SLOTS - 1)) : -1;
			const int key2 = (lenF >= 1 && read_type == OUT_SUCCESS && barcode >= 0) ? N_OUTCOME_SLOTS + (barcode & 0xFF) : -1;
#pragma unroll
			for (int pass = 0; pass < 2; pass++) {
				const int key = pass ? key2 : key1;
				unsigned long long todo = __builtin_amdgcn_ballot_w64(key >= 0);
				while (todo) {   // one round per distinct value among the wave's reads
					const int leader = __builtin_ctzll(todo);
					const int kv = __builtin_amdgcn_readlane(key, leader);
					const unsigned long long same = __builtin_amdgcn_ballot_w64(key == kv);
					if (lane == leader) atomicAdd(&ka.counters[kv], (unsigned long long)__builtin_popcountll(same));
					todo &= ~same;
				}
			}
		}
		TDS_PHASE(9);   // outputs
	}
#ifdef TDS_ENDSTATS
	if (lane == 0) {
		const unsigned long long t_end = wall_clock64();
		atomicMin(&ka.counters[TDS_DIAG(200)], t_start); atomicMax(&ka.counters[TDS_DIAG(201)], t_start);
		atomicMin(&ka.counters[TDS_DIAG(202)], t_end); atomicMax(&ka.counters[TDS_DIAG(203)], t_end);
		atomicAdd(&ka.counters[TDS_DIAG(204)], t_end); atomicAdd(&ka.counters[TDS_DIAG(205)], 1ull);
		atomicAdd(&ka.counters[TDS_DIAG(208 + (blockIdx.x & 7))], t_end - t_start);        // by XCD (round-robin dispatch)
		atomicAdd(&ka.counters[TDS_DIAG(216 + ((threadIdx.x >> 6) & 7))], t_end - t_start); // by wave in the workgroup
		atomicMax(&ka.counters[TDS_DIAG(192 + (blockIdx.x & 7))], t_end - t_start);
	}
#endif
}

// ---------------------------------------------------------------------------------------------------------
// Self-check of lsum() as compiled, run once by the host after the module is loaded: the clamp-free form leans on an LDS
// read past the workgroup's allocation returning 0 and on g_T sitting at LDS address 0.  Each lane evaluates one operand
// pair (chosen at run time, so nothing folds) with lsum() and with the reference's own formula (src/misc.c:72-78, written
// out with the clamp); *bad counts the lanes whose results differ in any bit.
// ---------------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(TDS_BLOCK) void td_spec_selfcheck(const float* __restrict__ logsum, const float* __restrict__ pairs,
                                                                           int n_pairs, int* __restrict__ bad)
{
	for (int k = threadIdx.x; k < TDS_TABLE_N; k += TDS_BLOCK) g_T[k] = (k < TD_LOGSUM_LIVE) ? logsum[k] : 0.0f;
	__syncthreads();
	const int t = threadIdx.x;
	if (t >= n_pairs) return;
	const float a = pairs[2 * t], b = pairs[2 * t + 1];
	const float got = lsum(a, b);
	const float mx = fmaxf(a, b), mn = fminf(a, b);
	float want;
	if (mn == NEG_INF || mx - mn >= 15.7f) want = mx;
	else want = mx + logsum[(int)((mx - mn) * 1000.0f)];
	if (__builtin_bit_cast(unsigned, got) != __builtin_bit_cast(unsigned, want) && !(got != got && want != want)) atomicAdd(bad, 1);
}
