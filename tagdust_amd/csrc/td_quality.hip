// td_quality.hip -- the base-quality filter (include/tagdust_quality.h): reads with too many low-quality barcode or UMI bases are
// dropped, judged on the device.
//
// The threshold is applied on the host while a batch is staged (qual_stage: td_qual_pack's pass on the context's workers, into the
// slot's page-locked words), so one bit per base crosses the link.  Behind every TD_MODE_GET_LABEL launch of a context with the
// filter on, one small kernel reads what the decode kernel left in device order -- the outcome and the lane-interleaved label
// bytes -- and counts each eligible read's bases that are both low and of a judged segment; a read with more than max_low of
// them gets outcome TD_EXTRACT_FAIL_LOW_BASE_QUALITY.  One read per lane, one tile per wave, like the decode kernels and the
// census.  It stands behind the mate join and the -ref hits and in front of sample assignment, census and molecule count in
// launch_end (td_batch.hip): they all read one verdict per read.  The same definition over host arrays (td_qual_host) and the pack
// are in td_quality_host.cpp.
#include <hip/hip_runtime.h>

#include "td_ctx.h"

__global__ __launch_bounds__(KT_BLOCK) void td_qual_judge_kernel(const TdQualArgs a)
{
	// per label: 1 = a base of a judged segment, 2 = a segment behind the last judged one (only where the path cannot come back)
	__shared__ uint8_t s_cls[128];
	kt_label_classes(s_cls, a.label, a.H, [&](int seg) { return seg > a.last_judged ? 2 : (seg < TD_MAX_SEGMENTS ? (int)((a.judged >> seg) & 1ull) : 0); });
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int tile = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
	if (tile >= a.n_tiles) return;                    // (whole waves; no workgroup barrier below)
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	bool elig = false;
	int len = 0;
	int64_t g0 = 0;
	if (k < a.n_reads) {                              // the outcome first: the other lanes read nothing more
		elig = a.out_type[k] == TD_EXTRACT_SUCCESS;
		if (elig) {
			len = a.lens[k];
			if (len > a.lmax) len = a.lmax;           // (the batch's longest read: every label index below stays inside the tile's array)
			g0 = a.offs[a.read_at ? (int64_t)a.read_at[k] : k];
		}
	}
	if (__builtin_amdgcn_ballot_w64(elig) == 0ull) return;
	int tmax = len;
	for (int o = 32; o >= 1; o >>= 1) { const int t2 = __shfl_xor(tmax, o); tmax = t2 > tmax ? t2 : tmax; }
	const int8_t* lb = a.labels + (int64_t)tile * (a.lmax + 1) * TD_WAVE + lane;
	int n_low = 0;
	bool behind = false;                              // the lane's path has left the last judged segment for good
	for (int p0 = 0; p0 < tmax; p0 += 32) {
		// the low flags of bases p0 .. p0 + 31 of the lane's read: its own word and the one behind it, shifted together (the spare
		// zero word at the end keeps the second load inside the buffer)
		uint32_t low = 0u;
		if (p0 < len && !behind) {
			const int64_t g = g0 + p0;
			int64_t w = g >> 5;
			if (w > a.n_words - 2) w = a.n_words - 2;
			low = __builtin_amdgcn_alignbit(a.words[w + 1], a.words[w], (uint32_t)g & 31u);
			if (len - p0 < 32) low &= (1u << (len - p0)) - 1u;
		}
		const bool walk = low != 0u;
		if (__builtin_amdgcn_ballot_w64(walk) == 0ull) continue;        // no low base in any lane's block: its labels are not read at all
		// the block's labels of every lane with a low base in it: 32 loads that do not wait for one another, then one popcount
		uint32_t judged = 0u;
		const int nb = len - p0;
#pragma unroll
		for (int q = 0; q < 32; q++) {
			if (walk && q < nb) {
				const uint32_t lab = (uint8_t)lb[(int64_t)(p0 + q + 1) * TD_WAVE];   // labels[p + 1] belongs to base p
				const uint32_t cls = lab < 128u ? (uint32_t)s_cls[lab] : 0u;
				judged |= (cls == 1u ? 1u : 0u) << q;
				behind = behind || cls == 2u;                                 // no judged base follows: the lane's later blocks are not read
			}
		}
		n_low += __builtin_popcount(judged & low);
	}
	const bool failed = elig && n_low > a.max_low;
	if (failed) a.out_type[k] = TD_EXTRACT_FAIL_LOW_BASE_QUALITY;
	// tallies: one add per wave and tally, into the workgroup's copy of them (QL_COPIES copies, a cache line each: the adds of
	// every wave of a launch on one address queue up behind one another); passed is eligible - failed
	const int n_elig = __builtin_popcountll(__builtin_amdgcn_ballot_w64(elig));
	const int n_failed = __builtin_popcountll(__builtin_amdgcn_ballot_w64(failed));
	const int low_sum = kt_wave_sum(n_low);
	if (lane == 0) {
		unsigned long long* t = a.tallies + (size_t)(blockIdx.x & (QL_COPIES - 1)) * QL_COPY_WORDS;
		atomicAdd(&t[QL_ELIGIBLE], (kt_u64)n_elig);
		if (n_failed) atomicAdd(&t[QL_FAILED], (kt_u64)n_failed);
		if (low_sum) atomicAdd(&t[QL_LOW_BASES], (kt_u64)low_sum);
	}
}

void qual_release(td_ctx* c)
{
	TdQualState& z = c->quality;
	if (z.d_label) (void)hipFree(z.d_label);
	if (z.d_tallies) (void)hipFree(z.d_tallies);
	kt_pair_destroy(z.ev);
	const int32_t gen = z.gen;
	z = TdQualState();
	z.gen = gen;
}

int qual_check(td_ctx* c, int64_t n, const char* who)
{
	TdQualState& z = c->quality;
	if (!z.named)
		return fail(c, "%s: the base-quality filter is on (td_qual_enable) and no qualities are named for this batch of %lld reads (td_qual_next "
		            "first); nothing was decoded", who, (long long)n);
	if (z.next_reads != n) {
		z.named = false;
		return fail(c, "%s: the named qualities are those of %lld reads, the batch has %lld: read i's bytes are at qual + offs[i]; the name is "
		            "dropped (td_qual_next again), nothing was decoded", who, (long long)z.next_reads, (long long)n);
	}
	return TD_OK;
}

int qual_stage(td_ctx* c, TdSlot& s, const int64_t* offs, int64_t n, hipStream_t up)
{
	TdQualState& z = c->quality;
	const uint8_t* qual = z.next_qual;
	z.named = false;                                  // consumed, whatever happens below
	const int64_t base = offs[0], n_bases = n > 0 ? offs[n] - base : 0;
	if (n_bases > 0 && !qual) return fail(c, "td_qual_next: no quality bytes for a batch of %lld bases", (long long)n_bases);
	const int64_t n_blocks = (n_bases + 31) / 32, n_words = n_blocks + 1;
	if (ensure_pinned(c, &s.h_qual_w, &s.cap_h_qual_w, (size_t)n_words * 4) != TD_OK || ensure(c, &s.d_qual_w, &s.cap_qual_w, (size_t)n_words * 4) != TD_OK)
		return TD_FAIL;
	// every worker takes whole words: a range starts at a multiple of 32 bases
	const int32_t thr = z.plan.thr;
	uint32_t* words = s.h_qual_w;
	const uint8_t* src = qual + base;
	c->pool.ranges(n_blocks, c->host_threads, [=](int64_t lo, int64_t hi) {
		qual_pack_range(src, lo * 32, hi * 32 < n_bases ? hi * 32 : n_bases, thr, words);
	});
	words[n_blocks] = 0u;
	HIPCHK(c, hipMemcpyAsync(s.d_qual_w, s.h_qual_w, (size_t)n_words * 4, hipMemcpyHostToDevice, up));
	s.qual_gen = z.gen;
	s.qual_words = n_words;
	return TD_OK;
}

int qual_slot(td_ctx* c, TdSlot& s, int32_t* out_type, const int8_t* labels)
{
	const TdQualState& z = c->quality;
	TdQualArgs a{};
	a.labels = labels; a.lens = s.d_lens; a.out_type = out_type; a.offs = s.d_offs; a.read_at = s.sorted ? s.d_read_at : nullptr;
	a.words = s.d_qual_w; a.label = z.d_label; a.judged = z.plan.judged; a.last_judged = z.last_judged;
	a.n_reads = s.n_reads; a.n_words = s.qual_words; a.n_tiles = s.n_tiles; a.lmax = s.lmax; a.H = z.H; a.max_low = z.plan.p.max_low;
	a.tallies = z.d_tallies;
	if (kt_launch_slot(c, z.ev, s, (const void*)td_qual_judge_kernel, &a) != TD_OK) return TD_FAIL;
	return kt_slot_read_behind(c, s);
}

extern "C" int td_qual_enable(td_ctx* c, int32_t min_quality, int32_t offset, int32_t max_low, int32_t segments)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_qual_enable: no model uploaded");
	if (tickets_outstanding(c)) return fail(c, "td_qual_enable: td_submit tickets are outstanding (td_wait them first)");
	const td_qual_params p{ min_quality, offset, max_low, segments };
	TdQualPlan plan;
	if (qual_plan_build(c, "td_qual_enable", &c->model.d, &p, plan) != TD_OK) return TD_FAIL;
	if (c->match_len > 0) return fail(c, "td_qual_enable: a -start/-end window is set (td_set_window): labels behind a window do not mark the bases");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	qual_release(c);
	TdQualState& z = c->quality;
	const td_model_desc& m = c->model.d;
	hipError_t e = hipMalloc((void**)&z.d_label, sizeof(int32_t) * (size_t)m.H);
	if (e == hipSuccess) e = hipMalloc((void**)&z.d_tallies, QL_TALLY_BYTES);
	if (e == hipSuccess) e = hipMemcpy(z.d_label, m.label, sizeof(int32_t) * (size_t)m.H, hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemset(z.d_tallies, 0, QL_TALLY_BYTES);
	if (e == hipSuccess) e = kt_pair_create(z.ev);
	if (e != hipSuccess) {
		qual_release(c);
		return fail(c, "td_qual_enable: the filter could not be set up: %s", hipGetErrorString(e));
	}
	z.plan = plan;
	z.H = m.H;
	// where model.label's segments never decrease with the HMM index a path never comes back to a segment it has left: the walk of
	// a read ends at the first low base behind the last judged segment (the census's rule, td_census.hip); else it never ends early
	bool ordered = true;
	for (int h = 0; h + 1 < m.H; h++) if ((m.label[h] & 0xFFFF) > (m.label[h + 1] & 0xFFFF)) ordered = false;
	z.last_judged = TD_MAX_SEGMENTS;
	if (ordered) for (int j = 0; j < m.S; j++) if ((plan.judged >> j) & 1ull) z.last_judged = j;
	z.gen++;
	z.on = true;
	return TD_OK;
}

extern "C" int td_qual_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	if (!c->quality.on) return TD_OK;
	if (tickets_outstanding(c)) return fail(c, "td_qual_disable: td_submit tickets are outstanding (td_wait them first)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	qual_release(c);
	return TD_OK;
}

extern "C" int td_qual_reset(td_ctx* c)
{
	if (!c) return TD_FAIL;
	TdQualState& z = c->quality;
	if (!z.on) return fail(c, "td_qual_reset: the base-quality filter is off (td_qual_enable)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;   // (verdicts of pipelined batches may still be queued, on either compute stream)
	HIPCHK(c, hipMemsetAsync(z.d_tallies, 0, QL_TALLY_BYTES, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return TD_OK;
}

extern "C" int td_qual_get(td_ctx* c, td_qual_totals* totals)
{
	if (!c) return TD_FAIL;
	TdQualState& z = c->quality;
	if (!z.on) return fail(c, "td_qual_get: the base-quality filter is off (td_qual_enable)");
	if (!totals) return fail(c, "td_qual_get: bad arguments");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	kt_u64 t[QL_COPIES * QL_COPY_WORDS];
	HIPCHK(c, hipMemcpy(t, z.d_tallies, sizeof t, hipMemcpyDeviceToHost));
	td_qual_totals sum{};
	for (int k = 0; k < QL_COPIES; k++) {
		sum.eligible += (int64_t)t[k * QL_COPY_WORDS + QL_ELIGIBLE]; sum.failed += (int64_t)t[k * QL_COPY_WORDS + QL_FAILED];
		sum.low_bases += (int64_t)t[k * QL_COPY_WORDS + QL_LOW_BASES];
	}
	sum.passed = sum.eligible - sum.failed;
	*totals = sum;
	return TD_OK;
}

extern "C" int td_qual_next(td_ctx* c, const uint8_t* qual, int64_t n_reads)
{
	if (!c) return fail(nullptr, "td_qual_next: no context");
	TdQualState& z = c->quality;
	if (!z.on) return fail(c, "td_qual_next: the base-quality filter is off (td_qual_enable)");
	if (n_reads < 0) return fail(c, "td_qual_next: bad arguments");
	z.next_qual = qual; z.next_reads = n_reads; z.named = true;
	return TD_OK;
}

// the judge kernel's time of the last batch, for tools/quality_bench.py (option "quality_kernel_us" of td_get_option)
int qual_last_kernel_us(td_ctx* c, int32_t* us)
{
	if (!c->quality.on) return fail(c, "td_get_option: quality_kernel_us: the base-quality filter is off");
	return kt_last_kernel_us(c, c->quality.ev, us, "td_get_option: quality_kernel_us: no batch has been judged yet");
}
