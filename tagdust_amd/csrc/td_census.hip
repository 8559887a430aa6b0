// td_census.hip -- the census of barcode spellings (include/tagdust_census.h): what stood where the barcode should have been.
//
// Behind every TD_MODE_GET_LABEL launch of a context with the census on, one small kernel reads what the decode kernel left in
// device order -- the outcome, the lane-interleaved label bytes, the packed bases with their N mask -- builds each eligible read's
// word for the chosen 'B' segment and counts it in an open-addressing table in HBM.  One read per lane, one tile per wave, like
// the decode kernels.  Lanes of a wave that hold the same key leave as one probe and one add of their number; the distinct keys
// of a wave probe side by side.  Nothing is ever removed from the table and the probe window is fixed, so a key finds or claims
// its slot on every attempt or fails on every attempt: a reported count is exact, what did not fit is in the overflow tally.
// The same definition over host arrays (td_census_host), td_census_merge and td_census_key_text are in td_census_host.cpp.
#include <hip/hip_runtime.h>

#include "../../include/tagdust_census.h"
#include "td_ctx.h"

__global__ __launch_bounds__(KT_BLOCK) void td_census_count_kernel(const TdCensusArgs a)
{
	// per label: 1 = the segment, 2 = a later segment, 0 = an earlier one
	__shared__ uint8_t s_cls[128];
	kt_label_classes(s_cls, a.label, a.H, [&](int seg) { return seg == a.segment ? 1 : (seg > a.segment ? 2 : 0); });
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int tile = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
	if (tile >= a.n_tiles) return;                    // (whole waves; no workgroup barrier below)
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	bool elig = false;
	int len = 0;
	if (k < a.n_reads) {                              // the outcome first: the other lanes read nothing more
		const uint32_t t = (uint32_t)a.out_type[k] & 0xFFu;
		elig = t < 8u && ((a.mask >> t) & 1u) != 0u;
		if (elig) len = a.lens[k];
	}
	if (__builtin_amdgcn_ballot_w64(elig) == 0ull) return;
	kt_u64 w = 0ull;
	int n = 0;
	bool has_n = false;
	kt_walk_tile(a.tile, s_cls, tile, lane, len, [&](uint32_t cls, uint32_t base, bool base_is_n) {
		if (cls == 1u) {
			n++;
			if (n <= TD_CENSUS_MAX_WORD) { w = (w << 2) | (kt_u64)base; has_n = has_n || base_is_n; }
		} else if (cls == 2u && a.ordered) return false;             // the path has left the segment for good
		return true;
	});
	const bool is_empty = elig && n == 0, is_long = elig && n > TD_CENSUS_MAX_WORD;
	const bool is_n = elig && !is_empty && !is_long && has_n;
	const bool has_key = elig && !is_empty && !is_long && !has_n;
	const KtWaveAdded added = kt_wave_add(a.table, has_key, has_key ? (((kt_u64)n << 56) | w) : 0ull, lane);
	// tallies: one add per wave and tally
	const int n_elig = __builtin_popcountll(__builtin_amdgcn_ballot_w64(elig));
	const int n_empty = __builtin_popcountll(__builtin_amdgcn_ballot_w64(is_empty));
	const int n_long = __builtin_popcountll(__builtin_amdgcn_ballot_w64(is_long));
	const int n_n = __builtin_popcountll(__builtin_amdgcn_ballot_w64(is_n));
	if (lane == 0) {
		atomicAdd(&a.tallies[TDC_ELIGIBLE], (kt_u64)n_elig);
		if (added.counted) atomicAdd(&a.tallies[TDC_COUNTED], (kt_u64)added.counted);
		if (n_empty) atomicAdd(&a.tallies[TDC_EMPTY], (kt_u64)n_empty);
		if (n_long) atomicAdd(&a.tallies[TDC_LONG], (kt_u64)n_long);
		if (n_n) atomicAdd(&a.tallies[TDC_N], (kt_u64)n_n);
		if (added.overflow) atomicAdd(&a.tallies[TDC_OVERFLOW], (kt_u64)added.overflow);
		if (added.fresh) atomicAdd(&a.tallies[TDC_DISTINCT], (kt_u64)added.fresh);
	}
}

void census_release(td_ctx* c)
{
	kt_table_release(c->census.table);
	c->census = TdCensusState();
}

int census_count_slot(td_ctx* c, TdSlot& s, const int32_t* out_type, const int8_t* labels)
{
	const TdCensusState& z = c->census;
	TdCensusArgs a{};
	a.tile = kt_tile_view(s, labels); a.lens = s.d_lens; a.out_type = out_type; a.label = z.table.d_label;
	a.n_reads = s.n_reads; a.n_tiles = s.n_tiles; a.H = z.table.H;
	a.segment = z.segment; a.ordered = z.ordered ? 1 : 0; a.mask = z.mask;
	a.table = kt_table_view(z.table); a.tallies = z.table.d_tallies;
	if (kt_launch_slot(c, z.table.ev, s, (const void*)td_census_count_kernel, &a) != TD_OK) return TD_FAIL;
	return kt_slot_read_behind(c, s);
}

extern "C" int td_census_enable(td_ctx* c, int32_t segment, uint32_t outcome_mask, int32_t log2_slots)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_census_enable: no model uploaded");
	if (tickets_outstanding(c)) return fail(c, "td_census_enable: td_submit tickets are outstanding (td_wait them first)");
	int32_t seg = -1;
	if (census_pick_segment(c, "td_census_enable", &c->model.d, segment, &seg) != TD_OK) return TD_FAIL;
	if (!census_mask_ok(outcome_mask)) return fail(c, "td_census_enable: outcome_mask 0x%x is not a non-empty subset of bits 0..7", outcome_mask);
	if (log2_slots < 4 || log2_slots > 26) return fail(c, "td_census_enable: log2_slots = %d (4..26 supported)", log2_slots);
	if (c->match_len > 0) return fail(c, "td_census_enable: a -start/-end window is set (td_set_window): labels behind a window do not spell the barcode");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	census_release(c);
	TdCensusState& z = c->census;
	const td_model_desc& m = c->model.d;
	const hipError_t e = kt_table_create(z.table, m.label, m.H, log2_slots, TDC_TALLY_WORDS);
	if (e != hipSuccess) {
		census_release(c);
		return fail(c, "td_census_enable: a table of 2^%d slots could not be set up: %s", log2_slots, hipGetErrorString(e));
	}
	z.segment = seg; z.mask = outcome_mask;
	z.ordered = true;
	for (int h = 0; h + 1 < m.H; h++) if ((m.label[h] & 0xFFFF) > (m.label[h + 1] & 0xFFFF)) z.ordered = false;
	z.on = true;
	return TD_OK;
}

extern "C" int td_census_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	if (!c->census.on) return TD_OK;
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	census_release(c);
	return TD_OK;
}

extern "C" int td_census_reset(td_ctx* c)
{
	if (!c) return TD_FAIL;
	TdCensusState& z = c->census;
	if (!z.on) return fail(c, "td_census_reset: the census is off (td_census_enable)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;   // (counts of pipelined batches may still be queued, on either compute stream)
	HIPCHK(c, kt_table_zero(z.table, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return TD_OK;
}

extern "C" int td_census_get(td_ctx* c, td_census_entry* entries, int64_t cap, int64_t* n, td_census_totals* totals)
{
	if (!c) return TD_FAIL;
	TdCensusState& z = c->census;
	if (!z.on) return fail(c, "td_census_get: the census is off (td_census_enable)");
	kt_u64 t[TDC_TALLY_WORDS];
	if (kt_table_entries(c, "td_census_get", z.table, TDC_DISTINCT, TDC_CURSOR, entries, cap, n, t) != TD_OK) return TD_FAIL;
	if (totals) {
		totals->eligible = (int64_t)t[TDC_ELIGIBLE]; totals->counted = (int64_t)t[TDC_COUNTED]; totals->skipped_empty = (int64_t)t[TDC_EMPTY];
		totals->skipped_long = (int64_t)t[TDC_LONG]; totals->skipped_n = (int64_t)t[TDC_N]; totals->overflow = (int64_t)t[TDC_OVERFLOW];
		totals->distinct = *n;
	}
	return TD_OK;
}

// the count kernel's time of the last batch, for tools/census_bench.py (option "census_kernel_us" of td_get_option)
int census_last_kernel_us(td_ctx* c, int32_t* us)
{
	const TdCountTable& t = c->census.table;
	if (!c->census.on) return fail(c, "td_get_option: census_kernel_us: the census is off");
	return kt_last_kernel_us(c, t.ev, us, "td_get_option: census_kernel_us: no batch has been counted yet");
}
