// td_samples.hip -- sample assignment by all 'B' segments (include/tagdust_samples.h): a read's sample is the tuple of its barcode calls.
//
// Behind every TD_MODE_GET_LABEL launch of a context with samples on, one small kernel reads what the decode kernel left in device
// order -- the outcome and the lane-interleaved label bytes -- takes each eligible read's call for every chosen segment (the last
// position with a label of that segment wins), looks the tuple up in the sheet and rewrites the read's outcome or barcode; every
// eligible read's tuple is counted in an open-addressing table in HBM (td_keytable.h).  One read per lane, one tile per wave, like
// the decode kernels and the census.  It stands in front of the census and the molecule count in launch_end (td_batch.hip): both
// read one sample per read.  The rewrite never depends on the table.  A read's class and key are td_samples_def.h's, the text
// td_samples_host (td_samples_host.cpp) compiles too.
#include <hip/hip_runtime.h>

#include "td_ctx.h"

__global__ __launch_bounds__(KT_BLOCK) void td_samples_kernel(const TdSamplesArgs a)
{
	// the class of a label is the label itself (+ 1; H <= 127), what it means to a read's calls is s_tc's; the sheet, sorted
	__shared__ uint8_t s_cls[128];
	__shared__ uint16_t s_tc[128];
	__shared__ uint32_t s_row[256];
	__shared__ uint8_t s_sample[256];
	const int n_samples = a.plan->n_samples, m = a.plan->m;
	for (int h = threadIdx.x; h < 128; h += KT_BLOCK) { s_cls[h] = h < a.H ? (uint8_t)(h + 1) : (uint8_t)0; s_tc[h] = a.plan->tc[h]; }
	for (int k = threadIdx.x; k < 256; k += KT_BLOCK) { s_row[k] = k < n_samples ? a.plan->row[k] : 0xFFFFFFFFu; s_sample[k] = a.plan->sample[k]; }
	__syncthreads();
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int tile = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
	if (tile >= a.n_tiles) return;                    // (whole waves; no workgroup barrier below)
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	bool elig = false;
	int len = 0;
	if (k < a.n_reads) {                              // the outcome first: the other lanes read nothing more
		elig = a.out_type[k] == TD_EXTRACT_SUCCESS;
		if (elig) len = a.lens[k];
	}
	if (__builtin_amdgcn_ballot_w64(elig) == 0ull) return;
	const bool ordered = a.plan->ordered != 0;
	uint32_t calls = 0u;                              // byte t = call_t + 1
	kt_walk_tile(a.tile, s_cls, tile, lane, len, [&](uint32_t cls, uint32_t, bool) {
		const uint32_t e = s_tc[cls & 127u];
		if (e & SMP_TC_CHOSEN) calls = smp_take(calls, e);
		else if ((e & SMP_TC_BEHIND) && ordered) return false;           // the path has left the last chosen segment for good
		return true;
	});
	const bool incomplete = elig && smp_incomplete(calls, a.plan->decoy, m);
	const int s = elig && !incomplete ? smp_find(s_row, s_sample, n_samples, calls) : -1;
	const bool assigned = s >= 0, unlisted = elig && !incomplete && s < 0;
	if (assigned) a.out_barcode[k] = (a.plan->last_seg << 16) | s;
	else if (elig) a.out_type[k] = TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND;
	const KtWaveAdded added = kt_wave_add(a.table, elig, elig ? smp_key(calls, m) : 0ull, lane);
	// tallies: one add per wave and tally
	const int n_elig = __builtin_popcountll(__builtin_amdgcn_ballot_w64(elig));
	const int n_assigned = __builtin_popcountll(__builtin_amdgcn_ballot_w64(assigned));
	const int n_unlisted = __builtin_popcountll(__builtin_amdgcn_ballot_w64(unlisted));
	const int n_incomplete = __builtin_popcountll(__builtin_amdgcn_ballot_w64(incomplete));
	if (lane == 0) {
		atomicAdd(&a.tallies[SMP_ELIGIBLE], (kt_u64)n_elig);
		if (n_assigned) atomicAdd(&a.tallies[SMP_ASSIGNED], (kt_u64)n_assigned);
		if (n_unlisted) atomicAdd(&a.tallies[SMP_UNLISTED], (kt_u64)n_unlisted);
		if (n_incomplete) atomicAdd(&a.tallies[SMP_INCOMPLETE], (kt_u64)n_incomplete);
		if (added.overflow) atomicAdd(&a.tallies[SMP_OVERFLOW], (kt_u64)added.overflow);
		if (added.fresh) atomicAdd(&a.tallies[SMP_DISTINCT], (kt_u64)added.fresh);
	}
}

void samples_release(td_ctx* c)
{
	TdSamplesState& z = c->samples;
	kt_table_release(z.table);
	if (z.d_plan) (void)hipFree(z.d_plan);
	const int32_t gen = z.gen;
	z = TdSamplesState();
	z.gen = gen;
}

int samples_slot(td_ctx* c, TdSlot& s, int32_t* out_type, int32_t* out_barcode, const int8_t* labels)
{
	const TdSamplesState& z = c->samples;
	TdSamplesArgs a{};
	a.tile = kt_tile_view(s, labels); a.lens = s.d_lens; a.out_type = out_type; a.out_barcode = out_barcode; a.plan = z.d_plan;
	a.n_reads = s.n_reads; a.n_tiles = s.n_tiles; a.H = z.table.H;
	a.table = kt_table_view(z.table); a.tallies = z.table.d_tallies;
	if (kt_launch_slot(c, z.table.ev, s, (const void*)td_samples_kernel, &a) != TD_OK) return TD_FAIL;
	return kt_slot_read_behind(c, s);
}

extern "C" int td_samples_enable(td_ctx* c, const int32_t* tuples, const char* const* names, int32_t n_samples, int32_t log2_slots)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_samples_enable: no model uploaded");
	if (tickets_outstanding(c)) return fail(c, "td_samples_enable: td_submit tickets are outstanding (td_wait them first)");
	TdSamplePlan plan;
	std::vector<std::string> checked;
	if (smp_plan_build(c, "td_samples_enable", &c->model.d, tuples, n_samples, plan) != TD_OK) return TD_FAIL;
	if (smp_names_check(c, "td_samples_enable", names, n_samples, checked) != TD_OK) return TD_FAIL;
	if (log2_slots < 4 || log2_slots > 26) return fail(c, "td_samples_enable: log2_slots = %d (4..26 supported)", log2_slots);
	if (c->match_len > 0) return fail(c, "td_samples_enable: a -start/-end window is set (td_set_window): labels behind a window do not mark the barcodes");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	samples_release(c);
	TdSamplesState& z = c->samples;
	const td_model_desc& m = c->model.d;
	hipError_t e = kt_table_create(z.table, m.label, m.H, log2_slots, SMP_TALLY_WORDS);
	if (e == hipSuccess) e = hipMalloc((void**)&z.d_plan, sizeof(TdSamplePlan));
	if (e == hipSuccess) e = hipMemcpy(z.d_plan, &plan, sizeof(TdSamplePlan), hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		samples_release(c);
		return fail(c, "td_samples_enable: a table of 2^%d slots could not be set up: %s", log2_slots, hipGetErrorString(e));
	}
	z.plan = plan;
	z.names.swap(checked);
	z.gen++;
	z.on = true;
	return TD_OK;
}

extern "C" int td_samples_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	if (!c->samples.on) return TD_OK;
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	samples_release(c);
	return TD_OK;
}

extern "C" int td_samples_reset(td_ctx* c)
{
	if (!c) return TD_FAIL;
	TdSamplesState& z = c->samples;
	if (!z.on) return fail(c, "td_samples_reset: sample assignment is off (td_samples_enable)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;   // (counts of pipelined batches may still be queued, on either compute stream)
	HIPCHK(c, kt_table_zero(z.table, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return TD_OK;
}

extern "C" int td_samples_get(td_ctx* c, td_census_entry* entries, int64_t cap, int64_t* n, td_samples_totals* totals)
{
	if (!c) return TD_FAIL;
	TdSamplesState& z = c->samples;
	if (!z.on) return fail(c, "td_samples_get: sample assignment is off (td_samples_enable)");
	kt_u64 t[SMP_TALLY_WORDS];
	if (kt_table_entries(c, "td_samples_get", z.table, SMP_DISTINCT, SMP_CURSOR, entries, cap, n, t) != TD_OK) return TD_FAIL;
	if (totals) {
		totals->eligible = (int64_t)t[SMP_ELIGIBLE]; totals->assigned = (int64_t)t[SMP_ASSIGNED]; totals->unlisted = (int64_t)t[SMP_UNLISTED];
		totals->incomplete = (int64_t)t[SMP_INCOMPLETE]; totals->overflow = (int64_t)t[SMP_OVERFLOW];
	}
	return TD_OK;
}

extern "C" const char* td_samples_name(td_ctx* c, int32_t s)
{
	if (!c || !c->samples.on || s < 0 || s >= (int32_t)c->samples.names.size()) return nullptr;
	return c->samples.names[(size_t)s].c_str();
}

// the kernel's time of the last batch, for tools/samples_bench.py (option "samples_kernel_us" of td_get_option)
int samples_last_kernel_us(td_ctx* c, int32_t* us)
{
	if (!c->samples.on) return fail(c, "td_get_option: samples_kernel_us: sample assignment is off");
	return kt_last_kernel_us(c, c->samples.table.ev, us, "td_get_option: samples_kernel_us: no batch has been assigned yet");
}
