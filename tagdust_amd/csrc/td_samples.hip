// td_samples.hip -- sample assignment by all 'B' segments (include/tagdust_samples.h): a read's sample is the tuple of its barcode calls.
//
// Behind every TD_MODE_GET_LABEL launch of a context with samples on, one small kernel reads what the decode kernel left in device
// order -- the outcome and the lane-interleaved label bytes -- takes each eligible read's call for every chosen segment (the last
// position with a label of that segment wins), looks the tuple up in the sheet and rewrites the read's outcome or barcode; every
// eligible read's tuple is counted in an open-addressing table in HBM (td_keytable.h).  One read per lane, one tile per wave, like
// the decode kernels and the census.  It stands in front of the census and the molecule count in launch_end (td_batch.hip): both
// read one sample per read.  The rewrite never depends on the table.  A read's class and key are td_samples_def.h's, the text
// td_samples_host (td_samples_host.cpp) compiles too.
//
// The join across input files (dual-index runs) has two more kernels here: an exporter context's, which leaves one word of calls per
// read in the caller's order, and the primary's, the assignment above with the partners' words OR-ed into the read's own calls.
#include <hip/hip_runtime.h>

#include "td_ctx.h"

// One text for the plain assignment and for the join across input files (JOIN): there a read's partner word -- staged with the
// batch in the caller's order, gathered to the lane's device position -- is OR-ed into its own calls, and a read whose partner
// failed is not eligible: nothing of it changes, it is only tallied.
template <bool JOIN>
__device__ __forceinline__ void samples_tile(const TdSamplesArgs& a)
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
	bool elig = false, partner_failed = false;
	uint32_t calls = 0u;                              // byte t = call_t + 1
	int len = 0;
	if (k < a.n_reads) {                              // the outcome first: the other lanes read nothing more
		elig = a.out_type[k] == TD_EXTRACT_SUCCESS;
		if (JOIN && elig) {
			calls = a.partner[a.read_at ? (int64_t)a.read_at[k] : k];   // (read_at[k] in 0..n_reads-1: the stage sort's permutation)
			partner_failed = calls == SMP_PARTNER_FAILED;
			elig = !partner_failed;
		}
		if (elig) len = a.lens[k];
	}
	if (JOIN) {
		const int n_failed = __builtin_popcountll(__builtin_amdgcn_ballot_w64(partner_failed));
		if (lane == 0 && n_failed) atomicAdd(&a.tallies[SMP_PARTNER_FAILED_TALLY], (kt_u64)n_failed);
	}
	if (__builtin_amdgcn_ballot_w64(elig) == 0ull) return;
	if (!elig) calls = 0u;
	const bool ordered = a.plan->ordered != 0;
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

__global__ __launch_bounds__(KT_BLOCK) void td_samples_kernel(const TdSamplesArgs a) { samples_tile<false>(a); }
__global__ __launch_bounds__(KT_BLOCK) void td_samples_join_kernel(const TdSamplesArgs a) { samples_tile<true>(a); }

// The exporter side of the join: every read's word -- its own calls at the bytes of its columns, all ones when it was not
// extracted -- to the read's position in the CALLER's order (a sorted slot's device order differs from it).  The same walk.
__global__ __launch_bounds__(KT_BLOCK) void td_samples_export_kernel(const TdSamplesExportArgs a)
{
	__shared__ uint8_t s_cls[128];
	__shared__ uint16_t s_tc[128];
	for (int h = threadIdx.x; h < 128; h += KT_BLOCK) { s_cls[h] = h < a.H ? (uint8_t)(h + 1) : (uint8_t)0; s_tc[h] = a.plan->tc[h]; }
	__syncthreads();
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int tile = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
	if (tile >= a.n_tiles) return;                    // (whole waves; no workgroup barrier below)
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	const bool mine = k < a.n_reads;
	const bool extracted = mine && a.out_type[k] == TD_EXTRACT_SUCCESS;
	const int len = extracted ? a.lens[k] : 0;
	const bool ordered = a.plan->ordered != 0;
	uint32_t calls = 0u;
	kt_walk_tile(a.tile, s_cls, tile, lane, len, [&](uint32_t cls, uint32_t, bool) {
		const uint32_t e = s_tc[cls & 127u];
		if (e & SMP_TC_CHOSEN) calls = smp_take(calls, e);
		else if ((e & SMP_TC_BEHIND) && ordered) return false;
		return true;
	});
	if (mine) a.words[a.read_at ? (int64_t)a.read_at[k] : k] = smp_export_word(extracted, calls);   // (read_at[k] in 0..n_reads-1)
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
	if (z.join) { a.partner = s.d_smp_w; a.read_at = s.sorted ? s.d_read_at : nullptr; }
	if (kt_launch_slot(c, z.table.ev, s, z.join ? (const void*)td_samples_join_kernel : (const void*)td_samples_kernel, &a) != TD_OK) return TD_FAIL;
	return kt_slot_read_behind(c, s);
}

// the sheet's plan and names are checked: table and plan on the device, samples on (the plain assignment's enable and the join's)
static int samples_switch_on(td_ctx* c, const char* who, const TdSamplePlan& plan, std::vector<std::string>& checked, int32_t log2_slots, bool join)
{
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	samples_release(c);
	TdSamplesState& z = c->samples;
	const td_model_desc& m = c->model.d;
	hipError_t e = kt_table_create(z.table, m.label, m.H, log2_slots, SMP_TALLY_WORDS);
	if (e == hipSuccess) e = hipMalloc((void**)&z.d_plan, sizeof(TdSamplePlan));
	if (e == hipSuccess) e = hipMemcpy(z.d_plan, &plan, sizeof(TdSamplePlan), hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		samples_release(c);
		return fail(c, "%s: a table of 2^%d slots could not be set up: %s", who, log2_slots, hipGetErrorString(e));
	}
	z.plan = plan;
	z.names.swap(checked);
	z.gen++;
	z.on = true;
	z.join = join;
	return TD_OK;
}

extern "C" int td_samples_enable(td_ctx* c, const int32_t* tuples, const char* const* names, int32_t n_samples, int32_t log2_slots)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_samples_enable: no model uploaded");
	if (tickets_outstanding(c)) return fail(c, "td_samples_enable: td_submit tickets are outstanding (td_wait them first)");
	if (c->samples_export.on) return fail(c, "td_samples_enable: the context exports its barcode calls (td_samples_export_disable first)");
	TdSamplePlan plan;
	std::vector<std::string> checked;
	if (smp_plan_build(c, "td_samples_enable", &c->model.d, tuples, n_samples, plan) != TD_OK) return TD_FAIL;
	if (smp_names_check(c, "td_samples_enable", names, n_samples, checked) != TD_OK) return TD_FAIL;
	if (log2_slots < 4 || log2_slots > 26) return fail(c, "td_samples_enable: log2_slots = %d (4..26 supported)", log2_slots);
	if (c->match_len > 0) return fail(c, "td_samples_enable: a -start/-end window is set (td_set_window): labels behind a window do not mark the barcodes");
	return samples_switch_on(c, "td_samples_enable", plan, checked, log2_slots, false);
}

// ---- the join across input files ----
extern "C" int td_samples_join_enable(td_ctx* c, const int32_t* tuples, const char* const* names, int32_t n_samples, int32_t log2_slots,
                                      int32_t m_total, int32_t first_column, const int32_t* column_hmms)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_samples_join_enable: no model uploaded");
	if (tickets_outstanding(c)) return fail(c, "td_samples_join_enable: td_submit tickets are outstanding (td_wait them first)");
	if (c->samples_export.on) return fail(c, "td_samples_join_enable: the context exports its barcode calls (td_samples_export_disable first)");
	TdSamplePlan plan;
	std::vector<std::string> checked;
	if (smp_join_plan_build(c, "td_samples_join_enable", &c->model.d, tuples, n_samples, m_total, first_column, column_hmms, plan) != TD_OK) return TD_FAIL;
	if (smp_names_check(c, "td_samples_join_enable", names, n_samples, checked) != TD_OK) return TD_FAIL;
	if (log2_slots < 4 || log2_slots > 26) return fail(c, "td_samples_join_enable: log2_slots = %d (4..26 supported)", log2_slots);
	if (c->match_len > 0) return fail(c, "td_samples_join_enable: a -start/-end window is set (td_set_window): labels behind a window do not mark the barcodes");
	return samples_switch_on(c, "td_samples_join_enable", plan, checked, log2_slots, true);
}

static int words_next(td_ctx* c, const char* who, bool on, const char* off_text, TdSamplesNamed& nx, uint32_t* out, const uint32_t* in, int64_t n_reads)
{
	if (!on) return fail(c, "%s: %s", who, off_text);
	if (n_reads < 0 || (n_reads > 0 && !out && !in)) { nx.named = false; return fail(c, "%s: no array of words for a batch of %lld reads", who, (long long)n_reads); }
	nx.out = out; nx.in = in; nx.reads = n_reads; nx.named = true;
	return TD_OK;
}

extern "C" int td_samples_join_next(td_ctx* c, const uint32_t* words, int64_t n_reads)
{
	if (!c) return fail(nullptr, "td_samples_join_next: no context");
	return words_next(c, "td_samples_join_next", c->samples.on && c->samples.join, "the join is off (td_samples_join_enable)", c->samples.next, nullptr, words, n_reads);
}

extern "C" int td_samples_export_next(td_ctx* c, uint32_t* words, int64_t n_reads)
{
	if (!c) return fail(nullptr, "td_samples_export_next: no context");
	return words_next(c, "td_samples_export_next", c->samples_export.on, "the export is off (td_samples_export_enable)", c->samples_export.next, words, nullptr, n_reads);
}

extern "C" int td_samples_join_get(td_ctx* c, td_census_entry* entries, int64_t cap, int64_t* n, td_samples_join_totals* totals)
{
	if (!c) return TD_FAIL;
	TdSamplesState& z = c->samples;
	if (!z.on || !z.join) return fail(c, "td_samples_join_get: the join is off (td_samples_join_enable)");
	kt_u64 t[SMP_TALLY_WORDS];
	if (kt_table_entries(c, "td_samples_join_get", z.table, SMP_DISTINCT, SMP_CURSOR, entries, cap, n, t) != TD_OK) return TD_FAIL;
	if (totals) {
		totals->t.eligible = (int64_t)t[SMP_ELIGIBLE]; totals->t.assigned = (int64_t)t[SMP_ASSIGNED]; totals->t.unlisted = (int64_t)t[SMP_UNLISTED];
		totals->t.incomplete = (int64_t)t[SMP_INCOMPLETE]; totals->t.overflow = (int64_t)t[SMP_OVERFLOW];
		totals->partner_failed = (int64_t)t[SMP_PARTNER_FAILED_TALLY];
	}
	return TD_OK;
}

void samples_export_release(td_ctx* c)
{
	TdSamplesExportState& x = c->samples_export;
	if (x.d_plan) (void)hipFree(x.d_plan);
	kt_pair_destroy(x.ev);
	const int32_t gen = x.gen;
	x = TdSamplesExportState();
	x.gen = gen;
}

extern "C" int td_samples_export_enable(td_ctx* c, int32_t first_column)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_samples_export_enable: no model uploaded");
	if (tickets_outstanding(c)) return fail(c, "td_samples_export_enable: td_submit tickets are outstanding (td_wait them first)");
	if (c->samples.on)
		return fail(c, "td_samples_export_enable: %s is on in this context (td_samples_disable first): a context assigns or exports", c->samples.join ? "the join" : "sample assignment");
	TdSamplePlan plan;
	if (smp_export_plan_build(c, "td_samples_export_enable", &c->model.d, first_column, plan) != TD_OK) return TD_FAIL;
	if (c->match_len > 0) return fail(c, "td_samples_export_enable: a -start/-end window is set (td_set_window): labels behind a window do not mark the barcodes");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	samples_export_release(c);
	TdSamplesExportState& x = c->samples_export;
	hipError_t e = hipMalloc((void**)&x.d_plan, sizeof(TdSamplePlan));
	if (e == hipSuccess) e = hipMemcpy(x.d_plan, &plan, sizeof(TdSamplePlan), hipMemcpyHostToDevice);
	if (e == hipSuccess) e = kt_pair_create(x.ev);
	if (e != hipSuccess) {
		samples_export_release(c);
		return fail(c, "td_samples_export_enable: the export could not be set up: %s", hipGetErrorString(e));
	}
	x.H = c->model.d.H;
	x.gen++;
	x.on = true;
	return TD_OK;
}

extern "C" int td_samples_export_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	if (!c->samples_export.on) return TD_OK;
	if (tickets_outstanding(c)) return fail(c, "td_samples_export_disable: td_submit tickets are outstanding (td_wait them first)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	samples_export_release(c);
	return TD_OK;
}

int samples_export_slot(td_ctx* c, TdSlot& s, const int32_t* out_type, const int8_t* labels)
{
	const TdSamplesExportState& x = c->samples_export;
	TdSamplesExportArgs a{};
	a.tile = kt_tile_view(s, labels); a.lens = s.d_lens; a.out_type = out_type; a.plan = x.d_plan;
	a.words = s.d_smp_w; a.read_at = s.sorted ? s.d_read_at : nullptr;
	a.n_reads = s.n_reads; a.n_tiles = s.n_tiles; a.H = x.H;
	if (kt_launch_slot(c, x.ev, s, (const void*)td_samples_export_kernel, &a) != TD_OK) return TD_FAIL;
	return kt_slot_read_behind(c, s);
}

// whichever side of the join the context is on: the state that names the next batch's words, NULL when it is on neither
static TdSamplesNamed* words_side(td_ctx* c, const char*& next_fn)
{
	if (c->samples_export.on) { next_fn = "td_samples_export_next"; return &c->samples_export.next; }
	if (c->samples.on && c->samples.join) { next_fn = "td_samples_join_next"; return &c->samples.next; }
	return nullptr;
}

int samples_words_check(td_ctx* c, int64_t n, const char* who)
{
	const char* next_fn = "";
	TdSamplesNamed* nx = words_side(c, next_fn);
	if (!nx) return TD_OK;
	if (!nx->named)
		return fail(c, "%s: the context %s and no words are named for this batch of %lld reads (%s first); nothing was decoded", who,
		            c->samples_export.on ? "exports its barcode calls" : "joins its partners' barcode calls", (long long)n, next_fn);
	if (nx->reads != n) {
		nx->named = false;
		return fail(c, "%s: the named words are those of %lld reads, the batch has %lld: one word per read; the name is dropped (%s again), nothing "
		            "was decoded", who, (long long)nx->reads, (long long)n, next_fn);
	}
	return TD_OK;
}

int samples_words_stage(td_ctx* c, TdSlot& s, int64_t n, hipStream_t up)
{
	const char* next_fn = "";
	TdSamplesNamed* nx = words_side(c, next_fn);
	if (!nx) return TD_OK;
	const TdSamplesNamed named = *nx;
	nx->named = false;                                // consumed, whatever happens below
	const size_t bytes = (size_t)n * sizeof(uint32_t);
	if (ensure(c, &s.d_smp_w, &s.cap_smp_w, bytes) != TD_OK || ensure_pinned(c, &s.h_smp_w, &s.cap_h_smp_w, bytes) != TD_OK) return TD_FAIL;
	if (c->samples_export.on) {
		s.smp_dst = named.out;
		s.export_gen = c->samples_export.gen;
		return TD_OK;
	}
	if (n > 0) {
		memcpy(s.h_smp_w, named.in, bytes);
		HIPCHK(c, hipMemcpyAsync(s.d_smp_w, s.h_smp_w, bytes, hipMemcpyHostToDevice, up));
	}
	s.join_words = true;
	return TD_OK;
}

int samples_export_issue_copy(td_ctx* c, TdSlot& s, hipStream_t down)
{
	if (s.n_reads > 0) HIPCHK(c, hipMemcpyAsync(s.h_smp_w, s.d_smp_w, (size_t)s.n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost, down));
	return TD_OK;
}

void samples_export_copy_out(TdSlot& s)
{
	if (s.n_reads > 0 && s.smp_dst) memcpy(s.smp_dst, s.h_smp_w, (size_t)s.n_reads * sizeof(uint32_t));
}

int samples_export_last_kernel_us(td_ctx* c, int32_t* us)
{
	if (!c->samples_export.on) return fail(c, "td_get_option: samples_export_kernel_us: the export is off");
	return kt_last_kernel_us(c, c->samples_export.ev, us, "td_get_option: samples_export_kernel_us: no batch has been exported yet");
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
