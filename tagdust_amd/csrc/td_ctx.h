// td_ctx.h -- what the three host units of the C-ABI layer share: the context (td_api.hip keeps house in it) and its batch slots
// (td_batch.hip runs them), the state of the model-specialised kernel inside the context (td_spec_host.hip runs that), the few
// helpers they call.  Nothing here is exported.
// (The plain C++ units they apply -- td_model_flat.cpp, td_batch_plan.cpp, td_spec_plan.cpp, td_spec_bounds.cpp -- know nothing of it.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <memory>
#include <string>
#include <vector>
#include "../../include/tagdust_hip.h"
#include "td_device.h"
#include "td_batch_plan.h"
#include "td_jit.h"
#include "td_stage.h"
#include "td_host_inner.h"
#include "td_census.h"
#include "td_molecules.h"
#include "td_samples.h"
#include "td_quality.h"

#define TD_HIDDEN __attribute__((visibility("hidden")))
#define TD_MAX_PIPELINE 4
// the device counter block: what the ABI reports, then the diagnostic tail of the development knobs (td_diag_get)
#define TD_COUNTER_WORDS (TD_NUM_COUNTERS + TD_NUM_DIAG_COUNTERS)

// One batch on its way through the device (see "batches" in td_batch.hip).  What a slot knows about ITS BATCH lives in three groups,
// each value-initialised as a whole by the step that owns it -- so that nothing a branch of that step does not set can survive from
// the batch before (round 3's soak fault was exactly that: a label-run table of the previous, smaller batch):
//   TdStaged  <- slot_stage():       the reads as staged on the device and the workspace geometry chosen for them
//   TdDecoded <- slot_decode():      what the last launch over the staged batch was and left behind
//   TdFetch   <- slot_fetch_begin(): where the results go, and the plan of the form they travel in (td_batch_plan.cpp, plan_egress)
// slot_stage() also resets the two later groups, slot_decode() the last one.  What is left in TdSlot itself belongs to the slot,
// not to a batch: device / pinned buffers with their capacities, events, the ticket.
struct TdRoute {             // where a batch runs (chosen by the caller of slot_stage, per batch)
	hipStream_t cs = nullptr;   // the compute stream (c->stream, or c->stream2 for every other pipelined batch)
	hipStream_t aux = nullptr;  // the stream of its sort / pack kernels: cs itself, or the context's high-priority stream for them
	hipStream_t fin = nullptr;  // ... and of its finish kernel (a stream of its own: it waits for the decode kernel, the next batch's pack must not)
	int wsi = 0;                // ... and the workspace (0 / 1) that goes with cs
	bool pipelined = false;     // a td_submit batch (the synchronous calls use slot 0 with pipelined = false)
};
struct TdStaged : TdRoute {
	int64_t n_reads = 0, n_bases = 0;
	int32_t n_tiles = 0, lmax = 0, nw2 = 0, nw1 = 0;
	int is_ascii = 0;
	bool sorted = false;      // device order differs from the caller's (reads of several lengths)
	bool staged = false;      // inputs are packed on the device: td_run may launch
	bool for_spec = false;    // ... and the workspace geometry is the specialised kernel's: a batch is decoded by the kernel it was staged
	                          // for, also when a background compile is handed over between its upload and its td_run
	bool raw_direct = false;  // the upload read the caller's page-locked buffer itself (no staging copy)
	int32_t mate_m = 0;       // mate mode: d_mate_w / d_mate_n hold this batch's mates, made with M = mate_m (0: no mate batch was staged)
	bool mate_direct = false; // ... and the upload read the caller's page-locked mate buffer itself
	bool mate_judged = false; // the mate filter was on when the mate batch was staged: the batch's outcomes are joined with the mates'
	bool mate_typed = false;  // ... and the filter kernel ran (dust != 0 or artifacts set): d_mate_type holds this batch's mate types;
	                          // judged and not typed: every mate type is 0, d_mate_type is not read
	int32_t samples_gen = 0;  // sample assignment (td_samples.hip) as it stood when the batch was staged: the enable's number, 0 = off
	int32_t export_gen = 0;   // the join's exporter side: the td_samples_export_enable under which the batch's word array was named, 0 = none was
	bool join_words = false;  // ... its primary side: d_smp_w holds this batch's partner words
	uint32_t* smp_dst = nullptr;   // ... the exporter's array the batch's words go to (valid until the batch has been waited for)
	int32_t qual_gen = 0;     // the base-quality filter (td_quality.hip): the enable under which the batch's qualities were staged, 0 = none were
	int64_t qual_words = 0;   // ... and the words of d_qual_w that are this batch's (the spare zero word included)
	const uint8_t* raw_host = nullptr;   // the batch's bases on the host, valid until the batch has been waited for: the pinned staging
	                                     // copy, or the caller's own page-locked buffer under the "stable_input" contract; else NULL
	TdStageBatch sb{};
	TdWsLayout lay{};
	TdSpecLayout slay{};
	int32_t n_wave_slots = 0;
	int64_t ws_slot_bytes = 0;
	// length classes (specialised kernel): the n_long longest tiles are longer than lmax_small, the geometry of most wave slots;
	// n_big >= n_long slots keep the geometry of the batch's longest read (slay_big).  n_long = 0: one geometry.
	int32_t n_long = 0, lmax_small = 0, n_big = 0;
	TdSpecLayout slay_big{};
	int64_t ws_bytes = 0;       // workspace bytes this batch's launch uses
};
struct TdDecoded {
	int mode = 0;
	bool ran = false;
	float last_ms = -1.0f;
	int32_t runs_cap = 0;       // entries per read in d_runs (0: the last launch left no label runs)
	bool hits_queued = false;   // the per-artifact hit count is queued behind the launch (ev_hits): it reads d_out like the finish kernel
};
struct TdFetch {
	td_read_result* u_res = nullptr; int8_t* u_labels = nullptr; uint8_t* u_seq = nullptr;   // the caller's output buffers
	TdEgressPlan plan;              // per output: not wanted, compact (keep bits / label runs), straight into the caller's page-locked buffer, staged
	bool copies_deferred = false;   // td_wait issues the device-to-host copies (pipelined calls)
	bool finished = false;          // the finish kernel is queued: slot_fetch_end has something to collect
};
struct TdSlot : TdStaged, TdDecoded, TdFetch {
	int64_t ticket = 0;       // td_submit: 0 = free
	void reset_staged(const TdRoute& r) { static_cast<TdStaged&>(*this) = TdStaged(); static_cast<TdRoute&>(*this) = r; reset_decoded(); }
	void reset_decoded() { static_cast<TdDecoded&>(*this) = TdDecoded(); reset_fetch(); }
	void reset_fetch() { static_cast<TdFetch&>(*this) = TdFetch(); }
	// device
	uint8_t* d_raw = nullptr;      size_t cap_raw = 0;
	int64_t* d_offs = nullptr;     size_t cap_offs = 0;
	int32_t* d_read_at = nullptr;  size_t cap_read_at = 0;
	uint32_t* d_keys = nullptr;    size_t cap_keys = 0;
	int32_t* d_vals = nullptr;     size_t cap_vals = 0;
	uint8_t* d_sort_tmp = nullptr; size_t cap_sort_tmp = 0;
	uint32_t* d_packed = nullptr;  size_t cap_packed = 0;
	int32_t* d_lens = nullptr;     size_t cap_lens = 0;
	uint8_t* d_art_left = nullptr; size_t cap_art_left = 0;
	uint8_t* d_out = nullptr;      size_t cap_out = 0;    // decode-kernel outputs, device order
	uint8_t* d_res = nullptr;      size_t cap_res = 0;    // results in the caller's order
	uint8_t* d_seq = nullptr;      size_t cap_seq = 0;
	int8_t*  d_lab = nullptr;      size_t cap_lab = 0;
	// compact egress: what the host rebuilds the rewritten sequences and the labels from (slot_fetch_begin)
	uint32_t* d_keepo = nullptr;   size_t cap_keepo = 0;
	uint32_t* d_rle = nullptr;     size_t cap_rle = 0;     // (+ one word behind the runs: the overflow flag)
	uint32_t* d_runs = nullptr;    size_t cap_runs = 0;    // label runs in device order, left by the specialised kernel (+ the overflow flag)
	int32_t* d_judged = nullptr;   size_t cap_judged = 0;  // dedup: every read's slot in the molecule table between its two passes (-1: not judged)
	// mate mode (td_molecules.hip): the mate batch as uploaded, and what the mate kernel makes of it, in the caller's order
	uint8_t* d_mate_raw = nullptr; size_t cap_mate_raw = 0;
	int64_t* d_mate_offs = nullptr; size_t cap_mate_offs = 0;
	unsigned long long* d_mate_w = nullptr; size_t cap_mate_w = 0;
	uint8_t* d_mate_n = nullptr;   size_t cap_mate_n = 0;
	int32_t* d_mate_type = nullptr; size_t cap_mate_type = 0;   // the mate filter's verdicts (td_mate_filter.hip), allocated by its first launch
	// the base-quality filter (td_quality.hip): one low flag per base of the batch, packed on the host into page-locked words
	uint32_t* d_qual_w = nullptr;  size_t cap_qual_w = 0;
	uint32_t* h_qual_w = nullptr;  size_t cap_h_qual_w = 0;
	// the join across input files (td_samples.hip): one word per read in the caller's order -- the partner words in, or the export words out
	uint32_t* d_smp_w = nullptr;   size_t cap_smp_w = 0;
	uint32_t* h_smp_w = nullptr;   size_t cap_h_smp_w = 0;
	uint8_t* h_mate_raw = nullptr; size_t cap_h_mate_raw = 0;   // (pinned staging, as h_raw and h_offs)
	int64_t* h_mate_offs = nullptr; size_t cap_h_mate_offs = 0;
	uint32_t* h_keepo = nullptr;   size_t cap_h_keepo = 0;
	uint32_t* h_rle = nullptr;     size_t cap_h_rle = 0;
	// pinned host staging for pageable caller memory
	uint8_t* h_raw = nullptr;      size_t cap_h_raw = 0;
	int64_t* h_offs = nullptr;     size_t cap_h_offs = 0;
	uint8_t* h_res = nullptr;      size_t cap_h_res = 0;
	uint8_t* h_seq = nullptr;      size_t cap_h_seq = 0;
	int8_t*  h_lab = nullptr;      size_t cap_h_lab = 0;
	hipEvent_t ev_up = nullptr, ev_k0 = nullptr, ev_k1 = nullptr, ev_done = nullptr, ev_down = nullptr, ev_pack = nullptr, ev_hits = nullptr;
};

// The uploaded description, deep-copied: a reload of the specialised kernel works on the context's copy, a background compile on
// a copy of its own (SpecJob).
struct ModelCopy {
	td_model_desc d{};
	std::vector<int32_t> n_hmm, n_col, finger_len, label;
	std::vector<float> skip, trans, eM, eI, sM, sI, A;
	std::vector<int8_t> seg_type;
	void assign(const td_model_desc* m)
	{
		auto own = [](auto& v, const auto* p, size_t n) { v.assign(p, p + n); return v.data(); };   // a table, and where it now lives
		const size_t S = (size_t)m->S, H = (size_t)m->H, C = (size_t)m->C;
		td_model_desc t = *m;
		t.n_hmm = own(n_hmm, m->n_hmm, S); t.n_col = own(n_col, m->n_col, S); t.skip = own(skip, m->skip, S);
		t.seg_type = own(seg_type, m->seg_type, S); t.finger_len = own(finger_len, m->finger_len, S);
		t.trans = own(trans, m->trans, C * 9); t.eM = own(eM, m->eM, C * 5); t.eI = own(eI, m->eI, C * 5);
		t.sM = own(sM, m->sM, C); t.sI = own(sI, m->sI, C); t.label = own(label, m->label, H); t.A = own(A, m->A, H * H);
		d = t;
	}
};

// The model as the generic kernel reads it from HBM: header, columns, per-HMM info, label predecessor lists.
struct DevModel {
	TdModelHeader h{};
	TdModelHeader* d_hdr = nullptr; TdCol* d_cols = nullptr; uint32_t* d_hinfo = nullptr;
	int32_t* d_pred_off = nullptr, * d_pred_idx = nullptr;
};

// Everything a context knows about its model-specialised kernel (td_spec_kernel.inc through hiprtc); td_spec_host.hip runs its life.
struct SpecJob;
struct TdSpecState {
	int specialize = 1;
	bool ready = false;         // the loaded kernel decodes the batches staged from now on
	hipModule_t mod = nullptr;  hipFunction_t fn = nullptr;
	TdSpecPlan plan;            // what the specialised kernel is for c->model.d, under the TD_SPEC_* knobs as they stood at the upload
	bool oob = false;           // the loaded kernel uses the clamp-free logsum
	bool window = false;        // the loaded kernel has the -start/-end window arithmetic compiled in
	bool oob_unsafe = false;    // the clamp-free form failed its self-check once: never again in this context
	float maxabs = 0.0f;        // largest |finite parameter|
	int block = 256, waves_per_cu = 8;
	// background compile and load-time probe (tagdust_hip.h, td_spec_wait / td_spec_probe)
	int async_compile = 0;      // TD_ASYNC_COMPILE ["async_compile"]
	int probe = 1;              // ["spec_probe"]
	int state = 0;              // "spec_state" (1 / 2 are told apart when asked: is the job done?)
	int batches_generic = 0;    // "spec_batches_generic"
	int probe_us = 0;           // "spec_probe_us"
	std::shared_ptr<SpecJob> job;                   // the compile this context waits for (nullptr: none)
	int job_oob = 0, job_window = 0;                // ... and the variant it is
	std::vector<std::shared_ptr<SpecJob>> retired;  // superseded jobs: never loaded, waited for when the context goes
	std::string job_err;                            // the compiler's log of a failed background compile
	double lsum_limit = 1.0e6;  // TD_SPEC_LSUM_LIMIT (tests: force the switch to the clamped logsum)
	int selfcheck_fail = 0;     // TD_SPEC_SELFCHECK_FAIL (tests: exercise the fallback)
	// position pruning tables (td_spec_prune_tables), for reads up to prune_lcap bases
	float* d_prune = nullptr;   int prune_lcap = 0, prune_stride = 0;
	bool prune_live = false;    // ... and they are real bounds (not the all-zero tables of reads beyond 8192 bases)
};

struct td_ctx {
	int device = 0;
	// Host threads the context may use for its copies between pageable caller memory and pinned staging (option "host_threads";
	// td_multi_create shares the machine's threads out over its devices), and the threads themselves: started by the first batch
	// that needs them, reused by every later one.
	int host_threads = td_context_threads();
	TdWorkers pool;
	hipStream_t stream = nullptr;
	std::string err;
	int n_cu = 0;
	size_t hbm_total = 0;

	// model
	bool have_model = false;
	ModelCopy model;            // the description as uploaded (a few KB)
	DevModel dev;               // ... and its tables for the generic kernel
	float* d_logsum = nullptr;
	unsigned long long* d_counters = nullptr;
	TdSpecState spec;

	// params
	float threshold = 0.0f;
	int32_t minlen = 16, dust = 100;

	// -ref artifact filter
	uint8_t* d_art_text = nullptr; int32_t* d_art_index = nullptr;
	uint32_t* d_art_pk = nullptr; int32_t* d_art_seq = nullptr;   // the same text as 2-bit codes for TD_MODE_RNA_DUST (td_rnadust.hip)
	int32_t art_n = 0, art_fe = 0, art_threads = 1;
	unsigned long long* d_art_hits = nullptr;   // [art_n] reads per artifact sequence (td_artifact_hits_get)
	TdCensusState census;       // include/tagdust_census.h: off unless td_census_enable switched it on
	TdMolState molecules;       // include/tagdust_molecules.h: off unless td_mol_enable switched it on
	TdSamplesState samples;     // include/tagdust_samples.h: off unless td_samples_enable switched it on
	TdSamplesExportState samples_export;   // ... its exporter side of the join: off unless td_samples_export_enable switched it on
	TdQualState quality;        // include/tagdust_quality.h: off unless td_qual_enable switched it on
	int64_t win_first = 0, win_total = 0;   // td_set_batch_window
	int32_t match_start = 0, match_len = 0;  // td_set_window (-start / -end); match_len = 0: whole reads
	// batches: slot 0 is the resident batch of the synchronous calls; td_submit rotates over pipeline_depth slots
	TdSlot slots[TD_MAX_PIPELINE];
	int pipeline_depth = 3, next_slot = 0, last_slot = 0;
	bool counted = false;   // td_ctx_create finished: this context counts among the live ones (the last one to go frees the stream cache)
	int poison = 0;   // option "poison_workspace": fill the workspace with 0xFF bytes before every decode launch (tests)
	// development / test knobs: read from the environment ONCE, when the context is created (never on the per-batch path), and
	// settable afterwards through td_set_option under the names in brackets
	int compact_egress = 1;    // TD_COMPACT_EGRESS ["compact_egress"]: keep bits + label runs instead of plain copies
	int stable_input = 0;      // ["stable_input"]: the caller leaves a page-locked input buffer alone until td_wait (see tagdust_hip.h)
	int rle_cap_forced = 0;    // TD_RLE_CAP ["rle_cap"]: entries of the label-run table (0: S + 2)
	int length_classes = 1;    // TD_NO_LENGTH_CLASSES ["length_classes_enabled"]
	int debug_wait = 0;        // TD_DEBUG_WAIT ["debug_wait"]
	int debug_alloc = 0;       // TD_DEBUG_ALLOC
	long wave_slots_forced = 0;   // TD_WAVE_SLOTS
	int ws_candidates = 3;     // TD_WS_CANDIDATES
	int64_t ticket_counter = 0;
	hipStream_t s_up = nullptr, s_down = nullptr;   // copy streams of the pipelined calls
	uint8_t* d_ws = nullptr;      size_t cap_ws = 0;  // workspace of the decode kernels on `stream` (they run one after the other)
	// Pipelined batches alternate between two compute streams with a workspace each: a launch ends with its slowest wave
	// (the waves of some XCDs take ~10 % longer for the same tiles), and the next batch's workgroups move in as the first
	// one's retire instead of waiting for the last (option "overlap_decode", TD_OVERLAP; off when HBM cannot hold both).
	hipStream_t stream2 = nullptr;
	// With two decode kernels queued the machine never falls idle, so the small kernels around them (sort / pack of the next
	// batch, finish of the last one) and the download's blit kernels would wait for a whole decode kernel: they run on a
	// high-priority stream and take the compute units the retiring workgroups free before the next decode kernel does.
	hipStream_t s_aux = nullptr, s_fin = nullptr;
	uint8_t* d_ws2 = nullptr;     size_t cap_ws2 = 0;
	int overlap = 1, submit_parity = 0;
	bool half_slots = false;   // two workspaces of the full slot count do not fit: the pipelined launches use half the slots each
	int32_t* d_tile_next = nullptr, * d_tile_next2 = nullptr;   // tile counters of the specialised kernel's dynamic tile assignment, one per workspace
	hipEvent_t ev_origin = nullptr;   // td_timeline_origin: the common origin of td_last_kernel_times
};

TD_HIDDEN int fail(td_ctx* c, const char* fmt, ...);   // (td_api.hip) TD_FAIL, and the message for td_last_error
TD_HIDDEN bool is_pinned(const void* p);                // (td_batch.hip) this host pointer is page-locked: the DMA engines can use it directly
TD_HIDDEN bool tickets_outstanding(const td_ctx* c);   // (td_batch.hip) a td_submit batch has not been waited for
TD_HIDDEN void slot_release(TdSlot& s);                 // (td_batch.hip) a slot's buffers and events go (td_ctx_destroy)
TD_HIDDEN int build_dev_model(td_ctx* c, const td_model_desc* m, DevModel& out);   // (td_api.hip) a description validated and its tables on the device
TD_HIDDEN void free_dev_model(DevModel& d);                                         // (td_api.hip) ... and gone again (td_arch_scores brings candidates of its own)

#define HIPCHK(c, call)                                                                       \
	do {                                                                                      \
		hipError_t e_ = (call);                                                               \
		if (e_ != hipSuccess) return fail((c), "%s failed: %s", #call, hipGetErrorString(e_)); \
	} while (0)

// everything queued on the compute streams has finished
static hipError_t sync_compute(td_ctx* c)
{
	hipError_t e = hipStreamSynchronize(c->stream);
	if (e == hipSuccess && c->stream2) e = hipStreamSynchronize(c->stream2);
	if (e == hipSuccess && c->s_aux) e = hipStreamSynchronize(c->s_aux);
	if (e == hipSuccess && c->s_fin) e = hipStreamSynchronize(c->s_fin);
	return e;
}

// the context's device is the current one and nothing is queued on its compute streams any more
static int wait_compute(td_ctx* c)
{
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	return TD_OK;
}

template <typename T>
static int ensure(td_ctx* c, T** p, size_t* cap, size_t bytes)
{
	if (*cap >= bytes && *p) return TD_OK;
	if (*p) { HIPCHK(c, hipFree(*p)); *p = nullptr; *cap = 0; }
	if (bytes == 0) bytes = 256;
	HIPCHK(c, hipMalloc((void**)p, bytes));
	*cap = bytes;
	if (c && c->debug_alloc && bytes > (1u << 30)) fprintf(stderr, "tagdust_hip: hipMalloc(%zu) = %p\n", bytes, (void*)*p);
	return TD_OK;
}

template <typename T>
static int ensure_pinned(td_ctx* c, T** p, size_t* cap, size_t bytes)
{
	if (*cap >= bytes && *p) return TD_OK;
	if (*p) { HIPCHK(c, hipHostFree(*p)); *p = nullptr; *cap = 0; }
	if (bytes == 0) bytes = 256;
	bytes += bytes / 4;   // head room: batches of a run differ a little in size
	HIPCHK(c, hipHostMalloc((void**)p, bytes, hipHostMallocPortable));   // (several devices of one process may DMA from it)
	*cap = bytes;
	return TD_OK;
}

// td_kernels.hip: the generic decode kernel
extern "C" TD_HIDDEN hipError_t td_launch_decode(const TdKernelArgs* ka, hipStream_t stream);
extern "C" TD_HIDDEN int td_kernel_block_threads(void);
extern "C" TD_HIDDEN hipError_t td_launch_decode_multi(const TdKernelArgs* d_args, int n_models, int max_slots, hipStream_t stream);

// td_batch.hip
TD_HIDDEN double wall_ms();

// the output pointers of a launch's argument struct into such a block (out_labels where the struct has one: run_rna_dust has none)
template <typename Args> static auto point_labels(Args& a, int8_t* p, int) -> decltype((void)a.out_labels) { a.out_labels = p; }
template <typename Args> static void point_labels(Args&, int8_t*, long) {}
template <typename Args>
static void point_outputs(Args& a, uint8_t* out, const OutLayout& ol)
{
	float* soa = (float*)out;
	const int64_t st = ol.soa_stride / 4;
	a.out_f = soa; a.out_b = soa + st; a.out_r = soa + 2 * st; a.out_bar = soa + 3 * st; a.out_q = soa + 4 * st;
	a.out_type = (int32_t*)(soa + 5 * st); a.out_barcode = (int32_t*)(soa + 6 * st); a.out_finger = (int32_t*)(soa + 7 * st);
	a.out_keep = (uint32_t*)(out + ol.keep);
	point_labels(a, (int8_t*)(out + ol.labels), 0);
}

// what the specialised kernel's arguments share with the generic kernel's (layouts, bound tables, tile counter, label runs: the caller's)
static TdSpecArgs spec_args_from(const TdKernelArgs& ka)
{
	TdSpecArgs sa{};
	sa.logsum = ka.logsum; sa.packed = ka.packed; sa.lens = ka.lens;
	sa.n_tiles = ka.n_tiles; sa.n_slots = ka.n_slots; sa.lmax = ka.lmax; sa.nw2 = ka.nw2; sa.nw1 = ka.nw1;
	sa.mode = ka.mode; sa.threshold = ka.threshold; sa.minlen = ka.minlen; sa.dust = ka.dust;
	sa.win_start = ka.win_start; sa.win_len = ka.win_len;
	sa.out_f = ka.out_f; sa.out_b = ka.out_b; sa.out_r = ka.out_r; sa.out_bar = ka.out_bar; sa.out_q = ka.out_q;
	sa.out_type = ka.out_type; sa.out_barcode = ka.out_barcode; sa.out_finger = ka.out_finger;
	sa.out_keep = ka.out_keep; sa.out_labels = ka.out_labels; sa.counters = ka.counters;
	sa.art_text = ka.art_text; sa.art_index = ka.art_index; sa.art_left = ka.art_left; sa.art_n = ka.art_n; sa.art_fe = ka.art_fe;
	sa.ws = ka.ws;
	return sa;
}

// td_spec_host.hip: the specialised kernel's life in a context.  The compute streams are idle wherever a kernel is loaded.
TD_HIDDEN int spec_model_uploaded(td_ctx* c);            // the tables of a new model are up: plan, compile now or in the background
TD_HIDDEN int spec_handover(td_ctx* c, bool block);      // a finished background compile takes over (block: wait for it)
TD_HIDDEN int spec_before_batch(td_ctx* c, int lmax);    // reads this long: the logsum form that is safe for them, their bound tables
TD_HIDDEN int spec_load_window_variant(td_ctx* c);       // the first batch through a -start/-end window
TD_HIDDEN hipError_t spec_launch(td_ctx* c, const TdSpecArgs& sa, hipStream_t stream);
TD_HIDDEN int spec_state_now(td_ctx* c);                 // option "spec_state"
TD_HIDDEN void spec_retire_jobs(td_ctx* c, bool wait);   // the pending compile may finish, it is never loaded (wait: the context goes)
TD_HIDDEN int spec_unload(td_ctx* c);
