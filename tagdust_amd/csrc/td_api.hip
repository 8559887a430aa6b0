// td_api.hip -- C-ABI host layer of libtagdust_hip.so (declared in include/tagdust_hip.h).
//
// Replaces the reference's run_pHMM() fan-out (src/barcode_hmm.c:1895-2029): instead of T pthreads with
// private model copies, one context per GPU holds the flattened model in HBM and launches the decode
// kernel (td_kernels.hip) over a resident batch.  No torch, no CPU fallback: every entry point fails
// with TD_FAIL (and a message in td_last_error) when HIP does.  What is decided without the device stands in plain C++ units
// and is only applied here: a description checked and flattened, the -ref text packed, the logsum table (td_model_flat.cpp),
// the geometry of a batch (td_batch_plan.cpp).
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include <mutex>
#include <thread>

#include "../../include/tagdust_model.h"
#include "td_ctx.h"
#include "td_model_flat.h"
#include "td_rnadust.h"
#include "td_stats.h"

static std::string g_create_error;

// The copy threads of one context: started once, reused by every batch (the calling thread takes a share of each copy itself).
// The pipelined calls keep six streams busy (two compute streams, upload, download and two for the small kernels around the
// decode).  The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues, four unless told otherwise: two of the
// six then share one, and whatever sits behind a 20 ms decode launch in its queue waits for it.  Eight leaves every stream its
// own queue (measured on one box: 17.6 / 17.6 ms per 2^20-read step against 17.6 / 18.5 with four).  The runtime reads the
// variable when it initialises, at the process's first HIP call; a value the user has set is left alone.
// That works when this library is loaded before the process's first HIP call (the drop-in binary, the Python harness); a host
// that initialised HIP first keeps the runtime's own default, and can see so: td_get_option("hw_queues") is what the runtime
// was configured with when it initialised as far as this library can tell, "hw_queues_late" says the request came too late.
// (Whether the runtime is up is read off the process's open files: initialising it opens /dev/kfd.)
static int g_hwq_user = 0;       // GPU_MAX_HW_QUEUES as the user had set it when the library was loaded (0: not set)
static bool g_hwq_late = false;  // ... the HIP runtime was already initialised then
static bool kfd_is_open()
{
	char path[64], target[64];
	for (int fd = 0; fd < 256; fd++) {
		snprintf(path, sizeof path, "/proc/self/fd/%d", fd);
		const ssize_t n = readlink(path, target, sizeof target - 1);
		if (n <= 0) continue;
		target[n] = 0;
		if (!strcmp(target, "/dev/kfd")) return true;
	}
	return false;
}
__attribute__((constructor)) static void td_want_hw_queues()
{
	if (const char* e = getenv("GPU_MAX_HW_QUEUES")) { g_hwq_user = atoi(e) > 0 ? atoi(e) : 0; if (g_hwq_user) return; }
	g_hwq_late = kfd_is_open();
	if (!g_hwq_late) setenv("GPU_MAX_HW_QUEUES", "8", 0);
}

int fail(td_ctx* c, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	if (c) c->err = buf; else g_create_error = buf;
	return TD_FAIL;
}

extern "C" const char* td_last_error(const td_ctx* ctx)
{
	return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

extern "C" void td_stream_release(void);   // td_stream_reader.cpp: the page-locked batch buffers td_stream_run keeps between runs
static std::mutex g_live_mu;
static int g_live_ctx = 0;

extern "C" int td_ctx_create(int device, td_ctx** out)
{
	if (!out) return fail(nullptr, "td_ctx_create: out is NULL");
	*out = nullptr;
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	if (e != hipSuccess || ndev <= 0)
		return fail(nullptr, "td_ctx_create: no HIP device available (%s) -- this library has no CPU path",
		            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
	if (device < 0 || device >= ndev) return fail(nullptr, "td_ctx_create: device %d out of range (0..%d)", device, ndev - 1);
	td_ctx* c = new td_ctx();
	c->device = device;
	hipDeviceProp_t prop;
	if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
		delete c;
		return fail(nullptr, "td_ctx_create: cannot select device %d", device);
	}
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		std::string arch = prop.gcnArchName;
		delete c;
		return fail(nullptr, "td_ctx_create: device %d is %s; this library is built for gfx950 (MI355X) only", device, arch.c_str());
	}
	c->n_cu = prop.multiProcessorCount;
	if (const char* e = getenv("TD_SPECIALIZE")) c->spec.specialize = atoi(e) != 0;
	if (const char* e = getenv("TD_OVERLAP")) c->overlap = atoi(e) != 0;
	if (const char* e = getenv("TD_COMPACT_EGRESS")) c->compact_egress = atoi(e) != 0;
	if (const char* e = getenv("TD_RLE_CAP")) { const int v = atoi(e); if (v >= 1 && v <= 127) c->rle_cap_forced = v; }
	if (getenv("TD_NO_LENGTH_CLASSES")) c->length_classes = 0;
	if (getenv("TD_DEBUG_WAIT")) c->debug_wait = 1;
	if (getenv("TD_DEBUG_ALLOC")) c->debug_alloc = 1;
	if (const char* e = getenv("TD_WAVE_SLOTS")) { const long v = atol(e); if (v > 0) c->wave_slots_forced = v; }
	if (const char* e = getenv("TD_WS_CANDIDATES")) c->ws_candidates = atoi(e);
	if (const char* e = getenv("TD_SPEC_LSUM_LIMIT")) c->spec.lsum_limit = atof(e);
	if (getenv("TD_SPEC_SELFCHECK_FAIL")) c->spec.selfcheck_fail = 1;
	if (const char* e = getenv("TD_ASYNC_COMPILE")) c->spec.async_compile = atoi(e) != 0;
	c->hbm_total = prop.totalGlobalMem;
	bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
	          hipMalloc((void**)&c->d_logsum, sizeof(float) * TD_LOGSUM_LIVE) == hipSuccess &&
	          hipMalloc((void**)&c->d_counters, sizeof(unsigned long long) * TD_COUNTER_WORDS) == hipSuccess &&
	          hipMemcpy(c->d_logsum, td_logsum_table(), sizeof(float) * TD_LOGSUM_LIVE, hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemset(c->d_counters, 0, sizeof(unsigned long long) * TD_COUNTER_WORDS) == hipSuccess;
	if (!ok) {
		td_ctx_destroy(c);
		return fail(nullptr, "td_ctx_create: HIP resource allocation failed: %s", hipGetErrorString(hipGetLastError()));
	}
	{ std::lock_guard<std::mutex> lk(g_live_mu); g_live_ctx++; c->counted = true; }
	*out = c;
	return TD_OK;
}

static void slot_release(TdSlot& s);

static void free_dev_model(DevModel& d)
{
	void* p[] = { d.d_hdr, d.d_cols, d.d_hinfo, d.d_pred_off, d.d_pred_idx };
	for (void* q : p) if (q) (void)hipFree(q);
	d = DevModel();
}

extern "C" void td_ctx_destroy(td_ctx* c)
{
	if (!c) return;
	spec_retire_jobs(c, true);   // the background compiles this context started finish first
	(void)hipSetDevice(c->device);
	hipStream_t streams[] = { c->stream, c->stream2, c->s_aux, c->s_fin, c->s_up, c->s_down };
	for (hipStream_t st : streams) if (st) (void)hipStreamSynchronize(st);
	free_dev_model(c->dev);
	census_release(c);
	mol_release(c);
	void* bufs[] = { c->d_logsum, c->d_counters, c->d_ws, c->d_art_text, c->d_art_index, c->d_art_pk, c->d_art_seq, c->d_art_hits,
	                 c->spec.d_prune, c->d_tile_next, c->d_ws2, c->d_tile_next2 };
	for (void* p : bufs) if (p) (void)hipFree(p);
	for (int k = 0; k < TD_MAX_PIPELINE; k++) slot_release(c->slots[k]);
	if (c->ev_origin) (void)hipEventDestroy(c->ev_origin);
	(void)spec_unload(c);
	for (hipStream_t st : streams) if (st) (void)hipStreamDestroy(st);
	bool last = false;
	if (c->counted) { std::lock_guard<std::mutex> lk(g_live_mu); last = --g_live_ctx == 0; }
	delete c;
	// td_stream_run keeps up to 1 GiB of page-locked batch buffers for the next run of the process: with the last context gone
	// there is no next run to serve
	if (last) td_stream_release();
}

// ---------------------------------------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------------------------------------
// validate a description (td_model_flat.cpp) and put its tables on the device (synchronous copies)
static int build_dev_model(td_ctx* c, const td_model_desc* m, DevModel& out)
{
	TdFlatModel f;
	std::string why;
	if (!td_flatten_model(m, f, why)) return fail(c, "%s", why.c_str());
	DevModel d;
	d.h = f.h;
	bool ok = hipMalloc((void**)&d.d_hdr, sizeof f.h) == hipSuccess && hipMalloc((void**)&d.d_cols, sizeof(TdCol) * f.cols.size()) == hipSuccess &&
	          hipMalloc((void**)&d.d_hinfo, sizeof(uint32_t) * f.hinfo.size()) == hipSuccess &&
	          hipMalloc((void**)&d.d_pred_off, sizeof(int32_t) * f.pred_off.size()) == hipSuccess &&
	          hipMalloc((void**)&d.d_pred_idx, sizeof(int32_t) * f.pred_idx.size()) == hipSuccess &&
	          hipMemcpy(d.d_hdr, &f.h, sizeof f.h, hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemcpy(d.d_cols, f.cols.data(), sizeof(TdCol) * f.cols.size(), hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemcpy(d.d_hinfo, f.hinfo.data(), sizeof(uint32_t) * f.hinfo.size(), hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemcpy(d.d_pred_off, f.pred_off.data(), sizeof(int32_t) * f.pred_off.size(), hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemcpy(d.d_pred_idx, f.pred_idx.data(), sizeof(int32_t) * f.pred_idx.size(), hipMemcpyHostToDevice) == hipSuccess;
	if (!ok) { free_dev_model(d); return fail(c, "td_model_upload: device tables: %s", hipGetErrorString(hipGetLastError())); }
	out = d;
	return TD_OK;
}

extern "C" int td_model_upload(td_ctx* c, const td_model_desc* m)
{
	if (!c || !m) return fail(c, "td_model_upload: NULL argument");
	HIPCHK(c, hipSetDevice(c->device));
	// a rejected upload (tickets in flight, an invalid description) leaves the context as it was
	if (tickets_outstanding(c)) return fail(c, "td_model_upload: td_submit tickets are outstanding (td_wait them first)");
	spec_retire_jobs(c, false);   // a pending background compile is superseded: its result may land in the caches, never in this context
	DevModel dm;
	if (build_dev_model(c, m, dm) != TD_OK) return TD_FAIL;
	// from here on the context holds no usable model / batch until every step below has succeeded
	c->have_model = false;
	for (int k = 0; k < TD_MAX_PIPELINE; k++) { c->slots[k].staged = false; c->slots[k].ran = false; }   // batches are staged per model
	HIPCHK(c, sync_compute(c));
	census_release(c);   // a census counts one model's segment: a new model switches it off
	mol_release(c);      // ... and the molecule count reads one model's labels
	free_dev_model(c->dev);
	c->dev = dm;
	c->model.assign(m);
	c->half_slots = false;   // the workspace geometry belongs to the model
	if (spec_model_uploaded(c) != TD_OK) return TD_FAIL;
	c->have_model = true;
	return TD_OK;
}

extern "C" int td_set_option(td_ctx* c, const char* name, int32_t value)
{
	if (!c || !name) return TD_FAIL;
	if (!strcmp(name, "specialize")) {
		c->spec.specialize = value != 0; // takes effect at the next td_model_upload
		return TD_OK;
	}
	if (!strcmp(name, "poison_workspace")) { c->poison = value != 0; return TD_OK; }
	if (!strcmp(name, "async_compile")) { c->spec.async_compile = value != 0; return TD_OK; }   // ... the next td_model_upload
	if (!strcmp(name, "spec_probe")) { c->spec.probe = value != 0; return TD_OK; }         // ... the next load of a specialised kernel
	if (!strcmp(name, "compact_egress")) { c->compact_egress = value != 0; return TD_OK; }          // takes effect with the next download / td_submit
	if (!strcmp(name, "stable_input")) {
		if (tickets_outstanding(c)) return fail(c, "td_set_option: stable_input cannot change while tickets are outstanding");
		c->stable_input = value != 0;
		return TD_OK;
	}
	if (!strcmp(name, "length_classes_enabled")) { c->length_classes = value != 0; return TD_OK; }  // ... the next upload
	if (!strcmp(name, "debug_wait")) { c->debug_wait = value != 0; return TD_OK; }
	if (!strcmp(name, "spec_lsum_limit")) { c->spec.lsum_limit = value > 0 ? (double)value : 1.0e6; return TD_OK; }   // tests; next upload
	if (!strcmp(name, "rle_cap")) {
		if (value < 0 || value > 127) return fail(c, "td_set_option: rle_cap must be 0 (default) .. 127");
		c->rle_cap_forced = value;
		return TD_OK;
	}
	if (!strcmp(name, "host_threads")) {
		if (value < 1 || value > 16) return fail(c, "td_set_option: host_threads must be 1..16");
		c->host_threads = value;
		return TD_OK;
	}
	if (!strcmp(name, "overlap_decode")) {
		if (tickets_outstanding(c)) return fail(c, "td_set_option: overlap_decode cannot change while tickets are outstanding");
		c->overlap = value != 0; c->submit_parity = 0;
		return TD_OK;
	}
	if (!strcmp(name, "pipeline_depth")) {
		if (value < 1 || value > TD_MAX_PIPELINE) return fail(c, "td_set_option: pipeline_depth must be 1..%d", TD_MAX_PIPELINE);
		if (tickets_outstanding(c)) return fail(c, "td_set_option: pipeline_depth cannot change while tickets are outstanding");
		c->pipeline_depth = value; c->next_slot = 0;
		return TD_OK;
	}
	return fail(c, "td_set_option: unknown option %s", name);
}

extern "C" int td_get_option(td_ctx* c, const char* name, int32_t* value)
{
	if (!c || !name || !value) return TD_FAIL;
	if (!strcmp(name, "specialize")) { *value = c->spec.specialize; return TD_OK; }
	if (!strcmp(name, "spec_lsum_clamped")) { *value = c->spec.ready && !c->spec.oob; return TD_OK; }
	if (!strcmp(name, "pipeline_depth")) { *value = c->pipeline_depth; return TD_OK; }
	if (!strcmp(name, "async_compile")) { *value = c->spec.async_compile; return TD_OK; }
	if (!strcmp(name, "spec_probe")) { *value = c->spec.probe; return TD_OK; }
	if (!strcmp(name, "spec_state")) { *value = spec_state_now(c); return TD_OK; }
	if (!strcmp(name, "spec_batches_generic")) { *value = c->spec.batches_generic; return TD_OK; }
	if (!strcmp(name, "spec_compiles_started")) { *value = td_spec_compiles_started(); return TD_OK; }
	if (!strcmp(name, "spec_probe_us")) { *value = c->spec.probe_us; return TD_OK; }
	if (!strcmp(name, "host_threads")) { *value = c->host_threads; return TD_OK; }
	if (!strcmp(name, "artifacts_active")) { *value = c->art_n > 0; return TD_OK; }
	if (!strcmp(name, "dust")) { *value = c->dust; return TD_OK; }   // param->dust as td_set_params set it
	if (!strcmp(name, "length_classes")) { *value = c->slots[c->last_slot].n_big; return TD_OK; }   // wave slots of the long geometry in the last batch
	if (!strcmp(name, "overlap_decode")) { *value = c->overlap; return TD_OK; }
	if (!strcmp(name, "compact_egress")) { *value = c->compact_egress; return TD_OK; }
	if (!strcmp(name, "stable_input")) { *value = c->stable_input; return TD_OK; }
	if (!strcmp(name, "length_classes_enabled")) { *value = c->length_classes; return TD_OK; }
	// hardware queues of the HIP runtime as far as the library can tell (see td_want_hw_queues): the user's GPU_MAX_HW_QUEUES, else
	// the 8 the library asked for when it was loaded before the runtime initialised, else the runtime's own default of 4
	if (!strcmp(name, "hw_queues")) { *value = g_hwq_user ? g_hwq_user : (g_hwq_late ? 4 : 8); return TD_OK; }
	if (!strcmp(name, "hw_queues_late")) { *value = g_hwq_late ? 1 : 0; return TD_OK; }
	// which fast paths the model / the last batch actually got (read-only)
	if (!strcmp(name, "prune_active")) {
		// the loaded specialised kernel prunes by position AND the bound tables of the last batch's geometry are live
		*value = c->spec.ready && c->spec.prune_live && (c->spec.plan.prune_segs > 0 || c->spec.plan.sfx_first < c->spec.plan.S);
		return TD_OK;
	}
	if (!strcmp(name, "census_active")) { *value = c->census.on; return TD_OK; }
	if (!strcmp(name, "census_kernel_us")) return census_last_kernel_us(c, value);   // the count kernel's time of the last counted batch
	if (!strcmp(name, "molecules_active")) { *value = c->molecules.on; return TD_OK; }
	if (!strcmp(name, "dedup_active")) { *value = c->molecules.dedup.on; return TD_OK; }
	if (!strcmp(name, "dedup_frozen")) { *value = c->molecules.frozen.on; return TD_OK; }   // td_mol_dedup_freeze: batches are replayed
	if (!strcmp(name, "mate_bases")) { *value = c->molecules.mate.bases; return TD_OK; }   // td_mol_mate_enable's M, 0 = off
	if (!strcmp(name, "collapse_active")) { *value = c->molecules.collapse.on; return TD_OK; }
	// molecules_, dedup_, collapse_origin_, dedup_replay_ and mate_kernel_us: the stage's time of the last batch (-1: none of them)
	if (const int rc = mol_kernel_us(c, name, value); rc >= 0) return rc;
	if (!strcmp(name, "overlap_active")) {
		// pipelined batches alternate between two compute streams / workspaces (off: option, generic kernel, depth 1, or HBM
		// could not hold the second workspace)
		*value = c->overlap && c->pipeline_depth > 1 && c->spec.ready && c->stream2 != nullptr && c->d_ws2 != nullptr;
		return TD_OK;
	}
	return fail(c, "td_get_option: unknown option %s", name);
}

extern "C" int td_set_artifacts(td_ctx* c, const uint8_t* string, const int32_t* s_index, int32_t n_seq,
                                int32_t filter_error, int32_t n_threads)
{
	if (!c) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	if (c->d_art_text) { HIPCHK(c, hipFree(c->d_art_text)); c->d_art_text = nullptr; }
	if (c->d_art_index) { HIPCHK(c, hipFree(c->d_art_index)); c->d_art_index = nullptr; }
	if (c->d_art_pk) { HIPCHK(c, hipFree(c->d_art_pk)); c->d_art_pk = nullptr; }
	if (c->d_art_seq) { HIPCHK(c, hipFree(c->d_art_seq)); c->d_art_seq = nullptr; }
	if (c->d_art_hits) { HIPCHK(c, sync_compute(c)); HIPCHK(c, hipFree(c->d_art_hits)); c->d_art_hits = nullptr; }   // (a count may still be queued)
	c->art_n = 0;
	if (n_seq <= 0) return TD_OK;
	if (!string || !s_index) return fail(c, "td_set_artifacts: null argument");
	if (n_threads < 1) return fail(c, "td_set_artifacts: n_threads = %d", n_threads);
	// the text as TD_MODE_RNA_DUST reads it (td_model_flat.cpp)
	std::vector<int32_t> seq;
	std::vector<uint32_t> pk;
	std::string why;
	if (!td_pack_artifacts(string, s_index, n_seq, seq, pk, why)) return fail(c, "%s", why.c_str());
	const size_t bytes = (size_t)s_index[n_seq];
	HIPCHK(c, hipMalloc((void**)&c->d_art_text, bytes ? bytes : 1));
	HIPCHK(c, hipMalloc((void**)&c->d_art_index, sizeof(int32_t) * ((size_t)n_seq + 1)));
	if (bytes) HIPCHK(c, hipMemcpy(c->d_art_text, string, bytes, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->d_art_index, s_index, sizeof(int32_t) * ((size_t)n_seq + 1), hipMemcpyHostToDevice));
	HIPCHK(c, hipMalloc((void**)&c->d_art_pk, pk.size() * 4));
	HIPCHK(c, hipMalloc((void**)&c->d_art_seq, seq.size() * 4));
	HIPCHK(c, hipMemcpy(c->d_art_pk, pk.data(), pk.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(c, hipMemcpy(c->d_art_seq, seq.data(), seq.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(c, hipMalloc((void**)&c->d_art_hits, sizeof(unsigned long long) * (size_t)n_seq));
	HIPCHK(c, hipMemset(c->d_art_hits, 0, sizeof(unsigned long long) * (size_t)n_seq));
	c->art_n = n_seq; c->art_fe = filter_error; c->art_threads = n_threads;
	return TD_OK;
}

extern "C" int td_set_window(td_ctx* c, int32_t matchstart, int32_t matchend)
{
	if (!c) return TD_FAIL;
	if (matchstart == -1 && matchend == -1) { c->match_start = 0; c->match_len = 0; return TD_OK; }
	if (matchstart < 0 || matchend <= matchstart) return fail(c, "td_set_window: need 0 <= matchstart < matchend (or -1, -1 for none)");
	if (c->census.on) return fail(c, "td_set_window: a census is on (td_census_disable first): labels behind a window do not spell the barcode");
	if (c->molecules.on) return fail(c, "td_set_window: a molecule count is on (td_mol_disable first): labels behind a window do not mark the read's bases");
	c->match_start = matchstart; c->match_len = matchend - matchstart;
	return TD_OK;
}

extern "C" int td_set_batch_window(td_ctx* c, int64_t first_read, int64_t total_reads)
{
	if (!c) return TD_FAIL;
	if (first_read < 0 || total_reads < 0) return fail(c, "td_set_batch_window: negative argument");
	c->win_first = first_read; c->win_total = total_reads;
	return TD_OK;
}

extern "C" int td_set_params(td_ctx* c, float threshold, int32_t minlen, int32_t dust)
{
	if (!c) return TD_FAIL;
	c->threshold = threshold; c->minlen = minlen; c->dust = dust;
	return TD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// batches
// ---------------------------------------------------------------------------------------------------------
// A batch lives in a slot.  The host hands over the reads as they are (base codes or FASTQ sequence text + offsets) and
// gets per-read records, rewritten sequences and labels back in the same order; everything in between -- base coding,
// the stable sort by length, 2-bit packing and lane interleave, and on the way back un-permuting and de-interleaving --
// runs on the device (td_stage.hip), so a transfer is one copy of contiguous bytes each way.  The synchronous calls
// (td_batch_upload / td_run / td_batch_download) work on slot 0; td_submit / td_wait rotate over `pipeline_depth` slots
// with the copies on their own streams, so that the upload of batch k+1 and the download of batch k-1 overlap the decode
// kernel of batch k.  One HBM workspace serves all slots (decode kernels are serialised on the compute stream).
// is this host pointer page-locked (hipHostMalloc / hipHostRegister)?  Then the DMA engines can use it directly.
bool is_pinned(const void* p)
{
	if (!p) return false;
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
	return a.type == hipMemoryTypeHost;
}

// memcpy on the context's host threads (pageable caller memory <-> pinned staging)
static void parallel_copy(td_ctx* c, void* dst, const void* src, size_t bytes)
{
	c->pool.copy(dst, src, bytes, c->host_threads);
}

static int slot_events(td_ctx* c, TdSlot& s)
{
	if (s.ev_k0) return TD_OK;
	HIPCHK(c, hipEventCreate(&s.ev_k0));
	HIPCHK(c, hipEventCreate(&s.ev_k1));
	HIPCHK(c, hipEventCreateWithFlags(&s.ev_up, hipEventDisableTiming));
	HIPCHK(c, hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
	HIPCHK(c, hipEventCreateWithFlags(&s.ev_down, hipEventDisableTiming));
	HIPCHK(c, hipEventCreateWithFlags(&s.ev_pack, hipEventDisableTiming));
	HIPCHK(c, hipEventCreateWithFlags(&s.ev_hits, hipEventDisableTiming));
	return TD_OK;
}

static void slot_release(TdSlot& s)
{
	void* dev[] = { s.d_raw, s.d_offs, s.d_read_at, s.d_keys, s.d_vals, s.d_sort_tmp, s.d_packed, s.d_lens, s.d_art_left,
	                s.d_out, s.d_res, s.d_seq, s.d_lab, s.d_keepo, s.d_rle, s.d_runs, s.d_judged, s.d_mate_raw, s.d_mate_offs, s.d_mate_w,
	                s.d_mate_n };
	for (void* p : dev) if (p) (void)hipFree(p);
	void* pinned[] = { s.h_raw, s.h_offs, s.h_res, s.h_seq, s.h_lab, s.h_keepo, s.h_rle, s.h_mate_raw, s.h_mate_offs };
	for (void* p : pinned) if (p) (void)hipHostFree(p);
	hipEvent_t ev[] = { s.ev_up, s.ev_k0, s.ev_k1, s.ev_done, s.ev_down, s.ev_pack, s.ev_hits };
	for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
	s = TdSlot();
}

// the device's free memory, when the workspace plan asks for it
static int hbm_free(td_ctx* c, size_t& free_b)
{
	size_t total_b = 0;
	HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
	return TD_OK;
}

// Size the shared workspace for a batch with this geometry: td_batch_plan.cpp decides, this applies the decision and does what
// needs the device.  Growing the workspace (or switching the kernel to the clamped logsum) waits for the decode kernels in flight first.
static int ensure_workspace(td_ctx* c, TdSlot& s)
{
	if (spec_before_batch(c, s.lmax) != TD_OK) return TD_FAIL;
	make_layout(s.lay, c->dev.h.S, c->dev.h.H, c->dev.h.C, s.lmax, c->dev.h.max_ncol);
	TdWsRequest rq;
	rq.small_slot_bytes = rq.big_slot_bytes = s.lay.slot_bytes;
	if (c->spec.ready) {
		td_spec_layout(s.slay, c->spec.plan, s.n_long > 0 ? s.lmax_small : s.lmax);   // the geometry of the many
		td_spec_layout(s.slay_big, c->spec.plan, s.lmax);
		rq.small_slot_bytes = s.slay.slot_bytes; rq.big_slot_bytes = s.slay_big.slot_bytes;
	}
	rq.n_tiles = s.n_tiles; rq.n_long = s.n_long; rq.lmax_small = s.lmax_small; rq.lmax = s.lmax;
	rq.wpb = (c->spec.ready ? c->spec.block : td_kernel_block_threads()) / TD_WAVE;
	rq.want_slots = c->wave_slots_forced > 0 ? c->wave_slots_forced : (int64_t)c->n_cu * (c->spec.ready ? c->spec.waves_per_cu : 2 * rq.wpb);
	rq.spec_ready = c->spec.ready; rq.pipelined = s.pipelined; rq.overlap = c->overlap; rq.pipeline_depth = c->pipeline_depth;
	rq.half_slots = c->half_slots; rq.wsi = s.wsi;
	rq.cap_ws = c->cap_ws; rq.cap_ws2 = c->cap_ws2; rq.ws_candidates = c->ws_candidates;
	const TdWsPlan p = plan_workspace(rq, [](void* ctx, size_t* free_b) { return hbm_free((td_ctx*)ctx, *free_b) == TD_OK; }, c);
	c->half_slots = p.half_slots;
	if (p.overlap_given_up) { c->overlap = 0; s.wsi = 0; s.cs = c->stream; }
	s.n_long = p.n_long; s.lmax_small = p.lmax_small; s.n_big = p.n_big;
	if (p.one_geometry) s.slay = s.slay_big;
	if (p.query_failed) return TD_FAIL;   // (hbm_free left the message)
	if (p.no_fit) return fail(c, "td_batch_upload: workspace of %lld bytes per wave does not fit in HBM", (long long)p.ws_slot_bytes);
	if (p.alloc_bytes > 0) {
		uint8_t*& ws = s.wsi ? c->d_ws2 : c->d_ws;
		size_t& cap_ws = s.wsi ? c->cap_ws2 : c->cap_ws;
		const size_t need = p.alloc_bytes;
		HIPCHK(c, sync_compute(c));
		if (p.n_candidates <= 1) {
			if (ensure(c, &ws, &cap_ws, need) != TD_OK) return TD_FAIL;
		} else {   // candidates that exist side by side: a memory-side probe runs over each, the fastest stays, the others are freed
			if (ws) { HIPCHK(c, hipFree(ws)); ws = nullptr; cap_ws = 0; }
			uint8_t* cand[4] = { nullptr, nullptr, nullptr, nullptr };
			float ms[4] = { 0, 0, 0, 0 };
			int n_ok = 0, best = -1;
			for (int k = 0; k < p.n_candidates; k++) {
				if (hipMalloc((void**)&cand[k], need) != hipSuccess) { (void)hipGetLastError(); cand[k] = nullptr; break; }
				n_ok++;
			}
			for (int k = 0; k < n_ok; k++) {
				if (td_ws_probe(cand[k], p.ws_slot_bytes, p.n_wave_slots, c->stream, &ms[k]) != hipSuccess) ms[k] = 1e30f;
				if (best < 0 || ms[k] < ms[best]) best = k;
			}
			if (best < 0) return fail(c, "td_batch_upload: workspace of %zu bytes could not be allocated", need);
			if (c->debug_alloc) fprintf(stderr, "tagdust_hip: workspace candidates: probe %.2f %.2f %.2f %.2f ms -> #%d\n", ms[0], ms[1], ms[2], ms[3], best);
			for (int k = 0; k < n_ok; k++) if (k != best) (void)hipFree(cand[k]);
			ws = cand[best]; cap_ws = need;
		}
	}
	s.n_wave_slots = p.n_wave_slots;
	s.ws_slot_bytes = p.ws_slot_bytes;
	s.ws_bytes = p.ws_bytes;
	return TD_OK;
}

// Reads -> device, sorted and packed.  Copies go on `up` (the compute stream itself for the synchronous calls); the
// kernels on the compute stream wait for them through ev_up.
static int slot_stage(td_ctx* c, TdSlot& s, const TdRoute& route, const void* bases, int is_ascii, const int64_t* offs, int64_t n, hipStream_t up, bool with_workspace = true, bool take_mate = false)
{
	s.reset_staged(route);   // nothing of the slot's previous batch survives (nor of its launch, nor of its download)
	if (with_workspace && !c->have_model) return fail(c, "td_batch_upload: no model uploaded");
	if (!offs || n < 0 || (!bases && n > 0 && offs[n] > offs[0])) return fail(c, "td_batch_upload: bad arguments");
	if (n > 0x7fffffffLL - TD_WAVE) return fail(c, "td_batch_upload: %lld reads in one batch", (long long)n);
	HIPCHK(c, hipSetDevice(c->device));
	if (slot_events(c, s) != TD_OK) return TD_FAIL;
	const int64_t base = offs[0];   // a sub-range of a larger batch keeps the caller's offsets (td_multi_decode)
	// offsets: one pass that copies them into pinned memory and finds the longest / shortest read
	if (ensure_pinned(c, &s.h_offs, &s.cap_h_offs, (size_t)(n + 1) * 8) != TD_OK) return TD_FAIL;
	int lmax = 1, lmin = 0x7fffffff;
	int64_t bad = -1;
	s.h_offs[0] = 0;
	for (int64_t i = 0; i < n; i++) {
		const int64_t l = offs[i + 1] - offs[i];
		s.h_offs[i + 1] = offs[i + 1] - base;
		if (l < 0 || l > 100000) { bad = i; break; }
		if (l > lmax) lmax = (int)l;
		if (l < lmin) lmin = (int)l;
	}
	if (bad >= 0) return fail(c, "td_batch_upload: read %lld has length %lld", (long long)bad, (long long)(offs[bad + 1] - offs[bad]));
	const int64_t n_bases = n > 0 ? offs[n] - base : 0;
	const int64_t n_tiles = (n + TD_WAVE - 1) / TD_WAVE;
	// length classes (td_batch_plan.cpp): do the batch's longest tiles get wave slots of their own geometry?
	const TdLengthClasses lc = plan_length_classes(offs, n, lmin, lmax, n_tiles, c->spec.ready && with_workspace && c->length_classes);
	s.n_long = lc.n_long; s.lmax_small = lc.lmax_small;
	const int nw2 = (lmax + 15) / 16, nw1 = (lmax + 31) / 32;
	const bool sorted = n > 0 && lmin != lmax;

	// device buffers
	const size_t n_packed = (size_t)(n_tiles * (int64_t)(nw2 + nw1) * TD_WAVE), n_lanes = (size_t)(n_tiles * TD_WAVE);
	const OutLayout ol = out_layout(n_tiles, lmax, nw1);
	if (ensure(c, &s.d_raw, &s.cap_raw, (size_t)n_bases) != TD_OK || ensure(c, &s.d_offs, &s.cap_offs, (size_t)(n + 1) * 8) != TD_OK ||
	    ensure(c, &s.d_packed, &s.cap_packed, n_packed * 4) != TD_OK || ensure(c, &s.d_lens, &s.cap_lens, n_lanes * 4) != TD_OK ||
	    ensure(c, &s.d_art_left, &s.cap_art_left, n_lanes) != TD_OK || ensure(c, &s.d_out, &s.cap_out, (size_t)ol.total) != TD_OK)
		return TD_FAIL;
	size_t sort_tmp = 0;
	if (sorted) {
		sort_tmp = td_stage_sort_temp_bytes(n, lmax);
		if (ensure(c, &s.d_read_at, &s.cap_read_at, (size_t)n * 4) != TD_OK || ensure(c, &s.d_keys, &s.cap_keys, (size_t)n * 8) != TD_OK ||
		    ensure(c, &s.d_vals, &s.cap_vals, (size_t)n * 4) != TD_OK || ensure(c, &s.d_sort_tmp, &s.cap_sort_tmp, sort_tmp) != TD_OK)
			return TD_FAIL;
	}
	s.lmax = lmax; s.nw2 = nw2; s.nw1 = nw1; s.n_tiles = (int32_t)n_tiles;
	if (with_workspace && ensure_workspace(c, s) != TD_OK) { s.n_tiles = 0; return TD_FAIL; }
	s.for_spec = with_workspace && c->spec.ready;
	s.n_tiles = 0;

	// host -> device: page-locked caller memory goes straight to the DMA engine, anything else through pinned staging
	const void* src = (const uint8_t*)bases + base;
	s.raw_direct = n_bases > 0 && is_pinned(src);
	if (n_bases > 0 && !s.raw_direct) {
		if (ensure_pinned(c, &s.h_raw, &s.cap_h_raw, (size_t)n_bases) != TD_OK) return TD_FAIL;
		parallel_copy(c, s.h_raw, src, (size_t)n_bases);
		src = s.h_raw;
		s.raw_host = s.h_raw;
	} else if (n_bases > 0 && c->stable_input && s.pipelined) {
		s.raw_host = (const uint8_t*)src;   // the caller's promise: untouched until td_wait -- the compact egress rebuilds from it
	}
	HIPCHK(c, hipMemcpyAsync(s.d_offs, s.h_offs, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, up));
	if (n_bases > 0) HIPCHK(c, hipMemcpyAsync(s.d_raw, src, (size_t)n_bases, hipMemcpyHostToDevice, up));
	if (take_mate && mol_mate_stage(c, s, n, up) != TD_OK) return TD_FAIL;   // mate mode: the named mate batch travels with its reads
	if (up != s.aux) {
		HIPCHK(c, hipEventRecord(s.ev_up, up));
		HIPCHK(c, hipStreamWaitEvent(s.aux, s.ev_up, 0));
	}
	if (sorted)
		HIPCHK(c, td_stage_sort(s.d_offs, n, lmax, s.d_read_at, s.d_keys, s.d_keys + n, s.d_vals, s.d_sort_tmp, sort_tmp, s.aux));
	TdStageBatch& b = s.sb;
	b = TdStageBatch{};
	b.raw = s.d_raw; b.offs = s.d_offs; b.n_reads = n; b.is_ascii = is_ascii;
	b.n_tiles = (int32_t)n_tiles; b.lmax = lmax; b.nw2 = nw2; b.nw1 = nw1;
	b.read_at = sorted ? s.d_read_at : nullptr;
	b.packed = s.d_packed; b.lens = s.d_lens; b.art_left = s.d_art_left;
	b.out_soa = s.d_out; b.soa_stride = ol.soa_stride;
	b.keep = (const uint32_t*)(s.d_out + ol.keep); b.labels = (const int8_t*)(s.d_out + ol.labels);
	HIPCHK(c, td_stage_pack(b, s.aux));
	if (take_mate && mol_mate_launch(c, s, n) != TD_OK) return TD_FAIL;   // (in front of ev_pack: the decode stream's wait covers it)
	if (s.aux != s.cs) {   // the decode kernel's stream waits for the packed batch
		HIPCHK(c, hipEventRecord(s.ev_pack, s.aux));
		HIPCHK(c, hipStreamWaitEvent(s.cs, s.ev_pack, 0));
	}

	s.n_reads = n; s.n_bases = n_bases; s.n_tiles = (int32_t)n_tiles; s.is_ascii = is_ascii; s.sorted = sorted;
	s.staged = true;
	return TD_OK;
}

// entries of a read's label-run table: a path visits one label per segment (+ the zeros behind a window, + one to spare)
static int rle_capacity(const td_ctx* c)
{
	int cap = c->dev.h.S + 2 < c->dev.h.H ? c->dev.h.S + 2 : c->dev.h.H;
	if (c->rle_cap_forced > 0) cap = c->rle_cap_forced;   // tests: force the overflow route
	return cap;
}

// the decode kernel over a staged slot
static int slot_rna_dust(td_ctx* c, TdSlot& s);

// -ref: the batch's reads per artifact sequence, added to the context's running hits on the batch's stream right behind the
// launch that left out_type (and behind ev_k1, so that the kernel times stay the launch's own).  Only called while a filter is
// set: a run without -ref launches nothing here.  The finish kernel waits for ev_hits, so that a slot whose batch has been
// waited for is no longer read by this count either.
static int slot_count_hits(td_ctx* c, TdSlot& s, const int32_t* out_type)
{
	HIPCHK(c, td_stage_art_hits(out_type, s.n_reads, c->art_n, c->d_art_hits, s.cs));
	HIPCHK(c, hipEventRecord(s.ev_hits, s.cs));
	s.hits_queued = true;
	return TD_OK;
}

static int slot_decode(td_ctx* c, TdSlot& s, int mode, bool want_labels = true)
{
	if (mode == TD_MODE_RNA_DUST) return slot_rna_dust(c, s);
	if (!c->have_model) return fail(c, "td_run: no model uploaded");
	if (mode != TD_MODE_GET_LABEL && mode != TD_MODE_GET_PROB && mode != TD_MODE_ARCH_COMP) return fail(c, "td_run: unsupported mode %d", mode);
	if (!s.staged) return fail(c, "td_run: no batch resident (td_batch_upload failed or was not called)");
	if (s.n_tiles > 0 && s.n_wave_slots == 0) return fail(c, "td_run: the resident batch was staged for TD_MODE_RNA_DUST, without a decode workspace (upload it again)");
	HIPCHK(c, hipSetDevice(c->device));
	// mate mode: a batch that was staged without its mates (or with those of another M) is not counted, and not decoded either
	if (mode == TD_MODE_GET_LABEL && c->molecules.mate.bases > 0 && c->molecules.mate.bases != s.mate_m) {
		c->molecules.mate.named = false;
		return fail(c, "td_run: mate mode is on (td_mol_mate_enable, %d bases) and the resident batch of %lld reads was staged without a mate "
		            "batch of as many reads: td_mol_mate_next first, then td_batch_upload; nothing was counted", c->molecules.mate.bases, (long long)s.n_reads);
	}
	s.reset_decoded();   // (runs_cap above all: a launch of the generic kernel, or an empty batch, must not hand the label runs of this
	                     // slot's previous launch to the finish kernel)
	s.mode = mode;
	if (s.n_tiles == 0) { s.ran = true; s.last_ms = 0.0f; return TD_OK; }
	if (c->spec.ready && s.for_spec && c->match_len > 0 && !c->spec.window) {   // first batch through a window: the kernel variant that applies it
		HIPCHK(c, sync_compute(c));
		if (spec_load_window_variant(c) != TD_OK) return TD_FAIL;
		if (!c->spec.ready) {   // the probe rejected that variant: this batch gets the generic kernel's workspace geometry after all
			s.n_long = 0; s.lmax_small = s.lmax;
			if (ensure_workspace(c, s) != TD_OK) return TD_FAIL;
			s.for_spec = false;
		}
	}
	// a batch is decoded by the kernel it was staged for: one staged before a background compile was handed over stays generic
	const bool use_spec = c->spec.ready && s.for_spec;
	if (s.for_spec && !c->spec.ready) return fail(c, "td_run: the resident batch was staged for a specialised kernel that is no longer loaded (upload it again)");
	const OutLayout ol = out_layout(s.n_tiles, s.lmax, s.nw1);
	TdKernelArgs ka{};
	ka.hdr = c->dev.d_hdr; ka.cols = c->dev.d_cols; ka.hinfo = c->dev.d_hinfo;
	ka.pred_off = c->dev.d_pred_off; ka.pred_idx = c->dev.d_pred_idx; ka.logsum = c->d_logsum;
	ka.packed = s.d_packed; ka.lens = s.d_lens;
	ka.n_tiles = s.n_tiles; ka.n_slots = s.n_wave_slots; ka.lmax = s.lmax; ka.nw2 = s.nw2; ka.nw1 = s.nw1;
	ka.mode = mode; ka.threshold = c->threshold; ka.minlen = c->minlen; ka.dust = c->dust; ka.want_labels = 1;
	ka.win_start = c->match_start; ka.win_len = c->match_len;
	point_outputs(ka, s.d_out, ol);
	ka.counters = c->d_counters;
	ka.ws = s.wsi ? c->d_ws2 : c->d_ws; ka.lay = s.lay;
	if (c->art_n > 0 && mode == TD_MODE_GET_LABEL) {
		s.sb.art_threads = c->art_threads;
		s.sb.art_first = c->win_first; s.sb.art_total = c->win_total;
		HIPCHK(c, td_stage_art_left(s.sb, s.cs));
		ka.art_text = c->d_art_text; ka.art_index = c->d_art_index; ka.art_left = s.d_art_left;
		ka.art_n = c->art_n; ka.art_fe = c->art_fe;
	}
	// tests: every byte of the workspace the kernel reads must have been written by this launch -- garbage (NaN floats,
	// all-ones masks) in place of whatever an earlier batch or model left there makes a read-before-write show
	if (c->poison) HIPCHK(c, hipMemsetAsync(ka.ws, 0xFF, (size_t)s.ws_bytes, s.cs));
	if (use_spec) {   // the tile counter of the dynamic tile assignment starts at zero (the first tiles go by slot number)
		int32_t*& tn = s.wsi ? c->d_tile_next2 : c->d_tile_next;
		if (!tn) HIPCHK(c, hipMalloc((void**)&tn, 256));
		HIPCHK(c, hipMemsetAsync(tn, 0, sizeof(int32_t), s.cs));
	}
	HIPCHK(c, hipEventRecord(s.ev_k0, s.cs));
	if (use_spec) {
		TdSpecArgs sa = spec_args_from(ka);
		sa.lay = s.slay;
		sa.lmax = s.n_big > 0 ? s.lmax_small : s.lmax;
		sa.n_big = s.n_big; sa.lmax_big = s.lmax; sa.lay_big = s.slay_big; sa.out_lmax = s.lmax;
		// the label runs for the compact egress, and the flag that says a read had more of them -- only for a batch whose labels
		// somebody will fetch (td_submit knows; a td_run batch may still be asked for them by td_batch_download)
		if (mode == TD_MODE_GET_LABEL && want_labels && c->compact_egress) {
			const int cap = rle_capacity(c);
			const size_t words = (size_t)s.n_tiles * (size_t)cap * TD_WAVE + 1;
			if (ensure(c, &s.d_runs, &s.cap_runs, words * 4) != TD_OK) return TD_FAIL;
			if (c->poison) HIPCHK(c, hipMemsetAsync(s.d_runs, 0xFF, (words - 1) * 4, s.cs));   // (tests: a run the finish kernel reads must be this launch's)
			HIPCHK(c, hipMemsetAsync(s.d_runs + words - 1, 0, 4, s.cs));
			sa.out_runs = s.d_runs; sa.rle_overflow = (int32_t*)(s.d_runs + words - 1); sa.rle_cap = cap;
			s.runs_cap = cap;
		}
		sa.prune = c->spec.d_prune; sa.prune_stride = c->spec.prune_stride;
		sa.tile_next = s.wsi ? c->d_tile_next2 : c->d_tile_next;
		HIPCHK(c, spec_launch(c, sa, s.cs));
	} else {
		HIPCHK(c, td_launch_decode(&ka, s.cs));
		c->spec.batches_generic++;
	}
	HIPCHK(c, hipEventRecord(s.ev_k1, s.cs));
	if (ka.art_n > 0 && slot_count_hits(c, s, ka.out_type) != TD_OK) return TD_FAIL;
	if (c->census.on && mode == TD_MODE_GET_LABEL && census_count_slot(c, s, ka.out_type, ka.out_labels) != TD_OK) return TD_FAIL;
	// the molecule count last: dedup's second pass, the last launch in there, rewrites the outcomes the counts above read
	if (c->molecules.on && mode == TD_MODE_GET_LABEL && mol_slot_decoded(c, s, ka.out_type, ka.out_barcode, ka.out_finger, ka.out_labels) != TD_OK) return TD_FAIL;
	s.ran = true;
	s.last_ms = -1.0f;
	c->last_slot = (int)(&s - c->slots);
	return TD_OK;
}

// run_rna_dust over a staged slot (TD_MODE_RNA_DUST, td_rnadust.hip): no model, no workspace.  The outputs take the decode
// kernels' place, so that the finish kernel and the downloads are the same.
static int slot_rna_dust(td_ctx* c, TdSlot& s)
{
	if (!s.staged) return fail(c, "td_run: no batch resident (td_batch_upload failed or was not called)");
	HIPCHK(c, hipSetDevice(c->device));
	s.reset_decoded();
	s.mode = TD_MODE_RNA_DUST;
	if (s.n_tiles == 0) { s.ran = true; s.last_ms = 0.0f; return TD_OK; }
	const OutLayout ol = out_layout(s.n_tiles, s.lmax, s.nw1);
	TdRnaDustArgs ra{};
	ra.packed = s.d_packed; ra.lens = s.d_lens; ra.n_tiles = s.n_tiles; ra.nw2 = s.nw2; ra.nw1 = s.nw1;
	ra.raw = s.d_raw; ra.offs = s.d_offs; ra.read_at = s.sorted ? s.d_read_at : nullptr; ra.n_reads = s.n_reads; ra.is_ascii = s.is_ascii;
	ra.dust = c->dust;
	if (c->art_n > 0) {
		s.sb.art_threads = c->art_threads;
		s.sb.art_first = c->win_first; s.sb.art_total = c->win_total;
		HIPCHK(c, td_stage_art_left(s.sb, s.cs));
		ra.art_pk = c->d_art_pk; ra.art_seq = c->d_art_seq; ra.art_left = s.d_art_left;
		ra.art_n = c->art_n; ra.art_fe = c->art_fe;
	}
	point_outputs(ra, s.d_out, ol);
	ra.counters = c->d_counters;
	HIPCHK(c, hipEventRecord(s.ev_k0, s.cs));
	HIPCHK(c, td_launch_rna_dust(ra, s.cs));
	HIPCHK(c, hipEventRecord(s.ev_k1, s.cs));
	if (ra.art_n > 0 && slot_count_hits(c, s, ra.out_type) != TD_OK) return TD_FAIL;
	s.ran = true;
	s.last_ms = -1.0f;
	c->last_slot = (int)(&s - c->slots);
	return TD_OK;
}

// Results into the caller's order on the device (finish kernel on the compute stream), then device -> host.  A page-locked
// destination is written by the DMA engine directly; anything else is reached through pinned staging and copied out by
// slot_fetch_end.  The synchronous calls queue the copies behind the finish kernel on the compute stream.  The pipelined
// calls must not: a copy queued behind an event is carried out by a blit *kernel*, which then competes for CUs with the
// next batch's decode kernel -- a persistent kernel that owns every register file -- and finishes when that does (measured:
// 41 ms instead of 3).  So td_wait waits for the finish kernel on the host and issues the copies then, with nothing
// pending in front of them: they go to the SDMA engines and run beside the decode kernel.
static int slot_issue_copies(td_ctx* c, TdSlot& s, hipStream_t down)
{
	const int64_t n = s.n_reads;
	const size_t res_bytes = (size_t)n * sizeof(td_read_result), seq_bytes = (size_t)s.n_bases, lab_bytes = (size_t)(s.n_bases + n);
	if (s.u_res) HIPCHK(c, hipMemcpyAsync(s.res_direct ? (void*)s.u_res : (void*)s.h_res, s.d_res, res_bytes, hipMemcpyDeviceToHost, down));
	if (s.u_seq && seq_bytes) {
		if (s.use_keep) HIPCHK(c, hipMemcpyAsync(s.h_keepo, s.d_keepo, (size_t)n * (size_t)s.nw1 * 4, hipMemcpyDeviceToHost, down));
		else HIPCHK(c, hipMemcpyAsync(s.seq_direct ? (void*)s.u_seq : (void*)s.h_seq, s.d_seq, seq_bytes, hipMemcpyDeviceToHost, down));
	}
	if (s.u_labels) {
		if (s.use_rle) {
			// (the overflow flag travels behind the runs in the same copy -- the finish kernel folded the decode kernel's own flag
			// into it: a copy of a few bytes is carried out by a blit kernel, which gets no CU while a decode launch holds every
			// register file and made this wait last as long as that launch: tools/ubench/copy_kinds.cpp)
			HIPCHK(c, hipMemcpyAsync(s.h_rle, s.d_rle, ((size_t)n * (size_t)s.rle_cap + 1) * 4, hipMemcpyDeviceToHost, down));
		}
		else HIPCHK(c, hipMemcpyAsync(s.lab_direct ? (void*)s.u_labels : (void*)s.h_lab, s.d_lab, lab_bytes, hipMemcpyDeviceToHost, down));
	}
	HIPCHK(c, hipEventRecord(s.ev_down, down));
	return TD_OK;
}

static int slot_fetch_begin(td_ctx* c, TdSlot& s, td_read_result* res, int8_t* labels, uint8_t* seq_out, bool deferred)
{
	if (!s.ran) return fail(c, "td_batch_download: td_run has not been called on this batch");
	if (s.mode == TD_MODE_RNA_DUST && labels) return fail(c, "td_batch_download: TD_MODE_RNA_DUST has no labels (pass NULL)");
	s.reset_fetch();
	s.u_res = res; s.u_labels = labels; s.u_seq = seq_out;
	s.copies_deferred = deferred;
	const int64_t n = s.n_reads;
	if (n == 0) return TD_OK;
	const size_t res_bytes = (size_t)n * sizeof(td_read_result), seq_bytes = (size_t)s.n_bases, lab_bytes = (size_t)(s.n_bases + n);
	// Compact egress.  The rewritten sequence is the input with some positions turned into the spacer byte: the keep bits (one
	// per base) come back instead and the host rebuilds it from its staging copy of the input -- unless the caller's page-locked
	// buffer was the DMA source, which the caller may have refilled since.  ri->labels is a handful of runs per read (the path
	// moves through the segments in order): (length, label) pairs come back and the host expands them.  A fifth of the bytes
	// over PCIe, and that much less work for the download's blit kernels, which compete with the decode kernel for CUs.
	const bool compact = c->compact_egress != 0;
	s.use_keep = compact && seq_out && seq_bytes && s.raw_host != nullptr;
	s.use_rle = compact && labels;
	s.rle_cap = s.runs_cap > 0 ? s.runs_cap : rle_capacity(c);
	if (res && ensure(c, &s.d_res, &s.cap_res, res_bytes) != TD_OK) return TD_FAIL;
	if (seq_out && !s.use_keep && ensure(c, &s.d_seq, &s.cap_seq, seq_bytes) != TD_OK) return TD_FAIL;
	if (labels && !s.use_rle && ensure(c, &s.d_lab, &s.cap_lab, lab_bytes) != TD_OK) return TD_FAIL;
	if (res && !(s.res_direct = is_pinned(res)) && ensure_pinned(c, &s.h_res, &s.cap_h_res, res_bytes) != TD_OK) return TD_FAIL;
	if (seq_out && !s.use_keep && !(s.seq_direct = is_pinned(seq_out)) && ensure_pinned(c, &s.h_seq, &s.cap_h_seq, seq_bytes) != TD_OK) return TD_FAIL;
	if (labels && !s.use_rle && !(s.lab_direct = is_pinned(labels)) && ensure_pinned(c, &s.h_lab, &s.cap_h_lab, lab_bytes) != TD_OK) return TD_FAIL;
	const size_t keepo_bytes = (size_t)n * (size_t)s.nw1 * 4, rle_bytes = ((size_t)n * (size_t)s.rle_cap + 2) * 4;
	if (s.use_keep && (ensure(c, &s.d_keepo, &s.cap_keepo, keepo_bytes) != TD_OK || ensure_pinned(c, &s.h_keepo, &s.cap_h_keepo, keepo_bytes) != TD_OK)) return TD_FAIL;
	if (s.use_rle) {
		if (ensure(c, &s.d_rle, &s.cap_rle, rle_bytes) != TD_OK || ensure_pinned(c, &s.h_rle, &s.cap_h_rle, rle_bytes) != TD_OK) return TD_FAIL;
		if (c->poison) HIPCHK(c, hipMemsetAsync(s.d_rle, 0xFF, (size_t)n * (size_t)s.rle_cap * 4, s.fin));   // (tests: every entry the host expands must be this batch's)
		HIPCHK(c, hipMemsetAsync(s.d_rle + (size_t)n * (size_t)s.rle_cap, 0, 4, s.fin));   // the overflow flag
	}
	if (s.use_keep && c->poison) HIPCHK(c, hipMemsetAsync(s.d_keepo, 0xFF, keepo_bytes, s.fin));
	s.sb.res = res ? s.d_res : nullptr;
	s.sb.seq_out = (seq_out && !s.use_keep) ? s.d_seq : nullptr;
	s.sb.labels_out = (labels && !s.use_rle) ? s.d_lab : nullptr;
	s.sb.keep_out = s.use_keep ? s.d_keepo : nullptr;
	s.sb.rle_out = s.use_rle ? s.d_rle : nullptr;
	s.sb.rle_cap = s.rle_cap;
	s.sb.runs = (s.use_rle && s.runs_cap > 0) ? s.d_runs : nullptr;
	s.sb.rle_overflow = s.use_rle ? (int32_t*)(s.d_rle + (size_t)n * (size_t)s.rle_cap) : nullptr;
	s.sb.runs_overflow = (s.use_rle && s.runs_cap > 0) ? (const int32_t*)(s.d_runs + (size_t)s.n_tiles * (size_t)s.runs_cap * TD_WAVE) : nullptr;
	if (s.fin != s.cs) HIPCHK(c, hipStreamWaitEvent(s.fin, s.hits_queued ? s.ev_hits : s.ev_k1, 0));
	HIPCHK(c, td_stage_finish(s.sb, s.fin));
	if (deferred) HIPCHK(c, hipEventRecord(s.ev_done, s.fin));
	else if (slot_issue_copies(c, s, s.fin) != TD_OK) return TD_FAIL;
	s.finished = true;
	return TD_OK;
}

double wall_ms()
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

static int slot_fetch_end(td_ctx* c, TdSlot& s)
{
	if (s.n_reads == 0 || !s.finished) return TD_OK;
	const bool dbg = c->debug_wait != 0;
	const double t0 = dbg ? wall_ms() : 0.0;
	double t1 = t0;
	if (s.copies_deferred) {
		HIPCHK(c, hipEventSynchronize(s.ev_done));
		t1 = dbg ? wall_ms() : 0.0;
		if (slot_issue_copies(c, s, c->s_down) != TD_OK) return TD_FAIL;
	}
	HIPCHK(c, hipEventSynchronize(s.ev_down));
	const double t2 = dbg ? wall_ms() : 0.0;
	struct Rep { bool on; double t0, t1, t2; ~Rep() { if (on) fprintf(stderr, "td_wait: device %.2f ms, download %.2f ms, host %.2f ms\n", t1 - t0, t2 - t1, wall_ms() - t2); } } rep_{ dbg, t0, t1, t2 };
	const int64_t n = s.n_reads;
	if (s.use_rle && s.u_labels && s.h_rle[(size_t)n * (size_t)s.rle_cap] != 0) {
		// a read with more label runs than the table holds (a model whose labels are not one per segment): the labels as they are
		const size_t lab_bytes = (size_t)(s.n_bases + n);
		if (ensure(c, &s.d_lab, &s.cap_lab, lab_bytes) != TD_OK) return TD_FAIL;
		if (!(s.lab_direct = is_pinned(s.u_labels)) && ensure_pinned(c, &s.h_lab, &s.cap_h_lab, lab_bytes) != TD_OK) return TD_FAIL;
		TdStageBatch b2 = s.sb;
		b2.res = nullptr; b2.seq_out = nullptr; b2.keep_out = nullptr; b2.rle_out = nullptr; b2.labels_out = s.d_lab;
		HIPCHK(c, td_stage_finish(b2, s.fin));
		HIPCHK(c, hipStreamSynchronize(s.fin));
		HIPCHK(c, hipMemcpy(s.lab_direct ? (void*)s.u_labels : (void*)s.h_lab, s.d_lab, lab_bytes, hipMemcpyDeviceToHost));
		s.use_rle = false;
	}
	if (s.u_res && !s.res_direct) parallel_copy(c, s.u_res, s.h_res, (size_t)n * sizeof(td_read_result));
	if (s.u_seq && s.n_bases) {
		if (s.use_keep) {
			td_host_rebuild_sequences(c->pool, c->host_threads, n, s.raw_host, s.h_offs, s.h_keepo, s.nw1, s.is_ascii, s.u_seq);
		} else if (!s.seq_direct) parallel_copy(c, s.u_seq, s.h_seq, (size_t)s.n_bases);
	}
	if (s.u_labels) {
		if (s.use_rle) {
			td_host_expand_labels(c->pool, c->host_threads, n, s.h_offs, s.h_rle, s.rle_cap, s.u_labels);
		} else if (!s.lab_direct) parallel_copy(c, s.u_labels, s.h_lab, (size_t)(s.n_bases + n));
	}
	return TD_OK;
}

bool tickets_outstanding(const td_ctx* c)
{
	for (int k = 0; k < TD_MAX_PIPELINE; k++) if (c->slots[k].ticket) return true;
	return false;
}

// slot routing of the synchronous calls: everything on the context's first stream and workspace
static TdRoute sync_route(const td_ctx* c) { return TdRoute{ c->stream, c->stream, c->stream, 0, false }; }

static int upload_common(td_ctx* c, const void* bases, int is_ascii, const int64_t* offs, int64_t n)
{
	if (!c) return TD_FAIL;
	if (tickets_outstanding(c)) return fail(c, "td_batch_upload: td_submit tickets are outstanding (td_wait them first)");
	if (spec_handover(c, false) != TD_OK) return TD_FAIL;   // a finished background compile takes over before any geometry is chosen
	TdSlot& s = c->slots[0];
	const TdRoute rt = sync_route(c);
	// mate mode: the mode is td_run's to say, so the named mate batch is taken now when it is this batch's
	const bool take_mate = c->molecules.mate.bases > 0 && c->molecules.mate.named && c->molecules.mate.reads == n;
	if (slot_stage(c, s, rt, bases, is_ascii, offs, n, c->stream, true, take_mate) != TD_OK) return TD_FAIL;
	HIPCHK(c, hipStreamSynchronize(c->stream));   // the caller may reuse its buffers
	c->last_slot = 0;
	return TD_OK;
}

extern "C" int td_batch_upload(td_ctx* c, const uint8_t* codes, const int64_t* offs, int64_t n)
{
	return upload_common(c, codes, 0, offs, n);
}

extern "C" int td_batch_upload_ascii(td_ctx* c, const char* bases, const int64_t* offs, int64_t n)
{
	return upload_common(c, bases, 1, offs, n);
}

extern "C" int td_run(td_ctx* c, int mode)
{
	if (!c) return TD_FAIL;
	if (!c->have_model && mode != TD_MODE_RNA_DUST) return fail(c, "td_run: no model uploaded");
	return slot_decode(c, c->slots[0], mode);
}

extern "C" int td_sync(td_ctx* c)
{
	if (!c) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	return TD_OK;
}

extern "C" int td_batch_download(td_ctx* c, td_read_result* res, int8_t* labels, uint8_t* seq_out)
{
	if (!c) return TD_FAIL;
	TdSlot& s = c->slots[0];
	HIPCHK(c, hipSetDevice(c->device));
	if (slot_fetch_begin(c, s, res, labels, seq_out, false) != TD_OK) return TD_FAIL;
	return slot_fetch_end(c, s);
}

// ---- pipelined batches ----
extern "C" int td_submit(td_ctx* c, const void* bases, int32_t is_ascii, const int64_t* offs, int64_t n_reads, int mode,
                         td_read_result* res, int8_t* labels, uint8_t* seq_out, int64_t* ticket)
{
	if (!c || !ticket) return fail(c, "td_submit: NULL argument");
	*ticket = 0;
	HIPCHK(c, hipSetDevice(c->device));
	if (!c->s_up) {
		int lo = 0, hi = 0;   // (numerically lower = higher priority)
		HIPCHK(c, hipDeviceGetStreamPriorityRange(&lo, &hi));
		HIPCHK(c, hipStreamCreateWithFlags(&c->s_up, hipStreamNonBlocking));
		HIPCHK(c, hipStreamCreateWithPriority(&c->s_down, hipStreamNonBlocking, hi));
		HIPCHK(c, hipStreamCreateWithPriority(&c->s_aux, hipStreamNonBlocking, hi));
		HIPCHK(c, hipStreamCreateWithPriority(&c->s_fin, hipStreamNonBlocking, hi));
	}
	int k = -1;
	for (int j = 0; j < c->pipeline_depth; j++) {   // the slot after the one used last, if free
		const int cand = (c->next_slot + j) % c->pipeline_depth;
		if (!c->slots[cand].ticket) { k = cand; break; }
	}
	if (k < 0) return fail(c, "td_submit: all %d pipeline slots hold batches that have not been waited for", c->pipeline_depth);
	if (mode == TD_MODE_RNA_DUST && labels) return fail(c, "td_submit: TD_MODE_RNA_DUST has no labels (pass NULL)");
	if (spec_handover(c, false) != TD_OK) return TD_FAIL;   // a finished background compile takes over before any geometry is chosen
	const bool take_mate = c->molecules.mate.bases > 0 && mode == TD_MODE_GET_LABEL;   // (no other mode needs or consumes a mate)
	if (take_mate && mol_mate_check(c, n_reads, "td_submit") != TD_OK) return TD_FAIL;
	TdSlot& s = c->slots[k];
	TdRoute rt = sync_route(c);
	rt.pipelined = true;
	if (c->overlap && c->pipeline_depth > 1 && c->spec.ready) {   // every other batch on the second stream / workspace
		if (!c->stream2) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
		if (c->submit_parity) { rt.cs = c->stream2; rt.wsi = 1; }
		c->submit_parity ^= 1;
		rt.aux = c->s_aux; rt.fin = c->s_fin;
	}
	if (slot_stage(c, s, rt, bases, is_ascii != 0, offs, n_reads, c->s_up, mode != TD_MODE_RNA_DUST, take_mate) != TD_OK) return TD_FAIL;
	if (slot_decode(c, s, mode, labels != nullptr) != TD_OK) return TD_FAIL;
	if (slot_fetch_begin(c, s, res, labels, seq_out, true) != TD_OK) return TD_FAIL;
	// "returns once the reads have left the caller's buffers": a page-locked source is read by the DMA engine itself, so wait
	// for that copy (a few ms at PCIe rate, beside the previous batch's kernel; everything of this batch is queued already)
	if ((s.raw_direct || s.mate_direct) && !c->stable_input) HIPCHK(c, hipEventSynchronize(s.ev_up));
	s.ticket = ++c->ticket_counter;
	c->next_slot = (k + 1) % c->pipeline_depth;
	*ticket = s.ticket;
	return TD_OK;
}

extern "C" int td_wait(td_ctx* c, int64_t ticket)
{
	if (!c) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	for (int k = 0; k < TD_MAX_PIPELINE; k++) {
		TdSlot& s = c->slots[k];
		if (ticket != 0 && s.ticket == ticket) {
			const int rc = slot_fetch_end(c, s);
			s.ticket = 0;
			c->last_slot = k;   // td_last_kernel_ms / td_batch_info now describe this batch
			return rc;
		}
	}
	return fail(c, "td_wait: no batch with ticket %lld is in flight", (long long)ticket);
}

// ---- architecture comparison: every candidate model over one batch, backward() only, one launch ----
extern "C" int td_arch_scores(td_ctx* c, const td_model_desc* const* models, int32_t n_models, const uint8_t* codes,
                              const int64_t* offs, int64_t n_reads, float* b_scores)
{
	if (!c || !models || n_models < 1 || !offs || !b_scores || n_reads < 0) return fail(c, "td_arch_scores: bad arguments");
	if (tickets_outstanding(c)) return fail(c, "td_arch_scores: td_submit tickets are outstanding (td_wait them first)");
	HIPCHK(c, hipSetDevice(c->device));
	TdSlot& s = c->slots[0];
	// the reads are staged (sorted by length, packed) once; no model of the context is involved
	const TdRoute rt = sync_route(c);
	if (slot_stage(c, s, rt, codes, 0, offs, n_reads, c->stream, false) != TD_OK) return TD_FAIL;
	s.staged = false;                      // not a batch td_run could use: it has no workspace geometry
	if (s.n_tiles == 0) return TD_OK;
	const int wpb = td_kernel_block_threads() / TD_WAVE;
	const int64_t n_lanes = (int64_t)s.n_tiles * TD_WAVE;
	const int64_t wave_budget = (int64_t)c->n_cu * 2 * wpb;
	std::vector<DevModel> dm((size_t)n_models);
	int rc = TD_OK;
	float* d_b = nullptr;
	TdKernelArgs* d_args = nullptr;
	std::vector<float> h_b;
	std::vector<int32_t> h_read_at;
	auto cleanup = [&]() {
		for (auto& d : dm) free_dev_model(d);
		if (d_b) (void)hipFree(d_b);
		if (d_args) (void)hipFree(d_args);
	};
	if (hipMalloc((void**)&d_b, sizeof(float) * (size_t)(n_lanes * n_models)) != hipSuccess ||
	    hipMalloc((void**)&d_args, sizeof(TdKernelArgs) * (size_t)n_models) != hipSuccess) { cleanup(); return fail(c, "td_arch_scores: out of device memory"); }
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { cleanup(); return fail(c, "td_arch_scores: hipMemGetInfo failed"); }
	const int64_t ws_budget = (int64_t)((double)(free_b + c->cap_ws) * 0.85);
	// candidates go in chunks whose workspaces fit side by side; within a chunk the chip's wave slots are shared out evenly
	std::vector<TdKernelArgs> args((size_t)n_models);
	int k0 = 0;
	while (k0 < n_models && rc == TD_OK) {
		int k1 = k0;
		int64_t ws_total = 0;
		std::vector<int64_t> ws_off;
		int max_slots = 0;
		// first guess: all remaining candidates in one launch
		int chunk = n_models - k0;
		for (;;) {
			int64_t per = wave_budget / chunk / wpb * wpb;
			if (per < wpb) per = wpb;
			int64_t cap = ((int64_t)s.n_tiles + wpb - 1) / wpb * wpb;
			if (per > cap) per = cap;
			ws_total = 0; ws_off.clear(); max_slots = (int)per;
			bool fits = true;
			for (int k = k0; k < k0 + chunk; k++) {
				if (!dm[(size_t)k].d_hdr && build_dev_model(c, models[k], dm[(size_t)k]) != TD_OK) { cleanup(); return TD_FAIL; }
				TdWsLayout lay;
				make_layout(lay, dm[(size_t)k].h.S, dm[(size_t)k].h.H, dm[(size_t)k].h.C, s.lmax, dm[(size_t)k].h.max_ncol);
				ws_off.push_back(ws_total);
				ws_total += align256(per * lay.slot_bytes);
				if (ws_total > ws_budget) { fits = false; break; }
			}
			if (fits) { k1 = k0 + chunk; break; }
			if (chunk == 1) { cleanup(); return fail(c, "td_arch_scores: the workspace of candidate %d does not fit in HBM", k0); }
			chunk = (chunk + 1) / 2;
		}
		HIPCHK(c, sync_compute(c));
		if (ensure(c, &c->d_ws, &c->cap_ws, (size_t)ws_total) != TD_OK) { cleanup(); return TD_FAIL; }
		for (int k = k0; k < k1; k++) {
			const DevModel& d = dm[(size_t)k];
			TdKernelArgs ka{};
			ka.hdr = d.d_hdr; ka.cols = d.d_cols; ka.hinfo = d.d_hinfo; ka.pred_off = d.d_pred_off; ka.pred_idx = d.d_pred_idx;
			ka.logsum = c->d_logsum; ka.packed = s.d_packed; ka.lens = s.d_lens;
			ka.n_tiles = s.n_tiles; ka.n_slots = max_slots; ka.lmax = s.lmax; ka.nw2 = s.nw2; ka.nw1 = s.nw1;
			ka.mode = TD_MODE_ARCH_COMP; ka.threshold = 0.0f; ka.minlen = c->minlen; ka.dust = 0; ka.want_labels = 0;
			ka.out_b = d_b + (int64_t)k * n_lanes;       // backward-only mode writes nothing else
			ka.counters = c->d_counters;
			ka.ws = c->d_ws + ws_off[(size_t)(k - k0)];
			make_layout(ka.lay, d.h.S, d.h.H, d.h.C, s.lmax, d.h.max_ncol);
			args[(size_t)k] = ka;
		}
		if (hipMemcpyAsync(d_args + k0, args.data() + k0, sizeof(TdKernelArgs) * (size_t)(k1 - k0), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
		    td_launch_decode_multi(d_args + k0, k1 - k0, max_slots, c->stream) != hipSuccess ||
		    hipStreamSynchronize(c->stream) != hipSuccess) {   // args.data() must outlive the copy
			rc = fail(c, "td_arch_scores: launch failed: %s", hipGetErrorString(hipGetLastError()));
		}
		k0 = k1;
	}
	if (rc == TD_OK) {
		h_b.resize((size_t)(n_lanes * n_models));
		if (hipMemcpy(h_b.data(), d_b, sizeof(float) * h_b.size(), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(c, "td_arch_scores: download failed");
		if (rc == TD_OK && s.sorted) {
			h_read_at.resize((size_t)n_reads);
			if (hipMemcpy(h_read_at.data(), s.d_read_at, sizeof(int32_t) * (size_t)n_reads, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(c, "td_arch_scores: download failed");
		}
	}
	if (rc == TD_OK) {
		for (int k = 0; k < n_models; k++) {
			const float* src = h_b.data() + (int64_t)k * n_lanes;
			float* dst = b_scores + (int64_t)k * n_reads;
			if (s.sorted) for (int64_t p = 0; p < n_reads; p++) dst[h_read_at[(size_t)p]] = src[p];
			else memcpy(dst, src, sizeof(float) * (size_t)n_reads);
		}
	}
	cleanup();
	return rc;
}

extern "C" void* td_host_alloc(size_t bytes)
{
	void* p = nullptr;
	if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
	return p;
}

extern "C" void td_host_free(void* p)
{
	if (p) (void)hipHostFree(p);
}

extern "C" int td_last_kernel_ms(td_ctx* c, float* ms)
{
	if (!c || !ms) return TD_FAIL;
	TdSlot& s = c->slots[c->last_slot];
	if (!s.ran) return fail(c, "td_last_kernel_ms: nothing has run");
	HIPCHK(c, hipSetDevice(c->device));
	if (s.last_ms < 0.0f && s.n_tiles > 0) {
		HIPCHK(c, hipEventSynchronize(s.ev_k1));
		HIPCHK(c, hipEventElapsedTime(&s.last_ms, s.ev_k0, s.ev_k1));
	}
	*ms = s.last_ms;
	return TD_OK;
}

extern "C" int td_timeline_origin(td_ctx* c)
{
	if (!c) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	if (!c->ev_origin) HIPCHK(c, hipEventCreate(&c->ev_origin));
	HIPCHK(c, hipEventRecord(c->ev_origin, c->stream));
	HIPCHK(c, hipEventSynchronize(c->ev_origin));
	return TD_OK;
}

extern "C" int td_last_kernel_times(td_ctx* c, float* start_ms, float* stop_ms, int32_t* stream_index)
{
	if (!c || !start_ms || !stop_ms) return TD_FAIL;
	TdSlot& s = c->slots[c->last_slot];
	if (!s.ran) return fail(c, "td_last_kernel_times: nothing has run");
	if (!c->ev_origin) return fail(c, "td_last_kernel_times: td_timeline_origin has not been called");
	HIPCHK(c, hipSetDevice(c->device));
	*start_ms = *stop_ms = 0.0f;
	if (stream_index) *stream_index = s.wsi;
	if (s.n_tiles == 0) return TD_OK;
	HIPCHK(c, hipEventSynchronize(s.ev_k1));
	HIPCHK(c, hipEventElapsedTime(start_ms, c->ev_origin, s.ev_k0));
	HIPCHK(c, hipEventElapsedTime(stop_ms, c->ev_origin, s.ev_k1));
	return TD_OK;
}

extern "C" int td_batch_info(td_ctx* c, int64_t* n_reads, int64_t* workspace_bytes, int32_t* wave_slots)
{
	if (!c) return TD_FAIL;
	const TdSlot& s = c->slots[c->last_slot];
	if (n_reads) *n_reads = s.n_reads;
	if (workspace_bytes) *workspace_bytes = s.ws_bytes ? s.ws_bytes : (int64_t)s.n_wave_slots * s.ws_slot_bytes;
	if (wave_slots) *wave_slots = s.n_wave_slots;
	return TD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// counters
// ---------------------------------------------------------------------------------------------------------
extern "C" int td_counts_reset(td_ctx* c)
{
	if (!c) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));   // (kernels of pipelined batches may still be counting)
	HIPCHK(c, hipMemsetAsync(c->d_counters, 0, sizeof(unsigned long long) * TD_COUNTER_WORDS, c->stream));
	if (c->d_art_hits) HIPCHK(c, hipMemsetAsync(c->d_art_hits, 0, sizeof(unsigned long long) * (size_t)c->art_n, c->stream));
	if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream));
	return TD_OK;
}

extern "C" int td_counts_get(td_ctx* c, int64_t* counts)
{
	if (!c || !counts) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	HIPCHK(c, hipMemcpy(counts, c->d_counters, sizeof(int64_t) * TD_NUM_COUNTERS, hipMemcpyDeviceToHost));
	return TD_OK;
}

extern "C" int td_diag_get(td_ctx* c, int64_t* diag)
{
	if (!c || !diag) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	HIPCHK(c, hipMemcpy(diag, c->d_counters + TD_NUM_COUNTERS, sizeof(int64_t) * TD_NUM_DIAG_COUNTERS, hipMemcpyDeviceToHost));
	return TD_OK;
}

extern "C" int td_artifact_hits_get(td_ctx* c, int64_t* hits, int32_t cap)
{
	if (!c || !hits || cap < 0) return TD_FAIL;
	if (cap < c->art_n) return fail(c, "td_artifact_hits_get: room for %d sequences, the filter has %d", cap, c->art_n);
	memset(hits, 0, sizeof(int64_t) * (size_t)cap);
	if (c->art_n == 0) return TD_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	HIPCHK(c, hipMemcpy(hits, c->d_art_hits, sizeof(int64_t) * (size_t)c->art_n, hipMemcpyDeviceToHost));
	return TD_OK;
}

extern "C" void* td_counts_device_ptr(td_ctx* c) { return c ? (void*)c->d_counters : nullptr; }

// ---------------------------------------------------------------------------------------------------------
// sequence statistics with the counting on the device (td_stats.hip); the finish is td_sequence_stats' own
// ---------------------------------------------------------------------------------------------------------
extern "C" int td_sequence_stats_device(td_ctx* c, const td_arch* arch, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                                        int64_t scan_limit, int32_t matchstart, int32_t matchend, td_seq_stats* out)
{
	if (!c) return TD_FAIL;
	if (!arch || !codes || !offs || !out) return fail(c, "td_sequence_stats_device: null argument");
	if (n_reads <= 0 || scan_limit <= 0) return fail(c, "td_sequence_stats_device: no reads to take the statistics over (the reference divides by zero)");
	std::vector<uint8_t> five, three;
	td_stats_linkers(arch, five, three);
	TdSeqCounts k;
	char err[512] = "";
	if (td_stats_count_device(c->device, five, three, codes, offs, n_reads, scan_limit, &k, err, sizeof err) != TD_OK) return fail(c, "%s", err);
	td_stats_finish(arch, k, out);
	td_stats_apply_window(out, matchstart, matchend);
	return TD_OK;
}
