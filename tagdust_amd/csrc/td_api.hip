// td_api.hip -- C-ABI host layer of libtagdust_hip.so (declared in include/tagdust_hip.h): the housekeeping of a context -- its
// life, the model, options, the artifact filter, window and parameters, counters, statistics, page-locked host memory.  What runs
// once per batch (upload, decode, download, td_submit / td_wait, td_arch_scores) is td_batch.hip.
//
// Replaces the reference's run_pHMM() fan-out (src/barcode_hmm.c:1895-2029): instead of T pthreads with
// private model copies, one context per GPU holds the flattened model in HBM and launches the decode
// kernel (td_kernels.hip) over a resident batch.  No torch, no CPU fallback: every entry point fails
// with TD_FAIL (and a message in td_last_error) when HIP does.  What is decided without the device stands in plain C++ units
// and is only applied here: a description checked and flattened, the -ref text packed, the logsum table (td_model_flat.cpp).
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <mutex>
#include <thread>

#include "../../include/tagdust_model.h"
#include "td_ctx.h"
#include "td_model_flat.h"
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

void free_dev_model(DevModel& d)
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
	samples_release(c);
	samples_export_release(c);
	qual_release(c);
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
int build_dev_model(td_ctx* c, const td_model_desc* m, DevModel& out)
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
	samples_release(c);  // ... and a sheet lists one model's barcodes
	samples_export_release(c);   // ... as do the words a context exports
	qual_release(c);     // ... and the base-quality filter judges one model's segments
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
	if (!strcmp(name, "samples")) { *value = c->samples.on ? c->samples.plan.n_samples : 0; return TD_OK; }   // td_samples_enable's n_samples, 0 = off
	if (!strcmp(name, "samples_kernel_us")) return samples_last_kernel_us(c, value);   // the kernel's time of the last batch
	// the join across input files: the context is an exporter (1) / the primary (its sheet's n_samples), and the kernels' times
	if (!strcmp(name, "samples_export")) { *value = c->samples_export.on; return TD_OK; }
	if (!strcmp(name, "samples_join")) { *value = c->samples.on && c->samples.join ? c->samples.plan.n_samples : 0; return TD_OK; }
	// ... and whether the last batch's device order differs from the caller's (reads of several lengths): both sides of the join
	// then carry their words between the two orders
	if (!strcmp(name, "batch_sorted")) { *value = c->slots[c->last_slot].sorted ? 1 : 0; return TD_OK; }
	if (!strcmp(name, "samples_export_kernel_us")) return samples_export_last_kernel_us(c, value);
	if (!strcmp(name, "samples_join_kernel_us")) {
		if (!c->samples.on || !c->samples.join) return fail(c, "td_get_option: samples_join_kernel_us: the join is off");
		return samples_last_kernel_us(c, value);
	}
	if (!strcmp(name, "quality_filter")) { *value = c->quality.on; return TD_OK; }   // td_qual_enable: 1 = on
	if (!strcmp(name, "quality_kernel_us")) return qual_last_kernel_us(c, value);    // the judge kernel's time of the last batch
	if (!strcmp(name, "molecules_active")) { *value = c->molecules.on; return TD_OK; }
	if (!strcmp(name, "dedup_active")) { *value = c->molecules.dedup.on; return TD_OK; }
	if (!strcmp(name, "dedup_frozen")) { *value = c->molecules.frozen.on; return TD_OK; }   // td_mol_dedup_freeze: batches are replayed
	if (!strcmp(name, "mate_bases")) { *value = c->molecules.mate.bases; return TD_OK; }   // td_mol_mate_enable's M, 0 = off
	if (!strcmp(name, "mate_filter")) { *value = c->molecules.mate.filter ? 1 : 0; return TD_OK; }   // td_mol_mate_filter_enable
	if (!strcmp(name, "collapse_active")) { *value = c->molecules.collapse.on; return TD_OK; }
	// molecules_, dedup_, collapse_origin_, dedup_replay_, mate_, mate_filter_ and mate_join_kernel_us: the stage's time of the last
	// batch (-1: none of them)
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
	if (c->samples.on) return fail(c, "td_set_window: sample assignment is on (td_samples_disable first): labels behind a window do not mark the barcodes");
	if (c->samples_export.on) return fail(c, "td_set_window: the context exports its barcode calls (td_samples_export_disable first): labels behind a window do not mark the barcodes");
	if (c->quality.on) return fail(c, "td_set_window: the base-quality filter is on (td_qual_disable first): labels behind a window do not mark the bases");
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

extern "C" int td_sync(td_ctx* c)
{
	if (!c) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	return TD_OK;
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

extern "C" int td_timeline_origin(td_ctx* c)
{
	if (!c) return TD_FAIL;
	HIPCHK(c, hipSetDevice(c->device));
	if (!c->ev_origin) HIPCHK(c, hipEventCreate(&c->ev_origin));
	HIPCHK(c, hipEventRecord(c->ev_origin, c->stream));
	HIPCHK(c, hipEventSynchronize(c->ev_origin));
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
