// td_spec_host.hip -- the host life of the model-specialised kernel inside a context (c->spec, td_ctx.h): plan and compile at the
// model upload, now or on a host thread; module load, logsum self-check and whole-kernel probe before a compiled kernel takes over;
// the reloads a batch can ask for; the bound tables; the launch.  td_api.hip and td_batch.hip call in through the spec_* functions of td_ctx.h.
#include <stdlib.h>
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>

#include "td_ctx.h"

// One background compile.  The worker calls td_spec_compile on the job's own copies and nothing else: it touches no context and no
// device.  Contexts that want the same code object share the job (g_jobs, by cache key); whoever lets go of it last joins the
// thread, and every context waits for its jobs before it goes (td_ctx_destroy), so no thread is ever detached.
struct SpecJob {
	uint64_t key = 0;
	ModelCopy model;
	TdSpecPlan plan;
	int lsum_oob = 0, window = 0;
	std::mutex mu;
	std::condition_variable cv;
	bool done = false;
	int rc = TD_FAIL;
	std::vector<char> code;
	std::string log;
	std::thread th;
	void run()
	{
		std::vector<char> out;
		std::string lg;
		const int r = td_spec_compile(&model.d, plan, lsum_oob, window, out, lg);
		std::lock_guard<std::mutex> lk(mu);
		code.swap(out); log.swap(lg); rc = r; done = true;
		cv.notify_all();
	}
	bool finished() { std::lock_guard<std::mutex> lk(mu); return done; }
	void wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return done; }); }
	~SpecJob() { if (th.joinable()) th.join(); }
};
static std::mutex g_jobs_mu;
static std::map<uint64_t, std::weak_ptr<SpecJob>> g_jobs;   // by cache key: one compile per code object in flight per process

// A process that ends with a context it never destroyed must not run the library's static destructors under a compile that is
// still going: registered (once, with the first job -- so it runs before the destructors of the statics above and of the code
// cache in td_jit.hip, which were constructed when the library was loaded), this waits for every job in flight.  (Which unit holds
// them makes no difference: every static of the library is constructed before an entry point can start the first job.)
static void wait_for_all_spec_jobs()
{
	std::vector<std::shared_ptr<SpecJob>> live;
	{
		std::lock_guard<std::mutex> lk(g_jobs_mu);
		for (auto& kv : g_jobs) if (auto j = kv.second.lock()) live.push_back(j);
	}
	for (auto& j : live) j->wait();
}

// what the probe said about a code object on a device, for the life of the process
struct ProbeVerdict { int mismatches = 0, read = -1, field = -1; };
static std::mutex g_probe_mu;
static std::map<std::pair<uint64_t, int>, ProbeVerdict> g_probe_verdicts;

int spec_unload(td_ctx* c)
{
	if (c->spec.mod) { HIPCHK(c, hipModuleUnload(c->spec.mod)); c->spec.mod = nullptr; }
	c->spec.fn = nullptr; c->spec.ready = false;
	return TD_OK;
}

// the loaded kernel over sa.n_slots wave slots
hipError_t spec_launch(td_ctx* c, const TdSpecArgs& sa, hipStream_t stream)
{
	size_t sz = sizeof sa;
	void* cfg[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, (void*)&sa, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END };
	const int block = c->spec.block, wpb = block / TD_WAVE;
	return hipModuleLaunchKernel(c->spec.fn, (unsigned)((sa.n_slots + wpb - 1) / wpb), 1, 1, (unsigned)block, 1, 1, 0, stream, nullptr, cfg);
}

// bound tables of the position pruning, for reads up to lcap >= lmax bases (kernels in flight read the old ones)
static int ensure_prune_tables(td_ctx* c, int lmax)
{
	if (lmax <= c->spec.prune_lcap && c->spec.d_prune) return TD_OK;
	HIPCHK(c, sync_compute(c));
	const int lcap = (lmax + 2 + 255) / 256 * 256, stride = lcap + 24;   // (the scans request TDS_SCAN_B = 16 entries at a time: spare entries behind lcap)
	std::vector<float> tab;
	// (the bound recurrences cost columns x positions on the host: for reads beyond 8192 bases the tables stay zero, which
	// the kernel reads as "nothing can be pruned" -- every position violates the zero bound -- and decodes densely)
	c->spec.prune_live = (c->spec.plan.prune_segs > 0 || c->spec.plan.sfx_first < c->spec.plan.S) && lcap <= 8192;
	if (c->spec.prune_live) td_spec_prune_tables(&c->model.d, c->spec.plan, lcap, stride, tab);
	else tab.assign((size_t)TD_PRUNE_TABLES * stride, 0.0f);
	if (c->spec.d_prune) { HIPCHK(c, hipFree(c->spec.d_prune)); c->spec.d_prune = nullptr; }
	HIPCHK(c, hipMalloc((void**)&c->spec.d_prune, tab.size() * sizeof(float)));
	HIPCHK(c, hipMemcpy(c->spec.d_prune, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
	c->spec.prune_lcap = lcap; c->spec.prune_stride = stride;
	return TD_OK;
}

static const char* probe_field_name(int f)
{
	static const char* res[] = { "f_score", "b_score", "r_score", "bar_prob", "mapq", "read_type", "barcode", "fingerprint" };
	if (f >= 0 && f < 8) return res[f];
	return f == TD_PROBE_FIELD_LABELS ? "labels" : f == TD_PROBE_FIELD_SEQ ? "sequence" : f == TD_PROBE_FIELD_COUNTERS ? "counters" : "?";
}

// The whole-kernel probe (tagdust_hip.h, td_spec_probe): the loaded specialised kernel (c->spec.fn) and the generic kernel decode
// the probe reads under the fixed probe parameters, on scratch buffers of their own; a device kernel compares what a caller could
// see.  Nothing of the context's batches, slots or counters is touched.  The compute streams are idle when this runs.
static int probe_spec_kernel(td_ctx* c, int window, ProbeVerdict& v)
{
	std::vector<int64_t> offs(TD_PROBE_READS + 1);
	const int64_t n_bases = td_spec_probe(&c->model.d, nullptr, 0, offs.data());
	if (n_bases <= 0) return fail(c, "td_model_upload: the probe reads could not be made from this model");
	std::vector<uint8_t> codes((size_t)n_bases);
	(void)td_spec_probe(&c->model.d, codes.data(), n_bases, nullptr);
	const int n = TD_PROBE_READS, n_tiles = TD_PROBE_READS / TD_WAVE;
	int lmax = 1;
	for (int i = 0; i < n; i++) if (offs[(size_t)i + 1] - offs[(size_t)i] > lmax) lmax = (int)(offs[(size_t)i + 1] - offs[(size_t)i]);
	const int nw2 = (lmax + 15) / 16, nw1 = (lmax + 31) / 32;
	if (ensure_prune_tables(c, lmax) != TD_OK) return TD_FAIL;
	const TdModelHeader& h = c->dev.h;
	TdWsLayout glay{};
	make_layout(glay, h.S, h.H, h.C, lmax, h.max_ncol);
	TdSpecLayout slay{};
	td_spec_layout(slay, c->spec.plan, lmax);
	const int gwpb = td_kernel_block_threads() / TD_WAVE, swpb = c->spec.block / TD_WAVE;
	const int gslots = (n_tiles + gwpb - 1) / gwpb * gwpb, sslots = (n_tiles + swpb - 1) / swpb * swpb;
	const OutLayout ol = out_layout(n_tiles, lmax, nw1);
	// one scratch allocation, carved up
	int64_t o = 0;
	auto carve = [&](int64_t bytes) { const int64_t at = o; o = align256(o + bytes); return at; };
	const int64_t o_raw = carve(n_bases), o_offs = carve((int64_t)(n + 1) * 8), o_packed = carve((int64_t)n_tiles * (nw2 + nw1) * TD_WAVE * 4),
	              o_lens = carve((int64_t)n * 4), o_outa = carve(ol.total), o_outb = carve(ol.total),
	              o_cnt = carve((int64_t)2 * TD_COUNTER_WORDS * 8), o_cmp = carve(256), o_tile = carve(256);
	const int64_t small_bytes = o;
	const int64_t o_wsa = carve((int64_t)gslots * glay.slot_bytes), o_wsb = carve((int64_t)sslots * slay.slot_bytes);
	uint8_t* d = nullptr;
	HIPCHK(c, hipMalloc((void**)&d, (size_t)o));
	struct Free { uint8_t* p; ~Free() { (void)hipFree(p); } } free_{ d };
	hipStream_t st = c->stream;
	HIPCHK(c, hipMemsetAsync(d, 0, (size_t)small_bytes, st));
	HIPCHK(c, hipMemsetAsync(d + o_cmp, 0xFF, 256, st));   // "this tile agrees" = -1
	HIPCHK(c, hipMemsetAsync(d + o_cmp, 0, 4, st));
	HIPCHK(c, hipMemsetAsync(d + o_wsa, 0xFF, (size_t)(o - o_wsa), st));   // both workspaces poisoned: a read-before-write computes on NaNs
	HIPCHK(c, hipMemcpyAsync(d + o_raw, codes.data(), (size_t)n_bases, hipMemcpyHostToDevice, st));
	HIPCHK(c, hipMemcpyAsync(d + o_offs, offs.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
	TdStageBatch sb{};
	sb.raw = d + o_raw; sb.offs = (const int64_t*)(d + o_offs); sb.n_reads = n; sb.is_ascii = 0;
	sb.n_tiles = n_tiles; sb.lmax = lmax; sb.nw2 = nw2; sb.nw1 = nw1;
	sb.read_at = nullptr;   // the reads stay in the generator's order: ragged inside every tile
	sb.packed = (uint32_t*)(d + o_packed); sb.lens = (int32_t*)(d + o_lens);
	HIPCHK(c, td_stage_pack(sb, st));
	unsigned long long* cnt_a = (unsigned long long*)(d + o_cnt);
	unsigned long long* cnt_b = cnt_a + TD_COUNTER_WORDS;
	TdKernelArgs ka{};
	ka.hdr = c->dev.d_hdr; ka.cols = c->dev.d_cols; ka.hinfo = c->dev.d_hinfo; ka.pred_off = c->dev.d_pred_off; ka.pred_idx = c->dev.d_pred_idx; ka.logsum = c->d_logsum;
	ka.packed = sb.packed; ka.lens = sb.lens;
	ka.n_tiles = n_tiles; ka.n_slots = gslots; ka.lmax = lmax; ka.nw2 = nw2; ka.nw1 = nw1;
	ka.mode = TD_MODE_GET_LABEL; ka.threshold = TD_PROBE_THRESHOLD; ka.minlen = TD_PROBE_MINLEN; ka.dust = TD_PROBE_DUST; ka.want_labels = 1;
	if (window) { ka.win_start = TD_PROBE_WIN_START; ka.win_len = TD_PROBE_WIN_END - TD_PROBE_WIN_START; }
	point_outputs(ka, d + o_outa, ol);
	ka.counters = cnt_a;
	ka.ws = d + o_wsa; ka.lay = glay;
	HIPCHK(c, td_launch_decode(&ka, st));
	TdSpecArgs sa = spec_args_from(ka);
	sa.n_slots = sslots;
	point_outputs(sa, d + o_outb, ol);
	sa.counters = cnt_b;
	sa.ws = d + o_wsb; sa.lay = slay; sa.lay_big = slay;
	sa.n_big = 0; sa.lmax_big = lmax; sa.out_lmax = lmax;
	sa.prune = c->spec.d_prune; sa.prune_stride = c->spec.prune_stride;
	sa.tile_next = (int32_t*)(d + o_tile);
	HIPCHK(c, spec_launch(c, sa, st));
	TdProbeCmp pc{};
	pc.lens = sb.lens; pc.n_tiles = n_tiles; pc.lmax = lmax; pc.nw1 = nw1; pc.n_counters = TD_NUM_COUNTERS;
	pc.soa_a = d + o_outa; pc.soa_b = d + o_outb; pc.soa_stride = ol.soa_stride;
	pc.keep_a = ka.out_keep; pc.keep_b = sa.out_keep; pc.labels_a = ka.out_labels; pc.labels_b = sa.out_labels;
	pc.counters_a = cnt_a; pc.counters_b = cnt_b;
	pc.out = (int32_t*)(d + o_cmp);
	HIPCHK(c, td_probe_compare(pc, st));
	int32_t out[1 + 2 * (TD_PROBE_READS / TD_WAVE + 1)];
	HIPCHK(c, hipMemcpyAsync(out, d + o_cmp, sizeof out, hipMemcpyDeviceToHost, st));
	HIPCHK(c, hipStreamSynchronize(st));
	// the bound tables were laid out for the probe's reads: the first batch lays them out for its own (as without a probe)
	c->spec.prune_lcap = 0; c->spec.prune_live = false;
	v = ProbeVerdict();
	v.mismatches = out[0];
	for (int w = 0; w <= n_tiles && v.read < 0; w++) if (out[1 + 2 * w] >= 0) { v.read = out[1 + 2 * w]; v.field = out[2 + 2 * w]; }
	return TD_OK;
}

static int load_spec_kernel(td_ctx* c, int lsum_oob, int window = -1);
static int start_spec_job(td_ctx* c, int lsum_oob, int window);

// A compiled code object becomes the context's decode kernel: module load, logsum self-check, probe, spec.ready -- in that order.
// The compute streams are idle.  background: a self-check that demands the clamped form sends that compile to the background
// again (a hand-over) instead of compiling it here.  A kernel the probe rejects leaves the context on the generic kernel: TD_OK.
static int install_spec_kernel(td_ctx* c, const std::vector<char>& code, uint64_t key, int lsum_oob, int window, bool background)
{
	TdSpecState& sp = c->spec;
	if (spec_unload(c) != TD_OK) return TD_FAIL;
	HIPCHK(c, hipModuleLoadData(&sp.mod, code.data()));
	HIPCHK(c, hipModuleGetFunction(&sp.fn, sp.mod, "td_spec_kernel"));
	// lsum() as compiled against the reference's formula on the operand pairs that matter (either or both operands -inf,
	// gaps just below / at / above the 15.7 cut, huge gaps, equal operands).  The clamp-free form depends on hardware and
	// toolchain behaviour nobody documents; if it ever stops holding, the clamped form is loaded instead -- loudly.
	{
		static const float g[] = { 0.0f, 0.0005f, 0.001f, 1.0f, 15.699f, 15.6999f, 15.7f, 15.7001f, 16.639f, 16.64f, 16.7f, 100.0f, 1.0e5f, 1.0e6f };
		std::vector<float> pairs;
		for (float base : { 0.0f, -3.25f, -700.0f }) {
			for (float d : g) { pairs.push_back(base); pairs.push_back(base - d); pairs.push_back(base - d); pairs.push_back(base); }
			pairs.push_back(base); pairs.push_back(-INFINITY); pairs.push_back(-INFINITY); pairs.push_back(base);
		}
		pairs.push_back(-INFINITY); pairs.push_back(-INFINITY);
		const int n_pairs = (int)(pairs.size() / 2);
		hipFunction_t chk = nullptr;
		HIPCHK(c, hipModuleGetFunction(&chk, sp.mod, "td_spec_selfcheck"));
		float* d_pairs = nullptr; int* d_bad = nullptr; int bad = -1;
		HIPCHK(c, hipMalloc((void**)&d_pairs, pairs.size() * 4));
		HIPCHK(c, hipMalloc((void**)&d_bad, 4));
		HIPCHK(c, hipMemcpy(d_pairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
		HIPCHK(c, hipMemset(d_bad, 0, 4));
		struct { const float* logsum; const float* pairs; int n; int pad; int* bad; } a = { c->d_logsum, d_pairs, n_pairs, 0, d_bad };
		size_t sz = sizeof a;
		void* cfg[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END };
		const int block = sp.block;
		hipError_t e = n_pairs <= block ? hipModuleLaunchKernel(chk, 1, 1, 1, (unsigned)block, 1, 1, 0, c->stream, nullptr, cfg) : hipErrorInvalidValue;
		if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
		if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost);
		(void)hipFree(d_pairs); (void)hipFree(d_bad);
		if (e != hipSuccess) return fail(c, "td_model_upload: logsum self-check did not run: %s", hipGetErrorString(e));
		if (sp.selfcheck_fail && lsum_oob) bad = 1;   // tests: exercise the fallback
		if (bad != 0) {
			if (!lsum_oob) return fail(c, "td_model_upload: the compiled logsum differs from the reference formula on %d of %d operand pairs", bad, n_pairs);
			fprintf(stderr, "tagdust_hip: clamp-free logsum failed its self-check on this device / toolchain (%d of %d pairs); using the clamped form\n", bad, n_pairs);
			sp.oob_unsafe = true;
			if (background) {
				if (spec_unload(c) != TD_OK) return TD_FAIL;
				return start_spec_job(c, 0, window);
			}
			return load_spec_kernel(c, 0, window);
		}
	}
	// the whole kernel against the generic one, once per (code object, device) and process
	if (sp.probe) {
		ProbeVerdict v;
		bool known = false;
		{
			std::lock_guard<std::mutex> lk(g_probe_mu);
			auto it = g_probe_verdicts.find({ key, c->device });
			if (it != g_probe_verdicts.end()) { v = it->second; known = true; }
		}
		if (!known) {
			const double t0 = wall_ms();
			if (probe_spec_kernel(c, window, v) != TD_OK) return TD_FAIL;
			sp.probe_us = (int)((wall_ms() - t0) * 1000.0);
			std::lock_guard<std::mutex> lk(g_probe_mu);
			g_probe_verdicts[{ key, c->device }] = v;
		}
		if (v.mismatches != 0) {
			fprintf(stderr, "tagdust_hip: PROBE REJECTED the specialised kernel %016llx on device %d: %d of %d probe reads differ from the generic "
			        "kernel, first at read %d, field %s%s.  This context decodes with the generic kernel: correct, about ten times slower.\n",
			        (unsigned long long)key, c->device, v.mismatches, TD_PROBE_READS, v.read, probe_field_name(v.field), known ? " (verdict of an earlier load)" : "");
			if (spec_unload(c) != TD_OK) return TD_FAIL;
			sp.state = 4;
			return TD_OK;
		}
	}
	sp.ready = true; sp.window = window != 0; sp.oob = lsum_oob != 0;
	sp.state = 3;
	return TD_OK;
}

// Compile (or fetch from the cache) and load the model-specialised kernel, here and now.  lsum_oob selects the clamp-free logsum.
static int load_spec_kernel(td_ctx* c, int lsum_oob, int window)
{
	if (window < 0) window = c->match_len > 0;   // a context with a -start/-end window gets the kernel that can apply it
	if (spec_unload(c) != TD_OK) return TD_FAIL;
	std::vector<char> code;
	std::string log;
	uint64_t key = 0;
	if (td_spec_compile(&c->model.d, c->spec.plan, lsum_oob, window, code, log, &key) != TD_OK) {
		c->spec.state = 5;
		return fail(c, "td_model_upload: specialised kernel did not compile: %.400s", log.c_str());
	}
	return install_spec_kernel(c, code, key, lsum_oob, window, false);
}

// The same compile on a host thread (option "async_compile"): the context goes on with the generic kernel until
// spec_handover finds the job done.  Contexts that ask for the same code object share one job.
static int start_spec_job(td_ctx* c, int lsum_oob, int window)
{
	std::vector<char> none;
	std::string log;
	uint64_t key = 0;
	(void)td_spec_compile(&c->model.d, c->spec.plan, lsum_oob, window, none, log, &key, true);
	static std::once_flag at_exit_once;
	std::call_once(at_exit_once, [] { (void)atexit(wait_for_all_spec_jobs); });
	std::shared_ptr<SpecJob> job;
	{
		std::lock_guard<std::mutex> lk(g_jobs_mu);
		for (auto it = g_jobs.begin(); it != g_jobs.end();) { if (it->second.expired()) it = g_jobs.erase(it); else ++it; }
		auto it = g_jobs.find(key);
		if (it != g_jobs.end()) job = it->second.lock();
		if (!job) {
			job = std::make_shared<SpecJob>();
			job->key = key; job->model.assign(&c->model.d); job->plan = c->spec.plan; job->lsum_oob = lsum_oob; job->window = window;
			SpecJob* raw = job.get();   // (the job outlives its thread: its destructor joins)
			job->th = std::thread([raw] { raw->run(); });
			g_jobs[key] = job;
		}
	}
	c->spec.job = job; c->spec.job_oob = lsum_oob; c->spec.job_window = window;
	c->spec.state = 1;
	return TD_OK;
}

// Hand-over of a finished background compile, polled where a batch is staged (block: td_spec_wait).  Everything queued on the
// compute streams finishes first -- the step the mid-run reloads take too; outstanding tickets stay valid -- then the kernel is
// installed as after a synchronous compile.
int spec_handover(td_ctx* c, bool block)
{
	if (!c->spec.job) return c->spec.state == 5 && !c->spec.job_err.empty() ? fail(c, "%s", c->spec.job_err.c_str()) : TD_OK;
	if (!block && !c->spec.job->finished()) return TD_OK;
	c->spec.job->wait();
	const std::shared_ptr<SpecJob> job = std::move(c->spec.job);   // (which leaves c->spec.job empty)
	if (job->rc != TD_OK) {
		c->spec.state = 5;
		(void)fail(c, "td_model_upload: specialised kernel did not compile (background compile): %.400s", job->log.c_str());
		c->spec.job_err = c->err;
		return TD_FAIL;
	}
	c->spec.state = 2;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	return install_spec_kernel(c, job->code, job->key, c->spec.job_oob, c->spec.job_window, true);
}

extern "C" int td_spec_wait(td_ctx* c)
{
	if (!c) return TD_FAIL;
	while (c->spec.job) if (spec_handover(c, true) != TD_OK) return TD_FAIL;   // (a self-check fallback starts a second job)
	return spec_handover(c, false);
}

int spec_state_now(td_ctx* c) { return c->spec.job ? (c->spec.job->finished() ? 2 : 1) : c->spec.state; }
// The pending compile joins the superseded ones.  wait (the context goes): they all finish first -- as long as a compile at worst,
// and the code objects are in the caches afterwards; else (a new upload) those that have finished are let go.
void spec_retire_jobs(td_ctx* c, bool wait)
{
	if (c->spec.job) { c->spec.retired.push_back(c->spec.job); c->spec.job.reset(); }
	if (wait) { for (auto& j : c->spec.retired) j->wait(); c->spec.retired.clear(); return; }
	for (size_t k = 0; k < c->spec.retired.size();) { if (c->spec.retired[k]->finished()) c->spec.retired.erase(c->spec.retired.begin() + (long)k); else k++; }
	c->spec.job_err.clear();
}

// The clamp-free logsum of the specialised kernel turns |a - b| * 4000 into an LDS byte address (a saturating conversion; the
// shift form it replaced wrapped at |a - b| = 2^30 / 1000, and the limit still keeps that margin).  Every finite DP value is
// a sum of at most 2 parameters per position, and the posterior terms add two such values, so 4 * max|parameter| * (L + 2)
// bounds every finite difference; 6 * keeps a margin.
static bool spec_lsum_range_ok(const td_ctx* c, int lmax)
{
	const double limit = c->spec.lsum_limit;   // (1e6; tests lower it to force the switch to the clamped form)
	return 6.0 * (double)c->spec.maxabs * ((double)lmax + 2.0) < limit;
}

int spec_before_batch(td_ctx* c, int lmax)
{
	if (c->spec.ready && c->spec.oob && !spec_lsum_range_ok(c, lmax)) {
		HIPCHK(c, sync_compute(c));
		if (load_spec_kernel(c, 0) != TD_OK) return TD_FAIL;   // reads this long need the clamped logsum (seconds, once)
	}
	return c->spec.ready ? ensure_prune_tables(c, lmax) : TD_OK;
}

int spec_load_window_variant(td_ctx* c) { return load_spec_kernel(c, c->spec.oob ? 1 : 0, 1); }

// model-specialised kernel: compile now (seconds); a failure is an error, never a silent fallback
int spec_model_uploaded(td_ctx* c)
{
	TdSpecState& sp = c->spec;
	if (spec_unload(c) != TD_OK) return TD_FAIL;
	sp.prune_lcap = 0; sp.prune_live = false;   // the pruning tables belong to the model
	sp.state = 0; sp.batches_generic = 0; sp.probe_us = 0;
	if (!sp.specialize) return TD_OK;
	const td_model_desc* m = &c->model.d;
	float mx = 0.0f;
	auto scan = [&](const float* v, size_t n) { for (size_t i = 0; i < n; i++) if (std::isfinite(v[i]) && fabsf(v[i]) > mx) mx = fabsf(v[i]); };
	scan(m->trans, (size_t)m->C * 9); scan(m->eM, (size_t)m->C * 5); scan(m->eI, (size_t)m->C * 5);
	scan(m->sM, m->C); scan(m->sI, m->C); scan(m->skip, m->S); scan(m->bg, 5);
	sp.maxabs = mx;
	sp.plan = td_spec_plan(m, td_spec_knobs());
	sp.block = sp.plan.k.block;   // the launch geometry, of every launch of this model's kernel (the probe's too)
	// resident waves per CU: two LDS tables fit a CU; a 1024-thread workgroup fills it alone
	const int wpb = sp.block / TD_WAVE;
	const int blocks_per_cu = std::min(2, std::max(1, 32 / wpb));   // 32 waves per CU; two logsum tables (<= 66.5 KB each) per 160 KB of LDS
	sp.waves_per_cu = std::min(blocks_per_cu * wpb, 4 * sp.plan.k.min_waves);   // ... and the registers
	// ... or, with "async_compile", on a host thread: the generic kernel decodes until the hand-over (spec_handover)
	const int oob = sp.oob_unsafe ? 0 : sp.plan.k.lsum_oob;
	return sp.async_compile ? start_spec_job(c, oob, c->match_len > 0) : load_spec_kernel(c, oob);
}
