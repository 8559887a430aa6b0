// td_batch.hip -- the per-batch path of the C-ABI host layer (include/tagdust_hip.h; the context's housekeeping is td_api.hip):
// upload, decode, download, their pipelined form td_submit / td_wait, td_arch_scores, and what the last batch reports of itself.
// The only host code that runs once per batch.  What is decided without the device -- the geometry of a batch, the form its
// results come back in -- is td_batch_plan.cpp's and only applied here.
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "td_ctx.h"
#include "td_rnadust.h"

// ---------------------------------------------------------------------------------------------------------
// batches
// ---------------------------------------------------------------------------------------------------------
// A batch lives in a slot. The host hands over the reads as they are (base codes or FASTQ sequence text + offsets) and
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

void slot_release(TdSlot& s)
{
	void* dev[] = { s.d_raw, s.d_offs, s.d_read_at, s.d_keys, s.d_vals, s.d_sort_tmp, s.d_packed, s.d_lens, s.d_art_left,
	                s.d_out, s.d_res, s.d_seq, s.d_lab, s.d_keepo, s.d_rle, s.d_runs, s.d_judged, s.d_mate_raw, s.d_mate_offs, s.d_mate_w,
	                s.d_mate_n, s.d_mate_type, s.d_qual_w, s.d_smp_w };
	for (void* p : dev) if (p) (void)hipFree(p);
	void* pinned[] = { s.h_raw, s.h_offs, s.h_res, s.h_seq, s.h_lab, s.h_keepo, s.h_rle, s.h_mate_raw, s.h_mate_offs, s.h_qual_w, s.h_smp_w };
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
static int slot_stage(td_ctx* c, TdSlot& s, const TdRoute& route, const void* bases, int is_ascii, const int64_t* offs, int64_t n, hipStream_t up, bool with_workspace = true, bool take_mate = false, bool take_qual = false, bool take_words = false)
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
	if (take_qual && qual_stage(c, s, offs, n, up) != TD_OK) return TD_FAIL;  // the base-quality filter: the named qualities, one bit per base
	if (take_words && samples_words_stage(c, s, n, up) != TD_OK) return TD_FAIL;   // the join across input files: partner words in / the export's array named
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
	s.samples_gen = c->samples.on ? c->samples.gen : 0;
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

// The bracket every launch over a staged slot stands in, whichever kernel it is.  launch_begin: is there a batch this mode can
// run over, then nothing of the slot's previous launch survives; `empty`: the batch has no reads, and that was all.
static int launch_begin(td_ctx* c, TdSlot& s, int mode, bool& empty)
{
	if (!s.staged) return fail(c, "td_run: no batch resident (td_batch_upload failed or was not called)");
	if (mode != TD_MODE_RNA_DUST && s.n_tiles > 0 && s.n_wave_slots == 0) return fail(c, "td_run: the resident batch was staged for TD_MODE_RNA_DUST, without a decode workspace (upload it again)");
	HIPCHK(c, hipSetDevice(c->device));
	// mate mode: a batch that was staged without its mates (or with those of another M) is not counted, and not decoded either
	if (mode == TD_MODE_GET_LABEL && c->molecules.mate.bases > 0 && c->molecules.mate.bases != s.mate_m) {
		c->molecules.mate.named = false;
		return fail(c, "td_run: mate mode is on (td_mol_mate_enable, %d bases) and the resident batch of %lld reads was staged without a mate "
		            "batch of as many reads: td_mol_mate_next first, then td_batch_upload; nothing was counted", c->molecules.mate.bases, (long long)s.n_reads);
	}
	// the mate filter: a batch staged under the other state of the switch has the wrong verdicts, or none
	if (mode == TD_MODE_GET_LABEL && c->molecules.mate.bases > 0 && c->molecules.mate.filter != s.mate_judged) {
		c->molecules.mate.named = false;
		return fail(c, "td_run: the mate filter is %s (td_mol_mate_filter_%s) and the resident batch of %lld reads was staged while it was %s: "
		            "td_mol_mate_next first, then td_batch_upload; nothing was counted", c->molecules.mate.filter ? "on" : "off",
		            c->molecules.mate.filter ? "enable" : "disable", (long long)s.n_reads, s.mate_judged ? "on" : "off");
	}
	// sample assignment: a batch staged under another state of the switch, or another sheet, is not rewritten, and not decoded either
	if (mode == TD_MODE_GET_LABEL && s.samples_gen != (c->samples.on ? c->samples.gen : 0))
		return fail(c, "td_run: sample assignment is %s (td_samples_%s) and the resident batch of %lld reads was staged %s: upload it again; "
		            "nothing was assigned", c->samples.on ? "on" : "off", c->samples.on ? "enable" : "disable", (long long)s.n_reads,
		            s.samples_gen ? (c->samples.on ? "under an earlier sheet" : "while it was on") : "while it was off");
	// the join across input files: a batch staged without its partner words, or without an array for the words it exports
	if (mode == TD_MODE_GET_LABEL && c->samples.on && c->samples.join && !s.join_words) {
		c->samples.next.named = false;
		return fail(c, "td_run: the context joins its partners' barcode calls (td_samples_join_enable) and the resident batch of %lld reads was staged "
		            "without words named for as many reads: td_samples_join_next first, then td_batch_upload; nothing was decoded", (long long)s.n_reads);
	}
	if (mode == TD_MODE_GET_LABEL && s.export_gen != (c->samples_export.on ? c->samples_export.gen : 0)) {
		c->samples_export.next.named = false;
		if (!c->samples_export.on)
			return fail(c, "td_run: the export is off (td_samples_export_disable) and the resident batch of %lld reads was staged while it was on: "
			            "upload it again; nothing was decoded", (long long)s.n_reads);
		return fail(c, "td_run: the context exports its barcode calls (td_samples_export_enable) and the resident batch of %lld reads was staged %s: "
		            "td_samples_export_next first, then td_batch_upload; nothing was decoded", (long long)s.n_reads,
		            s.export_gen ? "under an earlier td_samples_export_enable" : "without an array named for as many words");
	}
	// the base-quality filter: a batch staged without its qualities, or under another enable, has no verdicts to give
	if (mode == TD_MODE_GET_LABEL && s.qual_gen != (c->quality.on ? c->quality.gen : 0)) {
		c->quality.named = false;
		if (!c->quality.on)
			return fail(c, "td_run: the base-quality filter is off (td_qual_disable) and the resident batch of %lld reads was staged while it was on: "
			            "upload it again; nothing was decoded", (long long)s.n_reads);
		return fail(c, "td_run: the base-quality filter is on (td_qual_enable) and the resident batch of %lld reads was staged %s: td_qual_next "
		            "first, then td_batch_upload; nothing was decoded", (long long)s.n_reads,
		            s.qual_gen ? "under an earlier td_qual_enable" : "without qualities named for as many reads");
	}
	s.reset_decoded();   // (runs_cap above all: a launch of the generic kernel, or an empty batch, must not hand the label runs of this
	                     // slot's previous launch to the finish kernel)
	s.mode = mode;
	empty = s.n_tiles == 0;
	if (empty) { s.ran = true; s.last_ms = 0.0f; }
	return TD_OK;
}

// -ref: which reads are the left-over ones of their thread range, queued in front of the launch that reads d_art_left
static int slot_art_left(td_ctx* c, TdSlot& s)
{
	s.sb.art_threads = c->art_threads;
	s.sb.art_first = c->win_first; s.sb.art_total = c->win_total;
	HIPCHK(c, td_stage_art_left(s.sb, s.cs));
	return TD_OK;
}

// ... launch_end, behind the launch (ev_k0 stands in front of it): its stop event, then the counts that read the outcomes it left
// -- the -ref hits when it ran with the filter, census and molecule count over a labelled batch -- and the slot has run.  With the
// mate filter on, the join of the mates' verdicts stands in front of all of them: they read one outcome per pair.  Sample assignment
// (td_samples.hip) rewrites outcome and barcode behind the join and the hits, in front of census and molecule count: they read one
// sample per read.  The base-quality filter (td_quality.hip) gives its verdicts behind the join and the hits and in front of all
// three: a read it drops is neither assigned nor counted.
static int launch_end(td_ctx* c, TdSlot& s, bool with_artifacts)
{
	HIPCHK(c, hipEventRecord(s.ev_k1, s.cs));
	TdKernelArgs o{};
	point_outputs(o, s.d_out, out_layout(s.n_tiles, s.lmax, s.nw1));
	if (c->molecules.mate.filter && s.mode == TD_MODE_GET_LABEL && mol_mate_join(c, s, o.out_type) != TD_OK) return TD_FAIL;
	if (with_artifacts && slot_count_hits(c, s, o.out_type) != TD_OK) return TD_FAIL;
	if (c->quality.on && s.mode == TD_MODE_GET_LABEL && qual_slot(c, s, o.out_type, o.out_labels) != TD_OK) return TD_FAIL;
	if (c->samples.on && s.mode == TD_MODE_GET_LABEL && samples_slot(c, s, o.out_type, o.out_barcode, o.out_labels) != TD_OK) return TD_FAIL;
	// (a context assigns or exports: the exporter side of the join stands at the same place and changes nothing of the batch)
	if (c->samples_export.on && s.mode == TD_MODE_GET_LABEL && samples_export_slot(c, s, o.out_type, o.out_labels) != TD_OK) return TD_FAIL;
	if (c->census.on && s.mode == TD_MODE_GET_LABEL && census_count_slot(c, s, o.out_type, o.out_labels) != TD_OK) return TD_FAIL;
	// the molecule count last: dedup's second pass, the last launch in there, rewrites the outcomes the counts above read
	if (c->molecules.on && s.mode == TD_MODE_GET_LABEL && mol_slot_decoded(c, s, o.out_type, o.out_barcode, o.out_finger, o.out_labels) != TD_OK) return TD_FAIL;
	s.ran = true;
	s.last_ms = -1.0f;
	c->last_slot = (int)(&s - c->slots);
	return TD_OK;
}

// What a launch of the generic kernel's argument struct takes from the context, a model's tables and a staged slot, whoever launches.
static void fill_kernel_args(TdKernelArgs& ka, const td_ctx* c, const DevModel& d, const TdSlot& s)
{
	ka.hdr = d.d_hdr; ka.cols = d.d_cols; ka.hinfo = d.d_hinfo; ka.pred_off = d.d_pred_off; ka.pred_idx = d.d_pred_idx;
	ka.logsum = c->d_logsum; ka.packed = s.d_packed; ka.lens = s.d_lens;
	ka.n_tiles = s.n_tiles; ka.lmax = s.lmax; ka.nw2 = s.nw2; ka.nw1 = s.nw1;
	ka.minlen = c->minlen; ka.counters = c->d_counters;
}

static int slot_decode(td_ctx* c, TdSlot& s, int mode, bool want_labels = true)
{
	if (mode == TD_MODE_RNA_DUST) return slot_rna_dust(c, s);
	if (!c->have_model) return fail(c, "td_run: no model uploaded");
	if (mode != TD_MODE_GET_LABEL && mode != TD_MODE_GET_PROB && mode != TD_MODE_ARCH_COMP) return fail(c, "td_run: unsupported mode %d", mode);
	bool empty = false;
	if (launch_begin(c, s, mode, empty) != TD_OK) return TD_FAIL;
	if (empty) return TD_OK;
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
	fill_kernel_args(ka, c, c->dev, s);
	ka.n_slots = s.n_wave_slots;
	ka.mode = mode; ka.threshold = c->threshold; ka.dust = c->dust; ka.want_labels = 1;
	ka.win_start = c->match_start; ka.win_len = c->match_len;
	point_outputs(ka, s.d_out, ol);
	ka.ws = s.wsi ? c->d_ws2 : c->d_ws; ka.lay = s.lay;
	if (c->art_n > 0 && mode == TD_MODE_GET_LABEL) {
		if (slot_art_left(c, s) != TD_OK) return TD_FAIL;
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
	return launch_end(c, s, ka.art_n > 0);
}

// run_rna_dust over a staged slot (TD_MODE_RNA_DUST, td_rnadust.hip): no model, no workspace.  The outputs take the decode
// kernels' place, so that the finish kernel and the downloads are the same.
static int slot_rna_dust(td_ctx* c, TdSlot& s)
{
	bool empty = false;
	if (launch_begin(c, s, TD_MODE_RNA_DUST, empty) != TD_OK) return TD_FAIL;
	if (empty) return TD_OK;
	const OutLayout ol = out_layout(s.n_tiles, s.lmax, s.nw1);
	TdRnaDustArgs ra{};
	ra.packed = s.d_packed; ra.lens = s.d_lens; ra.n_tiles = s.n_tiles; ra.nw2 = s.nw2; ra.nw1 = s.nw1;
	ra.raw = s.d_raw; ra.offs = s.d_offs; ra.read_at = s.sorted ? s.d_read_at : nullptr; ra.n_reads = s.n_reads; ra.is_ascii = s.is_ascii;
	ra.dust = c->dust;
	if (c->art_n > 0) {
		if (slot_art_left(c, s) != TD_OK) return TD_FAIL;
		ra.art_pk = c->d_art_pk; ra.art_seq = c->d_art_seq; ra.art_left = s.d_art_left;
		ra.art_n = c->art_n; ra.art_fe = c->art_fe;
	}
	point_outputs(ra, s.d_out, ol);
	ra.counters = c->d_counters;
	HIPCHK(c, hipEventRecord(s.ev_k0, s.cs));
	HIPCHK(c, td_launch_rna_dust(ra, s.cs));
	return launch_end(c, s, ra.art_n > 0);
}

// Results into the caller's order on the device (finish kernel on the compute stream), then device -> host.  A page-locked
// destination is written by the DMA engine directly; anything else is reached through pinned staging and copied out by
// slot_fetch_end.  The synchronous calls queue the copies behind the finish kernel on the compute stream.  The pipelined
// calls must not: a copy queued behind an event is carried out by a blit *kernel*, which then competes for CUs with the
// next batch's decode kernel -- a persistent kernel that owns every register file -- and finishes when that does (measured:
// 41 ms instead of 3).  So td_wait waits for the finish kernel on the host and issues the copies then, with nothing
// pending in front of them: they go to the SDMA engines and run beside the decode kernel.
// The three outputs by channel number (td_batch_plan.h): the caller's buffer, whether that is page-locked (the egress plan's one
// question to the device), and the output's copy from the device -- where it starts there and where it lands on the host, by the
// form the plan gave it.
static void* user_buffer(const TdSlot& s, int k)
{
	void* const u[TD_N_CHANNELS] = { s.u_res, s.u_seq, s.u_labels };
	return u[k];
}
static bool user_page_locked(void* slot, int k) { return is_pinned(user_buffer(*(const TdSlot*)slot, k)); }
static bool plain(const TdEgressChannel& ch) { return ch.form == TD_EG_DIRECT || ch.form == TD_EG_STAGED; }
struct TdLeg { void* dst; const void* src; };
static TdLeg egress_leg(const TdSlot& s, int k)
{
	const int form = s.plan.ch[k].form;
	if (form == TD_EG_COMPACT) return k == TD_CH_SEQ ? TdLeg{ s.h_keepo, s.d_keepo } : TdLeg{ s.h_rle, s.d_rle };
	void* const staging[TD_N_CHANNELS] = { s.h_res, s.h_seq, s.h_lab };
	const void* const dev[TD_N_CHANNELS] = { s.d_res, s.d_seq, s.d_lab };
	return TdLeg{ form == TD_EG_DIRECT ? user_buffer(s, k) : staging[k], dev[k] };
}

static int slot_issue_copies(td_ctx* c, TdSlot& s, hipStream_t down)
{
	// (the labels' overflow flag travels behind the runs in the same copy -- the finish kernel folded the decode kernel's own flag
	// into it: a copy of a few bytes is carried out by a blit kernel, which gets no CU while a decode launch holds every
	// register file and made this wait last as long as that launch: tools/ubench/copy_kinds.cpp)
	for (int k = 0; k < TD_N_CHANNELS; k++) {
		const TdLeg leg = egress_leg(s, k);
		if (s.plan.ch[k].copy_bytes) HIPCHK(c, hipMemcpyAsync(leg.dst, leg.src, s.plan.ch[k].copy_bytes, hipMemcpyDeviceToHost, down));
	}
	// a pipelined exporter's words travel with the results (td_run has copied a synchronous batch's out itself)
	if (s.pipelined && s.export_gen && s.mode == TD_MODE_GET_LABEL && samples_export_issue_copy(c, s, down) != TD_OK) return TD_FAIL;
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
	if (s.n_reads == 0) return TD_OK;
	// the form each output travels in, and every byte count that goes with it (td_batch_plan.cpp)
	TdEgressRequest rq;
	rq.n_reads = s.n_reads; rq.n_bases = s.n_bases; rq.nw1 = s.nw1; rq.n_tiles = s.n_tiles;
	rq.want[TD_CH_RES] = res != nullptr; rq.want[TD_CH_SEQ] = seq_out != nullptr; rq.want[TD_CH_LAB] = labels != nullptr;
	rq.compact_egress = c->compact_egress != 0; rq.raw_host = s.raw_host != nullptr;
	rq.runs_cap = s.runs_cap; rq.rle_capacity = rle_capacity(c);
	s.plan = plan_egress(rq, user_page_locked, &s);
	const TdEgressPlan& p = s.plan;
	const TdEgressChannel &R = p.ch[TD_CH_RES], &Q = p.ch[TD_CH_SEQ], &L = p.ch[TD_CH_LAB];
	const bool keep = Q.form == TD_EG_COMPACT, rle = L.form == TD_EG_COMPACT;
	if (plain(R) && ensure(c, &s.d_res, &s.cap_res, R.alloc_bytes) != TD_OK) return TD_FAIL;
	if (plain(Q) && ensure(c, &s.d_seq, &s.cap_seq, Q.alloc_bytes) != TD_OK) return TD_FAIL;
	if (plain(L) && ensure(c, &s.d_lab, &s.cap_lab, L.alloc_bytes) != TD_OK) return TD_FAIL;
	if (R.form == TD_EG_STAGED && ensure_pinned(c, &s.h_res, &s.cap_h_res, R.alloc_bytes) != TD_OK) return TD_FAIL;
	if (Q.form == TD_EG_STAGED && ensure_pinned(c, &s.h_seq, &s.cap_h_seq, Q.alloc_bytes) != TD_OK) return TD_FAIL;
	if (L.form == TD_EG_STAGED && ensure_pinned(c, &s.h_lab, &s.cap_h_lab, L.alloc_bytes) != TD_OK) return TD_FAIL;
	if (keep && (ensure(c, &s.d_keepo, &s.cap_keepo, Q.alloc_bytes) != TD_OK || ensure_pinned(c, &s.h_keepo, &s.cap_h_keepo, Q.alloc_bytes) != TD_OK)) return TD_FAIL;
	if (rle) {
		if (ensure(c, &s.d_rle, &s.cap_rle, L.alloc_bytes) != TD_OK || ensure_pinned(c, &s.h_rle, &s.cap_h_rle, L.alloc_bytes) != TD_OK) return TD_FAIL;
		if (c->poison) HIPCHK(c, hipMemsetAsync(s.d_rle, 0xFF, p.rle_flag_word * sizeof *s.d_rle, s.fin));   // (tests: every entry the host expands must be this batch's)
		HIPCHK(c, hipMemsetAsync(s.d_rle + p.rle_flag_word, 0, sizeof *s.d_rle, s.fin));   // the overflow flag
	}
	if (keep && c->poison) HIPCHK(c, hipMemsetAsync(s.d_keepo, 0xFF, Q.alloc_bytes, s.fin));
	s.sb.res = plain(R) ? s.d_res : nullptr;
	s.sb.seq_out = plain(Q) ? s.d_seq : nullptr;
	s.sb.labels_out = plain(L) ? s.d_lab : nullptr;
	s.sb.keep_out = keep ? s.d_keepo : nullptr;
	s.sb.rle_out = rle ? s.d_rle : nullptr;
	s.sb.rle_cap = p.rle_cap;
	s.sb.runs = p.finish_reads_runs ? s.d_runs : nullptr;
	s.sb.rle_overflow = rle ? (int32_t*)(s.d_rle + p.rle_flag_word) : nullptr;
	s.sb.runs_overflow = p.finish_reads_runs ? (const int32_t*)(s.d_runs + p.runs_flag_word) : nullptr;
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
	if (s.pipelined && s.export_gen && s.mode == TD_MODE_GET_LABEL) samples_export_copy_out(s);
	const double t2 = dbg ? wall_ms() : 0.0;
	struct Rep { bool on; double t0, t1, t2; ~Rep() { if (on) fprintf(stderr, "td_wait: device %.2f ms, download %.2f ms, host %.2f ms\n", t1 - t0, t2 - t1, wall_ms() - t2); } } rep_{ dbg, t0, t1, t2 };
	TdEgressPlan& p = s.plan;
	if (p.ch[TD_CH_LAB].form == TD_EG_COMPACT && s.h_rle[p.rle_flag_word] != 0) {
		// a read with more label runs than the table holds (a model whose labels are not one per segment): the labels as they are
		plan_labels_plain(p, user_page_locked, &s);
		const TdEgressChannel& L = p.ch[TD_CH_LAB];
		if (ensure(c, &s.d_lab, &s.cap_lab, L.alloc_bytes) != TD_OK) return TD_FAIL;
		if (L.form == TD_EG_STAGED && ensure_pinned(c, &s.h_lab, &s.cap_h_lab, L.alloc_bytes) != TD_OK) return TD_FAIL;
		TdStageBatch b2 = s.sb;
		b2.res = nullptr; b2.seq_out = nullptr; b2.keep_out = nullptr; b2.rle_out = nullptr; b2.labels_out = s.d_lab;
		HIPCHK(c, td_stage_finish(b2, s.fin));
		HIPCHK(c, hipStreamSynchronize(s.fin));
		const TdLeg leg = egress_leg(s, TD_CH_LAB);
		HIPCHK(c, hipMemcpy(leg.dst, leg.src, L.copy_bytes, hipMemcpyDeviceToHost));
	}
	// what did not land in the caller's buffer itself: staged bytes are copied out, a compact output is rebuilt from what came back
	for (int k = 0; k < TD_N_CHANNELS; k++) {
		const TdEgressChannel& ch = p.ch[k];
		if (!ch.copy_bytes) continue;   // (not wanted, or sequences of no bases)
		if (ch.form == TD_EG_STAGED) parallel_copy(c, user_buffer(s, k), egress_leg(s, k).dst, ch.copy_bytes);
		else if (ch.form == TD_EG_COMPACT && k == TD_CH_SEQ)
			td_host_rebuild_sequences(c->pool, c->host_threads, s.n_reads, s.raw_host, s.h_offs, s.h_keepo, s.nw1, s.is_ascii, s.u_seq);
		else if (ch.form == TD_EG_COMPACT)
			td_host_expand_labels(c->pool, c->host_threads, s.n_reads, s.h_offs, s.h_rle, p.rle_cap, s.u_labels);
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
	// ... and so are the named qualities while the base-quality filter is on
	const bool take_qual = c->quality.on && c->quality.named && c->quality.next_reads == n && offs && n >= 0;
	// ... and the words of the join across input files, on either side of it
	const TdSamplesNamed& words = c->samples_export.on ? c->samples_export.next : c->samples.next;
	const bool take_words = (c->samples_export.on || (c->samples.on && c->samples.join)) && words.named && words.reads == n && n >= 0;
	if (slot_stage(c, s, rt, bases, is_ascii, offs, n, c->stream, true, take_mate, take_qual, take_words) != TD_OK) return TD_FAIL;
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
	TdSlot& s = c->slots[0];
	if (slot_decode(c, s, mode) != TD_OK) return TD_FAIL;
	if (c->samples_export.on && mode == TD_MODE_GET_LABEL && s.n_reads > 0) {   // the exporter's words are valid when td_run returns
		if (samples_export_issue_copy(c, s, s.cs) != TD_OK) return TD_FAIL;
		HIPCHK(c, hipStreamSynchronize(s.cs));
		samples_export_copy_out(s);
	}
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
	const bool take_qual = c->quality.on && mode == TD_MODE_GET_LABEL;
	if (take_qual && qual_check(c, n_reads, "td_submit") != TD_OK) return TD_FAIL;
	const bool take_words = (c->samples_export.on || (c->samples.on && c->samples.join)) && mode == TD_MODE_GET_LABEL;
	if (take_words && samples_words_check(c, n_reads, "td_submit") != TD_OK) return TD_FAIL;
	TdSlot& s = c->slots[k];
	TdRoute rt = sync_route(c);
	rt.pipelined = true;
	if (c->overlap && c->pipeline_depth > 1 && c->spec.ready) {   // every other batch on the second stream / workspace
		if (!c->stream2) HIPCHK(c, hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
		if (c->submit_parity) { rt.cs = c->stream2; rt.wsi = 1; }
		c->submit_parity ^= 1;
		rt.aux = c->s_aux; rt.fin = c->s_fin;
	}
	if (slot_stage(c, s, rt, bases, is_ascii != 0, offs, n_reads, c->s_up, mode != TD_MODE_RNA_DUST, take_mate, take_qual, take_words) != TD_OK) return TD_FAIL;
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
			fill_kernel_args(ka, c, d, s);
			ka.n_slots = max_slots;
			ka.mode = TD_MODE_ARCH_COMP; ka.threshold = 0.0f; ka.dust = 0; ka.want_labels = 0;
			ka.out_b = d_b + (int64_t)k * n_lanes;       // backward-only mode writes nothing else
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
