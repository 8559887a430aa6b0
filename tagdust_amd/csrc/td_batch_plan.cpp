// td_batch_plan.cpp -- see td_batch_plan.h.  Plain C++: integers in, integers out.
#include "td_batch_plan.h"

#include "../../include/tagdust_hip.h"

#include <vector>

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

void make_layout(TdWsLayout& L, int S, int H, int C, int lmax, int max_ncol)
{
	int64_t o = 0;
	L.codes = o; o = align256(o + (int64_t)(lmax + 2) * TD_WAVE);
	L.sb = o;    o = align256(o + (int64_t)(S + 1) * (lmax + 2) * TD_WAVE * 4);
	L.sf = o;    o = align256(o + (int64_t)(S + 1) * (lmax + 2) * TD_WAVE * 4);
	L.bw = o;    o = align256(o + (int64_t)C * lmax * TD_WAVE * 8);
	L.fwrow = o; o = align256(o + (int64_t)max_ncol * TD_WAVE * 8);
	L.dp = o;    o = align256(o + (int64_t)lmax * H * TD_WAVE * 4);
	L.path = o;  o = align256(o + (int64_t)lmax * H * TD_WAVE);
	L.acc = o;   o = align256(o + (int64_t)H * TD_WAVE * 4);
	L.total = o; o = align256(o + (int64_t)H * TD_WAVE * 4);
	L.dust = o;  o = align256(o + (int64_t)64 * TD_WAVE);
	L.slot_bytes = o;
}

OutLayout out_layout(int64_t n_tiles, int lmax, int nw1)
{
	OutLayout o;
	o.soa_stride = n_tiles * TD_WAVE * 4;      // a multiple of 256
	int64_t p = 8 * o.soa_stride;
	o.keep = p; p = align256(p + n_tiles * nw1 * TD_WAVE * 4);
	o.labels = p; p = align256(p + n_tiles * (int64_t)(lmax + 1) * TD_WAVE);
	o.total = p;
	return o;
}

// Length classes.  The reads are sorted by length on the device, so tile t holds the reads ranked 64 t .. 64 t + 63: from the
// histogram of the lengths, the longest read of every tile.  When the batch's longest read is at least half as long again as
// the reads at the 99 % mark, the tiles beyond that mark (n_long of them) get wave slots of their own geometry and the rest
// keeps the geometry of the many -- one 1000-base read among 150-base reads no longer costs every slot 6.6 times the memory.
TdLengthClasses plan_length_classes(const int64_t* offs, int64_t n, int lmin, int lmax, int64_t n_tiles, bool wanted)
{
	TdLengthClasses lc = { 0, lmax };
	if (!wanted || lmin == lmax || n_tiles < 64) return lc;
	std::vector<int64_t> hist((size_t)lmax + 2, 0);
	for (int64_t i = 0; i < n; i++) hist[(size_t)(offs[i + 1] - offs[i])]++;
	// rank of the last read of the tile at the 99 % mark, its length, and the tiles that hold anything longer
	const int64_t t99 = n_tiles - 1 - (n_tiles + 99) / 100;
	const int64_t rank = t99 * TD_WAVE + TD_WAVE - 1;
	int64_t acc = 0;
	int l99 = lmax;
	for (int l = 0; l <= lmax; l++) { acc += hist[(size_t)l]; if (acc > rank) { l99 = l; break; } }
	if (l99 < 1) l99 = 1;
	if ((int64_t)lmax * 2 >= (int64_t)l99 * 3) {
		int64_t upto = 0;   // reads of length <= l99
		for (int l = 0; l <= l99; l++) upto += hist[(size_t)l];
		const int64_t first_long_tile = upto / TD_WAVE;                 // (a tile that mixes both kinds counts as long)
		lc.n_long = (int32_t)(n_tiles - first_long_tile);
		lc.lmax_small = l99;
	}
	return lc;
}

TdWsPlan plan_workspace(const TdWsRequest& rq, TdFreeMemFn free_mem, void* arg)
{
	TdWsPlan p;
	p.half_slots = rq.half_slots;
	int overlap = rq.overlap, wsi = rq.wsi;
	for (;;) {   // (a second round when the second workspace is given up: the same batch on workspace 0)
		p.n_long = rq.n_long; p.lmax_small = rq.lmax_small;
		p.one_geometry = false;
		int64_t slot_bytes = rq.small_slot_bytes;
		// wave slots: enough to fill the chip (2 workgroups of 4 waves per CU share the LDS), bounded by HBM
		const int wpb = rq.wpb;
		int64_t slots = rq.want_slots;
		if (slots > rq.n_tiles) slots = rq.n_tiles;
		if (slots < 1) slots = 1;
		slots = (slots + wpb - 1) / wpb * wpb; // whole workgroups
		// length classes: the long tiles need a slot each of the big geometry (they are the first tiles the lowest slots take); when
		// they are too many for that to pay -- more than a quarter of the slots -- the batch keeps one geometry
		p.n_big = 0;
		int64_t big_extra = 0;       // bytes the big slots take beyond a small slot each
		if (rq.spec_ready && p.n_long > 0) {
			if ((int64_t)p.n_long * 4 <= slots) {
				p.n_big = p.n_long;
				big_extra = (int64_t)p.n_big * (rq.big_slot_bytes - rq.small_slot_bytes);
			} else {
				p.n_long = 0; p.lmax_small = rq.lmax;
				p.one_geometry = true;
				slot_bytes = rq.big_slot_bytes;
			}
		}
		p.ws_slot_bytes = slot_bytes;
		const size_t cap_ws = wsi ? rq.cap_ws2 : rq.cap_ws;
		// Pipelined batches overlap their launches on two streams with a workspace each.  When HBM cannot hold two workspaces of the
		// full wave-slot count (config 5: 42 MiB per slot, 172 GB for 4096 slots) each launch gets half the slots instead -- two
		// launches side by side still fill every SIMD, and the machine stays busy while one launch's slowest waves finish.
		if (rq.pipelined && overlap && rq.pipeline_depth > 1 && rq.spec_ready && !p.half_slots) {
			size_t free_b = 0;
			if (!free_mem(arg, &free_b)) { p.query_failed = true; return p; }
			const double avail = (double)free_b + (double)rq.cap_ws + (double)rq.cap_ws2;
			if (2.0 * (double)(slots * slot_bytes + big_extra) > 0.8 * avail && (double)(slots * slot_bytes + big_extra) <= 0.8 * avail) p.half_slots = true;
		}
		if (p.half_slots && rq.pipelined) {
			int64_t half = (slots / 2 + wpb - 1) / wpb * wpb;
			if (half < wpb) half = wpb;
			if (half >= p.n_big * 4 || p.n_big == 0) slots = half;
		}
		if ((size_t)(slots * slot_bytes + big_extra) > cap_ws) {
			size_t free_b = 0;
			if (!free_mem(arg, &free_b)) { p.query_failed = true; return p; }
			if (wsi == 1 && (double)(slots * slot_bytes + big_extra) > (p.half_slots ? 0.6 : 0.4) * (double)(free_b + cap_ws)) {
				// HBM cannot hold a second workspace of this size beside the first: this and all later batches run on the first stream
				p.overlap_given_up = true;
				overlap = 0; wsi = 0;
				continue;
			}
			const int64_t budget = (int64_t)((double)(free_b + cap_ws) * 0.85);
			if (slots * slot_bytes + big_extra > budget) {
				if (big_extra > budget / 2) {   // not even the long tiles' slots fit beside a useful number of others: one geometry
					p.n_long = 0; p.lmax_small = rq.lmax; p.n_big = 0; big_extra = 0;
					p.one_geometry = true;
					slot_bytes = rq.big_slot_bytes;
					p.ws_slot_bytes = slot_bytes;
				}
				slots = (budget - big_extra) / slot_bytes / wpb * wpb;
			}
			if (slots < wpb || slots < p.n_big) { p.no_fit = true; return p; }
			if ((size_t)(slots * slot_bytes + big_extra) > cap_ws) {
				p.alloc_bytes = (size_t)(slots * slot_bytes + big_extra);
				// Where the driver places a large allocation decides how fast the kernel's spill stream runs over it (up to
				// 9 % on one box).  A large workspace is therefore chosen among a few candidates that
				// exist side by side (the caller probes each and keeps the fastest) -- unless it is small, or they would take
				// too much of the memory between them.
				p.n_candidates = rq.ws_candidates;
				if (p.n_candidates > 4) p.n_candidates = 4;
				if (p.alloc_bytes < ((size_t)2 << 30) || (double)p.alloc_bytes * p.n_candidates > 0.6 * (double)(free_b + cap_ws)) p.n_candidates = 1;
			}
		}
		p.n_wave_slots = (int32_t)slots;
		p.ws_bytes = slots * slot_bytes + big_extra;
		return p;
	}
}

// One output as plain bytes: into the caller's buffer when that is page-locked, else through pinned staging.
static TdEgressChannel plain_channel(int k, size_t bytes, TdPageLockedFn page_locked, void* arg)
{
	TdEgressChannel ch;
	ch.form = page_locked(arg, k) ? TD_EG_DIRECT : TD_EG_STAGED;
	ch.copy_bytes = ch.alloc_bytes = bytes;
	return ch;
}

static TdEgressChannel compact_channel(size_t copy_bytes, size_t alloc_bytes)
{
	TdEgressChannel ch;
	ch.form = TD_EG_COMPACT;
	ch.copy_bytes = copy_bytes; ch.alloc_bytes = alloc_bytes;
	return ch;
}

// Compact egress.  The rewritten sequence is the input with some positions turned into the spacer byte: the keep bits (one
// per base) come back instead and the host rebuilds it from its staging copy of the input -- unless the caller's page-locked
// buffer was the DMA source, which the caller may have refilled since.  ri->labels is a handful of runs per read (the path
// moves through the segments in order): (length, label) pairs come back and the host expands them.  A fifth of the bytes
// over PCIe, and that much less work for the download's blit kernels, which compete with the decode kernel for CUs.
TdEgressPlan plan_egress(const TdEgressRequest& rq, TdPageLockedFn page_locked, void* arg)
{
	TdEgressPlan p;
	if (rq.n_reads == 0) return p;
	const size_t n = (size_t)rq.n_reads, seq_bytes = (size_t)rq.n_bases;
	p.rle_cap = rq.runs_cap > 0 ? rq.runs_cap : rq.rle_capacity;
	p.lab_plain_bytes = (size_t)(rq.n_bases + rq.n_reads);   // (ri->labels has one entry more than the read has bases)
	if (rq.want[TD_CH_RES]) p.ch[TD_CH_RES] = plain_channel(TD_CH_RES, n * sizeof(td_read_result), page_locked, arg);
	if (rq.want[TD_CH_SEQ]) {
		const size_t keep_bytes = n * (size_t)rq.nw1 * 4;
		if (rq.compact_egress && seq_bytes && rq.raw_host) p.ch[TD_CH_SEQ] = compact_channel(keep_bytes, keep_bytes);
		else p.ch[TD_CH_SEQ] = plain_channel(TD_CH_SEQ, seq_bytes, page_locked, arg);   // (no bases: buffers, and nothing to copy)
	}
	if (rq.want[TD_CH_LAB]) {
		if (rq.compact_egress) {
			// the overflow flag travels behind the runs in the same copy (a copy of a few bytes of its own would be carried out by a blit
			// kernel); the table has a word to spare behind it
			const size_t runs = n * (size_t)p.rle_cap;
			p.ch[TD_CH_LAB] = compact_channel((runs + 1) * 4, (runs + 2) * 4);
			p.rle_flag_word = runs;
			p.finish_reads_runs = rq.runs_cap > 0;
			if (p.finish_reads_runs) p.runs_flag_word = (size_t)rq.n_tiles * (size_t)rq.runs_cap * TD_WAVE;
		} else p.ch[TD_CH_LAB] = plain_channel(TD_CH_LAB, p.lab_plain_bytes, page_locked, arg);
	}
	return p;
}

void plan_labels_plain(TdEgressPlan& p, TdPageLockedFn page_locked, void* arg)
{
	p.ch[TD_CH_LAB] = plain_channel(TD_CH_LAB, p.lab_plain_bytes, page_locked, arg);
}
