// batch_plan_host_check.cpp -- the batch geometry unit (tagdust_amd/csrc/td_batch_plan.cpp: length classes, workspace plan, egress plan) as a
// stand-alone program, for running it under the host sanitizers: no GPU is used, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tagdust_amd/csrc/td_batch_plan.cpp tools/batch_plan_host_check.cpp -o /tmp/batch_plan_host_check
//   /tmp/batch_plan_host_check                                   # (leak detection stays on)
//
// (a) cases whose expected values are derived by hand beside them; (b) a generated sweep held against old_lengths() / old_workspace(),
// the arithmetic as it stood inside td_api.hip's slot_stage() / ensure_workspace() before the unit existed, restated over plain
// integers (recursion and all) and sharing nothing with the unit: every field and the number of memory queries must agree, and every
// branch of (a) must be taken by at least 1 % of the cases; (c) what holds for every swept plan that succeeds.  The egress plan the
// same way: by hand, then the whole small input space against old_egress() / old_overflow() -- slot_fetch_begin(),
// slot_issue_copies() and slot_fetch_end() as they decided and counted before the plan existed -- with every form of every output
// taken by at least 1 % of the cases, every copy inside its buffers and both overflow flags inside theirs.  Exit status 0 when
// all of it agrees.
#define HOST_CHECK_NAME "batch_plan_host_check"
#include "host_check.h"
#include "../tagdust_amd/csrc/td_batch_plan.h"

// the device's free memory as the plan gets to see it: a fixed figure, and how often it was asked for
struct Hbm { size_t free_b = 0; int asked = 0; };
static bool hbm_free(void* arg, size_t* free_b) { Hbm* h = (Hbm*)arg; h->asked++; *free_b = h->free_b; return true; }

// ---------------------------------------------------------------------------------------------------------
// the restatements
// ---------------------------------------------------------------------------------------------------------
enum { LC_GATED, LC_MARK_LONG, LC_RATIO, LC_FOUND, LC_BRANCHES };
static const char* const lc_names[LC_BRANCHES] = { "gate closed", "read at the 99 % mark is long", "less than half as long again", "long tiles found" };

static void old_lengths(const int64_t* offs, int64_t n, int lmin, int lmax, int64_t n_tiles, bool spec_ready, bool with_workspace, int length_classes,
                        int32_t& n_long, int32_t& lmax_small, int& branch)
{
	n_long = 0; lmax_small = lmax;
	branch = LC_GATED;
	if (spec_ready && with_workspace && lmin != lmax && n_tiles >= 64 && length_classes) {
		std::vector<int64_t> hist((size_t)lmax + 2, 0);
		for (int64_t i = 0; i < n; i++) hist[(size_t)(offs[i + 1] - offs[i])]++;
		const int64_t t99 = n_tiles - 1 - (n_tiles + 99) / 100;
		const int64_t rank = t99 * 64 + 64 - 1;
		int64_t acc = 0;
		int l99 = lmax;
		for (int l = 0; l <= lmax; l++) { acc += hist[(size_t)l]; if (acc > rank) { l99 = l; break; } }
		if (l99 < 1) l99 = 1;
		branch = l99 == lmax ? LC_MARK_LONG : LC_RATIO;
		if ((int64_t)lmax * 2 >= (int64_t)l99 * 3) {
			int64_t upto = 0;
			for (int l = 0; l <= l99; l++) upto += hist[(size_t)l];
			const int64_t first_long_tile = upto / 64;
			n_long = (int32_t)(n_tiles - first_long_tile);
			lmax_small = l99;
			branch = LC_FOUND;
		}
	}
}

enum {
	B_SLOTS_BY_TILES, B_SLOTS_BY_WANT, B_LONG_KEPT, B_LONG_NOT_KEPT, B_HALF_TWICE_FITS, B_HALF_ONCE_DOES_NOT, B_HALF_SET, B_HALVED, B_HALVING_EXCEPTION,
	B_REFUSED_04, B_REFUSED_06, B_SHRINK_LONG_SURVIVE, B_SHRINK_ONE_GEOMETRY, B_NO_FIT, B_FITS_NO_QUERY, B_CAND_SMALL, B_CAND_TOO_MUCH, B_CAND_CAPPED, B_CAND_SEVERAL,
	B_BRANCHES
};
static const char* const b_names[B_BRANCHES] = {
	"slots bounded by the tiles", "slots bounded by the wanted count", "long tiles kept", "long tiles not kept (more than a quarter)",
	"half_slots: twice the need fits", "half_slots: not even the need fits", "half_slots set", "slots halved", "halving exception (half < 4 n_big)",
	"second workspace refused at 0.4", "second workspace refused at 0.6", "budget shrink, long tiles' slots survive", "budget shrink to one geometry",
	"does not fit", "fits as it is, no query", "one candidate: below 2 GiB", "one candidate: too much of memory", "candidates capped at 4", "several candidates"
};

// the context, slot and route of ensure_workspace() as far as its arithmetic reads or writes them, as plain integers
struct Old {
	// context
	bool spec_ready; int n_cu, spec_block, spec_waves_per_cu, generic_block; long wave_slots_forced;
	int overlap, pipeline_depth; bool half_slots; size_t cap_ws, cap_ws2; int ws_candidates;
	// slot
	int32_t n_tiles, lmax, n_long, lmax_small, n_big; int wsi; bool pipelined, on_first_stream;
	int64_t lay_bytes, slay_bytes, slay_big_bytes;                 // slot_bytes of s.lay, s.slay, s.slay_big
	int64_t spec_small_bytes, spec_big_bytes;                      // what td_spec_layout gives for lmax_small / lmax
	int32_t n_wave_slots; int64_t ws_slot_bytes, ws_bytes;
	// what the device part would be asked for
	size_t need; int n_cand; int64_t fail_slot_bytes;
	// the device
	size_t free_b; int asked;
	int hit[B_BRANCHES];
};
enum { OLD_OK, OLD_FAIL };

static int old_workspace(Old& o)
{
	int64_t slot_bytes = o.lay_bytes;
	if (o.spec_ready) {
		o.slay_bytes = o.n_long > 0 ? o.spec_small_bytes : o.spec_big_bytes;
		o.slay_big_bytes = o.spec_big_bytes;
		slot_bytes = o.slay_bytes;
	}
	const int wpb = (o.spec_ready ? o.spec_block : o.generic_block) / 64;
	int64_t want = (int64_t)o.n_cu * (o.spec_ready ? o.spec_waves_per_cu : 2 * wpb);
	if (o.wave_slots_forced > 0) want = o.wave_slots_forced;
	int64_t slots = want;
	if (slots > o.n_tiles) { slots = o.n_tiles; o.hit[B_SLOTS_BY_TILES] = 1; } else o.hit[B_SLOTS_BY_WANT] = 1;
	if (slots < 1) slots = 1;
	slots = (slots + wpb - 1) / wpb * wpb;
	o.n_big = 0;
	int64_t big_extra = 0;
	if (o.spec_ready && o.n_long > 0) {
		if ((int64_t)o.n_long * 4 <= slots) {
			o.n_big = o.n_long;
			big_extra = (int64_t)o.n_big * (o.slay_big_bytes - o.slay_bytes);
			o.hit[B_LONG_KEPT] = 1;
		} else {
			o.n_long = 0; o.lmax_small = o.lmax;
			o.slay_bytes = o.slay_big_bytes;
			slot_bytes = o.slay_bytes;
			o.hit[B_LONG_NOT_KEPT] = 1;
		}
	}
	size_t& cap_ws = o.wsi ? o.cap_ws2 : o.cap_ws;
	if (o.pipelined && o.overlap && o.pipeline_depth > 1 && o.spec_ready && !o.half_slots) {
		o.asked++;
		const double avail = (double)o.free_b + (double)o.cap_ws + (double)o.cap_ws2;
		if (2.0 * (double)(slots * slot_bytes + big_extra) > 0.8 * avail && (double)(slots * slot_bytes + big_extra) <= 0.8 * avail) { o.half_slots = true; o.hit[B_HALF_SET] = 1; }
		else if (2.0 * (double)(slots * slot_bytes + big_extra) > 0.8 * avail) o.hit[B_HALF_ONCE_DOES_NOT] = 1;
		else o.hit[B_HALF_TWICE_FITS] = 1;
	}
	if (o.half_slots && o.pipelined) {
		int64_t half = (slots / 2 + wpb - 1) / wpb * wpb;
		if (half < wpb) half = wpb;
		if (half >= o.n_big * 4 || o.n_big == 0) { if (half < slots) o.hit[B_HALVED] = 1; slots = half; }
		else o.hit[B_HALVING_EXCEPTION] = 1;
	}
	if ((size_t)(slots * slot_bytes + big_extra) > cap_ws) {
		o.asked++;
		if (o.wsi == 1 && (double)(slots * slot_bytes + big_extra) > (o.half_slots ? 0.6 : 0.4) * (double)(o.free_b + cap_ws)) {
			o.hit[o.half_slots ? B_REFUSED_06 : B_REFUSED_04] = 1;
			o.overlap = 0;
			o.wsi = 0; o.on_first_stream = true;
			return old_workspace(o);
		}
		const int64_t budget = (int64_t)((double)(o.free_b + cap_ws) * 0.85);
		if (slots * slot_bytes + big_extra > budget) {
			if (big_extra > budget / 2) {
				o.n_long = 0; o.lmax_small = o.lmax; o.n_big = 0; big_extra = 0;
				o.slay_bytes = o.slay_big_bytes;
				slot_bytes = o.slay_bytes;
				o.hit[B_SHRINK_ONE_GEOMETRY] = 1;
			} else if (o.n_big > 0) o.hit[B_SHRINK_LONG_SURVIVE] = 1;
			slots = (budget - big_extra) / slot_bytes / wpb * wpb;
		}
		if (slots < wpb || slots < o.n_big) {
			o.hit[B_NO_FIT] = 1; o.hit[B_SHRINK_LONG_SURVIVE] = 0;
			o.fail_slot_bytes = slot_bytes;
			return OLD_FAIL;
		}
		if ((size_t)(slots * slot_bytes + big_extra) > cap_ws) {
			const size_t need = (size_t)(slots * slot_bytes + big_extra);
			int n_cand = o.ws_candidates;
			if (n_cand > 4) { n_cand = 4; o.hit[B_CAND_CAPPED] = 1; }
			if (need < ((size_t)2 << 30)) { n_cand = 1; o.hit[B_CAND_SMALL] = 1; o.hit[B_CAND_CAPPED] = 0; }
			else if ((double)need * n_cand > 0.6 * (double)(o.free_b + cap_ws)) { n_cand = 1; o.hit[B_CAND_TOO_MUCH] = 1; o.hit[B_CAND_CAPPED] = 0; }
			if (n_cand > 1) o.hit[B_CAND_SEVERAL] = 1;
			o.need = need; o.n_cand = n_cand;
		}
	} else if (o.asked == 0) o.hit[B_FITS_NO_QUERY] = 1;
	o.n_wave_slots = (int32_t)slots;
	o.ws_slot_bytes = slot_bytes;
	o.ws_bytes = slots * slot_bytes + big_extra;
	return OLD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// (a) by hand
// ---------------------------------------------------------------------------------------------------------
// n reads of `len` bases, the last k of them `long_len` bases: their offsets
static std::vector<int64_t> offsets(int64_t n, int len, int64_t k, int long_len)
{
	std::vector<int64_t> offs{ 0 };
	for (int64_t i = 0; i < n; i++) offs.push_back(offs.back() + (i >= n - k ? long_len : len));
	return offs;
}

static TdLengthClasses classes(int64_t n, int len, int64_t k, int long_len, bool wanted = true)
{
	const std::vector<int64_t> offs = offsets(n, len, k, long_len);
	return plan_length_classes(offs.data(), n, len, k > 0 ? long_len : len, (n + 63) / 64, wanted);
}

// a request that no memory question touches: one stream, a workspace that holds anything
static TdWsRequest plain_request()
{
	TdWsRequest rq;
	rq.n_tiles = 1000; rq.lmax = rq.lmax_small = 150;
	rq.small_slot_bytes = rq.big_slot_bytes = 100;
	rq.wpb = 4; rq.want_slots = 64;
	rq.spec_ready = true; rq.overlap = 1; rq.pipeline_depth = 3;
	rq.cap_ws = rq.cap_ws2 = (size_t)1 << 50;
	rq.ws_candidates = 3;
	return rq;
}

static TdWsPlan plan_with(const TdWsRequest& rq, size_t free_b, int* asked = nullptr)
{
	Hbm h;
	h.free_b = free_b;
	const TdWsPlan p = plan_workspace(rq, hbm_free, &h);
	if (asked) *asked = h.asked;
	return p;
}

static int by_hand()
{
	// --- length classes.  4096 reads are 64 tiles: the 99 % mark is tile t99 = 64 - 1 - (64 + 99) / 100 = 62, whose last read has rank
	// 62 * 64 + 63 = 4031 among the lengths in rising order.  With k reads of 150 bases behind 4096 - k of 100, rank 4031 is a
	// 100-base read while 4096 - k > 4031, that is k <= 64.  150 * 2 >= 100 * 3 holds (300 >= 300), the first long tile is
	// (4096 - k) / 64 = 63 for k = 1 .. 64, so n_long = 64 - 63 = 1.
	for (int64_t k : { 1, 64 }) {
		const TdLengthClasses lc = classes(4096, 100, k, 150);
		CHECK(lc.n_long == 1 && lc.lmax_small == 100);
	}
	// k = 65: rank 4031 is a 150-base read, l99 = lmax, and 300 >= 450 fails
	{ const TdLengthClasses lc = classes(4096, 100, 65, 150); CHECK(lc.n_long == 0 && lc.lmax_small == 150); }
	// long reads of 149 bases: 149 * 2 = 298 < 300
	for (int64_t k : { 1, 64 }) { const TdLengthClasses lc = classes(4096, 100, k, 149); CHECK(lc.n_long == 0 && lc.lmax_small == 149); }
	// 63 tiles (4032 reads): too few tiles, whatever their lengths; and the gate's other inputs -- not wanted, one length
	{ const TdLengthClasses lc = classes(4032, 100, 1, 150); CHECK(lc.n_long == 0 && lc.lmax_small == 150); }
	{ const TdLengthClasses lc = classes(4096, 100, 1, 150, false); CHECK(lc.n_long == 0 && lc.lmax_small == 150); }
	{ const TdLengthClasses lc = classes(4096, 100, 0, 150); CHECK(lc.n_long == 0 && lc.lmax_small == 100); }
	// 12800 reads are 200 tiles: t99 = 200 - 1 - 299 / 100 = 197, rank 197 * 64 + 63 = 12671, a 100-base read while k <= 128.  The first long
	// tile is (12800 - k) / 64: 199 for k <= 64 (n_long = 1), 198 for k = 65 .. 128 (n_long = 2); k = 129: rank 12671 is long, none
	for (int64_t k : { 64, 65, 128, 129 }) {
		const TdLengthClasses lc = classes(12800, 100, k, 150);
		CHECK(lc.n_long == (k <= 64 ? 1 : k <= 128 ? 2 : 0) && lc.lmax_small == (k <= 128 ? 100 : 150));
	}
	// 6464 reads are 101 tiles, one beyond a hundred: t99 = 101 - 1 - 200 / 100 = 98, rank 98 * 64 + 63 = 6335, a 100-base read while k <= 128.
	// k = 100: the first long tile is 6364 / 64 = 99, n_long = 101 - 99 = 2
	{ const TdLengthClasses lc = classes(6464, 100, 100, 150); CHECK(lc.n_long == 2 && lc.lmax_small == 100); }

	// --- slots: the wanted count, at most the tiles, at least one, rounded up to whole workgroups of wpb = 4 waves
	{
		struct { int64_t n_tiles, want; int32_t slots; } cases[] = {
			{ 0, 1024, 4 },        // no tile: 1 slot -> 4
			{ 100, 1024, 100 },    // the tiles bound it; 100 is a multiple of 4
			{ 101, 1024, 104 },    // 101 -> 104
			{ 100, 50, 52 },       // the wanted count bounds it: 50 -> 52
			{ 101, 101, 104 },
			{ 100, 0, 4 },         // (a wanted count of 0 is 1 slot)
		};
		for (const auto& k : cases) {
			TdWsRequest rq = plain_request();
			rq.spec_ready = false; rq.n_tiles = k.n_tiles; rq.want_slots = k.want;
			int asked = -1;
			const TdWsPlan p = plan_with(rq, 0, &asked);
			CHECK(p.n_wave_slots == k.slots && p.ws_slot_bytes == 100 && p.ws_bytes == (int64_t)k.slots * 100);
			CHECK(asked == 0 && p.alloc_bytes == 0 && !p.no_fit && !p.one_geometry && !p.half_slots && !p.overlap_given_up && p.n_big == 0);
		}
	}
	// --- long tiles: a big slot (1000 bytes) each while they are at most a quarter of the slots.  wpb = 1, so that slots + 1 can be 4 n_long
	{
		TdWsRequest rq = plain_request();
		rq.wpb = 1; rq.n_long = 16; rq.lmax_small = 100; rq.big_slot_bytes = 1000;
		rq.want_slots = 64;    // 16 * 4 == 64: kept; 64 * 100 + 16 * 900 = 20800 bytes
		TdWsPlan p = plan_with(rq, 0);
		CHECK(p.n_wave_slots == 64 && p.n_big == 16 && p.n_long == 16 && p.lmax_small == 100 && !p.one_geometry && p.ws_slot_bytes == 100 && p.ws_bytes == 20800);
		rq.want_slots = 63;    // 16 * 4 == 63 + 1: not kept; 63 slots of the big geometry = 63000 bytes
		p = plan_with(rq, 0);
		CHECK(p.n_wave_slots == 63 && p.n_big == 0 && p.n_long == 0 && p.lmax_small == 150 && p.one_geometry && p.ws_slot_bytes == 1000 && p.ws_bytes == 63000);
		// without a specialised kernel the long tiles mean nothing to the plan (and stay as they came)
		rq.spec_ready = false; rq.small_slot_bytes = rq.big_slot_bytes = 700;
		p = plan_with(rq, 0);
		CHECK(p.n_wave_slots == 63 && p.n_big == 0 && p.n_long == 16 && !p.one_geometry && p.ws_bytes == 63 * 700);
	}
	// --- half_slots.  A pipelined batch on overlapping streams, nothing allocated yet: 8 slots of 128 bytes need 1024 bytes, all of the memory
	// is `free`.  (0.8 * 2560 and 0.8 * 1280 are 2048 and 1024 in double arithmetic, 0.8 * 1279 = 1023.2, 0.8 * 2559 = 2047.2.)
	{
		TdWsRequest rq = plain_request();
		rq.pipelined = true; rq.small_slot_bytes = rq.big_slot_bytes = 128; rq.want_slots = 8; rq.cap_ws = rq.cap_ws2 = 0;
		struct { size_t free_b; bool half, no_fit; int32_t slots; } cases[] = {
			{ 2560, false, false, 8 },   // twice the need (2048) is not above 0.8 * 2560 = 2048: both fit.  budget 2176
			{ 2559, true, false, 4 },    // 2048 > 2047.2, and 1024 <= 2047.2: half the slots each, (8 / 2 + 3) / 4 * 4 = 4
			{ 1280, true, false, 4 },    // the need is just at 0.8 * 1280 = 1024: still half_slots.  4 * 128 = 512 <= budget 1088
			{ 1279, false, false, 8 },   // 1024 > 1023.2: not even one fits that way, half_slots stays off; budget (int)(1279 * 0.85) = 1087 >= 1024
		};
		for (const auto& k : cases) {
			int asked = -1;
			const TdWsPlan p = plan_with(rq, k.free_b, &asked);
			CHECK(p.half_slots == k.half && p.no_fit == k.no_fit && p.n_wave_slots == k.slots && p.ws_bytes == (int64_t)k.slots * 128);
			CHECK(asked == 2 && p.alloc_bytes == (size_t)k.slots * 128 && p.n_candidates == 1 && !p.overlap_given_up);
		}
		// a pipelined batch whose workspace fits asks once, one that is not pipelined never
		rq.cap_ws = rq.cap_ws2 = 4096;
		int asked = -1;
		TdWsPlan p = plan_with(rq, 1 << 20, &asked);
		CHECK(asked == 1 && p.alloc_bytes == 0 && !p.half_slots && p.n_wave_slots == 8);
		rq.pipelined = false;
		p = plan_with(rq, 1 << 20, &asked);
		CHECK(asked == 0 && p.alloc_bytes == 0 && p.n_wave_slots == 8);
	}
	// --- halving, the context already on half_slots (no query for that).  64 slots, half = (32 + 3) / 4 * 4 = 32
	{
		TdWsRequest rq = plain_request();
		rq.pipelined = true; rq.half_slots = true; rq.big_slot_bytes = 1000; rq.lmax_small = 100;
		int asked = -1;
		TdWsPlan p = plan_with(rq, 0, &asked);          // no long tiles: halved
		CHECK(p.n_wave_slots == 32 && p.half_slots && asked == 0 && p.ws_bytes == 3200);
		rq.n_long = 8;                                  // 8 long tiles: 32 >= 4 * 8, halved; 32 * 100 + 8 * 900
		p = plan_with(rq, 0);
		CHECK(p.n_wave_slots == 32 && p.n_big == 8 && p.ws_bytes == 10400);
		rq.n_long = 9;                                  // 9: 32 < 36, the launch keeps its 64 slots; 64 * 100 + 9 * 900
		p = plan_with(rq, 0);
		CHECK(p.n_wave_slots == 64 && p.n_big == 9 && p.ws_bytes == 14500);
		rq.n_long = 0; rq.want_slots = 4;               // one workgroup stays one workgroup: (2 + 3) / 4 * 4 = 4
		p = plan_with(rq, 0);
		CHECK(p.n_wave_slots == 4);
		rq.want_slots = 64; rq.pipelined = false;       // the synchronous calls keep the full count
		p = plan_with(rq, 0);
		CHECK(p.n_wave_slots == 64 && p.half_slots);
	}
	// --- the second workspace.  Workspace 0 holds 16384 bytes, workspace 1 nothing; 8 slots of 128 bytes = 1024 bytes are asked of workspace 1
	{
		TdWsRequest rq = plain_request();
		rq.pipelined = true; rq.wsi = 1; rq.small_slot_bytes = rq.big_slot_bytes = 128; rq.want_slots = 8; rq.cap_ws = 16384; rq.cap_ws2 = 0;
		TdWsRequest rq0 = rq;
		rq0.wsi = 0; rq0.overlap = 0;
		int asked = -1;
		// free 2560: available 2560 + 16384, twice the need fits easily (no half_slots); 1024 > 0.4 * 2560 = 1024 fails: workspace 1 gets its
		// 1024 bytes (budget 2176)
		TdWsPlan p = plan_with(rq, 2560, &asked);
		CHECK(!p.overlap_given_up && !p.half_slots && p.alloc_bytes == 1024 && p.n_wave_slots == 8 && asked == 2);
		// free 2559: 1024 > 1023.6, refused -- the plan is workspace 0's, which holds the batch: two queries, none in the second round
		p = plan_with(rq, 2559, &asked);
		TdWsPlan p0 = plan_with(rq0, 2559);
		CHECK(p.overlap_given_up && !p0.overlap_given_up && asked == 2);
		CHECK(p.alloc_bytes == 0 && p.n_wave_slots == 8 && p.ws_bytes == 1024 && !p.half_slots && !p.no_fit);
		p0.overlap_given_up = true;
		CHECK(memcmp(&p, &p0, sizeof p) == 0);
		// on half_slots the launch has 4 slots = 512 bytes and the bound is 0.6: 0.6 * 854 = 512.4 holds it, 0.6 * 853 = 511.8 does not
		rq.half_slots = rq0.half_slots = true;
		p = plan_with(rq, 854, &asked);
		CHECK(!p.overlap_given_up && p.alloc_bytes == 512 && p.n_wave_slots == 4 && asked == 1);
		p = plan_with(rq, 853, &asked);
		p0 = plan_with(rq0, 853);
		CHECK(p.overlap_given_up && asked == 1 && p.alloc_bytes == 0 && p.n_wave_slots == 4 && p.half_slots && p.ws_bytes == 512);
		p0.overlap_given_up = true;
		CHECK(memcmp(&p, &p0, sizeof p) == 0);
		// refused with workspace 0 too small as well: the second round sizes workspace 0 (a third query), budget (int)(853 + 256) * 0.85 = 942
		rq.cap_ws = 256;
		p = plan_with(rq, 853, &asked);
		CHECK(p.overlap_given_up && asked == 2 && p.alloc_bytes == 512 && p.n_wave_slots == 4);
	}
	// --- the budget: 0.85 of (free + what the workspace holds).  One stream, nothing allocated, small slots 100 bytes, big 1000, 8 long tiles
	// (7200 bytes beyond a small slot each)
	{
		TdWsRequest rq = plain_request();
		rq.cap_ws = rq.cap_ws2 = 0; rq.n_long = 8; rq.lmax_small = 100; rq.big_slot_bytes = 1000; rq.want_slots = 128;
		int asked = -1;
		// 128 * 100 + 7200 = 20000 bytes.  free 24001: budget (int)20400.85 = 20400, no shrink
		TdWsPlan p = plan_with(rq, 24001, &asked);
		CHECK(p.n_wave_slots == 128 && p.n_big == 8 && p.ws_bytes == 20000 && p.alloc_bytes == 20000 && asked == 1 && !p.one_geometry);
		// free 20001: budget 17000 < 20000; 7200 <= 8500, the long tiles' slots survive; (17000 - 7200) / 100 = 98 -> 96 slots, 9600 + 7200
		p = plan_with(rq, 20001, &asked);
		CHECK(p.n_wave_slots == 96 && p.n_big == 8 && p.n_long == 8 && p.lmax_small == 100 && !p.one_geometry && p.ws_slot_bytes == 100 && p.ws_bytes == 16800 && p.alloc_bytes == 16800);
		// free 16001: budget 13600; 7200 > 6800: one geometry, 13600 / 1000 = 13 -> 12 slots of 1000 bytes
		p = plan_with(rq, 16001, &asked);
		CHECK(p.n_wave_slots == 12 && p.n_big == 0 && p.n_long == 0 && p.lmax_small == 150 && p.one_geometry && p.ws_slot_bytes == 1000 && p.ws_bytes == 12000 && p.alloc_bytes == 12000 && !p.no_fit);
		// free 4001: budget 3400; one geometry, 3 -> 0 slots: the failure, with the big geometry's bytes for the message
		p = plan_with(rq, 4001, &asked);
		CHECK(p.no_fit && p.one_geometry && p.ws_slot_bytes == 1000 && p.n_long == 0 && asked == 1);
		// the other failure: whole workgroups fit, the long tiles' slots do not.  wpb 1, 32 slots of 900 bytes + 8 * 100 = 29600; free 2001: budget 1700,
		// 800 <= 850 keeps the long tiles, (1700 - 800) / 900 = 1 slot < 8
		rq.wpb = 1; rq.want_slots = 32; rq.small_slot_bytes = 900;
		p = plan_with(rq, 2001, &asked);
		CHECK(p.no_fit && !p.one_geometry && p.ws_slot_bytes == 900 && p.n_big == 8);
		// a workspace that holds the batch is kept however little is free: no query
		rq.cap_ws = 29600;
		p = plan_with(rq, 0, &asked);
		CHECK(!p.no_fit && p.alloc_bytes == 0 && asked == 0 && p.n_wave_slots == 32 && p.ws_bytes == 29600);
	}
	// --- placement candidates: slots of 1 MiB on one stream, nothing allocated
	{
		const size_t GiB = (size_t)1 << 30;
		TdWsRequest rq = plain_request();
		rq.cap_ws = rq.cap_ws2 = 0; rq.n_tiles = 5000; rq.small_slot_bytes = rq.big_slot_bytes = 1 << 20;
		struct { int64_t want; int ws_candidates; size_t free_b; int n; } cases[] = {
			{ 2048, 3, 100 * GiB, 3 },   // 2 GiB exactly, 6 GiB of 60: the three that were asked for
			{ 2044, 3, 100 * GiB, 1 },   // 4 MiB below 2 GiB: one
			{ 2048, 9, 100 * GiB, 4 },   // at most 4
			{ 2048, 1, 100 * GiB, 1 },
			{ 2048, 3, 9 * GiB, 1 },     // 6 GiB > 0.6 * 9 GiB = 5.4 GiB: they would take too much of the memory (budget 7.65 GiB holds one)
			{ 2048, 3, 11 * GiB, 3 },    // 6 GiB <= 6.6 GiB
			{ 2048, 9, 11 * GiB, 1 },    // the cap comes first: 4 * 2 GiB = 8 GiB > 6.6 GiB
		};
		for (const auto& k : cases) {
			rq.want_slots = k.want; rq.ws_candidates = k.ws_candidates;
			const TdWsPlan p = plan_with(rq, k.free_b);
			CHECK(p.alloc_bytes == (size_t)k.want << 20 && p.n_candidates == k.n && p.n_wave_slots == k.want);
		}
	}
	// a memory query that fails ends the plan
	{
		TdWsRequest rq = plain_request();
		rq.cap_ws = 0;
		const TdWsPlan p = plan_workspace(rq, [](void*, size_t*) { return false; }, nullptr);
		CHECK(p.query_failed);
	}
	return 0;
}

// ---------------------------------------------------------------------------------------------------------
// (b), (c) the sweeps
// ---------------------------------------------------------------------------------------------------------
static int sweep_lengths(bool verbose)
{
	uint32_t s = 4711u;
	const int n_cases = 600;
	int64_t taken[LC_BRANCHES] = { 0, 0, 0, 0 };
	for (int q = 0; q < n_cases; q++) {
		// around 64 tiles, or a few hundred; most reads of one length with a little spread, k long ones around the 1 % of the tiles
		const int64_t n_tiles_about = rnd(s) % 3u == 0 ? 60 + rnd(s) % 10u : 64 + rnd(s) % 200u;
		const int64_t n = n_tiles_about * 64 - rnd(s) % 64u;
		const int len = 20 + (int)(rnd(s) % 200u), spread = (int)(rnd(s) % 4u);
		const int long_len = len * (120 + (int)(rnd(s) % 100u)) / 100;   // 1.2 .. 2.2 times as long
		const int64_t mark = ((n_tiles_about + 99) / 100) * 64;          // reads beyond the 99 % mark
		const int64_t k = rnd(s) % 8u == 0 ? 0 : (int64_t)(rnd(s) % (uint32_t)(2 * mark));
		std::vector<int64_t> offs{ 0 };
		int lmax = 1, lmin = 0x7fffffff;
		for (int64_t i = 0; i < n; i++) {
			const int l = rnd(s) % (uint32_t)n < (uint32_t)k ? long_len - (spread ? (int)(rnd(s) % (uint32_t)spread) : 0) : len - (spread ? (int)(rnd(s) % (uint32_t)spread) : 0);
			offs.push_back(offs.back() + l);
			if (l > lmax) lmax = l;
			if (l < lmin) lmin = l;
		}
		const int64_t n_tiles = (n + 63) / 64;
		const bool spec_ready = rnd(s) % 16u != 0, with_workspace = rnd(s) % 16u != 0;
		const int length_classes = rnd(s) % 16u != 0;
		int32_t n_long = -1, lmax_small = -1;
		int branch = -1;
		old_lengths(offs.data(), n, lmin, lmax, n_tiles, spec_ready, with_workspace, length_classes, n_long, lmax_small, branch);
		const TdLengthClasses lc = plan_length_classes(offs.data(), n, lmin, lmax, n_tiles, spec_ready && with_workspace && length_classes);
		CHECK(lc.n_long == n_long && lc.lmax_small == lmax_small);
		CHECK(lc.n_long >= 0 && lc.n_long <= n_tiles && lc.lmax_small <= lmax && (lc.n_long > 0) == (lc.lmax_small < lmax));
		taken[branch]++;
	}
	int bad = 0;
	for (int b = 0; b < LC_BRANCHES; b++) {
		if (verbose) printf("%8.2f %%  %s\n", 100.0 * (double)taken[b] / n_cases, lc_names[b]);
		if (taken[b] * 100 < n_cases) { fprintf(stderr, HOST_CHECK_NAME ": length sweep: \"%s\" in %lld of %d cases\n", lc_names[b], (long long)taken[b], n_cases); bad = 1; }
	}
	return bad;
}

// 2^(lo .. hi), evenly in the exponent
static int64_t pow2_between(uint32_t& s, int lo, int hi)
{
	const int e = lo + (int)(rnd(s) % (uint32_t)(hi - lo));
	return ((int64_t)1 << e) + (int64_t)(rnd(s) % (1u << 16)) * (((int64_t)1 << e) >> 16);
}

static int sweep_workspace(bool verbose)
{
	uint32_t s = 2718u;
	const int n_cases = 200000;
	int64_t taken[B_BRANCHES] = { 0 };
	for (int q = 0; q < n_cases; q++) {
		Old o{};
		o.spec_ready = rnd(s) % 8u != 0;
		o.n_cu = 1 << (rnd(s) % 9u);                        // 1 .. 256 compute units
		o.spec_block = 64 << (rnd(s) % 4u);                 // workgroups of 1, 2, 4 or 8 waves
		o.generic_block = 64 << (rnd(s) % 4u);
		o.spec_waves_per_cu = 4 << (rnd(s) % 3u);
		o.wave_slots_forced = rnd(s) % 4u == 0 ? 1 + (long)(rnd(s) % 600u) : 0;
		o.overlap = rnd(s) % 8u != 0;
		o.pipeline_depth = 1 + (int)(rnd(s) % 4u);
		if (rnd(s) % 4u != 0 && o.pipeline_depth == 1) o.pipeline_depth = 3;
		o.half_slots = rnd(s) % 3u == 0;
		o.pipelined = rnd(s) % 4u != 0;
		o.wsi = o.pipelined && o.overlap ? (int)(rnd(s) % 2u) : 0;
		o.ws_candidates = (int)(rnd(s) % 9u);
		o.n_tiles = (int32_t)(rnd(s) % 4u == 0 ? rnd(s) % 70u : rnd(s) % 5000u);
		o.lmax = 30 + (int)(rnd(s) % 1000u);
		// slots of 1 KiB .. 128 MiB, every other time of 4 MiB and more (a workspace of 2 GiB and more has placement candidates); the
		// specialised kernel's for the batch's longest read up to 8 times those of the many
		const int lo = rnd(s) % 2u == 0 ? 22 : 10;
		o.lay_bytes = pow2_between(s, lo, 27) & ~(int64_t)255;
		o.spec_small_bytes = pow2_between(s, lo, 27) & ~(int64_t)255;
		o.n_long = 0; o.lmax_small = o.lmax;
		o.spec_big_bytes = o.spec_small_bytes;
		const int wpb = (o.spec_ready ? o.spec_block : o.generic_block) / 64;
		int64_t slots = o.wave_slots_forced > 0 ? o.wave_slots_forced : (int64_t)o.n_cu * (o.spec_ready ? o.spec_waves_per_cu : 2 * wpb);
		if (slots > o.n_tiles) slots = o.n_tiles;
		if (slots < 1) slots = 1;
		if (rnd(s) % 2u == 0) {                             // long tiles: up to a third of the slots, so that a quarter is crossed
			o.n_long = (int32_t)(rnd(s) % (uint32_t)(slots / 3 + 2));
			if (o.n_long > 0) {
				o.lmax_small = 20 + (int)(rnd(s) % (uint32_t)(o.lmax - 20));
				o.spec_big_bytes = (o.spec_small_bytes * (int64_t)(100 + rnd(s) % 700u) / 100) & ~(int64_t)255;
			}
		}
		// memory, measured in what the batch would ask for: what the workspaces hold (nothing, or 1/8 .. 2 of it) and what is free (1/16 .. 4,
		// a quarter of the time up to 16, another quarter less than it asks for)
		const int64_t ask = slots * (o.spec_ready ? o.spec_small_bytes : o.lay_bytes) + (int64_t)o.n_long * (o.spec_big_bytes - o.spec_small_bytes);
		o.cap_ws = rnd(s) % 3u == 0 ? 0 : (size_t)(ask / 8 * (1 + rnd(s) % 16u));
		o.cap_ws2 = rnd(s) % 2u == 0 ? 0 : (size_t)(ask / 8 * (1 + rnd(s) % 16u));
		o.free_b = (size_t)(ask / 16 * (1 + rnd(s) % 64u)) + (size_t)(rnd(s) % 4096u);
		const uint32_t how_much = rnd(s) % 4u;
		if (how_much == 0) o.free_b = (size_t)(ask / 16 * (1 + rnd(s) % 256u));
		if (how_much == 1) o.free_b = (size_t)(ask / 16 * (1 + rnd(s) % 16u));

		TdWsRequest rq;
		rq.n_tiles = o.n_tiles; rq.n_long = o.n_long; rq.lmax_small = o.lmax_small; rq.lmax = o.lmax;
		rq.small_slot_bytes = o.spec_ready ? (o.n_long > 0 ? o.spec_small_bytes : o.spec_big_bytes) : o.lay_bytes;
		rq.big_slot_bytes = o.spec_ready ? o.spec_big_bytes : o.lay_bytes;
		rq.wpb = wpb;
		rq.want_slots = o.wave_slots_forced > 0 ? o.wave_slots_forced : (int64_t)o.n_cu * (o.spec_ready ? o.spec_waves_per_cu : 2 * wpb);
		rq.spec_ready = o.spec_ready; rq.pipelined = o.pipelined; rq.overlap = o.overlap; rq.pipeline_depth = o.pipeline_depth;
		rq.half_slots = o.half_slots; rq.wsi = o.wsi; rq.cap_ws = o.cap_ws; rq.cap_ws2 = o.cap_ws2; rq.ws_candidates = o.ws_candidates;
		Hbm h;
		h.free_b = o.free_b;
		const TdWsPlan p = plan_workspace(rq, hbm_free, &h);
		const int32_t n_long_in = o.n_long;
		const bool was_half = o.half_slots;
		const int rc = old_workspace(o);

		// (b) every field, and the queries
		CHECK(!p.query_failed && h.asked == o.asked);
		CHECK(p.no_fit == (rc == OLD_FAIL));
		CHECK(p.half_slots == o.half_slots && p.overlap_given_up == o.on_first_stream && (!p.overlap_given_up || (o.wsi == 0 && o.overlap == 0)));
		CHECK(p.n_long == o.n_long && p.lmax_small == o.lmax_small && p.n_big == o.n_big);
		CHECK(p.one_geometry == (o.spec_ready && n_long_in > 0 && o.n_long == 0));
		if (o.spec_ready) CHECK((p.one_geometry ? rq.big_slot_bytes : rq.small_slot_bytes) == o.slay_bytes);   // what the caller leaves in s.slay
		if (rc == OLD_FAIL) { CHECK(p.ws_slot_bytes == o.fail_slot_bytes); }
		else {
			CHECK(p.n_wave_slots == o.n_wave_slots && p.ws_slot_bytes == o.ws_slot_bytes && p.ws_bytes == o.ws_bytes);
			CHECK(p.alloc_bytes == o.need && (o.need == 0 || p.n_candidates == o.n_cand));
			// (c)
			CHECK(p.n_wave_slots % wpb == 0 && p.n_wave_slots >= wpb && p.n_wave_slots >= p.n_big);
			CHECK(p.ws_bytes == (int64_t)p.n_wave_slots * p.ws_slot_bytes + (int64_t)p.n_big * (rq.big_slot_bytes - rq.small_slot_bytes));
			const size_t cap = (p.overlap_given_up ? 0 : rq.wsi) ? rq.cap_ws2 : rq.cap_ws;
			if (p.alloc_bytes > 0) {
				const int64_t budget = (int64_t)((double)(o.free_b + cap) * 0.85);
				CHECK(p.alloc_bytes == (size_t)p.ws_bytes && p.ws_bytes <= ((int64_t)cap > budget ? (int64_t)cap : budget));
			} else CHECK((size_t)p.ws_bytes <= cap);
			CHECK(!was_half || p.half_slots);
		}
		for (int b = 0; b < B_BRANCHES; b++) taken[b] += o.hit[b];
	}
	int bad = 0;
	for (int b = 0; b < B_BRANCHES; b++) {
		if (verbose) printf("%8.2f %%  %s\n", 100.0 * (double)taken[b] / n_cases, b_names[b]);
		if (taken[b] * 100 < n_cases) { fprintf(stderr, HOST_CHECK_NAME ": workspace sweep: \"%s\" in %lld of %d cases\n", b_names[b], (long long)taken[b], n_cases); bad = 1; }
	}
	return bad;
}

// ---------------------------------------------------------------------------------------------------------
// the egress plan
// ---------------------------------------------------------------------------------------------------------
// the caller's three output buffers as the plan gets to see them: page-locked or not, and which of them it asked about, in order
struct Pins { bool pinned[3] = { false, false, false }; int asked[8] = { 0 }; int n_asked = 0; };
static bool page_locked(void* arg, int k) { Pins* q = (Pins*)arg; if (q->n_asked < 8) q->asked[q->n_asked] = k; q->n_asked++; return q->pinned[k]; }

// slot_fetch_begin() / slot_issue_copies() / slot_fetch_end() as they stood in td_api.hip, as far as they decide and count: the
// context and the slot as plain integers in, every ensure()d size, every copy and every host-side step out
enum { ACT_NONE, ACT_COPY, ACT_REBUILD, ACT_EXPAND };
struct OldEg {
	// context and slot
	int compact_egress, rle_cap_forced, S, H;
	int64_t n_reads, n_bases; int32_t nw1, n_tiles, runs_cap; bool raw_host;
	bool u_res, u_seq, u_labels;            // the caller passed a buffer
	bool pinned[3];
	// slot_fetch_begin
	bool use_keep, use_rle, res_direct, seq_direct, lab_direct; int32_t rle_cap;
	size_t d_res, d_seq, d_lab, h_res, h_seq, h_lab, d_keepo, h_keepo, d_rle, h_rle;   // bytes ensure()d (NOT: the buffer was not asked for)
	size_t rle_flag, runs_flag; bool sb_rle_out, sb_runs;
	int asked[8], n_asked;
	// slot_issue_copies: bytes per output, and whether the compact buffers were the source
	size_t copy[3]; bool copy_compact[3], copy_direct[3];
	// slot_fetch_end, host side
	int act[3]; size_t act_bytes[3];
};
static const size_t NOT = (size_t)-1;
static bool old_pinned(OldEg& o, int k) { if (o.n_asked < 8) o.asked[o.n_asked] = k; o.n_asked++; return o.pinned[k]; }
static int old_rle_capacity(const OldEg& o)
{
	int cap = o.S + 2 < o.H ? o.S + 2 : o.H;
	if (o.rle_cap_forced > 0) cap = o.rle_cap_forced;
	return cap;
}

static void old_egress(OldEg& o)
{
	o.use_keep = o.use_rle = o.res_direct = o.seq_direct = o.lab_direct = false; o.rle_cap = 0;
	o.d_res = o.d_seq = o.d_lab = o.h_res = o.h_seq = o.h_lab = o.d_keepo = o.h_keepo = o.d_rle = o.h_rle = NOT;
	o.rle_flag = o.runs_flag = 0; o.sb_rle_out = o.sb_runs = false; o.n_asked = 0;
	for (int k = 0; k < 3; k++) { o.copy[k] = 0; o.copy_compact[k] = o.copy_direct[k] = false; o.act[k] = ACT_NONE; o.act_bytes[k] = 0; }
	// --- slot_fetch_begin
	const int64_t n = o.n_reads;
	if (n == 0) return;
	const size_t res_bytes = (size_t)n * 32, seq_bytes = (size_t)o.n_bases, lab_bytes = (size_t)(o.n_bases + n);
	const bool compact = o.compact_egress != 0;
	o.use_keep = compact && o.u_seq && seq_bytes && o.raw_host;
	o.use_rle = compact && o.u_labels;
	o.rle_cap = o.runs_cap > 0 ? o.runs_cap : old_rle_capacity(o);
	if (o.u_res) o.d_res = res_bytes;
	if (o.u_seq && !o.use_keep) o.d_seq = seq_bytes;
	if (o.u_labels && !o.use_rle) o.d_lab = lab_bytes;
	if (o.u_res && !(o.res_direct = old_pinned(o, 0))) o.h_res = res_bytes;
	if (o.u_seq && !o.use_keep && !(o.seq_direct = old_pinned(o, 1))) o.h_seq = seq_bytes;
	if (o.u_labels && !o.use_rle && !(o.lab_direct = old_pinned(o, 2))) o.h_lab = lab_bytes;
	const size_t keepo_bytes = (size_t)n * (size_t)o.nw1 * 4, rle_bytes = ((size_t)n * (size_t)o.rle_cap + 2) * 4;
	if (o.use_keep) o.d_keepo = o.h_keepo = keepo_bytes;
	if (o.use_rle) { o.d_rle = o.h_rle = rle_bytes; o.rle_flag = (size_t)n * (size_t)o.rle_cap; }
	o.sb_rle_out = o.use_rle;
	o.sb_runs = o.use_rle && o.runs_cap > 0;
	if (o.sb_runs) o.runs_flag = (size_t)o.n_tiles * (size_t)o.runs_cap * 64;
	// --- slot_issue_copies
	if (o.u_res) { o.copy[0] = res_bytes; o.copy_direct[0] = o.res_direct; }
	if (o.u_seq && seq_bytes) {
		if (o.use_keep) { o.copy[1] = (size_t)n * (size_t)o.nw1 * 4; o.copy_compact[1] = true; }
		else { o.copy[1] = seq_bytes; o.copy_direct[1] = o.seq_direct; }
	}
	if (o.u_labels) {
		if (o.use_rle) { o.copy[2] = ((size_t)n * (size_t)o.rle_cap + 1) * 4; o.copy_compact[2] = true; }
		else { o.copy[2] = lab_bytes; o.copy_direct[2] = o.lab_direct; }
	}
	// --- slot_fetch_end, the run table did not overflow
	if (o.u_res && !o.res_direct) { o.act[0] = ACT_COPY; o.act_bytes[0] = (size_t)n * 32; }
	if (o.u_seq && o.n_bases) {
		if (o.use_keep) o.act[1] = ACT_REBUILD;
		else if (!o.seq_direct) { o.act[1] = ACT_COPY; o.act_bytes[1] = (size_t)o.n_bases; }
	}
	if (o.u_labels) {
		if (o.use_rle) o.act[2] = ACT_EXPAND;
		else if (!o.lab_direct) { o.act[2] = ACT_COPY; o.act_bytes[2] = (size_t)(o.n_bases + n); }
	}
}

// ... and slot_fetch_end's fall-back when it did (only reached with use_rle): the labels as they are, in a copy of their own
static void old_overflow(OldEg& o)
{
	const size_t lab_bytes = (size_t)(o.n_bases + o.n_reads);
	o.d_lab = lab_bytes;
	o.n_asked = 0;
	if (!(o.lab_direct = old_pinned(o, 2))) o.h_lab = lab_bytes;
	o.copy[2] = lab_bytes; o.copy_compact[2] = false; o.copy_direct[2] = o.lab_direct;
	o.use_rle = false;
	o.act[2] = ACT_NONE; o.act_bytes[2] = 0;
	if (!o.lab_direct) { o.act[2] = ACT_COPY; o.act_bytes[2] = lab_bytes; }
}

// what td_batch.hip's walk over the channels does on the host with channel k of a plan
static int plan_act(const TdEgressPlan& p, int k, size_t& bytes)
{
	const TdEgressChannel& ch = p.ch[k];
	bytes = 0;
	if (!ch.copy_bytes) return ACT_NONE;
	if (ch.form == TD_EG_STAGED) { bytes = ch.copy_bytes; return ACT_COPY; }
	if (ch.form == TD_EG_COMPACT) return k == TD_CH_SEQ ? ACT_REBUILD : ACT_EXPAND;
	return ACT_NONE;
}

static bool channel_is(const TdEgressChannel& ch, int form, size_t copy_bytes, size_t alloc_bytes)
{
	return ch.form == form && ch.copy_bytes == copy_bytes && ch.alloc_bytes == alloc_bytes;
}

static int egress_by_hand()
{
	// 65 reads of 40 bases: 2600 bases, nw1 = (40 + 31) / 32 = 2 keep words per read, 2 tiles; a model with S + 2 = 7 < H: 7 runs per read.
	// Records are 32 bytes: 65 * 32 = 2080.  Labels as plain bytes: 2600 + 65 = 2665.
	TdEgressRequest rq;
	rq.n_reads = 65; rq.n_bases = 2600; rq.nw1 = 2; rq.n_tiles = 2;
	rq.want[0] = rq.want[1] = rq.want[2] = true;
	rq.compact_egress = true; rq.raw_host = true; rq.runs_cap = 7; rq.rle_capacity = 7;
	// all three pageable, compact: the records through staging (the one plain channel, the one question); keep bits 65 * 2 * 4 = 520 bytes;
	// runs 65 * 7 = 455 words, the flag is word 455, 456 words = 1824 bytes travel, 457 words = 1828 bytes are allocated; the decode
	// kernel's own table has 2 * 7 * 64 = 896 words in front of its flag
	{
		Pins q;
		const TdEgressPlan p = plan_egress(rq, page_locked, &q);
		CHECK(channel_is(p.ch[TD_CH_RES], TD_EG_STAGED, 2080, 2080) && channel_is(p.ch[TD_CH_SEQ], TD_EG_COMPACT, 520, 520) && channel_is(p.ch[TD_CH_LAB], TD_EG_COMPACT, 1824, 1828));
		CHECK(p.rle_cap == 7 && p.rle_flag_word == 455 && p.finish_reads_runs && p.runs_flag_word == 896 && p.lab_plain_bytes == 2665);
		CHECK(q.n_asked == 1 && q.asked[0] == TD_CH_RES);
		// a read overflowed the table, the caller's label buffer is page-locked: 2665 bytes straight into it, one question
		TdEgressPlan p2 = p;
		Pins q2;
		q2.pinned[TD_CH_LAB] = true;
		plan_labels_plain(p2, page_locked, &q2);
		CHECK(channel_is(p2.ch[TD_CH_LAB], TD_EG_DIRECT, 2665, 2665) && q2.n_asked == 1 && q2.asked[0] == TD_CH_LAB);
		CHECK(memcmp(&p2.ch[TD_CH_RES], &p.ch[TD_CH_RES], sizeof p.ch[0]) == 0 && memcmp(&p2.ch[TD_CH_SEQ], &p.ch[TD_CH_SEQ], sizeof p.ch[0]) == 0 && p2.rle_cap == 7);
	}
	// the input was page-locked and read by the DMA engine, no "stable_input": the host has no copy to rebuild from, no keep bits -- the
	// sequences as plain bytes through staging, and a second question
	{
		TdEgressRequest r = rq;
		r.raw_host = false;
		Pins q;
		const TdEgressPlan p = plan_egress(r, page_locked, &q);
		CHECK(channel_is(p.ch[TD_CH_RES], TD_EG_STAGED, 2080, 2080) && channel_is(p.ch[TD_CH_SEQ], TD_EG_STAGED, 2600, 2600) && channel_is(p.ch[TD_CH_LAB], TD_EG_COMPACT, 1824, 1828));
		CHECK(q.n_asked == 2 && q.asked[0] == TD_CH_RES && q.asked[1] == TD_CH_SEQ);
	}
	// the generic kernel left no runs (runs_cap = 0): the finish kernel scans them from the labels into a table of rle_capacity = 7
	{
		TdEgressRequest r = rq;
		r.runs_cap = 0;
		Pins q;
		const TdEgressPlan p = plan_egress(r, page_locked, &q);
		CHECK(channel_is(p.ch[TD_CH_LAB], TD_EG_COMPACT, 1824, 1828) && p.rle_cap == 7 && p.rle_flag_word == 455 && !p.finish_reads_runs && p.runs_flag_word == 0);
		CHECK(channel_is(p.ch[TD_CH_SEQ], TD_EG_COMPACT, 520, 520) && q.n_asked == 1);
		// with the table forced to one entry (the tests' overflow route): 65 words of runs, 66 travel, 67 are allocated
		r.rle_capacity = 1;
		const TdEgressPlan p1 = plan_egress(r, page_locked, &q);
		CHECK(channel_is(p1.ch[TD_CH_LAB], TD_EG_COMPACT, 264, 268) && p1.rle_cap == 1 && p1.rle_flag_word == 65);
	}
	// results only, into a page-locked buffer: one direct copy, nothing else planned
	{
		TdEgressRequest r = rq;
		r.want[TD_CH_SEQ] = r.want[TD_CH_LAB] = false;
		Pins q;
		q.pinned[TD_CH_RES] = true;
		const TdEgressPlan p = plan_egress(r, page_locked, &q);
		CHECK(channel_is(p.ch[TD_CH_RES], TD_EG_DIRECT, 2080, 2080) && channel_is(p.ch[TD_CH_SEQ], TD_EG_NONE, 0, 0) && channel_is(p.ch[TD_CH_LAB], TD_EG_NONE, 0, 0));
		CHECK(p.rle_flag_word == 0 && !p.finish_reads_runs && p.runs_flag_word == 0 && q.n_asked == 1 && q.asked[0] == TD_CH_RES);
	}
	// 65 reads of no bases (nw1 = 1, nothing staged on the host): the sequences stay plain -- buffers of no bytes, no copy, but the
	// question is asked; labels are one entry per read, 65 * 7 runs all the same
	{
		TdEgressRequest r = rq;
		r.n_bases = 0; r.nw1 = 1; r.raw_host = false;
		Pins q;
		q.pinned[TD_CH_SEQ] = true;
		const TdEgressPlan p = plan_egress(r, page_locked, &q);
		CHECK(channel_is(p.ch[TD_CH_SEQ], TD_EG_DIRECT, 0, 0) && channel_is(p.ch[TD_CH_LAB], TD_EG_COMPACT, 1824, 1828) && p.lab_plain_bytes == 65);
		CHECK(q.n_asked == 2 && q.asked[1] == TD_CH_SEQ);
		r.raw_host = true;   // (even if the host had them)
		const TdEgressPlan pr = plan_egress(r, page_locked, &q);
		CHECK(channel_is(pr.ch[TD_CH_SEQ], TD_EG_DIRECT, 0, 0));
	}
	// no reads: nothing is planned and nothing asked
	{
		TdEgressRequest r = rq;
		r.n_reads = 0; r.n_bases = 0; r.n_tiles = 0;
		Pins q;
		const TdEgressPlan p = plan_egress(r, page_locked, &q);
		const TdEgressPlan none;
		CHECK(q.n_asked == 0 && p.rle_cap == 0 && p.rle_flag_word == 0 && p.runs_flag_word == 0 && !p.finish_reads_runs && p.lab_plain_bytes == 0);
		for (int k = 0; k < TD_N_CHANNELS; k++) CHECK(channel_is(p.ch[k], TD_EG_NONE, 0, 0) && channel_is(none.ch[k], TD_EG_NONE, 0, 0));
	}
	return 0;
}

// one plan against the restatement: every field, the questions, and what holds for any plan (c)
static int egress_agrees(const TdEgressPlan& p, const Pins& q, const OldEg& o)
{
	const bool wanted[3] = { o.u_res, o.u_seq, o.u_labels }, compact[3] = { false, o.use_keep, o.use_rle }, direct[3] = { o.res_direct, o.seq_direct, o.lab_direct };
	const size_t dev_plain[3] = { o.d_res, o.d_seq, o.d_lab }, host_plain[3] = { o.h_res, o.h_seq, o.h_lab };
	const size_t dev_compact[3] = { NOT, o.d_keepo, o.d_rle }, host_compact[3] = { NOT, o.h_keepo, o.h_rle };
	const size_t user_bytes[3] = { (size_t)o.n_reads * 32, (size_t)o.n_bases, (size_t)(o.n_bases + o.n_reads) };   // the caller's buffers, by the ABI
	CHECK(q.n_asked == o.n_asked && q.n_asked <= 3);
	for (int j = 0; j < q.n_asked; j++) CHECK(q.asked[j] == o.asked[j]);
	for (int k = 0; k < 3; k++) {
		const TdEgressChannel& ch = p.ch[k];
		const bool planned = o.n_reads > 0 && wanted[k];
		const int form = !planned ? TD_EG_NONE : compact[k] ? TD_EG_COMPACT : direct[k] ? TD_EG_DIRECT : TD_EG_STAGED;
		CHECK(ch.form == form && ch.copy_bytes == o.copy[k]);
		CHECK(o.copy[k] == 0 || (o.copy_compact[k] == (form == TD_EG_COMPACT) && o.copy_direct[k] == (form == TD_EG_DIRECT)));
		// the buffers: exactly those of the channel's form, of the plan's size
		const bool is_plain = form == TD_EG_DIRECT || form == TD_EG_STAGED;
		CHECK((dev_plain[k] != NOT) == is_plain && (host_plain[k] != NOT) == (form == TD_EG_STAGED));
		CHECK((dev_compact[k] != NOT) == (form == TD_EG_COMPACT) && (host_compact[k] != NOT) == (form == TD_EG_COMPACT));
		if (is_plain) CHECK(ch.alloc_bytes == dev_plain[k] && (form == TD_EG_DIRECT || ch.alloc_bytes == host_plain[k]));
		if (form == TD_EG_COMPACT) CHECK(ch.alloc_bytes == dev_compact[k] && ch.alloc_bytes == host_compact[k]);
		if (form == TD_EG_NONE) CHECK(ch.alloc_bytes == 0 && ch.copy_bytes == 0);
		size_t bytes = 0;
		CHECK(plan_act(p, k, bytes) == o.act[k] && bytes == o.act_bytes[k]);
		// (c) a copy stays inside its source and its destination
		CHECK(ch.copy_bytes <= ch.alloc_bytes && (form != TD_EG_DIRECT || ch.copy_bytes <= user_bytes[k]));
		CHECK(form != TD_EG_STAGED || bytes <= user_bytes[k]);
	}
	CHECK(p.rle_cap == o.rle_cap && p.rle_flag_word == o.rle_flag && p.finish_reads_runs == o.sb_runs && p.runs_flag_word == o.runs_flag);
	CHECK((p.ch[TD_CH_LAB].form == TD_EG_COMPACT) == o.sb_rle_out);
	CHECK(p.lab_plain_bytes == (o.n_reads > 0 ? user_bytes[2] : 0));
	// (c) the flags lie inside what is allocated -- the run table's also inside what travels, the host reads it from there; the decode
	// kernel's table is (n_tiles * runs_cap * 64 + 1) words (slot_decode)
	if (p.ch[TD_CH_LAB].form == TD_EG_COMPACT) CHECK((p.rle_flag_word + 1) * 4 <= p.ch[TD_CH_LAB].copy_bytes && (p.rle_flag_word + 1) * 4 <= p.ch[TD_CH_LAB].alloc_bytes);
	if (p.finish_reads_runs) CHECK(o.runs_cap > 0 && (p.runs_flag_word + 1) * 4 <= ((size_t)o.n_tiles * (size_t)o.runs_cap * 64 + 1) * 4);
	return 0;
}

static int sweep_egress(bool verbose)
{
	int64_t taken[3][4] = { { 0 } };
	int n_cases = 0;
	const int64_t reads[4] = { 0, 1, 64, 65 };
	for (int bits = 0; bits < 1 << 11; bits++) for (int ri = 0; ri < 4; ri++) {
		OldEg o{};
		o.u_res = bits & 1; o.u_seq = bits >> 1 & 1; o.u_labels = bits >> 2 & 1;
		o.pinned[0] = bits >> 3 & 1; o.pinned[1] = bits >> 4 & 1; o.pinned[2] = bits >> 5 & 1;
		o.compact_egress = bits >> 6 & 1; o.raw_host = bits >> 7 & 1;
		o.S = 5; o.H = 9;                                   // rle_capacity: 7 ...
		o.runs_cap = bits >> 8 & 1 ? 5 : 0;                 // (a launch that ran under another setting of the option left 5)
		o.rle_cap_forced = bits >> 9 & 1 ? 1 : 0;           // ... or the forced 1
		const int len = bits >> 10 & 1 ? 40 : 0;
		o.n_reads = reads[ri]; o.n_bases = o.n_reads * len; o.nw1 = ((len > 1 ? len : 1) + 31) / 32; o.n_tiles = (int32_t)((o.n_reads + 63) / 64);
		TdEgressRequest rq;
		rq.n_reads = o.n_reads; rq.n_bases = o.n_bases; rq.nw1 = o.nw1; rq.n_tiles = o.n_tiles;
		rq.want[TD_CH_RES] = o.u_res; rq.want[TD_CH_SEQ] = o.u_seq; rq.want[TD_CH_LAB] = o.u_labels;
		rq.compact_egress = o.compact_egress != 0; rq.raw_host = o.raw_host; rq.runs_cap = o.runs_cap; rq.rle_capacity = old_rle_capacity(o);
		Pins q;
		for (int k = 0; k < 3; k++) q.pinned[k] = o.pinned[k];
		TdEgressPlan p = plan_egress(rq, page_locked, &q);
		old_egress(o);
		if (egress_agrees(p, q, o)) { fprintf(stderr, HOST_CHECK_NAME ": egress sweep: case %d, %lld reads\n", bits, (long long)o.n_reads); return 1; }
		for (int k = 0; k < 3; k++) taken[k][p.ch[k].form]++;
		n_cases++;
		if (o.use_rle) {   // the run table overflowed: the label channel planned again, everything else as it was
			const TdEgressPlan before = p;
			Pins q2;
			for (int k = 0; k < 3; k++) q2.pinned[k] = o.pinned[k];
			plan_labels_plain(p, page_locked, &q2);
			old_overflow(o);
			CHECK(q2.n_asked == 1 && o.n_asked == 1 && q2.asked[0] == o.asked[0]);
			const TdEgressChannel& L = p.ch[TD_CH_LAB];
			CHECK(L.form == (o.lab_direct ? TD_EG_DIRECT : TD_EG_STAGED) && L.copy_bytes == o.copy[2] && L.alloc_bytes == o.d_lab && (o.lab_direct || L.alloc_bytes == o.h_lab));
			size_t bytes = 0;
			CHECK(plan_act(p, TD_CH_LAB, bytes) == o.act[2] && bytes == o.act_bytes[2] && L.copy_bytes <= L.alloc_bytes && L.copy_bytes <= (size_t)(o.n_bases + o.n_reads));
			CHECK(memcmp(&p.ch[TD_CH_RES], &before.ch[TD_CH_RES], sizeof p.ch[0]) == 0 && memcmp(&p.ch[TD_CH_SEQ], &before.ch[TD_CH_SEQ], sizeof p.ch[0]) == 0 && p.rle_cap == before.rle_cap);
		}
	}
	static const char* const ch_names[3] = { "results", "sequences", "labels" };
	static const char* const form_names[4] = { "none", "compact", "direct", "staged" };
	int bad = 0;
	for (int k = 0; k < 3; k++) for (int f = 0; f < 4; f++) {
		if (k == TD_CH_RES && f == TD_EG_COMPACT) { if (taken[k][f]) bad = 1; continue; }   // (the records have no compact form)
		if (verbose) printf("%8.2f %%  %s %s\n", 100.0 * (double)taken[k][f] / n_cases, ch_names[k], form_names[f]);
		if (taken[k][f] * 100 < n_cases) { fprintf(stderr, HOST_CHECK_NAME ": egress sweep: %s %s in %lld of %d cases\n", ch_names[k], form_names[f], (long long)taken[k][f], n_cases); bad = 1; }
	}
	return bad;
}

int main(int argc, char** argv)
{
	const bool verbose = argc > 1 && strcmp(argv[1], "-v") == 0;   // -v: the share of the swept cases that takes each branch
	if (by_hand() || sweep_lengths(verbose) || sweep_workspace(verbose) || egress_by_hand() || sweep_egress(verbose)) return 1;
	printf("batch_plan_host_check: ok\n");
	return 0;
}
