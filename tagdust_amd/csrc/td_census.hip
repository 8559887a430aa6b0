// td_census.hip -- the census of barcode spellings (include/tagdust_census.h): what stood where the barcode should have been.
//
// Behind every TD_MODE_GET_LABEL launch of a context with the census on, one small kernel reads what the decode kernel left in
// device order -- the outcome, the lane-interleaved label bytes, the packed bases with their N mask -- builds each eligible read's
// word for the chosen 'B' segment and counts it in an open-addressing table in HBM.  One read per lane, one tile per wave, like
// the decode kernels.  Lanes of a wave that hold the same key leave as one probe and one add of their number; the distinct keys
// of a wave probe side by side.  Nothing is ever removed from the table and the probe window is fixed, so a key finds or claims
// its slot on every attempt or fails on every attempt: a reported count is exact, what did not fit is in the overflow tally.
// td_census_host is the same definition over host arrays (no GPU), td_census_merge adds two results.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tagdust_census.h"
#include "td_ctx.h"

typedef kt_u64 cs_u64;

#define CS_BLOCK KT_BLOCK
#define CS_WAVES KT_WAVES

__global__ __launch_bounds__(CS_BLOCK) void td_census_count_kernel(const TdCensusArgs a)
{
	// per label: 1 = the segment, 2 = a later segment, 0 = an earlier one
	__shared__ uint8_t s_cls[128];
	for (int h = threadIdx.x; h < 128; h += CS_BLOCK) {
		uint8_t v = 0;
		if (h < a.H) { const int seg = a.label[h] & 0xFFFF; v = seg == a.segment ? 1 : (seg > a.segment ? 2 : 0); }
		s_cls[h] = v;
	}
	__syncthreads();
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int tile = blockIdx.x * CS_WAVES + (threadIdx.x >> 6);
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
	int tmax = len;
	for (int o = 32; o >= 1; o >>= 1) { const int t2 = __shfl_xor(tmax, o); tmax = t2 > tmax ? t2 : tmax; }
	if (tmax > a.lmax) tmax = a.lmax;                 // (the batch's longest read: every index below stays inside the tile's arrays)
	const uint32_t* pk = a.packed + (int64_t)tile * (a.nw2 + a.nw1) * TD_WAVE + lane;
	const int8_t* lb = a.labels + (int64_t)tile * (a.lmax + 1) * TD_WAVE + lane;

	cs_u64 w = 0ull;
	int n = 0;
	bool has_n = false, active = elig && len > 0;
	uint32_t w2 = 0u, wn = 0u;                        // the 16 bases / the 32 N flags around p (a lane is active from p = 0 on)
	for (int p = 0; p < tmax; p++) {
		if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
		if (active) {
			if ((p & 15) == 0) w2 = pk[(p >> 4) * TD_WAVE];
			if ((p & 31) == 0) wn = pk[(a.nw2 + (p >> 5)) * TD_WAVE];
			const uint32_t lab = (uint8_t)lb[(p + 1) * TD_WAVE];     // labels[p + 1] belongs to base p
			const uint32_t cls = lab < 128u ? s_cls[lab] : 0u;
			if (cls == 1u) {
				n++;
				if (n <= TD_CENSUS_MAX_WORD) {
					w = (w << 2) | (cs_u64)((w2 >> (2 * (p & 15))) & 3u);
					has_n = has_n || ((wn >> (p & 31)) & 1u) != 0u;
				}
			} else if (cls == 2u && a.ordered) active = false;       // the path has left the segment for good
			if (p + 1 >= len) active = false;
		}
	}
	const bool is_empty = elig && n == 0, is_long = elig && n > TD_CENSUS_MAX_WORD;
	const bool is_n = elig && !is_empty && !is_long && has_n;
	const bool has_key = elig && !is_empty && !is_long && !has_n;
	const cs_u64 key = has_key ? (((cs_u64)n << 56) | w) : 0ull;

	// lanes with the same key leave as one, the wave's distinct keys probe side by side (td_keytable.h)
	const int mine = kt_wave_merge(has_key, key, lane);
	bool placed = false, fresh = false;
	kt_probe_add(a.table, key, mine, placed, fresh);
	// tallies: one add per wave and tally
	const int n_elig = __builtin_popcountll(__builtin_amdgcn_ballot_w64(elig));
	const int n_empty = __builtin_popcountll(__builtin_amdgcn_ballot_w64(is_empty));
	const int n_long = __builtin_popcountll(__builtin_amdgcn_ballot_w64(is_long));
	const int n_n = __builtin_popcountll(__builtin_amdgcn_ballot_w64(is_n));
	const int n_fresh = __builtin_popcountll(__builtin_amdgcn_ballot_w64(fresh));
	const int n_counted = kt_wave_sum(placed ? mine : 0);
	const int n_over = kt_wave_sum(placed ? 0 : mine);
	if (lane == 0) {
		atomicAdd(&a.tallies[TDC_ELIGIBLE], (cs_u64)n_elig);
		if (n_counted) atomicAdd(&a.tallies[TDC_COUNTED], (cs_u64)n_counted);
		if (n_empty) atomicAdd(&a.tallies[TDC_EMPTY], (cs_u64)n_empty);
		if (n_long) atomicAdd(&a.tallies[TDC_LONG], (cs_u64)n_long);
		if (n_n) atomicAdd(&a.tallies[TDC_N], (cs_u64)n_n);
		if (n_over) atomicAdd(&a.tallies[TDC_OVERFLOW], (cs_u64)n_over);
		if (n_fresh) atomicAdd(&a.tallies[TDC_DISTINCT], (cs_u64)n_fresh);
	}
}

hipError_t td_census_launch_count(const TdCensusArgs& a, hipStream_t stream)
{
	if (a.n_tiles <= 0) return hipSuccess;
	const unsigned blocks = (unsigned)((a.n_tiles + CS_WAVES - 1) / CS_WAVES);
	hipLaunchKernelGGL(td_census_count_kernel, dim3(blocks), dim3(CS_BLOCK), 0, stream, a);
	return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------
// (td_census.h: shared with td_molecules.hip)
bool census_entry_before(const td_census_entry& x, const td_census_entry& y) { return x.count != y.count ? x.count > y.count : x.key < y.key; }

td_census_entry* census_copy_entries(const std::vector<td_census_entry>& v)
{
	td_census_entry* p = (td_census_entry*)malloc(sizeof(td_census_entry) * (v.size() ? v.size() : 1));
	if (p && !v.empty()) memcpy(p, v.data(), sizeof(td_census_entry) * v.size());
	return p;
}

// keys (any order, repeated) -> entries in the order of td_census_get
void census_tally_keys(std::vector<uint64_t>& keys, std::vector<td_census_entry>& out)
{
	std::sort(keys.begin(), keys.end());
	for (size_t i = 0; i < keys.size();) {
		size_t j = i;
		while (j < keys.size() && keys[j] == keys[i]) j++;
		out.push_back(td_census_entry{ keys[i], (int64_t)(j - i) });
		i = j;
	}
	std::sort(out.begin(), out.end(), census_entry_before);
}

namespace {

// the segment a census of this model counts: `segment` itself when it is a 'B' segment, the last 'B' segment for -1
bool pick_segment(const td_model_desc* m, int32_t segment, int32_t& out, std::string& why)
{
	if (!m || m->S < 1 || !m->seg_type || !m->label) { why = "no model"; return false; }
	int last = -1;
	for (int j = 0; j < m->S; j++) if (m->seg_type[j] == 'B') last = j;
	if (last < 0) { why = "the model has no 'B' segment: there is no barcode to take a census of"; return false; }
	if (segment == -1) { out = last; return true; }
	if (segment < 0 || segment >= m->S) { why = "segment " + std::to_string(segment) + " is out of range (0.." + std::to_string(m->S - 1) + ", or -1 for the last 'B' segment)"; return false; }
	if (m->seg_type[segment] != 'B') { why = "segment " + std::to_string(segment) + " is a '" + std::string(1, (char)m->seg_type[segment]) + "' segment, not a 'B' segment"; return false; }
	out = segment;
	return true;
}

bool mask_ok(uint32_t mask) { return mask != 0u && mask <= 0xFFu; }

}   // namespace

void census_release(td_ctx* c)
{
	TdCensusState& z = c->census;
	void* p[] = { z.d_label, z.d_keys, z.d_counts, z.d_tallies };
	for (void* q : p) if (q) (void)hipFree(q);
	hipEvent_t ev[] = { z.ev_c0, z.ev_c1 };
	for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
	z = TdCensusState();
}

int census_count_slot(td_ctx* c, TdSlot& s, const int32_t* out_type, const int8_t* labels)
{
	const TdCensusState& z = c->census;
	TdCensusArgs a{};
	a.packed = s.d_packed; a.lens = s.d_lens; a.out_type = out_type; a.labels = labels; a.label = z.d_label;
	a.n_reads = s.n_reads; a.n_tiles = s.n_tiles; a.lmax = s.lmax; a.nw2 = s.nw2; a.nw1 = s.nw1; a.H = z.H;   // (both decode kernels write labels with the stride of s.lmax)
	a.segment = z.segment; a.ordered = z.ordered ? 1 : 0; a.mask = z.mask;
	const uint64_t n_slots = 1ull << z.log2_slots;
	a.table.slot_mask = (uint32_t)(n_slots - 1);
	a.table.window = (uint32_t)std::min<uint64_t>(n_slots, KT_PROBE_WINDOW);
	a.table.keys = z.d_keys; a.table.counts = z.d_counts; a.tallies = z.d_tallies;
	HIPCHK(c, hipEventRecord(z.ev_c0, s.cs));
	HIPCHK(c, td_census_launch_count(a, s.cs));
	HIPCHK(c, hipEventRecord(z.ev_c1, s.cs));
	// the finish kernel waits for ev_hits: a slot whose batch has been waited for is no longer read by this count either
	HIPCHK(c, hipEventRecord(s.ev_hits, s.cs));
	s.hits_queued = true;
	return TD_OK;
}

extern "C" int td_census_enable(td_ctx* c, int32_t segment, uint32_t outcome_mask, int32_t log2_slots)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_census_enable: no model uploaded");
	for (int k = 0; k < TD_MAX_PIPELINE; k++)
		if (c->slots[k].ticket) return fail(c, "td_census_enable: td_submit tickets are outstanding (td_wait them first)");
	int32_t seg = -1;
	std::string why;
	if (!pick_segment(&c->model.d, segment, seg, why)) return fail(c, "td_census_enable: %s", why.c_str());
	if (!mask_ok(outcome_mask)) return fail(c, "td_census_enable: outcome_mask 0x%x is not a non-empty subset of bits 0..7", outcome_mask);
	if (log2_slots < 4 || log2_slots > 26) return fail(c, "td_census_enable: log2_slots = %d (4..26 supported)", log2_slots);
	if (c->match_len > 0) return fail(c, "td_census_enable: a -start/-end window is set (td_set_window): labels behind a window do not spell the barcode");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	census_release(c);
	TdCensusState& z = c->census;
	const td_model_desc& m = c->model.d;
	const size_t n_slots = (size_t)1 << log2_slots;
	bool ok = hipMalloc((void**)&z.d_label, sizeof(int32_t) * (size_t)m.H) == hipSuccess &&
	          hipMalloc((void**)&z.d_keys, sizeof(cs_u64) * n_slots) == hipSuccess &&
	          hipMalloc((void**)&z.d_counts, sizeof(cs_u64) * n_slots) == hipSuccess &&
	          hipMalloc((void**)&z.d_tallies, sizeof(cs_u64) * TDC_TALLY_WORDS) == hipSuccess &&
	          hipMemcpy(z.d_label, m.label, sizeof(int32_t) * (size_t)m.H, hipMemcpyHostToDevice) == hipSuccess &&
	          hipMemset(z.d_keys, 0, sizeof(cs_u64) * n_slots) == hipSuccess &&
	          hipMemset(z.d_counts, 0, sizeof(cs_u64) * n_slots) == hipSuccess &&
	          hipMemset(z.d_tallies, 0, sizeof(cs_u64) * TDC_TALLY_WORDS) == hipSuccess &&
	          hipEventCreate(&z.ev_c0) == hipSuccess && hipEventCreate(&z.ev_c1) == hipSuccess;
	if (!ok) {
		const std::string e = hipGetErrorString(hipGetLastError());
		census_release(c);
		return fail(c, "td_census_enable: a table of 2^%d slots could not be set up: %s", log2_slots, e.c_str());
	}
	z.segment = seg; z.mask = outcome_mask; z.log2_slots = log2_slots; z.H = m.H;
	z.ordered = true;
	for (int h = 0; h + 1 < m.H; h++) if ((m.label[h] & 0xFFFF) > (m.label[h + 1] & 0xFFFF)) z.ordered = false;
	z.on = true;
	return TD_OK;
}

extern "C" int td_census_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	if (!c->census.on) return TD_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	census_release(c);
	return TD_OK;
}

extern "C" int td_census_reset(td_ctx* c)
{
	if (!c) return TD_FAIL;
	TdCensusState& z = c->census;
	if (!z.on) return fail(c, "td_census_reset: the census is off (td_census_enable)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));   // (counts of pipelined batches may still be queued, on either compute stream)
	const size_t n_slots = (size_t)1 << z.log2_slots;
	HIPCHK(c, hipMemsetAsync(z.d_keys, 0, sizeof(cs_u64) * n_slots, c->stream));
	HIPCHK(c, hipMemsetAsync(z.d_counts, 0, sizeof(cs_u64) * n_slots, c->stream));
	HIPCHK(c, hipMemsetAsync(z.d_tallies, 0, sizeof(cs_u64) * TDC_TALLY_WORDS, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return TD_OK;
}

extern "C" int td_census_get(td_ctx* c, td_census_entry* entries, int64_t cap, int64_t* n, td_census_totals* totals)
{
	if (!c) return TD_FAIL;
	TdCensusState& z = c->census;
	if (!z.on) return fail(c, "td_census_get: the census is off (td_census_enable)");
	if (cap < 0 || (cap > 0 && !entries) || !n) return fail(c, "td_census_get: bad arguments");
	*n = 0;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	cs_u64 t[TDC_TALLY_WORDS];
	HIPCHK(c, hipMemcpy(t, z.d_tallies, sizeof t, hipMemcpyDeviceToHost));
	const int64_t distinct = (int64_t)t[TDC_DISTINCT];
	std::vector<td_census_entry> v((size_t)distinct);
	int64_t found = 0;
	const hipError_t e = kt_compact(z.d_keys, z.d_counts, z.log2_slots, v.data(), distinct, z.d_tallies + TDC_CURSOR, c->stream, &found);
	if (e != hipSuccess) return fail(c, "td_census_get: compaction failed: %s", hipGetErrorString(e));
	if (found != distinct) return fail(c, "td_census_get: the table holds %lld keys, its tally says %lld", (long long)found, (long long)distinct);
	std::sort(v.begin(), v.end(), census_entry_before);
	const int64_t take = std::min<int64_t>(cap, distinct);
	if (take > 0) memcpy(entries, v.data(), sizeof(td_census_entry) * (size_t)take);
	*n = distinct;
	if (totals) {
		totals->eligible = (int64_t)t[TDC_ELIGIBLE]; totals->counted = (int64_t)t[TDC_COUNTED]; totals->skipped_empty = (int64_t)t[TDC_EMPTY];
		totals->skipped_long = (int64_t)t[TDC_LONG]; totals->skipped_n = (int64_t)t[TDC_N]; totals->overflow = (int64_t)t[TDC_OVERFLOW];
		totals->distinct = distinct;
	}
	return TD_OK;
}

// the count kernel's time of the last batch, for tools/census_bench.py (option "census_kernel_us" of td_get_option)
int census_last_kernel_us(td_ctx* c, int32_t* us)
{
	TdCensusState& z = c->census;
	if (!z.on) return fail(c, "td_get_option: census_kernel_us: the census is off");
	HIPCHK(c, hipSetDevice(c->device));
	float ms = 0.0f;
	if (hipEventSynchronize(z.ev_c1) != hipSuccess || hipEventElapsedTime(&ms, z.ev_c0, z.ev_c1) != hipSuccess) {
		(void)hipGetLastError();
		return fail(c, "td_get_option: census_kernel_us: no batch has been counted yet");
	}
	*us = (int32_t)(ms * 1000.0f + 0.5f);
	return TD_OK;
}

extern "C" int td_census_host(const td_model_desc* m, int32_t segment, uint32_t outcome_mask, const uint8_t* codes, const int64_t* offs,
                              int64_t n_reads, const td_read_result* res, const int8_t* labels,
                              td_census_entry** entries, int64_t* n, td_census_totals* totals)
{
	if (entries) *entries = nullptr;
	if (n) *n = 0;
	int32_t seg = -1;
	std::string why;
	if (!pick_segment(m, segment, seg, why)) return fail(nullptr, "td_census_host: %s", why.c_str());
	if (!mask_ok(outcome_mask)) return fail(nullptr, "td_census_host: outcome_mask 0x%x is not a non-empty subset of bits 0..7", outcome_mask);
	if (!entries || !n || n_reads < 0 || (n_reads > 0 && (!offs || !res || !labels))) return fail(nullptr, "td_census_host: bad arguments");
	td_census_totals t{};
	std::vector<uint64_t> keys;
	for (int64_t i = 0; i < n_reads; i++) {
		const uint32_t type = (uint32_t)res[i].read_type & 0xFFu;
		if (type >= 8u || !((outcome_mask >> type) & 1u)) continue;
		t.eligible++;
		const int64_t len = offs[i + 1] - offs[i];
		const int8_t* lab = labels + offs[i] + i;
		const uint8_t* seq = codes + offs[i];
		uint64_t w = 0;
		int cnt = 0;
		bool has_n = false;
		for (int64_t p = 0; p < len; p++) {
			const int l = lab[p + 1];
			if (l < 0 || l >= m->H || (m->label[l] & 0xFFFF) != seg) continue;
			cnt++;
			if (cnt <= TD_CENSUS_MAX_WORD) {
				if (seq[p] > 3) has_n = true;
				w = (w << 2) | (uint64_t)(seq[p] & 3u);
			}
		}
		if (cnt == 0) t.skipped_empty++;
		else if (cnt > TD_CENSUS_MAX_WORD) t.skipped_long++;
		else if (has_n) t.skipped_n++;
		else { keys.push_back(((uint64_t)cnt << 56) | w); t.counted++; }
	}
	std::vector<td_census_entry> v;
	census_tally_keys(keys, v);
	t.distinct = (int64_t)v.size();
	if (!(*entries = census_copy_entries(v))) return fail(nullptr, "td_census_host: out of memory");
	*n = (int64_t)v.size();
	if (totals) *totals = t;
	return TD_OK;
}

extern "C" int td_census_merge(const td_census_entry* a, int64_t na, const td_census_entry* b, int64_t nb, td_census_entry** out, int64_t* n)
{
	if (!out || !n || na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b)) return fail(nullptr, "td_census_merge: bad arguments");
	std::vector<td_census_entry> all;
	all.insert(all.end(), a, a + na);
	all.insert(all.end(), b, b + nb);
	std::sort(all.begin(), all.end(), [](const td_census_entry& x, const td_census_entry& y) { return x.key < y.key; });
	std::vector<td_census_entry> v;
	for (const td_census_entry& e : all) {
		if (!v.empty() && v.back().key == e.key) v.back().count += e.count;
		else v.push_back(e);
	}
	std::sort(v.begin(), v.end(), census_entry_before);
	if (!(*out = census_copy_entries(v))) return fail(nullptr, "td_census_merge: out of memory");
	*n = (int64_t)v.size();
	return TD_OK;
}

extern "C" int td_census_key_text(uint64_t key, char buf[32])
{
	if (!buf) return TD_FAIL;
	buf[0] = 0;
	const int len = (int)(key >> 56);
	if (len < 1 || len > TD_CENSUS_MAX_WORD) return fail(nullptr, "td_census_key_text: 0x%llx is no key (length %d)", (unsigned long long)key, len);
	if (len < TD_CENSUS_MAX_WORD && ((key & 0x00FFFFFFFFFFFFFFull) >> (2 * len)) != 0) return fail(nullptr, "td_census_key_text: 0x%llx is no key (bits beyond its %d bases)", (unsigned long long)key, len);
	for (int i = 0; i < len; i++) buf[i] = "ACGT"[(key >> (2 * (len - 1 - i))) & 3u];
	buf[len] = 0;
	return TD_OK;
}

extern "C" void td_census_free(td_census_entry* entries) { free(entries); }
