// td_molecules.hip -- the molecule count (include/tagdust_molecules.h): how many molecules each barcode yielded.
//
// Behind every TD_MODE_GET_LABEL launch of a context with the count on, one small kernel reads what the decode kernel left in
// device order -- the outcome, barcode and fingerprint of every read, the lane-interleaved label bytes, the packed bases with their
// N mask -- builds each extracted read's key from its barcode, its fingerprint and the first P bases of its read segments, and
// counts it in the table of td_keytable.h, the census's.  One read per lane, one tile per wave, like the decode kernels.  Here
// almost every read is eligible and almost every key is its own: the cost is the table's random traffic (a load, mostly a CAS, an
// add per read), not the heavy hitter the census merges away -- the merge of equal keys in a wave stays, PCR copies sit together
// often enough.  A second kernel sweeps the table into one summary row per barcode bin (td_mol_get).  td_mol_host is the same
// definition over host arrays (no GPU), td_mol_summarise the same summary from entries.
//
// Dedup (td_mol_dedup_enable) adds two launches behind the count.  Pass 1 builds every read's key again -- mol_lane_key is the one
// text the count and it share --, finds the slot the count left the key in and lowers first[slot] to the read's ordinal, its
// number in the caller's order over the whole context.  Pass 2 marks every read whose ordinal is not its slot's first as
// TD_EXTRACT_DUPLICATE.  The minimum does not depend on the order the reads arrive in, so the two passes of neighbouring batches
// may overlap but for one thing: pass 2 waits for pass 1 of the batch before it (an event), since that batch holds smaller
// ordinals.  td_mol_dedup_host is the same decision on the host.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/tagdust_molecules.h"
#include "td_ctx.h"

#define KEY_LOW_MASK 0x00FFFFFFFFFFFFFFull

// the key of tagdust_molecules.h (host and device: the same integer arithmetic)
__host__ __device__ __forceinline__ kt_u64 mol_key(int32_t barcode, int32_t fingerprint, kt_u64 w, int n)
{
	const kt_u64 a = kt_mix(((kt_u64)(uint32_t)fingerprint << 8) | (kt_u64)n);
	kt_u64 low = kt_mix(w ^ a) & KEY_LOW_MASK;
	if (low == 0ull) low = 1ull;
	const kt_u64 bin = barcode == -1 ? 0ull : (kt_u64)(barcode & 0xFF);
	return (bin << 56) | low;
}

// per label: 1 = it belongs to an 'R' segment (the whole workgroup; ends in its barrier)
__device__ __forceinline__ void mol_r_labels(const TdMolArgs& a, uint8_t* s_r)
{
	kt_label_classes(s_r, a.label, a.H, [&](int seg) { return seg < 64 ? (int)((a.r_segs >> seg) & 1ull) : 0; });
}

// what a lane's read is to the count: eligible, and then exactly one of the three classes (has_key: counted under `key`)
struct MolLane { bool elig, is_empty, is_n, has_key; kt_u64 key; };

// The key of read k = tile * 64 + lane: the label walk, the prefix word and the N mask (whole waves).  false: no lane of the wave
// is eligible, nothing else was read.  The count kernel and dedup's pass 1 both call this: one text.
__device__ __forceinline__ bool mol_lane_key(const TdMolArgs& a, const uint8_t* s_r, int tile, int lane, int64_t k, MolLane& m)
{
	bool elig = false;
	if (k < a.n_reads) elig = ((uint32_t)a.out_type[k] & 0xFFu) == (uint32_t)TD_EXTRACT_SUCCESS;   // the outcome first: the other lanes read nothing more
	m.elig = elig; m.is_empty = false; m.is_n = false; m.has_key = false; m.key = 0ull;
	if (__builtin_amdgcn_ballot_w64(elig) == 0ull) return false;
	int len = 0, barcode = -1, finger = -1;
	if (elig) { len = a.lens[k]; barcode = a.out_barcode[k]; finger = a.out_finger[k]; }
	kt_u64 w = 0ull;
	int n = 0;
	bool has_n = false;
	kt_walk_tile(a.tile, s_r, tile, lane, len, [&](uint32_t cls, uint32_t base, bool base_is_n) {   // until P read bases are collected
		if (!cls) return true;
		w = (w << 2) | (kt_u64)base;
		has_n = has_n || base_is_n;
		return ++n < a.prefix;
	});
	m.is_empty = elig && n == 0;
	m.is_n = elig && n > 0 && has_n;
	m.has_key = elig && n > 0 && !has_n;
	m.key = m.has_key ? mol_key(barcode, finger, w, n) : 0ull;
	return true;
}

__global__ __launch_bounds__(KT_BLOCK) void td_mol_count_kernel(const TdMolArgs a)
{
	__shared__ uint8_t s_r[128];
	mol_r_labels(a, s_r);
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int tile = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
	if (tile >= a.n_tiles) return;                    // (whole waves; no workgroup barrier below)
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	MolLane m;
	if (!mol_lane_key(a, s_r, tile, lane, k, m)) return;
	const KtWaveAdded added = kt_wave_add(a.table, m.has_key, m.key, lane);
	// tallies: one add per wave and tally
	const int n_elig = __builtin_popcountll(__builtin_amdgcn_ballot_w64(m.elig));
	const int n_empty = __builtin_popcountll(__builtin_amdgcn_ballot_w64(m.is_empty));
	const int n_n = __builtin_popcountll(__builtin_amdgcn_ballot_w64(m.is_n));
	if (lane == 0) {
		atomicAdd(&a.tallies[TDM_ELIGIBLE], (kt_u64)n_elig);
		if (added.counted) atomicAdd(&a.tallies[TDM_COUNTED], (kt_u64)added.counted);
		if (n_empty) atomicAdd(&a.tallies[TDM_EMPTY], (kt_u64)n_empty);
		if (n_n) atomicAdd(&a.tallies[TDM_N], (kt_u64)n_n);
		if (added.overflow) atomicAdd(&a.tallies[TDM_OVERFLOW], (kt_u64)added.overflow);
		if (added.fresh) atomicAdd(&a.tallies[TDM_MOLECULES], (kt_u64)added.fresh);
	}
}

// Dedup, pass 1: behind the count kernel of the same batch on the same stream, so a counted read's key is in the table or has
// overflowed for good and a plain probe finds which.  Leaves every lane's slot (-1: not judged, not eligible included) for pass 2
// and lowers the slot's first ordinal to the read's own.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_first_kernel(const TdMolArgs a)
{
	__shared__ uint8_t s_r[128];
	mol_r_labels(a, s_r);
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int tile = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
	if (tile >= a.n_tiles) return;                    // (whole waves; no workgroup barrier below)
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	MolLane m;
	int32_t slot = -1;
	if (mol_lane_key(a, s_r, tile, lane, k, m) && m.has_key) {
		slot = kt_probe_find(a.table, m.key);
		if (slot >= 0) {
			const int64_t at = a.read_at ? (int64_t)a.read_at[k] : k;     // the caller's order, not the length-sorted one
			atomicMin(&a.first[slot], (kt_u64)(a.ordinal_base + at));
		}
	}
	a.judged[k] = slot;                               // (judged has n_tiles * 64 words)
}

// Dedup, pass 2: a judged read whose ordinal is not its slot's first is a duplicate.  Every pass 1 that could still lower that
// first -- this batch's and every earlier one's -- has finished (stream order and the event of the batch before).
__global__ __launch_bounds__(KT_BLOCK) void td_mol_mark_kernel(int32_t* __restrict__ out_type, const int32_t* __restrict__ judged,
                                                                const int32_t* __restrict__ read_at, const kt_u64* first, int64_t ordinal_base,
                                                                int64_t n_reads, int32_t n_tiles, kt_u64* __restrict__ tallies)
{
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int tile = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
	if (tile >= n_tiles) return;
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	int32_t type = 0;
	bool elig = false;
	if (k < n_reads) { type = out_type[k]; elig = ((uint32_t)type & 0xFFu) == (uint32_t)TD_EXTRACT_SUCCESS; }
	if (__builtin_amdgcn_ballot_w64(elig) == 0ull) return;
	const int32_t slot = elig ? judged[k] : -1;
	bool dup = false;
	if (slot >= 0) {
		const int64_t at = read_at ? (int64_t)read_at[k] : k;
		dup = __hip_atomic_load(&first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (kt_u64)(ordinal_base + at);
	}
	if (dup) out_type[k] = (int32_t)(((uint32_t)type & ~0xFFu) | (uint32_t)TD_EXTRACT_DUPLICATE);
	// tallies: one add per wave and tally
	const int n_elig = __builtin_popcountll(__builtin_amdgcn_ballot_w64(elig));
	const int n_dup = __builtin_popcountll(__builtin_amdgcn_ballot_w64(dup));
	const int n_unjudged = __builtin_popcountll(__builtin_amdgcn_ballot_w64(elig && slot < 0));
	if (lane == 0) {
		if (n_elig - n_dup) atomicAdd(&tallies[TDM_KEPT], (kt_u64)(n_elig - n_dup));
		if (n_dup) atomicAdd(&tallies[TDM_DUPLICATES], (kt_u64)n_dup);
		if (n_unjudged) atomicAdd(&tallies[TDM_UNJUDGED], (kt_u64)n_unjudged);
	}
}

// The table into one row per barcode bin.  Nearly all slots of a run fall into a handful of bins: a global atomic per slot would
// queue on three or four addresses ("The counters"), so a workgroup sums in LDS -- 256 bins x 12 words of 8
// bytes, 24 KB -- and adds what is not zero to the global rows once.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_summary_kernel(const kt_u64* __restrict__ keys, const kt_u64* __restrict__ counts,
                                                                   int64_t n_slots, kt_u64* __restrict__ rows)
{
	__shared__ kt_u64 s_rows[TD_NUM_BARCODE_BINS * TDM_ROW_WORDS];
	for (int q = threadIdx.x; q < TD_NUM_BARCODE_BINS * TDM_ROW_WORDS; q += KT_BLOCK) s_rows[q] = 0ull;
	__syncthreads();
	const int64_t step = (int64_t)gridDim.x * KT_BLOCK;
	for (int64_t i = (int64_t)blockIdx.x * KT_BLOCK + threadIdx.x; i < n_slots; i += step) {
		const kt_u64 kv = keys[i];
		if (kv == 0ull) continue;
		const kt_u64 cnt = counts[i];
		if (cnt == 0ull) continue;                    // (a claimed slot always has its add behind it once the stream is idle)
		kt_u64* row = s_rows + (int)(kv >> 56) * TDM_ROW_WORDS;
		const int level = (int)(cnt < (kt_u64)TD_MOL_LEVELS ? cnt : (kt_u64)TD_MOL_LEVELS) - 1;
		atomicAdd(&row[0], cnt);
		atomicAdd(&row[1], 1ull);
		atomicAdd(&row[2 + level], 1ull);
	}
	__syncthreads();
	for (int q = threadIdx.x; q < TD_NUM_BARCODE_BINS * TDM_ROW_WORDS; q += KT_BLOCK)
		if (s_rows[q] != 0ull) atomicAdd(&rows[q], s_rows[q]);
}

// ---------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------
namespace {

bool prefix_ok(int32_t p) { return p >= 1 && p <= TD_MOL_MAX_PREFIX; }

// what read i is to the count on the host (td_mol_host and td_mol_dedup_host): not eligible, or one of the three classes; *key of
// a counted read
enum { MOL_NOT_ELIGIBLE = 0, MOL_EMPTY, MOL_HAS_N, MOL_COUNTED };
int host_read_class(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t i,
                    const td_read_result* res, const int8_t* labels, uint64_t* key)
{
	if (((uint32_t)res[i].read_type & 0xFFu) != (uint32_t)TD_EXTRACT_SUCCESS) return MOL_NOT_ELIGIBLE;
	const int64_t len = offs[i + 1] - offs[i];
	const int8_t* lab = labels + offs[i] + i;
	const uint8_t* seq = codes + offs[i];
	uint64_t w = 0;
	int cnt = 0;
	bool has_n = false;
	for (int64_t p = 0; p < len && cnt < prefix_bases; p++) {
		const int l = lab[p + 1];
		if (l < 0 || l >= m->H) continue;
		const int seg = m->label[l] & 0xFFFF;
		if (seg >= m->S || m->seg_type[seg] != 'R') continue;
		cnt++;
		if (seq[p] > 3) has_n = true;
		w = (w << 2) | (uint64_t)(seq[p] & 3u);
	}
	if (cnt == 0) return MOL_EMPTY;
	if (has_n) return MOL_HAS_N;
	*key = mol_key(res[i].barcode, res[i].fingerprint, w, cnt);
	return MOL_COUNTED;
}

void totals_from(const kt_u64* t, td_mol_totals* out)
{
	out->eligible = (int64_t)t[TDM_ELIGIBLE]; out->counted = (int64_t)t[TDM_COUNTED]; out->skipped_empty = (int64_t)t[TDM_EMPTY];
	out->skipped_n = (int64_t)t[TDM_N]; out->overflow = (int64_t)t[TDM_OVERFLOW]; out->molecules = (int64_t)t[TDM_MOLECULES];
}

}   // namespace

// dedup's first ordinals and events freed (nothing of it is queued any more)
static void dedup_release(TdMolState& z)
{
	if (z.d_first) (void)hipFree(z.d_first);
	hipEvent_t ev[] = { z.ev_p1[0], z.ev_p1[1], z.ev_d0, z.ev_d1 };
	for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
	z.d_first = nullptr; z.ev_p1[0] = z.ev_p1[1] = z.ev_d0 = z.ev_d1 = nullptr;
	z.p1_queued[0] = z.p1_queued[1] = false;
	z.dedup = false;
}

void mol_release(td_ctx* c)
{
	TdMolState& z = c->molecules;
	kt_table_release(z.table);
	if (z.d_rows) (void)hipFree(z.d_rows);
	dedup_release(z);
	z = TdMolState();
}

// what the count kernel and dedup's pass 1 read of a decoded slot
static TdMolArgs mol_args(const TdMolState& z, const TdSlot& s, const int32_t* out_type, const int32_t* out_barcode, const int32_t* out_finger,
                          const int8_t* labels)
{
	TdMolArgs a{};
	a.tile = kt_tile_view(s, labels); a.lens = s.d_lens; a.out_type = out_type; a.out_barcode = out_barcode; a.out_finger = out_finger;
	a.label = z.table.d_label; a.n_reads = s.n_reads; a.n_tiles = s.n_tiles; a.H = z.table.H;
	a.r_segs = z.r_segs; a.prefix = z.prefix;
	a.table = kt_table_view(z.table); a.tallies = z.table.d_tallies;
	return a;
}

int mol_count_slot(td_ctx* c, TdSlot& s, const int32_t* out_type, const int32_t* out_barcode, const int32_t* out_finger, const int8_t* labels)
{
	TdMolArgs a = mol_args(c->molecules, s, out_type, out_barcode, out_finger, labels);
	return kt_count_slot(c, c->molecules.table, s, (const void*)td_mol_count_kernel, &a);
}

int mol_dedup_slot(td_ctx* c, TdSlot& s, int32_t* out_type, const int32_t* out_barcode, const int32_t* out_finger, const int8_t* labels)
{
	TdMolState& z = c->molecules;
	const int64_t base = z.next_ordinal;              // batches get their ordinals in the order they are submitted in
	z.next_ordinal += s.n_reads;
	if (s.n_tiles <= 0) return TD_OK;
	if (ensure(c, &s.d_judged, &s.cap_judged, (size_t)s.n_tiles * TD_WAVE * sizeof(int32_t)) != TD_OK) return TD_FAIL;
	TdMolArgs a = mol_args(z, s, out_type, out_barcode, out_finger, labels);
	a.read_at = s.sorted ? s.d_read_at : nullptr; a.first = z.d_first; a.judged = s.d_judged; a.ordinal_base = base;
	const unsigned blocks = (unsigned)((a.n_tiles + KT_WAVES - 1) / KT_WAVES);
	HIPCHK(c, hipEventRecord(z.ev_d0, s.cs));
	hipLaunchKernelGGL(td_mol_first_kernel, dim3(blocks), dim3(KT_BLOCK), 0, s.cs, a);
	HIPCHK(c, hipGetLastError());
	// The batch before this one may run on the other compute stream, and it holds the smaller ordinals: its pass 1 has to be over
	// before this batch's pass 2 reads a first ordinal.  (The batch before that one ran on this stream, or was waited for.)
	const int t = z.turn;
	HIPCHK(c, hipEventRecord(z.ev_p1[t], s.cs));
	z.p1_queued[t] = true;
	if (z.p1_queued[t ^ 1]) HIPCHK(c, hipStreamWaitEvent(s.cs, z.ev_p1[t ^ 1], 0));
	z.turn = t ^ 1;
	hipLaunchKernelGGL(td_mol_mark_kernel, dim3(blocks), dim3(KT_BLOCK), 0, s.cs, out_type, (const int32_t*)s.d_judged, a.read_at,
	                   (const kt_u64*)z.d_first, base, a.n_reads, a.n_tiles, z.table.d_tallies);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(z.ev_d1, s.cs));
	// the finish kernel copies out_type only behind pass 2, and the slot is not restaged under it
	HIPCHK(c, hipEventRecord(s.ev_hits, s.cs));
	s.hits_queued = true;
	return TD_OK;
}

extern "C" int td_mol_enable(td_ctx* c, int32_t prefix_bases, int32_t log2_slots)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_mol_enable: no model uploaded");
	for (int k = 0; k < TD_MAX_PIPELINE; k++)
		if (c->slots[k].ticket) return fail(c, "td_mol_enable: td_submit tickets are outstanding (td_wait them first)");
	if (!prefix_ok(prefix_bases)) return fail(c, "td_mol_enable: prefix_bases = %d (1..%d supported)", prefix_bases, TD_MOL_MAX_PREFIX);
	if (log2_slots == 0) log2_slots = TD_MOL_DEFAULT_LOG2_SLOTS;
	if (log2_slots < 4 || log2_slots > 30) return fail(c, "td_mol_enable: log2_slots = %d (4..30 supported, 0 = the default of %d)", log2_slots, TD_MOL_DEFAULT_LOG2_SLOTS);
	if (c->match_len > 0) return fail(c, "td_mol_enable: a -start/-end window is set (td_set_window): labels behind a window do not mark the read's bases");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	mol_release(c);
	TdMolState& z = c->molecules;
	const td_model_desc& m = c->model.d;
	hipError_t e = kt_table_create(z.table, m.label, m.H, log2_slots, TDM_TALLY_WORDS);
	if (e == hipSuccess) e = hipMalloc((void**)&z.d_rows, sizeof(kt_u64) * TD_NUM_BARCODE_BINS * TDM_ROW_WORDS);
	if (e != hipSuccess) {
		mol_release(c);
		return fail(c, "td_mol_enable: a table of 2^%d slots could not be set up: %s", log2_slots, hipGetErrorString(e));
	}
	z.prefix = prefix_bases;
	z.r_segs = 0;
	for (int j = 0; j < m.S && j < 64; j++) if (m.seg_type[j] == 'R') z.r_segs |= 1ull << j;
	z.on = true;
	return TD_OK;
}

extern "C" int td_mol_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	if (!c->molecules.on) return TD_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	mol_release(c);
	return TD_OK;
}

extern "C" int td_mol_reset(td_ctx* c)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_reset: the molecule count is off (td_mol_enable)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));   // (counts of pipelined batches may still be queued, on either compute stream)
	HIPCHK(c, kt_table_zero(z.table, c->stream));   // (dedup's three tallies among them)
	if (z.dedup) HIPCHK(c, hipMemsetAsync(z.d_first, 0xFF, sizeof(kt_u64) << z.table.log2_slots, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	z.next_ordinal = 0;
	z.p1_queued[0] = z.p1_queued[1] = false;          // (nothing is queued any more)
	return TD_OK;
}

extern "C" int td_mol_dedup_enable(td_ctx* c)
{
	if (!c) return fail(nullptr, "td_mol_dedup_enable: no context");
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_dedup_enable: the molecule count is off (td_mol_enable first): dedup judges the reads the count has keyed");
	for (int k = 0; k < TD_MAX_PIPELINE; k++)
		if (c->slots[k].ticket) return fail(c, "td_mol_dedup_enable: td_submit tickets are outstanding (td_wait them first)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	if (!z.dedup) {
		bool ok = hipMalloc((void**)&z.d_first, sizeof(kt_u64) << z.table.log2_slots) == hipSuccess &&
		          hipEventCreateWithFlags(&z.ev_p1[0], hipEventDisableTiming) == hipSuccess &&
		          hipEventCreateWithFlags(&z.ev_p1[1], hipEventDisableTiming) == hipSuccess &&
		          hipEventCreate(&z.ev_d0) == hipSuccess && hipEventCreate(&z.ev_d1) == hipSuccess;
		if (!ok) {
			const std::string e = hipGetErrorString(hipGetLastError());
			(void)td_mol_dedup_disable(c);
			return fail(c, "td_mol_dedup_enable: the first ordinals of 2^%d slots could not be set up: %s", z.table.log2_slots, e.c_str());
		}
		z.dedup = true;
	}
	return td_mol_reset(c);   // a first ordinal belongs to a key that entered the table with it: both start empty
}

extern "C" int td_mol_dedup_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.dedup && !z.d_first && !z.ev_p1[0] && !z.ev_p1[1] && !z.ev_d0 && !z.ev_d1) return TD_OK;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	dedup_release(z);
	return TD_OK;
}

extern "C" int td_mol_dedup_get(td_ctx* c, td_mol_dedup_totals* totals)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.dedup) return fail(c, "td_mol_dedup_get: dedup is off (td_mol_dedup_enable)");
	if (!totals) return fail(c, "td_mol_dedup_get: bad arguments");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	kt_u64 t[TDM_TALLY_WORDS];
	HIPCHK(c, hipMemcpy(t, z.table.d_tallies, sizeof t, hipMemcpyDeviceToHost));
	totals->kept = (int64_t)t[TDM_KEPT]; totals->duplicates = (int64_t)t[TDM_DUPLICATES]; totals->unjudged = (int64_t)t[TDM_UNJUDGED];
	return TD_OK;
}

extern "C" int td_mol_entries(td_ctx* c, td_census_entry* entries, int64_t cap, int64_t* n, td_mol_totals* totals)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_entries: the molecule count is off (td_mol_enable)");
	kt_u64 t[TDM_TALLY_WORDS];
	if (kt_table_entries(c, "td_mol_entries", z.table, TDM_MOLECULES, TDM_CURSOR, entries, cap, n, t) != TD_OK) return TD_FAIL;
	if (totals) totals_from(t, totals);
	return TD_OK;
}

extern "C" int td_mol_get(td_ctx* c, td_mol_row rows[TD_NUM_BARCODE_BINS], td_mol_totals* totals)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_get: the molecule count is off (td_mol_enable)");
	if (!rows) return fail(c, "td_mol_get: bad arguments");
	static_assert(sizeof(td_mol_row) == sizeof(kt_u64) * TDM_ROW_WORDS, "td_mol_row is the device row");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, sync_compute(c));
	const int64_t n_slots = (int64_t)1 << z.table.log2_slots;
	int64_t blocks = (n_slots + KT_BLOCK - 1) / KT_BLOCK;
	if (blocks > 1024) blocks = 1024;
	HIPCHK(c, hipMemsetAsync(z.d_rows, 0, sizeof(td_mol_row) * TD_NUM_BARCODE_BINS, c->stream));
	hipLaunchKernelGGL(td_mol_summary_kernel, dim3((unsigned)blocks), dim3(KT_BLOCK), 0, c->stream, z.table.d_keys, z.table.d_counts, n_slots, z.d_rows);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(rows, z.d_rows, sizeof(td_mol_row) * TD_NUM_BARCODE_BINS, hipMemcpyDeviceToHost));
	if (totals) {
		kt_u64 t[TDM_TALLY_WORDS];
		HIPCHK(c, hipMemcpy(t, z.table.d_tallies, sizeof t, hipMemcpyDeviceToHost));
		totals_from(t, totals);
	}
	return TD_OK;
}

// the count kernel's time of the last batch, for tools/molecules_bench.py (option "molecules_kernel_us" of td_get_option)
int mol_last_kernel_us(td_ctx* c, int32_t* us)
{
	const TdCountTable& t = c->molecules.table;
	if (!c->molecules.on) return fail(c, "td_get_option: molecules_kernel_us: the molecule count is off");
	return kt_last_kernel_us(c, t.ev_c0, t.ev_c1, us, "td_get_option: molecules_kernel_us: no batch has been counted yet");
}

// the two passes' time of the last batch (option "dedup_kernel_us" of td_get_option).  Between them the stream waits for the batch
// before: with batches in flight on both compute streams that wait is inside the figure, after a td_run it is not.
int mol_dedup_last_kernel_us(td_ctx* c, int32_t* us)
{
	const TdMolState& z = c->molecules;
	if (!z.dedup) return fail(c, "td_get_option: dedup_kernel_us: dedup is off");
	return kt_last_kernel_us(c, z.ev_d0, z.ev_d1, us, "td_get_option: dedup_kernel_us: no batch has been judged yet");
}

extern "C" int td_mol_summarise(const td_census_entry* entries, int64_t n, td_mol_row rows[TD_NUM_BARCODE_BINS])
{
	if (!rows || n < 0 || (n > 0 && !entries)) return fail(nullptr, "td_mol_summarise: bad arguments");
	memset(rows, 0, sizeof(td_mol_row) * TD_NUM_BARCODE_BINS);
	for (int64_t i = 0; i < n; i++) {
		if (entries[i].count <= 0) continue;
		td_mol_row& r = rows[td_mol_key_bin(entries[i].key)];
		r.reads += entries[i].count;
		r.molecules++;
		r.levels[std::min<int64_t>(entries[i].count, TD_MOL_LEVELS) - 1]++;
	}
	return TD_OK;
}

extern "C" int td_mol_host(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                           const td_read_result* res, const int8_t* labels, td_census_entry** entries, int64_t* n, td_mol_totals* totals)
{
	if (entries) *entries = nullptr;
	if (n) *n = 0;
	if (!m || m->S < 1 || m->H < 1 || !m->seg_type || !m->label) return fail(nullptr, "td_mol_host: no model");
	if (!prefix_ok(prefix_bases)) return fail(nullptr, "td_mol_host: prefix_bases = %d (1..%d supported)", prefix_bases, TD_MOL_MAX_PREFIX);
	if (!entries || !n || n_reads < 0 || (n_reads > 0 && (!offs || !res || !labels || !codes))) return fail(nullptr, "td_mol_host: bad arguments");
	td_mol_totals t{};
	std::vector<uint64_t> keys;
	for (int64_t i = 0; i < n_reads; i++) {
		uint64_t key = 0;
		const int cls = host_read_class(m, prefix_bases, codes, offs, i, res, labels, &key);
		if (cls == MOL_NOT_ELIGIBLE) continue;
		t.eligible++;
		if (cls == MOL_EMPTY) t.skipped_empty++;
		else if (cls == MOL_HAS_N) t.skipped_n++;
		else { keys.push_back(key); t.counted++; }
	}
	std::vector<td_census_entry> v;
	kt_tally_keys(keys, v);
	t.molecules = (int64_t)v.size();
	if (!(*entries = kt_copy_entries(v))) return fail(nullptr, "td_mol_host: out of memory");
	*n = (int64_t)v.size();
	if (totals) *totals = t;
	return TD_OK;
}

extern "C" int td_mol_dedup_host(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                                 const td_read_result* res, const int8_t* labels, uint8_t* is_duplicate, td_mol_dedup_totals* totals)
{
	if (!m || m->S < 1 || m->H < 1 || !m->seg_type || !m->label) return fail(nullptr, "td_mol_dedup_host: no model");
	if (!prefix_ok(prefix_bases)) return fail(nullptr, "td_mol_dedup_host: prefix_bases = %d (1..%d supported)", prefix_bases, TD_MOL_MAX_PREFIX);
	if (n_reads < 0 || (n_reads > 0 && (!offs || !res || !labels || !codes || !is_duplicate))) return fail(nullptr, "td_mol_dedup_host: bad arguments");
	td_mol_dedup_totals t{};
	std::unordered_set<uint64_t> seen;                // the keys of the reads so far: a read's ordinal is its index, the first one stays
	for (int64_t i = 0; i < n_reads; i++) {
		is_duplicate[i] = 0;
		uint64_t key = 0;
		const int cls = host_read_class(m, prefix_bases, codes, offs, i, res, labels, &key);
		if (cls == MOL_NOT_ELIGIBLE) continue;
		if (cls != MOL_COUNTED) { t.unjudged++; t.kept++; continue; }
		if (seen.insert(key).second) t.kept++;
		else { is_duplicate[i] = 1; t.duplicates++; }
	}
	if (totals) *totals = t;
	return TD_OK;
}

extern "C" uint64_t td_mol_key(int32_t barcode, int32_t fingerprint, uint64_t w, int32_t n) { return mol_key(barcode, fingerprint, w, n); }
extern "C" int32_t td_mol_key_bin(uint64_t key) { return (int32_t)(key >> 56); }
