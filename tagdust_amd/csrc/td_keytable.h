// td_keytable.h -- the counting table the census (td_census.hip) and the molecule count (td_molecules.hip) share: 64-bit keys, never
// 0, counted in an open-addressing table in HBM.  Here: the table as a context owns it (TdCountTable; its life and its results are
// in td_keytable.hip), and the device code both count kernels are made of -- the walk over a decoded tile, the probe, the wave's
// tail, a wave's places behind a cursor.  The device functions are inline: a probe belongs inside its kernel.  The arithmetic of a
// key and the host helpers of every td_census_entry result come from td_count_key.h, which the host units read without this file.
//
// Lanes of a wave that hold the same key leave as one probe and one add of their number (kt_wave_merge); the distinct keys of a
// wave probe side by side (kt_probe_add).  Nothing is ever removed from the table and the probe window is fixed, so a key finds or
// claims its slot on every attempt or fails on every attempt: a count in the table is exact, what did not fit is the caller's
// overflow tally.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>

#include "td_count_key.h"
#include "td_device.h"

struct TdSlot;

#define KT_BLOCK 256
#define KT_WAVES (KT_BLOCK / TD_WAVE)
// linear probing looks at this many slots from the key's hash (the whole table when that is smaller): the same on every attempt
#define KT_PROBE_WINDOW 128
#define KT_SLOT_BYTES 16   // a key and a count, 8 bytes each

struct TdKeyTable {
	kt_u64* __restrict__ keys;      // [slot_mask + 1], 0 = empty
	kt_u64* __restrict__ counts;    // [slot_mask + 1]
	uint32_t slot_mask, window;     // 2^log2_slots - 1; slots a key looks at
};

// a decoded tile in device order, as both decode kernels leave it: labels have the stride of the batch's lmax
struct TdTileView {
	const uint32_t* __restrict__ packed;   // [n_tiles][nw2 + nw1][64]  2-bit words then N-mask words
	const int8_t*   __restrict__ labels;   // [n_tiles][lmax + 1][64]
	int32_t lmax, nw2, nw1;
};

// Two timing events around what a stage queued for the last batch (the "*_kernel_us" options of td_get_option)
struct KtEventPair { hipEvent_t e0 = nullptr, e1 = nullptr; };
// both events, or on a failure none / both destroyed, the pair empty again
KT_HIDDEN hipError_t kt_pair_create(KtEventPair& ev);
KT_HIDDEN void kt_pair_destroy(KtEventPair& ev);

// a counting table that belongs to a context
struct TdCountTable {
	int32_t log2_slots = 0, H = 0, tally_words = 0;
	int32_t* d_label = nullptr;    // [H] model.label, the table's own copy
	kt_u64* d_keys = nullptr;      // [2^log2_slots], 0 = empty
	kt_u64* d_counts = nullptr;    // [2^log2_slots]
	kt_u64* d_tallies = nullptr;   // [tally_words] the owner's tallies, the compaction's cursor among them
	KtEventPair ev;                // around the last count launch
};

// label copy, table, tallies and events, all zeroed (a failure leaves what it got: kt_table_release) / all of it freed
KT_HIDDEN hipError_t kt_table_create(TdCountTable& t, const int32_t* label, int32_t H, int32_t log2_slots, int32_t tally_words);
KT_HIDDEN void kt_table_release(TdCountTable& t);
// keys, counts and tallies to zero, queued on `stream`
KT_HIDDEN hipError_t kt_table_zero(const TdCountTable& t, hipStream_t stream);
KT_HIDDEN TdKeyTable kt_table_view(const TdCountTable& t);
KT_HIDDEN TdTileView kt_tile_view(const TdSlot& s, const int8_t* labels);
// One launch over a decoded slot: `kernel` (KT_BLOCK threads, a tile per wave, *args its one argument) on the slot's compute stream,
// checked; a slot without tiles gets no launch.  kt_launch_slot: the same between the two events of `ev`, which are recorded either way.
KT_HIDDEN int kt_launch_tiles(td_ctx* c, TdSlot& s, const void* kernel, void* args);
KT_HIDDEN int kt_launch_slot(td_ctx* c, const KtEventPair& ev, TdSlot& s, const void* kernel, void* args);
// ... and behind the last launch that reads the decoded slot: the finish kernel waits for ev_hits, so a slot whose batch has been
// waited for is no longer read by these launches either
KT_HIDDEN int kt_slot_read_behind(td_ctx* c, TdSlot& s);
// The bracket around a sweep that fills dense arrays behind a cursor (kt_wave_place): up to two device arrays of `count` elements of
// size0 / size1 bytes (0: none), the cursor zeroed, launch(array 0, array 1) on the context's stream and waited for, the arrays
// copied down to out0 / out1 and freed; *found = what the cursor came to, the caller holds it against what it expects.  A HIP
// failure is "`who`: `what`: <its text>".
KT_HIDDEN int kt_sweep_dense(td_ctx* c, const char* who, const char* what, kt_u64* cursor, size_t count, void* out0, size_t size0, void* out1,
                             size_t size1, const std::function<void(void*, void*)>& launch, int64_t* found);
// What the table holds, in the order of td_census_get (`who`: the entry point, for its messages): tallies[t.tally_words] down,
// the occupied pairs -- tallies[distinct_word] of them, the compaction's cursor is tallies[cursor_word] -- held against that
// tally and sorted; *n = their number, entries[min(cap, *n)] the first of them.  Waits for the compute streams.
KT_HIDDEN int kt_table_entries(td_ctx* c, const char* who, const TdCountTable& t, int distinct_word, int cursor_word, td_census_entry* entries,
                               int64_t cap, int64_t* n, kt_u64* tallies);
// microseconds between a pair's two recorded events (waits for the second); `none_yet`: the message when they have not been recorded
KT_HIDDEN int kt_last_kernel_us(td_ctx* c, const KtEventPair& ev, int32_t* us, const char* none_yet);

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t kt_hash(kt_u64 k) { return (uint32_t)(kt_mix(k) >> 32); }

__device__ __forceinline__ kt_u64 kt_readlane64(kt_u64 v, int lane)
{
	const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
	const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
	return ((kt_u64)hi << 32) | lo;
}

__device__ __forceinline__ int kt_wave_sum(int v)
{
	for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
	return v;
}

// A wave's places in a dense array behind `cursor` (whole waves): the lanes with `take` get consecutive positions -- one add on the
// cursor by the first of them, the others behind it by their rank --, every other lane -1
__device__ __forceinline__ int64_t kt_wave_place(bool take, kt_u64* __restrict__ cursor, int lane)
{
	const kt_u64 hit = __builtin_amdgcn_ballot_w64(take);
	if (hit == 0ull) return -1;
	kt_u64 base = 0ull;
	if (lane == __builtin_ctzll(hit)) base = atomicAdd(cursor, (kt_u64)__builtin_popcountll(hit));
	base = kt_readlane64(base, __builtin_ctzll(hit));
	return take ? (int64_t)base + __builtin_popcountll(hit & ((1ull << lane) - 1ull)) : -1;
}

// lanes with the same key leave as one: the first of them gets their number, the others 0 (whole waves only)
__device__ __forceinline__ int kt_wave_merge(bool has_key, kt_u64 key, int lane)
{
	int mine = 0;
	kt_u64 todo = __builtin_amdgcn_ballot_w64(has_key);
	while (todo) {
		const int leader = __builtin_ctzll(todo);
		const kt_u64 kv = kt_readlane64(key, leader);
		const kt_u64 same = __builtin_amdgcn_ballot_w64(has_key && key == kv);
		if (lane == leader) mine = __builtin_popcountll(same);
		todo &= ~same;
	}
	return mine;
}

// `mine` reads under `key`: placed = they are in the table, fresh = this lane claimed the slot (the key is new to the table)
__device__ __forceinline__ void kt_probe_add(const TdKeyTable& t, kt_u64 key, int mine, bool& placed, bool& fresh)
{
	placed = false; fresh = false;
	if (mine <= 0) return;
	const uint32_t h = kt_hash(key);
	for (uint32_t i = 0; i < t.window; i++) {
		const uint32_t slot = (h + i) & t.slot_mask;
		kt_u64 cur = __hip_atomic_load(&t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a slot's key changes once, from 0)
		if (cur == 0ull) { cur = atomicCAS(&t.keys[slot], 0ull, key); fresh = cur == 0ull; if (fresh) cur = key; }
		if (cur == key) { atomicAdd(&t.counts[slot], (kt_u64)mine); placed = true; return; }
	}
}

// The slot that holds `key`, -1 when the table does not: a plain probe for a kernel queued behind the one that added the key.  The
// key then sits in its window for good or has failed for good (nothing is removed, and a key claims the first empty slot of its
// window: no empty slot lies in front of it).
__device__ __forceinline__ int32_t kt_probe_find(const TdKeyTable& t, kt_u64 key)
{
	const uint32_t h = kt_hash(key);
	for (uint32_t i = 0; i < t.window; i++) {
		const uint32_t slot = (h + i) & t.slot_mask;
		const kt_u64 cur = __hip_atomic_load(&t.keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == key) return (int32_t)slot;
		if (cur == 0ull) return -1;
	}
	return -1;
}

// The tail of a count kernel (whole waves): lanes with the same key leave as one, the wave's distinct keys probe side by side.
// What the wave's reads with a key came to: counted in the table, not fitted, keys new to the table.
struct KtWaveAdded { int counted, overflow, fresh; };
__device__ __forceinline__ KtWaveAdded kt_wave_add(const TdKeyTable& t, bool has_key, kt_u64 key, int lane)
{
	const int mine = kt_wave_merge(has_key, key, lane);
	bool placed = false, fresh = false;
	kt_probe_add(t, key, mine, placed, fresh);
	KtWaveAdded r;
	r.counted = kt_wave_sum(placed ? mine : 0);
	r.overflow = kt_wave_sum(placed ? 0 : mine);
	r.fresh = __builtin_popcountll(__builtin_amdgcn_ballot_w64(fresh));
	return r;
}

// s_cls[128], the class of every label a walk can meet: cls(segment) below H, 0 beyond (the whole workgroup; ends in its barrier)
template <typename Cls>
__device__ __forceinline__ void kt_label_classes(uint8_t* s_cls, const int32_t* __restrict__ label, int H, Cls cls)
{
	for (int h = threadIdx.x; h < 128; h += KT_BLOCK) s_cls[h] = h < H ? (uint8_t)cls(label[h] & 0xFFFF) : (uint8_t)0;
	__syncthreads();
}

// The walk of a wave over its decoded tile, one read per lane (whole waves): for base p = 0, 1, .. of the lane's read
// visit(class of labels[p + 1], the base's 2-bit code, the base is an N) until it returns false or the read's `len` bases are
// through (len = 0: the lane takes no part).  Label bytes are read only as far as some lane still walks.
template <typename Visit>
__device__ __forceinline__ void kt_walk_tile(const TdTileView& v, const uint8_t* s_cls, int tile, int lane, int len, Visit visit)
{
	bool active = len > 0;
	int tmax = len;
	for (int o = 32; o >= 1; o >>= 1) { const int t2 = __shfl_xor(tmax, o); tmax = t2 > tmax ? t2 : tmax; }
	if (tmax > v.lmax) tmax = v.lmax;                 // (the batch's longest read: every index below stays inside the tile's arrays)
	const uint32_t* pk = v.packed + (int64_t)tile * (v.nw2 + v.nw1) * TD_WAVE + lane;
	const int8_t* lb = v.labels + (int64_t)tile * (v.lmax + 1) * TD_WAVE + lane;
	uint32_t w2 = 0u, wn = 0u;                        // the 16 bases / the 32 N flags around p (a lane is active from p = 0 on)
	for (int p = 0; p < tmax; p++) {
		if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
		if (active) {
			if ((p & 15) == 0) w2 = pk[(p >> 4) * TD_WAVE];
			if ((p & 31) == 0) wn = pk[(v.nw2 + (p >> 5)) * TD_WAVE];
			const uint32_t lab = (uint8_t)lb[(p + 1) * TD_WAVE];     // labels[p + 1] belongs to base p
			if (!visit(lab < 128u ? (uint32_t)s_cls[lab] : 0u, (w2 >> (2 * (p & 15))) & 3u, ((wn >> (p & 31)) & 1u) != 0u)) active = false;
			if (p + 1 >= len) active = false;
		}
	}
}
#endif
