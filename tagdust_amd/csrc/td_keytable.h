// td_keytable.h -- the counting table the census (td_census.hip) and the molecule count (td_molecules.hip) share: 64-bit keys, never
// 0, counted in an open-addressing table in HBM.  Device code and the launch of the compaction kernel; each unit that includes it
// gets its own copy of the kernel (static), there is one text.
//
// Lanes of a wave that hold the same key leave as one probe and one add of their number (kt_wave_merge); the distinct keys of a
// wave probe side by side (kt_probe_add).  Nothing is ever removed from the table and the probe window is fixed, so a key finds or
// claims its slot on every attempt or fails on every attempt: a count in the table is exact, what did not fit is the caller's
// overflow tally.  kt_compact leaves the occupied (key, count) pairs in a dense array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tagdust_census.h"
#include "td_device.h"

typedef unsigned long long kt_u64;

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

#ifdef __HIPCC__
// splitmix64's finish: every bit of k reaches every bit of the result
__host__ __device__ __forceinline__ kt_u64 kt_mix(kt_u64 k)
{
	k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ull;
	k ^= k >> 27; k *= 0x94D049BB133111EBull;
	k ^= k >> 31;
	return k;
}

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

// the occupied (key, count) pairs into a dense array: one add on the cursor per wave, the lanes behind it by their rank
static __global__ __launch_bounds__(KT_BLOCK) void td_keytable_compact_kernel(const kt_u64* __restrict__ keys, const kt_u64* __restrict__ counts,
                                                                                int64_t n_slots, td_census_entry* __restrict__ out, int64_t cap,
                                                                                kt_u64* __restrict__ cursor)
{
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int64_t step = (int64_t)gridDim.x * KT_BLOCK;
	for (int64_t i0 = (int64_t)blockIdx.x * KT_BLOCK + (threadIdx.x - lane); i0 < n_slots; i0 += step) {   // (i0 is the wave's)
		const int64_t i = i0 + lane;
		const kt_u64 kv = i < n_slots ? keys[i] : 0ull;
		const kt_u64 occ = __builtin_amdgcn_ballot_w64(kv != 0ull);
		if (occ == 0ull) continue;
		kt_u64 base = 0ull;
		if (lane == __builtin_ctzll(occ)) base = atomicAdd(cursor, (kt_u64)__builtin_popcountll(occ));
		base = kt_readlane64(base, __builtin_ctzll(occ));
		const int64_t at = (int64_t)base + __builtin_popcountll(occ & ((1ull << lane) - 1ull));
		if (kv != 0ull && at < cap) { out[at].key = kv; out[at].count = (int64_t)counts[i]; }
	}
}

// the table's `distinct` occupied pairs into out[distinct] (host memory, any order); *found = what the sweep met.  Synchronous on
// `stream`; cursor is a device word of the caller's.
static hipError_t kt_compact(const kt_u64* keys, const kt_u64* counts, int log2_slots, td_census_entry* out, int64_t distinct,
                             kt_u64* cursor, hipStream_t stream, int64_t* found)
{
	*found = 0;
	if (distinct <= 0) return hipSuccess;
	td_census_entry* d_dense = nullptr;
	hipError_t e = hipMalloc((void**)&d_dense, sizeof(td_census_entry) * (size_t)distinct);
	if (e != hipSuccess) return e;
	const int64_t n_slots = (int64_t)1 << log2_slots;
	int64_t blocks = (n_slots + KT_BLOCK - 1) / KT_BLOCK;
	if (blocks > 2048) blocks = 2048;
	e = hipMemsetAsync(cursor, 0, sizeof(kt_u64), stream);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(td_keytable_compact_kernel, dim3((unsigned)blocks), dim3(KT_BLOCK), 0, stream, keys, counts, n_slots, d_dense, distinct, cursor);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipStreamSynchronize(stream);
	if (e == hipSuccess) e = hipMemcpy(out, d_dense, sizeof(td_census_entry) * (size_t)distinct, hipMemcpyDeviceToHost);
	kt_u64 f = 0;
	if (e == hipSuccess) e = hipMemcpy(&f, cursor, sizeof f, hipMemcpyDeviceToHost);
	(void)hipFree(d_dense);
	*found = (int64_t)f;
	return e;
}
#endif
