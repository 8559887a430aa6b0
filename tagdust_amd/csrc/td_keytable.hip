// td_keytable.hip -- the host side of td_keytable.h: the life of a context's counting table, the bracket around a launch over a decoded slot, the
// bracket around a sweep into dense arrays, and the table's contents as sorted entries (with the compaction kernel).  The host
// helpers of every td_census_entry result are in td_census_host.cpp.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "td_ctx.h"

// the occupied (key, count) pairs into a dense array: one add on the cursor per wave, the lanes behind it by their rank
__global__ __launch_bounds__(KT_BLOCK) void td_keytable_compact_kernel(const kt_u64* __restrict__ keys, const kt_u64* __restrict__ counts,
                                                                         int64_t n_slots, td_census_entry* __restrict__ out, int64_t cap,
                                                                         kt_u64* __restrict__ cursor)
{
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int64_t step = (int64_t)gridDim.x * KT_BLOCK;
	for (int64_t i0 = (int64_t)blockIdx.x * KT_BLOCK + (threadIdx.x - lane); i0 < n_slots; i0 += step) {   // (i0 is the wave's)
		const int64_t i = i0 + lane;
		const kt_u64 kv = i < n_slots ? keys[i] : 0ull;
		const int64_t at = kt_wave_place(kv != 0ull, cursor, lane);
		if (at >= 0 && at < cap) { out[at].key = kv; out[at].count = (int64_t)counts[i]; }
	}
}

hipError_t kt_table_create(TdCountTable& t, const int32_t* label, int32_t H, int32_t log2_slots, int32_t tally_words)
{
	t.log2_slots = log2_slots; t.H = H; t.tally_words = tally_words;
	const size_t n_slots = (size_t)1 << log2_slots;
	hipError_t e = hipMalloc((void**)&t.d_label, sizeof(int32_t) * (size_t)H);
	if (e == hipSuccess) e = hipMalloc((void**)&t.d_keys, sizeof(kt_u64) * n_slots);
	if (e == hipSuccess) e = hipMalloc((void**)&t.d_counts, sizeof(kt_u64) * n_slots);
	if (e == hipSuccess) e = hipMalloc((void**)&t.d_tallies, sizeof(kt_u64) * (size_t)tally_words);
	if (e == hipSuccess) e = hipMemcpy(t.d_label, label, sizeof(int32_t) * (size_t)H, hipMemcpyHostToDevice);
	if (e == hipSuccess) e = kt_table_zero(t, nullptr);
	if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
	if (e == hipSuccess) e = kt_pair_create(t.ev);
	return e;
}

void kt_table_release(TdCountTable& t)
{
	void* p[] = { t.d_label, t.d_keys, t.d_counts, t.d_tallies };
	for (void* q : p) if (q) (void)hipFree(q);
	kt_pair_destroy(t.ev);
	t = TdCountTable();
}

hipError_t kt_pair_create(KtEventPair& ev)
{
	hipError_t e = hipEventCreate(&ev.e0);
	if (e == hipSuccess) e = hipEventCreate(&ev.e1);
	if (e != hipSuccess) kt_pair_destroy(ev);
	return e;
}

void kt_pair_destroy(KtEventPair& ev)
{
	if (ev.e0) (void)hipEventDestroy(ev.e0);
	if (ev.e1) (void)hipEventDestroy(ev.e1);
	ev = KtEventPair();
}

hipError_t kt_table_zero(const TdCountTable& t, hipStream_t stream)
{
	const size_t n_slots = (size_t)1 << t.log2_slots;
	hipError_t e = hipMemsetAsync(t.d_keys, 0, sizeof(kt_u64) * n_slots, stream);
	if (e == hipSuccess) e = hipMemsetAsync(t.d_counts, 0, sizeof(kt_u64) * n_slots, stream);
	if (e == hipSuccess) e = hipMemsetAsync(t.d_tallies, 0, sizeof(kt_u64) * (size_t)t.tally_words, stream);
	return e;
}

TdKeyTable kt_table_view(const TdCountTable& t)
{
	const uint64_t n_slots = 1ull << t.log2_slots;
	return TdKeyTable{ t.d_keys, t.d_counts, (uint32_t)(n_slots - 1), (uint32_t)std::min<uint64_t>(n_slots, KT_PROBE_WINDOW) };
}

TdTileView kt_tile_view(const TdSlot& s, const int8_t* labels) { return TdTileView{ s.d_packed, labels, s.lmax, s.nw2, s.nw1 }; }

int kt_launch_tiles(td_ctx* c, TdSlot& s, const void* kernel, void* args)
{
	if (s.n_tiles > 0) HIPCHK(c, hipLaunchKernel(kernel, dim3((unsigned)((s.n_tiles + KT_WAVES - 1) / KT_WAVES)), dim3(KT_BLOCK), &args, 0, s.cs));
	return TD_OK;
}

int kt_launch_slot(td_ctx* c, const KtEventPair& ev, TdSlot& s, const void* kernel, void* args)
{
	HIPCHK(c, hipEventRecord(ev.e0, s.cs));
	if (kt_launch_tiles(c, s, kernel, args) != TD_OK) return TD_FAIL;
	HIPCHK(c, hipEventRecord(ev.e1, s.cs));
	return TD_OK;
}

int kt_slot_read_behind(td_ctx* c, TdSlot& s)
{
	HIPCHK(c, hipEventRecord(s.ev_hits, s.cs));
	s.hits_queued = true;
	return TD_OK;
}

int kt_sweep_dense(td_ctx* c, const char* who, const char* what, kt_u64* cursor, size_t count, void* out0, size_t size0, void* out1, size_t size1,
                   const std::function<void(void*, void*)>& launch, int64_t* found)
{
	void* d[2] = { nullptr, nullptr };
	void* const out[2] = { out0, out1 };
	const size_t bytes[2] = { size0 * count, size1 * count };
	kt_u64 met = 0;
	hipError_t e = hipSuccess;
	for (int k = 0; k < 2; k++) if (e == hipSuccess && bytes[k]) e = hipMalloc(&d[k], bytes[k]);
	if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, sizeof(kt_u64), c->stream);
	if (e == hipSuccess) { launch(d[0], d[1]); e = hipGetLastError(); }
	if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
	for (int k = 0; k < 2; k++) if (e == hipSuccess && bytes[k]) e = hipMemcpy(out[k], d[k], bytes[k], hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(&met, cursor, sizeof met, hipMemcpyDeviceToHost);
	for (void* p : d) if (p) (void)hipFree(p);
	if (e != hipSuccess) return fail(c, "%s: %s: %s", who, what, hipGetErrorString(e));
	*found = (int64_t)met;
	return TD_OK;
}

int kt_table_entries(td_ctx* c, const char* who, const TdCountTable& t, int distinct_word, int cursor_word, td_census_entry* entries,
                     int64_t cap, int64_t* n, kt_u64* tallies)
{
	if (cap < 0 || (cap > 0 && !entries) || !n) return fail(c, "%s: bad arguments", who);
	*n = 0;
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	HIPCHK(c, hipMemcpy(tallies, t.d_tallies, sizeof(kt_u64) * (size_t)t.tally_words, hipMemcpyDeviceToHost));
	const int64_t distinct = (int64_t)tallies[distinct_word];
	std::vector<td_census_entry> v((size_t)distinct);
	if (distinct > 0) {   // the occupied pairs into a dense array on the device, what the sweep met into the cursor
		kt_u64* cursor = t.d_tallies + cursor_word;
		int64_t found = 0;
		const int64_t n_slots = (int64_t)1 << t.log2_slots;
		const unsigned blocks = (unsigned)std::min<int64_t>((n_slots + KT_BLOCK - 1) / KT_BLOCK, 2048);
		if (kt_sweep_dense(c, who, "compaction failed", cursor, (size_t)distinct, v.data(), sizeof(td_census_entry), nullptr, 0, [&](void* d_dense, void*) {
			    hipLaunchKernelGGL(td_keytable_compact_kernel, dim3(blocks), dim3(KT_BLOCK), 0, c->stream, t.d_keys, t.d_counts, n_slots,
			                       (td_census_entry*)d_dense, distinct, cursor);
		    }, &found) != TD_OK) return TD_FAIL;
		if (found != distinct) return fail(c, "%s: the table holds %lld keys, its tally says %lld", who, (long long)found, (long long)distinct);
	}
	std::sort(v.begin(), v.end(), kt_entry_before);
	const int64_t take = std::min<int64_t>(cap, distinct);
	if (take > 0) memcpy(entries, v.data(), sizeof(td_census_entry) * (size_t)take);
	*n = distinct;
	return TD_OK;
}

int kt_last_kernel_us(td_ctx* c, const KtEventPair& ev, int32_t* us, const char* none_yet)
{
	HIPCHK(c, hipSetDevice(c->device));
	float ms = 0.0f;
	if (hipEventSynchronize(ev.e1) != hipSuccess || hipEventElapsedTime(&ms, ev.e0, ev.e1) != hipSuccess) {
		(void)hipGetLastError();
		return fail(c, "%s", none_yet);
	}
	*us = (int32_t)(ms * 1000.0f + 0.5f);
	return TD_OK;
}
