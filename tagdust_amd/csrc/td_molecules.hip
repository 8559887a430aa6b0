// td_molecules.hip -- the molecule count (include/tagdust_molecules.h): how many molecules each barcode yielded.
//
// Behind every TD_MODE_GET_LABEL launch of a context with the count on, one small kernel reads what the decode kernel left in
// device order -- the outcome, barcode and fingerprint of every read, the lane-interleaved label bytes, the packed bases with their
// N mask -- builds each extracted read's key from its barcode, its fingerprint and the first P bases of its read segments, and
// counts it in the table of td_keytable.h, the census's.  One read per lane, one tile per wave, like the decode kernels.  Here
// almost every read is eligible and almost every key is its own: the cost is the table's random traffic (a load, mostly a CAS, an
// add per read), not the heavy hitter the census merges away -- the merge of equal keys in a wave stays, PCR copies sit together
// often enough.  A second kernel sweeps the table into one summary row per barcode bin (td_mol_get).  The same definitions over
// host arrays (td_mol_host, td_mol_host_origins, td_mol_dedup_host, td_mol_collapse_host), td_mol_summarise and td_mol_key are in
// td_molecules_host.cpp (td_mol_dedup_collapsed_host, the frozen state's yardstick, with them); the key's arithmetic, one text for
// both sides, in td_count_key.h.
//
// Dedup (td_mol_dedup_enable) adds two launches behind the count.  Pass 1 builds every read's key again -- mol_lane_key is the one
// text the count and it share --, finds the slot the count left the key in and lowers first[slot] to the read's ordinal, its
// number in the caller's order over the whole context.  Pass 2 marks every read whose ordinal is not its slot's first as
// TD_EXTRACT_DUPLICATE.  The minimum does not depend on the order the reads arrive in, so the two passes of neighbouring batches
// may overlap but for one thing: pass 2 waits for pass 1 of the batch before it (an event), since that batch holds smaller
// ordinals.
//
// Collapse (td_mol_collapse_enable) adds one launch behind the count, in front of dedup: the origin pass builds every read's key
// once more, finds its slot and leaves what the key was made of beside it (16 bytes per slot).  The collapse itself runs when it
// is asked for, over an idle table: the occupied slots' indices gathered into a dense list, then one molecule per lane -- the
// parent pass probes the 3 * m keys one UMI mismatch away and keeps the best qualifying one, the root pass walks up and adds the
// molecule's count to its root's --, then the summary sweep above over the collapsed counts, or a gather of the roots.
//
// The frozen state (td_mol_dedup_freeze, with count, dedup and collapse on) is the second pass that makes dedup follow the
// collapse: the collapse runs once more, the keeper pass leaves beside every occupied slot the first ordinal of its root's own
// key, and from then on a batch gets one launch, the replay kernel -- key, probe, one load of keeper[slot], the compare with the
// read's ordinal.  The table is read-only then: no event orders neighbouring batches.
//
// Mate mode (td_mol_mate_enable) joins the first M bases of every read's mate, a read of a second file, into the key.  The mate batch
// travels with the batch's own input on the same upload stream into the batch's slot; the mate kernel, one mate per lane on the
// slot's aux stream between the upload event and ev_pack, turns it into a word and a byte per read in the caller's order, and
// mol_lane_key appends them behind the label walk.  The mates are not decoded, and their outcome takes no part -- unless the mate
// filter is on (td_mol_mate_filter_enable): then the filter kernel of td_mate_filter.hip follows the mate kernel on the same stream and
// judges every mate as TD_MODE_RNA_DUST would, and a join kernel behind the decode launch raises every read's outcome to its mate's
// before the -ref hit count, the census, the count and dedup read it (mol_mate_join, called by td_batch.hip's launch_end).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tagdust_molecules.h"
#include "td_ctx.h"
#include "td_mate_filter.h"

// The head of the three kernels with a tile per wave.  s_r[128], per label: 1 = it belongs to an 'R' segment (the whole workgroup;
// ends in its barrier, in front of any wave that leaves); then the lane and the wave's tile.  false: the wave has no tile.
__device__ __forceinline__ bool mol_wave_tile(const TdMolArgs& a, uint8_t* s_r, int& lane, int& tile)
{
	kt_label_classes(s_r, a.label, a.H, [&](int seg) { return seg < 64 ? (int)((a.r_segs >> seg) & 1ull) : 0; });
	lane = threadIdx.x & (TD_WAVE - 1);
	tile = blockIdx.x * KT_WAVES + (threadIdx.x >> 6);
	return tile < a.n_tiles;                          // (whole waves; no workgroup barrier behind this)
}

// read k of the device's order in the caller's order, which the length sort may have left (read_at NULL: it has not)
__device__ __forceinline__ int64_t mol_caller_at(const int32_t* __restrict__ read_at, int64_t k) { return read_at ? (int64_t)read_at[k] : k; }

// what a lane's read is to the count: eligible, and then exactly one of the three classes (has_key: counted under `key`)
// (w, n, finger: what the key was made of, for the collapse's origin pass)
struct MolLane { bool elig, is_empty, is_n, has_key; kt_u64 key, w; int32_t n, finger; };

// The key of read k = tile * 64 + lane: the label walk, the prefix word and the N mask (whole waves).  false: no lane of the wave
// is eligible, nothing else was read.  The count kernel, dedup's pass 1 and the origin pass all call this: one text.
__device__ __forceinline__ bool mol_lane_key(const TdMolArgs& a, const uint8_t* s_r, int tile, int lane, int64_t k, MolLane& m)
{
	bool elig = false;
	if (k < a.n_reads) elig = ((uint32_t)a.out_type[k] & 0xFFu) == (uint32_t)TD_EXTRACT_SUCCESS;   // the outcome first: the other lanes read nothing more
	m.elig = elig; m.is_empty = false; m.is_n = false; m.has_key = false; m.key = 0ull; m.w = 0ull; m.n = 0; m.finger = -1;
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
	if (a.mate_bases > 0 && elig) {                   // (mate mode is the launch's: one wave-uniform test when it is off)
		const int64_t at = mol_caller_at(a.read_at, k);
		const uint32_t mn = a.mate_n[at];
		const int n2 = (int)(mn & 0x7Fu);                                 // (n + n2 <= P + M <= 32: the shift is at most 62)
		w = (w << (2 * n2)) | a.mate_w[at];
		n += n2;
		has_n = has_n || (mn & 0x80u) != 0u;
	}
	m.is_empty = elig && n == 0;
	m.is_n = elig && n > 0 && has_n;
	m.has_key = elig && n > 0 && !has_n;
	m.key = m.has_key ? mol_key(barcode, finger, w, n) : 0ull;
	m.w = w; m.n = n; m.finger = finger;
	return true;
}

__global__ __launch_bounds__(KT_BLOCK) void td_mol_count_kernel(const TdMolArgs a)
{
	__shared__ uint8_t s_r[128];
	int lane, tile;
	if (!mol_wave_tile(a, s_r, lane, tile)) return;
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

// Mate mode: one mate per lane.  Reads the first min(len, M) bytes of mate i -- never past offs[i + 1], so never past the staged
// bytes -- and leaves, in the caller's order, its prefix word (two bits per base, the first base the most significant) and a byte:
// the number of bases in the low 7 bits, bit 7 set when one of them is not A, C, G or T.  The host has checked that offs ascends.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_mate_kernel(const uint8_t* __restrict__ raw, const int64_t* __restrict__ offs, int64_t n_reads,
                                                                int32_t mate_bases, kt_u64* __restrict__ mate_w, uint8_t* __restrict__ mate_n)
{
	const int64_t i = (int64_t)blockIdx.x * KT_BLOCK + threadIdx.x;
	if (i >= n_reads) return;
	const int64_t o0 = offs[i], len = offs[i + 1] - o0;
	const int n2 = len < (int64_t)mate_bases ? (len > 0 ? (int)len : 0) : mate_bases;
	const uint8_t* p = raw + o0;
	kt_u64 w = 0ull;
	uint32_t any_n = 0u;
	for (int q = 0; q < n2; q++) {
		const uint32_t b = p[q];
		any_n |= b > 3u ? 0x80u : 0u;
		w = (w << 2) | (kt_u64)(b & 3u);
	}
	mate_w[i] = w;
	mate_n[i] = (uint8_t)((uint32_t)n2 | any_n);
}

// The verdict on a wave's reads, the tail of dedup's pass 2 and of the replay (whole waves).  A duplicate's outcome becomes
// TD_EXTRACT_DUPLICATE -- `type` is the lane's outcome word as read, its upper 24 bits stay, and so does every other field --; an
// eligible read that is none is kept, without a slot it is tallied unjudged as well.  One add per wave and tally.
__device__ __forceinline__ void mol_wave_verdict(int32_t* out_type, kt_u64* tallies, int64_t k, int lane, int32_t type, bool elig, int32_t slot, bool dup)
{
	if (dup) out_type[k] = (int32_t)(((uint32_t)type & ~0xFFu) | (uint32_t)TD_EXTRACT_DUPLICATE);   // (the lane's own word)
	const int n_elig = __builtin_popcountll(__builtin_amdgcn_ballot_w64(elig));
	const int n_dup = __builtin_popcountll(__builtin_amdgcn_ballot_w64(dup));
	const int n_unjudged = __builtin_popcountll(__builtin_amdgcn_ballot_w64(elig && slot < 0));
	if (lane == 0) {
		if (n_elig - n_dup) atomicAdd(&tallies[TDM_KEPT], (kt_u64)(n_elig - n_dup));
		if (n_dup) atomicAdd(&tallies[TDM_DUPLICATES], (kt_u64)n_dup);
		if (n_unjudged) atomicAdd(&tallies[TDM_UNJUDGED], (kt_u64)n_unjudged);
	}
}

// Dedup, pass 1: behind the count kernel of the same batch on the same stream, so a counted read's key is in the table or has
// overflowed for good and a plain probe finds which.  Leaves every lane's slot (-1: not judged, not eligible included) for pass 2
// and lowers the slot's first ordinal to the read's own.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_first_kernel(const TdMolArgs a)
{
	__shared__ uint8_t s_r[128];
	int lane, tile;
	if (!mol_wave_tile(a, s_r, lane, tile)) return;
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	MolLane m;
	int32_t slot = -1;
	if (mol_lane_key(a, s_r, tile, lane, k, m) && m.has_key) {
		slot = kt_probe_find(a.table, m.key);
		if (slot >= 0) atomicMin(&a.first[slot], (kt_u64)(a.ordinal_base + mol_caller_at(a.read_at, k)));
	}
	a.judged[k] = slot;                               // (judged has n_tiles * 64 words)
}

// Dedup, pass 2: a judged read whose ordinal is not its slot's first is a duplicate.  Every pass 1 that could still lower that
// first -- this batch's and every earlier one's -- has finished (stream order and the event of the batch before).  It reads no
// label -- no LDS table, no barrier, so not the head of the other per-tile kernels -- and takes the eight values it needs by
// themselves: with the 208 bytes of TdMolArgs for its arguments the two passes measured 2 us in 300 slower (profiles/mol_stage_refactor_ab.json).
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
		const int64_t at = mol_caller_at(read_at, k);
		dup = __hip_atomic_load(&first[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (kt_u64)(ordinal_base + at);
	}
	mol_wave_verdict(out_type, tallies, k, lane, type, elig, slot, dup);
}

// The frozen state, the replay: one launch per batch, behind the decode.  The table and keeper[] are only read: a read whose key the
// table holds is a duplicate unless it is the one read its tree keeps; an eligible read without a key in the table -- empty, N, a
// key that overflowed in the survey or was never surveyed -- is kept and tallied unjudged.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_replay_kernel(const TdMolArgs a)
{
	__shared__ uint8_t s_r[128];
	int lane, tile;
	if (!mol_wave_tile(a, s_r, lane, tile)) return;
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	MolLane m;
	if (!mol_lane_key(a, s_r, tile, lane, k, m)) return;
	const int32_t slot = m.has_key ? kt_probe_find(a.table, m.key) : -1;
	bool dup = false;
	if (slot >= 0) {
		const int64_t at = mol_caller_at(a.read_at, k);
		dup = a.keeper[slot] != (kt_u64)(a.ordinal_base + at);
	}
	// (the outcome is the lane's own word, the kernel's one store into the decoded batch; the duplicates' lanes alone read it again)
	mol_wave_verdict(const_cast<int32_t*>(a.out_type), a.tallies, k, lane, dup ? a.out_type[k] : 0, m.elig, slot, dup);
}

// Collapse, the origin pass: behind the count kernel of the same batch on the same stream, so a counted read's key is in the table or
// has overflowed for good.  One lane per distinct key of the wave goes on; a slot without an origin yet (n == 0: a counted read has
// n >= 1) gets it in two plain 8-byte stores, n last.  Origin passes of two batches may meet in a slot: both write the same words.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_origin_kernel(const TdMolArgs a)
{
	__shared__ uint8_t s_r[128];
	int lane, tile;
	if (!mol_wave_tile(a, s_r, lane, tile)) return;
	const int64_t k = (int64_t)tile * TD_WAVE + lane;
	MolLane m;
	if (!mol_lane_key(a, s_r, tile, lane, k, m)) return;
	if (kt_wave_merge(m.has_key, m.key, lane) <= 0) return;
	const int32_t slot = kt_probe_find(a.table, m.key);
	if (slot < 0) return;                             // overflowed: it is in nobody's neighbourhood
	kt_u64* o = (kt_u64*)&a.origin[slot];
	if ((uint32_t)(__hip_atomic_load(&o[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32) != 0u) return;
	o[0] = m.w;
	o[1] = (kt_u64)(uint32_t)m.finger | ((kt_u64)(uint32_t)m.n << 32);
}

// Collapse: the indices of the occupied slots into a dense list, like td_keytable.hip's sweep over the pairs (kt_wave_place) -- a
// quarter-full table would leave three lanes in four idle below
__global__ __launch_bounds__(KT_BLOCK) void td_mol_occupied_kernel(const kt_u64* __restrict__ keys, int64_t n_slots, uint32_t* __restrict__ occ,
                                                                    int64_t cap, kt_u64* __restrict__ cursor)
{
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int64_t step = (int64_t)gridDim.x * KT_BLOCK;
	for (int64_t i0 = (int64_t)blockIdx.x * KT_BLOCK + (threadIdx.x - lane); i0 < n_slots; i0 += step) {   // (i0 is the wave's)
		const int64_t i = i0 + lane;
		const kt_u64 kv = i < n_slots ? keys[i] : 0ull;
		const int64_t at = kt_wave_place(kv != 0ull, cursor, lane);
		if (at >= 0 && at < cap) occ[at] = (uint32_t)i;
	}
}

// Collapse, the parent pass: one molecule per lane.  The three neighbours of a position probe side by side -- their first loads are
// independent, and most end there, at an empty slot.  Reads keys, counts and origins only; parent[slot] is the lane's own.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_parent_kernel(const TdKeyTable t, const td_mol_origin* __restrict__ origin,
                                                                  const uint32_t* __restrict__ occ, int64_t n_occ, uint32_t* __restrict__ parent)
{
	const int64_t q = (int64_t)blockIdx.x * KT_BLOCK + threadIdx.x;
	if (q >= n_occ) return;
	const uint32_t slot = occ[q];
	const kt_u64 ku = t.keys[slot], cu = t.counts[slot];
	const td_mol_origin o = origin[slot];
	const int m = o.n > 0 ? mol_umi_bases(o.fingerprint) : 0;
	uint32_t best = slot;
	kt_u64 kb = ku, cb = cu;                          // the best so far: u itself, which every qualifying neighbour comes before
	for (int i = 0; i < m; i++) {
		kt_u64 kv[3], first[3];
		uint32_t at[3];
#pragma unroll
		for (int d = 0; d < 3; d++) {
			kv[d] = mol_neighbour_key(ku, o, i, (uint32_t)d + 1u);
			at[d] = kt_hash(kv[d]) & t.slot_mask;
			first[d] = t.keys[at[d]];
		}
#pragma unroll
		for (int d = 0; d < 3; d++) {
			if (first[d] == 0ull) continue;               // not in the table
			const int32_t sv = first[d] == kv[d] ? (int32_t)at[d] : kt_probe_find(t, kv[d]);
			if (sv < 0) continue;
			const kt_u64 cv = t.counts[sv];
			if (cv + 1ull >= 2ull * cu && mol_before(cv, kv[d], cb, kb)) { best = (uint32_t)sv; kb = kv[d]; cb = cv; }
		}
	}
	parent[slot] = best;
}

// Collapse, the root pass: every molecule walks parent[] to its root -- each step is strictly earlier in the order of the slots'
// own (count, key), so it ends -- and adds its count there; the longest walk is a wave maximum, then one atomic per wave.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_root_kernel(const kt_u64* __restrict__ counts, const uint32_t* __restrict__ occ, int64_t n_occ,
                                                                const uint32_t* __restrict__ parent, kt_u64* __restrict__ collapsed,
                                                                kt_u64* __restrict__ tallies)
{
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int64_t q = (int64_t)blockIdx.x * KT_BLOCK + threadIdx.x;
	int steps = 0;
	bool is_root = false;
	if (q < n_occ) {
		const uint32_t slot = occ[q];
		uint32_t at = slot, up = parent[at];
		while (up != at && (int64_t)steps < n_occ) { at = up; up = parent[at]; steps++; }   // (no walk is longer than the list)
		is_root = at == slot;
		atomicAdd(&collapsed[at], counts[slot]);
	}
	for (int w = 32; w >= 1; w >>= 1) { const int s2 = __shfl_xor(steps, w); steps = s2 > steps ? s2 : steps; }
	const int n_roots = __builtin_popcountll(__builtin_amdgcn_ballot_w64(is_root));
	if (lane == 0) {
		if (n_roots) atomicAdd(&tallies[TDM_ROOTS], (kt_u64)n_roots);
		if (steps) atomicMax(&tallies[TDM_CHAIN], (kt_u64)steps);
	}
}

// The freeze, the keeper pass: one occupied slot per lane walks parent[] to its root as the root pass does and leaves the first
// ordinal of the root's own key -- not the minimum over the tree -- in its own word, one plain 8-byte store.
__global__ __launch_bounds__(KT_BLOCK) void td_mol_keeper_kernel(const uint32_t* __restrict__ occ, int64_t n_occ, const uint32_t* __restrict__ parent,
                                                                  const kt_u64* __restrict__ first, kt_u64* __restrict__ keeper)
{
	const int64_t q = (int64_t)blockIdx.x * KT_BLOCK + threadIdx.x;
	if (q >= n_occ) return;
	const uint32_t slot = occ[q];
	uint32_t at = slot, up = parent[at];
	for (int64_t steps = 0; up != at && steps < n_occ; steps++) { at = up; up = parent[at]; }   // (no walk is longer than the list)
	keeper[slot] = first[at];
}

// Collapse: (key, value, origin) of the listed slots whose value is not 0 into dense arrays -- every molecule with its count
// (td_mol_origins), or the roots with their collapsed counts
__global__ __launch_bounds__(KT_BLOCK) void td_mol_gather_kernel(const kt_u64* __restrict__ keys, const kt_u64* __restrict__ values,
                                                                  const td_mol_origin* __restrict__ origin, const uint32_t* __restrict__ occ,
                                                                  int64_t n_occ, td_census_entry* __restrict__ out, td_mol_origin* __restrict__ out_origin,
                                                                  int64_t cap, kt_u64* __restrict__ cursor)
{
	const int lane = threadIdx.x & (TD_WAVE - 1);
	const int64_t q = (int64_t)blockIdx.x * KT_BLOCK + threadIdx.x;
	uint32_t slot = 0u;
	kt_u64 v = 0ull;
	if (q < n_occ) { slot = occ[q]; v = values[slot]; }
	const int64_t at = kt_wave_place(v != 0ull, cursor, lane);
	if (at >= 0 && at < cap) { out[at].key = keys[slot]; out[at].count = (int64_t)v; out_origin[at] = origin[slot]; }
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
static unsigned blocks_for(int64_t n) { return (unsigned)((n + KT_BLOCK - 1) / KT_BLOCK); }

// the count's totals from its tallies as they came down
static void totals_from(const kt_u64* t, td_mol_totals* out)
{
	out->eligible = (int64_t)t[TDM_ELIGIBLE]; out->counted = (int64_t)t[TDM_COUNTED]; out->skipped_empty = (int64_t)t[TDM_EMPTY];
	out->skipped_n = (int64_t)t[TDM_N]; out->overflow = (int64_t)t[TDM_OVERFLOW]; out->molecules = (int64_t)t[TDM_MOLECULES];
}

// the summary sweep over the table's keys and `counts` (the count's own, or the collapsed ones: a slot that is no root has 0 there
// and is skipped), the rows down
static int summary_rows(td_ctx* c, const kt_u64* counts, td_mol_row rows[TD_NUM_BARCODE_BINS])
{
	TdMolState& z = c->molecules;
	static_assert(sizeof(td_mol_row) == sizeof(kt_u64) * TDM_ROW_WORDS, "td_mol_row is the device row");
	const int64_t n_slots = (int64_t)1 << z.table.log2_slots;
	HIPCHK(c, hipMemsetAsync(z.d_rows, 0, sizeof(td_mol_row) * TD_NUM_BARCODE_BINS, c->stream));
	hipLaunchKernelGGL(td_mol_summary_kernel, dim3(std::min(blocks_for(n_slots), 1024u)), dim3(KT_BLOCK), 0, c->stream, (const kt_u64*)z.table.d_keys,
	                   counts, n_slots, z.d_rows);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(rows, z.d_rows, sizeof(td_mol_row) * TD_NUM_BARCODE_BINS, hipMemcpyDeviceToHost));
	return TD_OK;
}

// one array of an element of `elem_bytes` per table slot: first ordinals, origins, parents, collapsed counts, keepers
static hipError_t alloc_per_slot(const TdMolState& z, void** p, size_t elem_bytes) { return hipMalloc(p, elem_bytes << z.table.log2_slots); }

// A stage's group released: what it owns freed, the group as it was before the stage was ever on (nothing of it is queued any more).
// A group's arrays and events exist while it is on and inside an enable that has not yet succeeded, which releases what it got.
static void frozen_release(TdMolState& z)
{
	if (z.frozen.d_keeper) (void)hipFree(z.frozen.d_keeper);
	kt_pair_destroy(z.frozen.ev);
	z.frozen = TdMolFrozen();
}

static void dedup_release(TdMolState& z)
{
	if (z.dedup.d_first) (void)hipFree(z.dedup.d_first);
	for (hipEvent_t e : z.dedup.ev_p1) if (e) (void)hipEventDestroy(e);
	kt_pair_destroy(z.dedup.ev);
	z.dedup = TdMolDedup();
	frozen_release(z);                                // the frozen state needs dedup and the collapse: it ends with either
}

static void collapse_release(TdMolState& z)
{
	void* p[] = { z.collapse.d_origin, z.collapse.d_occ, z.collapse.d_parent, z.collapse.d_collapsed };
	for (void* q : p) if (q) (void)hipFree(q);
	kt_pair_destroy(z.collapse.ev);
	z.collapse = TdMolCollapse();
	frozen_release(z);
}

void mol_release(td_ctx* c)
{
	TdMolState& z = c->molecules;
	kt_table_release(z.table);
	if (z.d_rows) (void)hipFree(z.d_rows);
	dedup_release(z);
	collapse_release(z);
	kt_pair_destroy(z.mate.ev);
	kt_pair_destroy(z.mate.ev_filter);
	kt_pair_destroy(z.mate.ev_join);
	z = TdMolState();                                 // (mate mode and the mate filter off with it, a named mate batch forgotten)
}

// A decoded slot's launches, queued on its compute stream: the count, then the collapse's origin pass, then dedup's two passes, each
// only when it is on and each between its own pair of events.  The order matters: dedup's pass 2 rewrites the outcomes the others
// read.  In the frozen state the replay kernel alone, between its own pair: keys, counts, origins, first ordinals and the count's
// tallies stay as the survey left them.
int mol_slot_decoded(td_ctx* c, TdSlot& s, int32_t* out_type, const int32_t* out_barcode, const int32_t* out_finger, const int8_t* labels)
{
	TdMolState& z = c->molecules;
	TdMolArgs a{};
	a.tile = kt_tile_view(s, labels); a.lens = s.d_lens; a.out_type = out_type; a.out_barcode = out_barcode; a.out_finger = out_finger;
	a.label = z.table.d_label; a.n_reads = s.n_reads; a.n_tiles = s.n_tiles; a.H = z.table.H;
	a.r_segs = z.r_segs; a.prefix = z.prefix;
	a.table = kt_table_view(z.table); a.tallies = z.table.d_tallies;
	if (z.mate.bases > 0) {                           // (slot_decode has checked that the slot holds this batch's mates, made with this M)
		a.mate_w = s.d_mate_w; a.mate_n = s.d_mate_n; a.mate_bases = z.mate.bases;
		a.read_at = s.sorted ? s.d_read_at : nullptr;
	}
	if (z.frozen.on) {
		a.ordinal_base = z.dedup.next_ordinal;        // reads submitted since the freeze: the rule of the survey
		z.dedup.next_ordinal += s.n_reads;
		a.read_at = s.sorted ? s.d_read_at : nullptr; a.keeper = z.frozen.d_keeper;
		if (kt_launch_slot(c, z.frozen.ev, s, (const void*)td_mol_replay_kernel, &a) != TD_OK) return TD_FAIL;
		return kt_slot_read_behind(c, s);
	}
	if (kt_launch_slot(c, z.table.ev, s, (const void*)td_mol_count_kernel, &a) != TD_OK) return TD_FAIL;
	if (z.collapse.on) {
		a.origin = z.collapse.d_origin;
		if (kt_launch_slot(c, z.collapse.ev, s, (const void*)td_mol_origin_kernel, &a) != TD_OK) return TD_FAIL;
	}
	if (z.dedup.on) {
		a.ordinal_base = z.dedup.next_ordinal;        // batches get their ordinals in the order they are submitted in
		z.dedup.next_ordinal += s.n_reads;
	}
	if (z.dedup.on && s.n_tiles > 0) {                // (a batch without tiles leaves dedup's pair as the batch before left it)
		TdMolDedup& d = z.dedup;
		if (ensure(c, &s.d_judged, &s.cap_judged, (size_t)s.n_tiles * TD_WAVE * sizeof(int32_t)) != TD_OK) return TD_FAIL;
		a.read_at = s.sorted ? s.d_read_at : nullptr; a.first = d.d_first; a.judged = s.d_judged;
		HIPCHK(c, hipEventRecord(d.ev.e0, s.cs));
		if (kt_launch_tiles(c, s, (const void*)td_mol_first_kernel, &a) != TD_OK) return TD_FAIL;
		// The batch before this one may run on the other compute stream, and it holds the smaller ordinals: its pass 1 has to be over
		// before this batch's pass 2 reads a first ordinal.  (The batch before that one ran on this stream, or was waited for.)
		const int t = d.turn;
		HIPCHK(c, hipEventRecord(d.ev_p1[t], s.cs));
		d.p1_queued[t] = true;
		if (d.p1_queued[t ^ 1]) HIPCHK(c, hipStreamWaitEvent(s.cs, d.ev_p1[t ^ 1], 0));
		d.turn = t ^ 1;
		hipLaunchKernelGGL(td_mol_mark_kernel, dim3((unsigned)((s.n_tiles + KT_WAVES - 1) / KT_WAVES)), dim3(KT_BLOCK), 0, s.cs, out_type,
		                   (const int32_t*)s.d_judged, a.read_at, (const kt_u64*)d.d_first, a.ordinal_base, a.n_reads, a.n_tiles, z.table.d_tallies);
		HIPCHK(c, hipGetLastError());
		HIPCHK(c, hipEventRecord(d.ev.e1, s.cs));
	}
	// behind the last of them: the finish kernel copies out_type only behind pass 2, and the slot is not restaged under any of these
	return kt_slot_read_behind(c, s);
}

extern "C" int td_mol_enable(td_ctx* c, int32_t prefix_bases, int32_t log2_slots)
{
	if (!c) return TD_FAIL;
	if (!c->have_model) return fail(c, "td_mol_enable: no model uploaded");
	if (tickets_outstanding(c)) return fail(c, "td_mol_enable: td_submit tickets are outstanding (td_wait them first)");
	if (!mol_prefix_ok(prefix_bases)) return fail(c, "td_mol_enable: prefix_bases = %d (1..%d supported)", prefix_bases, TD_MOL_MAX_PREFIX);
	if (log2_slots == 0) log2_slots = TD_MOL_DEFAULT_LOG2_SLOTS;
	if (log2_slots < 4 || log2_slots > 30) return fail(c, "td_mol_enable: log2_slots = %d (4..30 supported, 0 = the default of %d)", log2_slots, TD_MOL_DEFAULT_LOG2_SLOTS);
	if (c->match_len > 0) return fail(c, "td_mol_enable: a -start/-end window is set (td_set_window): labels behind a window do not mark the read's bases");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
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
	if (c->molecules.on && wait_compute(c) != TD_OK) return TD_FAIL;
	mol_release(c);   // (off: there is nothing to free)
	return TD_OK;
}

extern "C" int td_mol_reset(td_ctx* c)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_reset: the molecule count is off (td_mol_enable)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;   // (counts of pipelined batches may still be queued, on either compute stream)
	HIPCHK(c, kt_table_zero(z.table, c->stream));   // (dedup's three tallies among them)
	if (z.dedup.on) HIPCHK(c, hipMemsetAsync(z.dedup.d_first, 0xFF, sizeof(kt_u64) << z.table.log2_slots, c->stream));
	if (z.collapse.on) HIPCHK(c, hipMemsetAsync(z.collapse.d_origin, 0, sizeof(td_mol_origin) << z.table.log2_slots, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	z.dedup.start_over();                             // (nothing is queued any more)
	z.frozen.on = false;                              // (the table is empty: the context surveys again; the keepers wait for the next freeze)
	return TD_OK;
}

// ---- mate mode ----
extern "C" int td_mol_mate_enable(td_ctx* c, int32_t mate_bases)
{
	if (!c) return fail(nullptr, "td_mol_mate_enable: no context");
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_mate_enable: the molecule count is off (td_mol_enable first): the mate joins the count's key");
	if (tickets_outstanding(c)) return fail(c, "td_mol_mate_enable: td_submit tickets are outstanding (td_wait them first)");
	if (mate_bases < 1 || z.prefix + mate_bases > TD_MOL_MAX_PREFIX)
		return fail(c, "td_mol_mate_enable: mate_bases = %d with prefix_bases = %d (1..%d supported: both share one 64-bit word of %d bases)", mate_bases,
		            z.prefix, TD_MOL_MAX_PREFIX - z.prefix, TD_MOL_MAX_PREFIX);
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	if (!z.mate.ev.e0) HIPCHK(c, kt_pair_create(z.mate.ev));   // (the pair outlives td_mol_mate_disable: the count's release destroys it)
	z.mate.bases = mate_bases;
	z.mate.named = false;
	return td_mol_reset(c);   // a table never mixes keys made with and without a mate, or with two M
}

extern "C" int td_mol_mate_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.on || z.mate.bases == 0) return TD_OK;     // (off: there is nothing to do)
	if (tickets_outstanding(c)) return fail(c, "td_mol_mate_disable: td_submit tickets are outstanding (td_wait them first)");
	z.mate.bases = 0;
	z.mate.named = false;
	z.mate.filter = false;                            // (the filter judges mates: it goes with them)
	return td_mol_reset(c);
}

// ---- the mate filter ----
static int mate_filter_switch(td_ctx* c, bool on, const char* who)
{
	if (!c) return fail(nullptr, "%s: no context", who);
	TdMolState& z = c->molecules;
	if (!z.on || z.mate.bases == 0) return fail(c, "%s: mate mode is off (td_mol_mate_enable first): the filter judges the mates of a batch", who);
	if (tickets_outstanding(c)) return fail(c, "%s: td_submit tickets are outstanding (td_wait them first)", who);
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	if (on && !z.mate.ev_filter.e0) HIPCHK(c, kt_pair_create(z.mate.ev_filter));   // (the pairs outlive the switch: the count's release destroys them)
	if (on && !z.mate.ev_join.e0) HIPCHK(c, kt_pair_create(z.mate.ev_join));
	z.mate.filter = on;
	z.mate.named = false;
	return td_mol_reset(c);   // a table never holds counts made under two eligibility rules
}

extern "C" int td_mol_mate_filter_enable(td_ctx* c) { return mate_filter_switch(c, true, "td_mol_mate_filter_enable"); }
extern "C" int td_mol_mate_filter_disable(td_ctx* c) { return mate_filter_switch(c, false, "td_mol_mate_filter_disable"); }

extern "C" int td_mol_mate_types(td_ctx* c, int32_t* types, int64_t cap, int64_t* n)
{
	if (!c) return fail(nullptr, "td_mol_mate_types: no context");
	if (!n || cap < 0 || (!types && cap > 0)) return fail(c, "td_mol_mate_types: bad arguments");
	const TdMolState& z = c->molecules;
	if (!z.mate.filter) return fail(c, "td_mol_mate_types: the mate filter is off (td_mol_mate_filter_enable)");
	const TdSlot& s = c->slots[0];
	if (!s.staged || s.mate_m == 0 || !s.mate_judged)
		return fail(c, "td_mol_mate_types: no batch is resident that was staged with its mates while the filter was on (td_mol_mate_next, then td_batch_upload)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	*n = s.n_reads;
	const int64_t m = s.n_reads < cap ? s.n_reads : cap;
	if (m <= 0) return TD_OK;
	if (!s.mate_typed) { memset(types, 0, (size_t)m * sizeof(int32_t)); return TD_OK; }   // neither DUST nor artifacts: the kernel did not run
	HIPCHK(c, hipMemcpy(types, s.d_mate_type, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
	return TD_OK;
}

extern "C" int td_mol_mate_next(td_ctx* c, const uint8_t* codes, const int64_t* offs, int64_t n_reads)
{
	if (!c) return fail(nullptr, "td_mol_mate_next: no context");
	TdMolState& z = c->molecules;
	if (z.mate.bases == 0) return fail(c, "td_mol_mate_next: mate mode is off (td_mol_mate_enable)");
	if (!offs || n_reads < 0 || (!codes && n_reads > 0 && offs[n_reads] > offs[0])) return fail(c, "td_mol_mate_next: bad arguments");
	z.mate.codes = codes; z.mate.offs = offs; z.mate.reads = n_reads; z.mate.named = true;
	return TD_OK;
}

int mol_mate_check(td_ctx* c, int64_t n, const char* who)
{
	TdMolMate& z = c->molecules.mate;
	if (!z.named)
		return fail(c, "%s: mate mode is on (td_mol_mate_enable, %d bases) and no mate batch is named for this batch of %lld reads (td_mol_mate_next "
		            "first); nothing was counted", who, z.bases, (long long)n);
	if (z.reads != n) {
		z.named = false;
		return fail(c, "%s: the named mate batch has %lld reads, the batch %lld: mate i belongs to read i; the mate batch is dropped, nothing was counted",
		            who, (long long)z.reads, (long long)n);
	}
	return TD_OK;
}

int mol_mate_stage(td_ctx* c, TdSlot& s, int64_t n, hipStream_t up)
{
	TdMolMate& z = c->molecules.mate;
	const uint8_t* codes = z.codes;
	const int64_t* offs = z.offs;
	z.named = false;                                  // consumed, whatever happens below
	const int64_t base = offs[0];
	if (ensure_pinned(c, &s.h_mate_offs, &s.cap_h_mate_offs, (size_t)(n + 1) * 8) != TD_OK) return TD_FAIL;
	s.h_mate_offs[0] = 0;
	for (int64_t i = 0; i < n; i++) {                 // the kernel trusts these: every mate ends where the next begins, none is negative
		const int64_t l = offs[i + 1] - offs[i];
		if (l < 0 || l > 100000) return fail(c, "td_mol_mate_next: mate %lld has length %lld", (long long)i, (long long)l);
		s.h_mate_offs[i + 1] = offs[i + 1] - base;
	}
	const int64_t n_bases = n > 0 ? offs[n] - base : 0;
	// (the filter kernel loads whole dwords: the bytes up to the next multiple of 4 belong to the allocation, nobody uses their values)
	const size_t raw_bytes = z.filter ? ((size_t)n_bases + 3) & ~(size_t)3 : (size_t)n_bases;
	if (ensure(c, &s.d_mate_raw, &s.cap_mate_raw, raw_bytes) != TD_OK || ensure(c, &s.d_mate_offs, &s.cap_mate_offs, (size_t)(n + 1) * 8) != TD_OK ||
	    ensure(c, &s.d_mate_w, &s.cap_mate_w, (size_t)n * 8) != TD_OK || ensure(c, &s.d_mate_n, &s.cap_mate_n, (size_t)n) != TD_OK)
		return TD_FAIL;
	// host -> device as the batch's own bases go: page-locked caller memory straight to the DMA engine, anything else through pinned staging
	const void* src = codes + base;
	s.mate_direct = n_bases > 0 && is_pinned(src);
	if (n_bases > 0 && !s.mate_direct) {
		if (ensure_pinned(c, &s.h_mate_raw, &s.cap_h_mate_raw, (size_t)n_bases) != TD_OK) return TD_FAIL;
		c->pool.copy(s.h_mate_raw, src, (size_t)n_bases, c->host_threads);
		src = s.h_mate_raw;
	}
	HIPCHK(c, hipMemcpyAsync(s.d_mate_offs, s.h_mate_offs, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, up));
	if (n_bases > 0) HIPCHK(c, hipMemcpyAsync(s.d_mate_raw, src, (size_t)n_bases, hipMemcpyHostToDevice, up));
	s.mate_m = z.bases;
	return TD_OK;
}

int mol_mate_launch(td_ctx* c, TdSlot& s, int64_t n)
{
	const TdMolMate& z = c->molecules.mate;
	HIPCHK(c, hipEventRecord(z.ev.e0, s.aux));
	if (n > 0) {
		hipLaunchKernelGGL(td_mol_mate_kernel, dim3(blocks_for(n)), dim3(KT_BLOCK), 0, s.aux, (const uint8_t*)s.d_mate_raw, (const int64_t*)s.d_mate_offs, n,
		                   z.bases, s.d_mate_w, s.d_mate_n);
		HIPCHK(c, hipGetLastError());
	}
	HIPCHK(c, hipEventRecord(z.ev.e1, s.aux));
	if (!z.filter) return TD_OK;
	// The mate filter: the mates judged under the context's settings as they stand now.  Without DUST and artifacts every verdict is
	// 0: no launch, no buffer, and the join is left out as well.
	s.mate_judged = true;
	if (c->dust == 0 && c->art_n == 0) return TD_OK;
	if (ensure(c, &s.d_mate_type, &s.cap_mate_type, (size_t)n * sizeof(int32_t)) != TD_OK) return TD_FAIL;
	TdMateFilterArgs fa{};
	fa.raw = s.d_mate_raw; fa.offs = s.d_mate_offs; fa.n_reads = n; fa.dust = c->dust;
	fa.art_pk = c->d_art_pk; fa.art_seq = c->d_art_seq; fa.art_n = c->art_n; fa.art_fe = c->art_fe;
	fa.art_threads = c->art_threads; fa.win_first = c->win_first; fa.win_total = c->win_total;
	fa.mate_type = s.d_mate_type;
	HIPCHK(c, hipEventRecord(z.ev_filter.e0, s.aux));
	HIPCHK(c, td_launch_mate_filter(fa, s.aux));
	HIPCHK(c, hipEventRecord(z.ev_filter.e1, s.aux));
	s.mate_typed = true;
	return TD_OK;
}

// out_type[k] = max(out_type[k], the type of read k's mate) on the slot's compute stream: behind ev_k1, in front of the -ref hit
// count, the census and the count.  (The stream's wait for ev_pack covers the filter kernel.)
int mol_mate_join(td_ctx* c, TdSlot& s, int32_t* out_type)
{
	const TdMolMate& z = c->molecules.mate;
	if (!s.mate_typed) return TD_OK;                  // (every mate type is 0, and no outcome is below 0)
	HIPCHK(c, hipEventRecord(z.ev_join.e0, s.cs));
	HIPCHK(c, td_launch_mate_join(out_type, s.d_mate_type, s.sorted ? s.d_read_at : nullptr, s.n_reads, s.cs));
	HIPCHK(c, hipEventRecord(z.ev_join.e1, s.cs));
	return TD_OK;
}

extern "C" int td_mol_dedup_enable(td_ctx* c)
{
	if (!c) return fail(nullptr, "td_mol_dedup_enable: no context");
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_dedup_enable: the molecule count is off (td_mol_enable first): dedup judges the reads the count has keyed");
	if (tickets_outstanding(c)) return fail(c, "td_mol_dedup_enable: td_submit tickets are outstanding (td_wait them first)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	if (!z.dedup.on) {
		TdMolDedup& d = z.dedup;
		bool ok = alloc_per_slot(z, (void**)&d.d_first, sizeof(kt_u64)) == hipSuccess &&
		          hipEventCreateWithFlags(&d.ev_p1[0], hipEventDisableTiming) == hipSuccess &&
		          hipEventCreateWithFlags(&d.ev_p1[1], hipEventDisableTiming) == hipSuccess && kt_pair_create(d.ev) == hipSuccess;
		if (!ok) {
			const std::string e = hipGetErrorString(hipGetLastError());
			dedup_release(z);
			return fail(c, "td_mol_dedup_enable: the first ordinals of 2^%d slots could not be set up: %s", z.table.log2_slots, e.c_str());
		}
		z.dedup.on = true;
	}
	return td_mol_reset(c);   // a first ordinal belongs to a key that entered the table with it: both start empty
}

extern "C" int td_mol_dedup_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	if (c->molecules.dedup.on && wait_compute(c) != TD_OK) return TD_FAIL;
	if (c->molecules.frozen.on && td_mol_reset(c) != TD_OK) return TD_FAIL;   // the frozen state ends with an empty table
	dedup_release(c->molecules);   // (off: there is nothing to free)
	return TD_OK;
}

extern "C" int td_mol_dedup_get(td_ctx* c, td_mol_dedup_totals* totals)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.dedup.on) return fail(c, "td_mol_dedup_get: dedup is off (td_mol_dedup_enable)");
	if (!totals) return fail(c, "td_mol_dedup_get: bad arguments");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
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
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	if (summary_rows(c, z.table.d_counts, rows) != TD_OK) return TD_FAIL;
	if (totals) {
		kt_u64 t[TDM_TALLY_WORDS];
		HIPCHK(c, hipMemcpy(t, z.table.d_tallies, sizeof t, hipMemcpyDeviceToHost));
		totals_from(t, totals);
	}
	return TD_OK;
}

// ---- collapse ----
extern "C" int td_mol_collapse_enable(td_ctx* c)
{
	if (!c) return fail(nullptr, "td_mol_collapse_enable: no context");
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_collapse_enable: the molecule count is off (td_mol_enable first): the collapse reads the count's table");
	const td_model_desc& m = c->model.d;
	bool has_f = false;
	for (int j = 0; j < m.S; j++) has_f = has_f || m.seg_type[j] == 'F';
	if (!has_f) return fail(c, "td_mol_collapse_enable: the model has no 'F' segment: there is no UMI whose neighbours could be collapsed");
	if (tickets_outstanding(c)) return fail(c, "td_mol_collapse_enable: td_submit tickets are outstanding (td_wait them first)");
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	if (!z.collapse.on) {
		bool ok = alloc_per_slot(z, (void**)&z.collapse.d_origin, sizeof(td_mol_origin)) == hipSuccess && kt_pair_create(z.collapse.ev) == hipSuccess;
		if (!ok) {
			const std::string e = hipGetErrorString(hipGetLastError());
			collapse_release(z);
			return fail(c, "td_mol_collapse_enable: the origins of 2^%d slots could not be set up: %s", z.table.log2_slots, e.c_str());
		}
		z.collapse.on = true;
	}
	return td_mol_reset(c);   // an origin belongs to a key that entered the table with it: both start empty
}

extern "C" int td_mol_collapse_disable(td_ctx* c)
{
	if (!c) return TD_FAIL;
	if (c->molecules.collapse.on && wait_compute(c) != TD_OK) return TD_FAIL;
	if (c->molecules.frozen.on && td_mol_reset(c) != TD_OK) return TD_FAIL;   // the frozen state ends with an empty table
	collapse_release(c->molecules);   // (off: there is nothing to free)
	return TD_OK;
}

namespace {

// Waits for the context's work; tallies[TDM_TALLY_WORDS] down, and the occupied slots' indices in the collapse's d_occ: *n_occ of them, held
// against the count's own tally of distinct keys
int collapse_occupied(td_ctx* c, const char* who, kt_u64* tallies, int64_t* n_occ)
{
	TdMolState& z = c->molecules;
	if (wait_compute(c) != TD_OK) return TD_FAIL;
	HIPCHK(c, hipMemcpy(tallies, z.table.d_tallies, sizeof(kt_u64) * TDM_TALLY_WORDS, hipMemcpyDeviceToHost));
	const int64_t distinct = (int64_t)tallies[TDM_MOLECULES];
	*n_occ = distinct;
	if (distinct == 0) return TD_OK;
	if (ensure(c, &z.collapse.d_occ, &z.collapse.cap_occ, sizeof(uint32_t) * (size_t)distinct) != TD_OK) return TD_FAIL;
	const int64_t n_slots = (int64_t)1 << z.table.log2_slots;
	kt_u64* cursor = z.table.d_tallies + TDM_GATHERED;
	int64_t found = 0;
	if (kt_sweep_dense(c, who, "the sweep over the occupied slots failed", cursor, 0, nullptr, 0, nullptr, 0, [&](void*, void*) {
		    hipLaunchKernelGGL(td_mol_occupied_kernel, dim3(std::min(blocks_for(n_slots), 2048u)), dim3(KT_BLOCK), 0, c->stream,
		                       (const kt_u64*)z.table.d_keys, n_slots, z.collapse.d_occ, distinct, cursor);
	    }, &found) != TD_OK) return TD_FAIL;
	if (found != distinct) return fail(c, "%s: the table holds %lld keys, its tally says %lld", who, (long long)found, (long long)distinct);
	return TD_OK;
}

// The listed slots whose `values` word is not 0 as sorted entries with their origins: `expect` of them; *n = their number, the first
// min(cap, *n) copied
int collapse_gather(td_ctx* c, const char* who, const kt_u64* values, int64_t n_occ, int64_t expect, td_census_entry* entries,
                    td_mol_origin* origins, int64_t cap, int64_t* n)
{
	TdMolState& z = c->molecules;
	*n = expect;
	if (expect == 0) return TD_OK;
	std::vector<td_census_entry> v((size_t)expect);
	std::vector<td_mol_origin> vo((size_t)expect);
	kt_u64* cursor = z.table.d_tallies + TDM_GATHERED;
	int64_t found = 0;
	if (kt_sweep_dense(c, who, "the gather failed", cursor, (size_t)expect, v.data(), sizeof(td_census_entry), vo.data(), sizeof(td_mol_origin),
	                   [&](void* d_e, void* d_o) {
		    hipLaunchKernelGGL(td_mol_gather_kernel, dim3(blocks_for(n_occ)), dim3(KT_BLOCK), 0, c->stream, (const kt_u64*)z.table.d_keys, values,
		                       (const td_mol_origin*)z.collapse.d_origin, (const uint32_t*)z.collapse.d_occ, n_occ, (td_census_entry*)d_e, (td_mol_origin*)d_o, expect, cursor);
	    }, &found) != TD_OK) return TD_FAIL;
	if (found != expect) return fail(c, "%s: %lld entries were gathered, %lld expected", who, (long long)found, (long long)expect);
	mol_emit_ordered(v.data(), vo.data(), expect, cap, entries, origins);
	return TD_OK;
}

// The collapse on the device: d_occ, d_parent and d_collapsed of the table as it stands; the totals
int collapse_run(td_ctx* c, const char* who, int64_t* n_occ, td_mol_collapse_totals* totals)
{
	TdMolState& z = c->molecules;
	TdMolCollapse& o = z.collapse;
	if (!o.on) return fail(c, "%s: the collapse is off (td_mol_collapse_enable)", who);
	kt_u64 t[TDM_TALLY_WORDS];
	if (collapse_occupied(c, who, t, n_occ) != TD_OK) return TD_FAIL;
	if (!o.d_parent) HIPCHK(c, alloc_per_slot(z, (void**)&o.d_parent, sizeof(uint32_t)));
	if (!o.d_collapsed) HIPCHK(c, alloc_per_slot(z, (void**)&o.d_collapsed, sizeof(kt_u64)));
	HIPCHK(c, hipMemsetAsync(o.d_collapsed, 0, sizeof(kt_u64) << z.table.log2_slots, c->stream));
	HIPCHK(c, hipMemsetAsync(z.table.d_tallies + TDM_ROOTS, 0, sizeof(kt_u64) * 2, c->stream));   // (TDM_ROOTS, TDM_CHAIN)
	static_assert(TDM_CHAIN == TDM_ROOTS + 1, "the two are zeroed together");
	if (*n_occ > 0) {
		hipLaunchKernelGGL(td_mol_parent_kernel, dim3(blocks_for(*n_occ)), dim3(KT_BLOCK), 0, c->stream, kt_table_view(z.table),
		                   (const td_mol_origin*)o.d_origin, (const uint32_t*)o.d_occ, *n_occ, o.d_parent);
		HIPCHK(c, hipGetLastError());
		hipLaunchKernelGGL(td_mol_root_kernel, dim3(blocks_for(*n_occ)), dim3(KT_BLOCK), 0, c->stream, (const kt_u64*)z.table.d_counts,
		                   (const uint32_t*)o.d_occ, *n_occ, (const uint32_t*)o.d_parent, o.d_collapsed, z.table.d_tallies);
		HIPCHK(c, hipGetLastError());
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
	kt_u64 rc[2];
	HIPCHK(c, hipMemcpy(rc, z.table.d_tallies + TDM_ROOTS, sizeof rc, hipMemcpyDeviceToHost));
	totals->molecules_before = *n_occ; totals->molecules_after = (int64_t)rc[0];
	totals->absorbed = *n_occ - (int64_t)rc[0]; totals->longest_chain = (int64_t)rc[1];
	return TD_OK;
}

}   // namespace

extern "C" int td_mol_origins(td_ctx* c, td_census_entry* entries, td_mol_origin* origins, int64_t cap, int64_t* n, td_mol_totals* totals)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!z.collapse.on) return fail(c, "td_mol_origins: the collapse is off (td_mol_collapse_enable)");
	if (cap < 0 || (cap > 0 && (!entries || !origins)) || !n) return fail(c, "td_mol_origins: bad arguments");
	*n = 0;
	kt_u64 t[TDM_TALLY_WORDS];
	int64_t n_occ = 0;
	if (collapse_occupied(c, "td_mol_origins", t, &n_occ) != TD_OK) return TD_FAIL;
	if (collapse_gather(c, "td_mol_origins", z.table.d_counts, n_occ, n_occ, entries, origins, cap, n) != TD_OK) return TD_FAIL;
	if (totals) totals_from(t, totals);
	return TD_OK;
}

extern "C" int td_mol_collapse_get(td_ctx* c, td_mol_row rows[TD_NUM_BARCODE_BINS], td_mol_collapse_totals* totals)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (!rows) return fail(c, "td_mol_collapse_get: bad arguments");
	int64_t n_occ = 0;
	td_mol_collapse_totals t{};
	if (collapse_run(c, "td_mol_collapse_get", &n_occ, &t) != TD_OK) return TD_FAIL;
	if (summary_rows(c, z.collapse.d_collapsed, rows) != TD_OK) return TD_FAIL;   // the count's own sweep over the collapsed counts
	if (totals) *totals = t;
	return TD_OK;
}

extern "C" int td_mol_collapse_entries(td_ctx* c, td_census_entry* entries, td_mol_origin* origins, int64_t cap, int64_t* n,
                                       td_mol_collapse_totals* totals)
{
	if (!c) return TD_FAIL;
	TdMolState& z = c->molecules;
	if (cap < 0 || (cap > 0 && (!entries || !origins)) || !n) return fail(c, "td_mol_collapse_entries: bad arguments");
	*n = 0;
	int64_t n_occ = 0;
	td_mol_collapse_totals t{};
	if (collapse_run(c, "td_mol_collapse_entries", &n_occ, &t) != TD_OK) return TD_FAIL;
	if (collapse_gather(c, "td_mol_collapse_entries", z.collapse.d_collapsed, n_occ, t.molecules_after, entries, origins, cap, n) != TD_OK) return TD_FAIL;
	if (totals) *totals = t;
	return TD_OK;
}

// ---- the frozen state ----
extern "C" int td_mol_dedup_freeze(td_ctx* c, td_mol_collapse_totals* totals)
{
	if (!c) return fail(nullptr, "td_mol_dedup_freeze: no context");
	TdMolState& z = c->molecules;
	if (!z.on) return fail(c, "td_mol_dedup_freeze: the molecule count is off (td_mol_enable)");
	if (!z.dedup.on) return fail(c, "td_mol_dedup_freeze: dedup is off (td_mol_dedup_enable)");
	if (!z.collapse.on) return fail(c, "td_mol_dedup_freeze: the collapse is off (td_mol_collapse_enable)");
	if (tickets_outstanding(c)) return fail(c, "td_mol_dedup_freeze: td_submit tickets are outstanding (td_wait them first)");
	int64_t n_occ = 0;
	td_mol_collapse_totals t{};
	if (collapse_run(c, "td_mol_dedup_freeze", &n_occ, &t) != TD_OK) return TD_FAIL;   // (waits for the context's queued work)
	if (!z.frozen.d_keeper) {
		const bool ok = alloc_per_slot(z, (void**)&z.frozen.d_keeper, sizeof(kt_u64)) == hipSuccess && kt_pair_create(z.frozen.ev) == hipSuccess;
		if (!ok) {
			const std::string e = hipGetErrorString(hipGetLastError());
			frozen_release(z);
			return fail(c, "td_mol_dedup_freeze: the keepers of 2^%d slots could not be set up: %s", z.table.log2_slots, e.c_str());
		}
	}
	if (n_occ > 0) {
		hipLaunchKernelGGL(td_mol_keeper_kernel, dim3(blocks_for(n_occ)), dim3(KT_BLOCK), 0, c->stream, (const uint32_t*)z.collapse.d_occ, n_occ,
		                   (const uint32_t*)z.collapse.d_parent, (const kt_u64*)z.dedup.d_first, z.frozen.d_keeper);
		HIPCHK(c, hipGetLastError());
	}
	HIPCHK(c, hipMemsetAsync(z.table.d_tallies + TDM_KEPT, 0, sizeof(kt_u64) * 3, c->stream));   // (TDM_KEPT, TDM_DUPLICATES, TDM_UNJUDGED)
	static_assert(TDM_DUPLICATES == TDM_KEPT + 1 && TDM_UNJUDGED == TDM_KEPT + 2, "the three are zeroed together");
	HIPCHK(c, hipStreamSynchronize(c->stream));
	z.dedup.start_over();                             // (nothing is queued any more: the replay's ordinals are those of the reads since)
	z.frozen.on = true;
	if (totals) *totals = t;
	return TD_OK;
}

// ---- the "*_kernel_us" options ----
// One row per option: the stage's pair, whether the stage is on, and what it refuses with while it is off / before its first batch.
// dedup_kernel_us: between the two passes the stream waits for the batch before -- with batches in flight on both compute streams
// that wait is inside the figure, after a td_run it is not.
static const struct {
	const char* name;
	const KtEventPair& (*pair)(const TdMolState&);
	bool (*on)(const TdMolState&);
	const char* off;
	const char* none_yet;
} kMolKernelUs[] = {
	{ "molecules_kernel_us", [](const TdMolState& z) -> const KtEventPair& { return z.table.ev; }, [](const TdMolState& z) { return z.on; },
	  "td_get_option: molecules_kernel_us: the molecule count is off", "td_get_option: molecules_kernel_us: no batch has been counted yet" },
	{ "dedup_kernel_us", [](const TdMolState& z) -> const KtEventPair& { return z.dedup.ev; }, [](const TdMolState& z) { return z.dedup.on; },
	  "td_get_option: dedup_kernel_us: dedup is off", "td_get_option: dedup_kernel_us: no batch has been judged yet" },
	{ "collapse_origin_kernel_us", [](const TdMolState& z) -> const KtEventPair& { return z.collapse.ev; }, [](const TdMolState& z) { return z.collapse.on; },
	  "td_get_option: collapse_origin_kernel_us: the collapse is off", "td_get_option: collapse_origin_kernel_us: no batch has left its origins yet" },
	{ "dedup_replay_kernel_us", [](const TdMolState& z) -> const KtEventPair& { return z.frozen.ev; }, [](const TdMolState& z) { return z.frozen.on; },
	  "td_get_option: dedup_replay_kernel_us: the context is not frozen (td_mol_dedup_freeze)",
	  "td_get_option: dedup_replay_kernel_us: no batch has been replayed yet" },
	{ "mate_kernel_us", [](const TdMolState& z) -> const KtEventPair& { return z.mate.ev; }, [](const TdMolState& z) { return z.mate.bases != 0; },
	  "td_get_option: mate_kernel_us: mate mode is off", "td_get_option: mate_kernel_us: no mate batch has been staged yet" },
	{ "mate_filter_kernel_us", [](const TdMolState& z) -> const KtEventPair& { return z.mate.ev_filter; }, [](const TdMolState& z) { return z.mate.filter; },
	  "td_get_option: mate_filter_kernel_us: the mate filter is off", "td_get_option: mate_filter_kernel_us: no mate batch has been judged yet" },
	{ "mate_join_kernel_us", [](const TdMolState& z) -> const KtEventPair& { return z.mate.ev_join; }, [](const TdMolState& z) { return z.mate.filter; },
	  "td_get_option: mate_join_kernel_us: the mate filter is off", "td_get_option: mate_join_kernel_us: no batch has been joined yet" },
};

int mol_kernel_us(td_ctx* c, const char* name, int32_t* us)
{
	for (const auto& o : kMolKernelUs) {
		if (strcmp(name, o.name) != 0) continue;
		if (!o.on(c->molecules)) return fail(c, "%s", o.off);
		return kt_last_kernel_us(c, o.pair(c->molecules), us, o.none_yet);
	}
	return -1;
}
