// td_count_key.h -- what the device units of the two counts (td_census.hip, td_molecules.hip, td_keytable.hip) and their host units
// (td_census_host.cpp, td_molecules_host.cpp) share: the integer arithmetic of a key, the same text for both sides, and the few
// hidden functions one side needs of the other.  No HIP header and nothing of the context comes with it: the host units and the
// stand-alone programs over them (tools/*_host_check.cpp) build with a plain C++ compiler.  <vector> is here for kt_copy_entries
// and kt_tally_keys alone.  Nothing here is exported.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/tagdust_census.h"
#include "../../include/tagdust_molecules.h"

#ifdef __HIPCC__
#define KT_BOTH __host__ __device__ inline __attribute__((always_inline))   // (__forceinline__, spelled out: that macro is a HIP header's)
#else
#define KT_BOTH static inline
#endif
#define KT_HIDDEN __attribute__((visibility("hidden")))
#define KEY_LOW_MASK 0x00FFFFFFFFFFFFFFull

typedef unsigned long long kt_u64;

struct td_ctx;
KT_HIDDEN int fail(td_ctx* c, const char* fmt, ...);   // (td_api.hip) TD_FAIL, and the message for td_last_error

// splitmix64's finish: every bit of k reaches every bit of the result
KT_BOTH kt_u64 kt_mix(kt_u64 k)
{
	k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ull;
	k ^= k >> 27; k *= 0x94D049BB133111EBull;
	k ^= k >> 31;
	return k;
}

// the key of tagdust_molecules.h
KT_BOTH kt_u64 mol_key(int32_t barcode, int32_t fingerprint, kt_u64 w, int n)
{
	const kt_u64 a = kt_mix(((kt_u64)(uint32_t)fingerprint << 8) | (kt_u64)n);
	kt_u64 low = kt_mix(w ^ a) & KEY_LOW_MASK;
	if (low == 0ull) low = 1ull;
	const kt_u64 bin = barcode == -1 ? 0ull : (kt_u64)(barcode & 0xFF);
	return (bin << 56) | low;
}

// (count, key) of v comes strictly before that of u in the order of td_census_get
KT_BOTH bool mol_before(kt_u64 cv, kt_u64 kv, kt_u64 cu, kt_u64 ku) { return cv != cu ? cv > cu : kv < ku; }
// UMI bases that take part: what an int fingerprint of (bases << 8 | length) still holds; none without a fingerprint
KT_BOTH int mol_umi_bases(int32_t fingerprint)
{
	if (fingerprint == -1) return 0;
	const int L = fingerprint & 0xFF;
	return L < 12 ? L : 12;
}
// the key of u's neighbour with base i changed by d (1..3)
KT_BOTH kt_u64 mol_neighbour_key(kt_u64 key, const td_mol_origin& o, int i, uint32_t d)
{
	return mol_key((int32_t)(key >> 56), (int32_t)((uint32_t)o.fingerprint ^ (d << (8 + 2 * i))), o.w, o.n);
}

// td_census_host.cpp: the host helpers of every result made of td_census_entry -- the order of td_census_get; a malloc'd copy for
// td_census_free (NULL: out of memory); keys (any order, repeated) -> entries in that order
KT_HIDDEN bool kt_entry_before(const td_census_entry& x, const td_census_entry& y);
KT_HIDDEN td_census_entry* kt_copy_entries(const std::vector<td_census_entry>& v);
KT_HIDDEN void kt_tally_keys(std::vector<uint64_t>& keys, std::vector<td_census_entry>& out);
// ... and what td_census_enable and td_census_host both ask of their arguments.  The segment a census of this model counts:
// `segment` itself when it is a 'B' segment, the last 'B' segment for -1; TD_FAIL with who's message when there is none
KT_HIDDEN int census_pick_segment(td_ctx* c, const char* who, const td_model_desc* m, int32_t segment, int32_t* out);
KT_HIDDEN bool census_mask_ok(uint32_t mask);
// td_molecules_host.cpp: out_e[q], out_o[q] for q < take = the entries (distinct keys) and their origins in the order of td_census_get
KT_HIDDEN void mol_emit_ordered(const td_census_entry* e, const td_mol_origin* o, int64_t n, int64_t take, td_census_entry* out_e,
                                td_mol_origin* out_o);
// what td_mol_enable and the td_mol_*host functions ask of prefix_bases
static inline bool mol_prefix_ok(int32_t p) { return p >= 1 && p <= TD_MOL_MAX_PREFIX; }
