// td_samples_def.h -- sample assignment by all 'B' segments (include/tagdust_samples.h): the one text of a read's class and key that
// the kernel (td_samples.hip) and the host definition (td_samples_host.cpp) both compile, and the plan a sheet is turned into.  No
// HIP header and nothing of the context comes with it: the host unit and stand-alone programs over it build with a plain C++
// compiler.  Nothing here is exported.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/tagdust_samples.h"
#include "td_count_key.h"

// an entry of TdSamplePlan::tc: a label of chosen segment t with call + 1 in the low byte, or a label of a segment behind j_m
#define SMP_TC_CHOSEN 0x8000u
#define SMP_TC_BEHIND 0x4000u

// What a sheet over a model comes to.  A read's calls are one 32-bit word, byte t = call_t + 1 (0: no position had a label of
// segment j_t) -- the low word of its key; a sheet row is the same word, the rows sorted for the lookup.
struct TdSamplePlan {
	int32_t m, n_samples, last_seg, ordered;   // chosen segments; rows; j_m; model.label's segments never decrease with the HMM index
	uint32_t decoy;                            // byte t = n_hmm[j_t]: what the all-N decoy of segment j_t leaves in a calls word
	uint16_t tc[128];                          // by class byte = label + 1 (0: none): SMP_TC_CHOSEN | t << 8 | call + 1, SMP_TC_BEHIND, or 0
	uint32_t row[256];                         // [n_samples] the rows as calls words, ascending
	uint8_t sample[256];                       // [n_samples] the sample of row[k]
};

// the calls word with label entry e (SMP_TC_CHOSEN) taken: a later position of the same segment overwrites an earlier one
KT_BOTH uint32_t smp_take(uint32_t calls, uint32_t e)
{
	const int sh = 8 * (int)((e >> 8) & 3u);
	return (calls & ~(0xFFu << sh)) | ((e & 0xFFu) << sh);
}

// some call is missing or the decoy
KT_BOTH bool smp_incomplete(uint32_t calls, uint32_t decoy, int m)
{
	bool bad = false;
	for (int t = 0; t < TD_SAMPLES_MAX_SEGMENTS; t++) {
		const uint32_t b = (calls >> (8 * t)) & 0xFFu;
		if (t < m && (b == 0u || b == ((decoy >> (8 * t)) & 0xFFu))) bad = true;
	}
	return bad;
}

// the sample whose row equals `calls`, -1 when the sheet has none (row ascending, n >= 1)
KT_BOTH int smp_find(const uint32_t* row, const uint8_t* sample, int n, uint32_t calls)
{
	int lo = 0, hi = n - 1;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if (row[mid] < calls) lo = mid + 1; else hi = mid;
	}
	return row[lo] == calls ? (int)sample[lo] : -1;
}

KT_BOTH kt_u64 smp_key(uint32_t calls, int m) { return ((kt_u64)m << 56) | (kt_u64)calls; }

// The join across input files: what an exporter hands over for a read that was not extracted.  OR-ed with any other word it stays
// all ones, so the words of several exporters combine without a special case.
#define SMP_PARTNER_FAILED 0xFFFFFFFFu

// the export word of a read: its own calls (bytes first_column.., the plan's tc puts them there) when it was extracted
KT_BOTH uint32_t smp_export_word(bool extracted, uint32_t calls) { return extracted ? calls : SMP_PARTNER_FAILED; }

// td_samples_host.cpp: the model's 'B' segments and the sheet checked, the plan filled; TD_FAIL with who's message (naming the row)
KT_HIDDEN int smp_plan_build(td_ctx* c, const char* who, const td_model_desc* m, const int32_t* tuples, int32_t n_samples, TdSamplePlan& out);
// ... the plan of a join: m_total columns of column_hmms[t] HMMs each, the model's own 'B' segments at first_column.. (their entries
// of column_hmms are held against the model), a sheet of m_total columns; last_seg is the last OWN segment
KT_HIDDEN int smp_join_plan_build(td_ctx* c, const char* who, const td_model_desc* m, const int32_t* tuples, int32_t n_samples, int32_t m_total,
                                  int32_t first_column, const int32_t* column_hmms, TdSamplePlan& out);
// ... and of an exporter: no sheet, only tc (the own calls at bytes first_column..), ordered and last_seg are read
KT_HIDDEN int smp_export_plan_build(td_ctx* c, const char* who, const td_model_desc* m, int32_t first_column, TdSamplePlan& out);
// ... and the names: 1..64 characters of [A-Za-z0-9._-], pairwise different, "S<s+1>" for a NULL one
KT_HIDDEN int smp_names_check(td_ctx* c, const char* who, const char* const* names, int32_t n_samples, std::vector<std::string>& out);

