// td_quality_def.h -- the base-quality filter (include/tagdust_quality.h): what its host unit (td_quality_host.cpp) and its device
// unit (td_quality.hip) share -- the plan a model and the parameters come to, and the pack of a range of quality bytes.  No HIP
// header and nothing of the context comes with it: the host unit and stand-alone programs over it build with a plain C++
// compiler.  Nothing here is exported.
#pragma once
#include <stdint.h>

#include "../../include/tagdust_quality.h"
#include "td_count_key.h"

// What the parameters over a model come to: the threshold byte, and which segments' bases are judged (bit j: segment j;
// TD_MAX_SEGMENTS = 64 of them fit one word).
struct TdQualPlan {
	td_qual_params p;
	int32_t thr;
	kt_u64 judged;
};

// td_quality_host.cpp: the parameters and the model checked, the plan filled; TD_FAIL with who's message
KT_HIDDEN int qual_plan_build(td_ctx* c, const char* who, const td_model_desc* m, const td_qual_params* p, TdQualPlan& out);
// ... and the low flags of bases [lo, hi) of `qual` into their words, lo a multiple of 32: words[lo >> 5 .. (hi + 31) >> 5) are
// written, the bits at and beyond hi zero, no other word touched -- so ranges that meet on a multiple of 32 pack side by side
KT_HIDDEN void qual_pack_range(const uint8_t* qual, int64_t lo, int64_t hi, int32_t thr, uint32_t* words);
