// td_model_inner.h -- what the plain C++ units of the model path share (td_model.cpp, td_model_flat.cpp, td_calibrate.cpp): the
// reference's scaled-probability scalars, the sequence statistics with a scan limit, and the host arithmetic of the two entry points
// that drive a context (td_calibrate.cpp) -- kept in td_model.cpp, so that a stand-alone program reaches it without a context
// (tools/model_host_check.cpp).  No HIP header.  Nothing here is exported.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/tagdust_model.h"

#ifndef TD_HIDDEN
#define TD_HIDDEN __attribute__((visibility("hidden")))
#endif

inline float p2sp(float p) { return (p == 0.0) ? -INFINITY : (float)log((double)p); }   // prob2scaledprob, misc.c:85-92
inline float sp2p(float p) { return (p == -INFINITY) ? 0.0f : (float)exp((double)p); }  // scaledprob2prob, misc.c:98-105

inline float logsum_f(float a, float b) // logsum, misc.c:72-78
{
	const float* T = td_logsum_table();
	const float mx = (a > b) ? a : b;
	const float mn = (a < b) ? a : b;
	if (mn == -INFINITY || (mx - mn) >= 15.7f) return mx;
	return mx + T[(int)((mx - mn) * 1000.0f)];
}

// td_sequence_stats with the number of reads the reference scans as an argument (td_model.cpp)
TD_HIDDEN int sequence_stats_limit(const td_arch* a, const uint8_t* codes, const int64_t* offs, int64_t n_reads, td_seq_stats* ssi, int64_t scan_limit);

// td_estimate_threshold: the calibration reads in up to three length classes (up to the 75th / 95th percentile of the lengths / the
// rest; a class that would be empty is left out).  idx: the class's reads in their order, codes / offs: those reads as a batch of
// their own (codes is never empty: a batch of empty reads holds one 0).
struct TdCalClass { std::vector<int64_t> idx, offs; std::vector<uint8_t> codes; };
TD_HIDDEN std::vector<TdCalClass> td_calibration_classes(const uint8_t* codes, const int64_t* offs, int64_t n);

// td_compare_architectures: the backward scores b[n_arch][n_score] of the candidates combined into posterior[n_arch] and *best as
// the reference's n_threads threads would have summed them
TD_HIDDEN void td_arch_posteriors(const float* b, int32_t n_arch, int64_t n_score, int32_t n_threads, float* posterior, int32_t* best);
