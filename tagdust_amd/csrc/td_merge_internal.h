// td_merge_internal.h -- shared between td_merge.cpp (tables, host path, command line), td_merge.hip (the kernel and its host side)
// and td_merge_stream.cpp (td_merge_stream's pipeline, on the readers of td_stream_internal.h)
#pragma once
#include <math.h>
#include <stdint.h>

#include <functional>
#include <string>

#include "../../include/tagdust_merge.h"
#include "td_workers.h"

#if defined(__HIPCC__)
#define TD_MERGE_HD __host__ __device__
#else
#define TD_MERGE_HD
#endif

// reads longer than this are not staged by the kernel: such a pair is done by the host path (td_merge_batch)
#define TD_MERGE_STAGE_BASES 512

// rev_nuc_code[] (src/nuc_code.c): A <-> T, C <-> G, N stays 4
TD_MERGE_HD inline int td_merge_rc(int x) { return x < 4 ? 3 - x : x; }

// The letter where the two bases differ (merge.c:585-598): the c of the largest profile entry, scanned over c = 0..3, read 1
// before read 2, with a strict >.  profile: td_merge_tables::profile; q the dense quality index, x the base code.
TD_MERGE_HD inline int td_merge_pick(const float* profile, int qf, int xf, int qr, int xr)
{
	float best = -INFINITY;
	int nuc = 0;
	for (int c = 0; c < 4; c++) {
		const float a = xf > 3 ? 0.25f : profile[2 * qf + (c == xf ? 0 : 1)];
		if (a > best) { best = a; nuc = c; }
		const float b = xr > 3 ? 0.25f : profile[2 * qr + (c == xr ? 0 : 1)];
		if (b > best) { best = b; nuc = c; }
	}
	return nuc;
}

// does candidate (s, d) replace (bs, bd)?  The reference takes candidates in d order with a strict > from -inf: the largest
// score wins, among equal scores the smallest d, and a score of -inf never wins.
TD_MERGE_HD inline bool td_merge_better(float s, int d, float bs, int bd)
{
	return s > bs || (s == bs && bd >= 0 && d < bd);
}

// id / aligned >= threshold in float (merge.c:681): the quotient of two floats through double is the correctly rounded float quotient
TD_MERGE_HD inline bool td_merge_passes(int id, int aligned, float threshold)
{
	return (float)((double)(float)id / (double)(float)aligned) >= threshold;
}

// one batch of pairs: base codes and quality bytes of each file contiguous under the same offsets, read 2 as it stands in its file
struct TdMergeView {
	int64_t n = 0;
	const uint8_t* codes1 = nullptr; const uint8_t* qual1 = nullptr; const int64_t* offs1 = nullptr;
	const uint8_t* codes2 = nullptr; const uint8_t* qual2 = nullptr; const int64_t* offs2 = nullptr;
};

void td_merge_set_error(const std::string& msg);
// the tables for the quality characters marked in present[256]
td_merge_tables* td_merge_tables_from_set(const bool* present);
// overlap_reads() for pair p; seq / qual: room for len_f + len_r characters
void td_merge_pair_host(const TdMergeView& v, int64_t p, const td_merge_tables& t, int min_overlap, float threshold,
                        td_merge_record* rec, char* seq, char* qual);

// the kernel's host side (td_merge.hip): device buffers that grow and stay for the next batch
struct TdMergeDevice;
TdMergeDevice* td_merge_device_open(int device, std::string& err);
void td_merge_device_close(TdMergeDevice* d);
// runs the kernel over the view; rec / seq / qual as td_merge_result (out_off[p] = offs1[p] + offs2[p]).  Pairs with a read longer
// than TD_MERGE_STAGE_BASES are left untouched.
bool td_merge_device_run(TdMergeDevice* d, const TdMergeView& v, const td_merge_tables& t, int min_overlap, float threshold,
                         int placement, td_merge_record* rec, char* seq, char* qual, int* table_in_lds, float* kernel_ms, std::string& err);

// One batch, the whole of it: the checks ('.' codes), the tables, every pair on `dev` (NULL: on host threads; pairs the kernel does
// not take on the host), the host's share on `pool` (NULL: on o.n_threads threads made for this batch), out_off and the counts.  res: rec / out_off / seq / qual are allocated here (malloc).
// tables_s / kernel_ms may be NULL.
bool td_merge_batch(const TdMergeView& v, const td_merge_opts& o, TdMergeDevice* dev, TdWorkers* pool, td_merge_result* res, double* tables_s, std::string& err);
// the pipeline under td_merge_stream (td_merge_stream.cpp): readers, checks, writer; merge_batch fills a result (td_merge_batch)
// for the view it is given, on the pool of n_threads that the run owns
int td_merge_stream_run(const char* in1, const char* in2, const char* out_path, int n_threads, int batch_pairs, bool pinned,
                        const std::function<bool(const TdMergeView&, TdWorkers&, td_merge_result*, std::string&)>& merge_batch, td_merge_stats* stats, std::string& error);
