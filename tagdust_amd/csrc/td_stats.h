// td_stats.h -- get_sequence_stats() (src/io.c:52-300) in two halves: "count" (everything that looks at the reads; on the
// host in td_model.cpp, on the device in td_stats.hip) and "finish" (means, standard deviations, rounding, log frequencies:
// td_model.cpp, shared by both).  Every counted quantity is an integer -- the reference's doubles hold counts -- so the
// device sums them as 64-bit integers and the result does not depend on the order they were added in.  Library-internal.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/tagdust_model.h"

struct TdSeqCounts {
	int64_t n_reads = 0;          // reads looked at: min(n_reads, scan_limit)
	int64_t base[5] = { 0, 0, 0, 0, 0 };   // bases per code (codes above 4 count as 4)
	int64_t len_sum = 0, len_max = 0;
	int64_t five[3] = { 0, 0, 0 };         // s0, s1, s2 of the 5' linker match lengths (io.c:141-156)
	int64_t three[3] = { 0, 0, 0 };        // ... of the 3' linker's (:158-173)
};

// base codes (nuc_code) of the leading / trailing 'P' segment's first sequence; empty when the architecture has none
void td_stats_linkers(const td_arch* a, std::vector<uint8_t>& five, std::vector<uint8_t>& three);
// counts -> td_seq_stats (io.c:190-270)
void td_stats_finish(const td_arch* a, const TdSeqCounts& k, td_seq_stats* out);
// with -start / -end the average length is the window's (io.c:258-260)
void td_stats_apply_window(td_seq_stats* ssi, int32_t matchstart, int32_t matchend);

// The counting on `device` (td_stats.hip): uploads codes[offs[0] .. offs[n]) and offs[0 .. n], n = min(n_reads, scan_limit),
// into buffers of its own and works on a stream of its own.  offs must be ascending with reads shorter than 2^31 (checked).
// TD_OK / TD_FAIL with the text in err.
int td_stats_count_device(int device, const std::vector<uint8_t>& five, const std::vector<uint8_t>& three, const uint8_t* codes,
                          const int64_t* offs, int64_t n_reads, int64_t scan_limit, TdSeqCounts* out, char* err, size_t errcap);
