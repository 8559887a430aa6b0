// td_batch_plan.h -- the geometry of a batch, decided in plain integers: the byte layouts of a wave slot and of the output block, which
// of the batch's tiles count as long (length classes), and the workspace plan -- how many wave slots the launch gets, of which
// geometry, and what has to be allocated for them -- and the egress plan: in which form each output comes back, and every byte
// count of the way back.  No HIP header and nothing of the context comes with it: td_batch.hip fills a
// request from the context, the slot and the route, applies the result to them and does what needs the device; the unit and the
// stand-alone program over it (tools/batch_plan_host_check.cpp) build with a plain C++ compiler.  Nothing here is exported.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "td_device.h"

#ifndef TD_HIDDEN
#define TD_HIDDEN __attribute__((visibility("hidden")))
#endif

TD_HIDDEN int64_t align256(int64_t v);
TD_HIDDEN void make_layout(TdWsLayout& L, int S, int H, int C, int lmax, int max_ncol);
// output block of the decode kernels: eight SoA arrays over n_tiles*64 reads (f, b, r, bar, q, type, barcode, finger: equal
// strides), then keep words, then labels -- all in device order
struct OutLayout { int64_t soa_stride, keep, labels, total; };
TD_HIDDEN OutLayout out_layout(int64_t n_tiles, int lmax, int nw1);

// Length classes: the n_long longest tiles of the batch are longer than lmax_small, the geometry of most wave slots (n_long = 0,
// lmax_small = lmax: one geometry).  offs[0..n] are the caller's read offsets, lmin / lmax the shortest / longest read among them;
// `wanted`: a specialised kernel decodes the batch, it gets a workspace and the option "length_classes_enabled" is on.
struct TdLengthClasses { int32_t n_long, lmax_small; };
TD_HIDDEN TdLengthClasses plan_length_classes(const int64_t* offs, int64_t n, int lmin, int lmax, int64_t n_tiles, bool wanted);

// The workspace plan of one batch.  What the request says of the context is the context's state as the batch meets it; what the plan
// changes of it comes back in the result.
struct TdWsRequest {
	int64_t n_tiles = 0;
	int32_t n_long = 0, lmax_small = 0, lmax = 0;             // the batch's length classes
	int64_t small_slot_bytes = 0, big_slot_bytes = 0;         // a wave slot for reads up to lmax_small / lmax bases (both the generic kernel's
	                                                          // slot when no specialised kernel is loaded; equal when n_long = 0)
	int wpb = 1;                                              // waves per workgroup
	int64_t want_slots = 0;                                   // what fills the chip (compute units x waves per unit), or the forced count
	bool spec_ready = false, pipelined = false;
	int overlap = 0, pipeline_depth = 1;
	bool half_slots = false;
	int wsi = 0;                                              // the workspace (0 / 1) of the batch's compute stream
	size_t cap_ws = 0, cap_ws2 = 0;                           // what the two workspaces hold now
	int ws_candidates = 1;
};
struct TdWsPlan {
	int32_t n_wave_slots = 0, n_big = 0, n_long = 0, lmax_small = 0;
	bool one_geometry = false;         // the long tiles do not keep a geometry of their own: every slot has the big one
	int64_t ws_slot_bytes = 0, ws_bytes = 0;
	bool half_slots = false;           // the context's, from now on
	bool overlap_given_up = false;     // no second workspace beside the first: this plan is for workspace 0 on the first stream, as are all later ones
	size_t alloc_bytes = 0;            // the workspace has to become this large (0: it holds the batch as it is)
	int n_candidates = 1;              // ... chosen among this many allocations that exist side by side
	bool no_fit = false;               // not even one workgroup's slots (or the long tiles') fit in HBM: ws_slot_bytes says of what size
	bool query_failed = false;         // free_mem said so
};
// free_mem(arg, &bytes): the device's free memory now; false when it cannot be told.  Asked only where the plan depends on it.
typedef bool (*TdFreeMemFn)(void* arg, size_t* free_bytes);
TD_HIDDEN TdWsPlan plan_workspace(const TdWsRequest& rq, TdFreeMemFn free_mem, void* arg);

// The egress plan of one batch: which of the three outputs come back from the device, and in which form.
//   compact: the host rebuilds the output from something smaller -- the rewritten sequences from one keep bit per base (and its copy
//            of the input), the labels from a table of rle_cap (length, label) runs per read with an overflow flag in the word behind it;
//   direct:  plain bytes, copied into the caller's buffer, which is page-locked;
//   staged:  plain bytes through pinned staging, copied out by the host.
enum { TD_CH_RES = 0, TD_CH_SEQ = 1, TD_CH_LAB = 2, TD_N_CHANNELS = 3 };   // results, rewritten sequences, labels
enum { TD_EG_NONE = 0, TD_EG_COMPACT, TD_EG_DIRECT, TD_EG_STAGED };
struct TdEgressRequest {
	int64_t n_reads = 0, n_bases = 0;
	int32_t nw1 = 0, n_tiles = 0;
	bool want[TD_N_CHANNELS] = { false, false, false };
	bool compact_egress = false;      // the option
	bool raw_host = false;            // the batch's bases are still on the host (staging copy, or the caller's own under "stable_input")
	int32_t runs_cap = 0;             // entries per read of the label runs the decode launch left (0: none)
	int32_t rle_capacity = 0;         // ... and of a table the finish kernel scans from the labels
};
struct TdEgressChannel {
	int form = TD_EG_NONE;
	size_t copy_bytes = 0;            // what the device-to-host copy moves (0: there is none)
	size_t alloc_bytes = 0;           // what its device buffer and its pinned landing hold (compact: d_keepo / h_keepo, d_rle / h_rle)
};
struct TdEgressPlan {
	TdEgressChannel ch[TD_N_CHANNELS];
	int32_t rle_cap = 0;              // entries per read of the run table
	size_t rle_flag_word = 0;         // its overflow flag: the word behind the runs (labels compact)
	bool finish_reads_runs = false;   // the finish kernel takes the runs from d_runs, whose own flag is at
	size_t runs_flag_word = 0;        // ... this word
	size_t lab_plain_bytes = 0;       // the labels as plain bytes, should the run table overflow
};
// page_locked(arg, channel): is the caller's buffer of this output page-locked?  Asked only for a channel that travels as plain bytes,
// in the order results, sequences, labels.
typedef bool (*TdPageLockedFn)(void* arg, int channel);
TD_HIDDEN TdEgressPlan plan_egress(const TdEgressRequest& rq, TdPageLockedFn page_locked, void* arg);
// a read had more label runs than the table holds: the labels travel as plain bytes after all
TD_HIDDEN void plan_labels_plain(TdEgressPlan& p, TdPageLockedFn page_locked, void* arg);
