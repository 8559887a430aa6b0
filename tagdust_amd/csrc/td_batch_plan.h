// td_batch_plan.h -- the geometry of a batch, decided in plain integers: the byte layouts of a wave slot and of the output block, which
// of the batch's tiles count as long (length classes), and the workspace plan -- how many wave slots the launch gets, of which
// geometry, and what has to be allocated for them.  No HIP header and nothing of the context comes with it: td_api.hip fills a
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
