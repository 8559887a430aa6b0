// td_jit.h -- interface between the C-ABI layer (td_spec_host.hip, td_api.hip, td_batch.hip) and the model-specialised kernel builder (td_spec_plan.cpp:
// knobs, plan, model section, layout; td_spec_bounds.cpp: the bound tables -- both plain C++; td_jit.hip: full source, compile + cache)
#pragma once
#include <string>
#include <vector>
#include "../../include/tagdust_hip.h"
#include "td_device.h"

#ifndef TD_HIDDEN
#define TD_HIDDEN __attribute__((visibility("hidden")))
#endif

// The TD_SPEC_* environment knobs (DESIGN.md has the table).  They are read when a model is uploaded, or when a context-free
// query is made, and hold for that model.
struct TdSpecKnobs {
	int block = 512;          // TD_SPEC_BLOCK: threads per workgroup, 64..1024 in multiples of 64
	int min_waves = 4;        // TD_SPEC_MINWAVES: waves per SIMD of __launch_bounds__, 1..8
	int lsum_oob = 1;         // TD_SPEC_LSUM_OOB: clamp-free logsum (LDS out-of-range reads as 0), see td_spec_kernel.inc.  The form a
	                          // model starts with: a loaded kernel's own form is td_spec_compile's lsum_oob argument
	int rt_min = 16;          // TD_SPEC_RT_MIN: HMMs a segment needs for the run-time HMM loop
	int groupcols = 18;       // TD_SPEC_GROUPCOLS: columns swept together (> 0)
	int groupcols_fwd = 12;   // TD_SPEC_GROUPCOLS_FWD: ... in the forward sweep (<= 0: as groupcols)
	int prune = 1;            // TD_SPEC_PRUNE: position pruning
	int prune_sfx = 1;        // TD_SPEC_PRUNE_SFX: ... of the trailing segments too
	int restart = -1;         // TD_SPEC_RESTART: restarted sweeps (-1: by the size of the leading segments)
	int firstseg = -1;        // TD_SPEC_FIRSTSEG: the first segment's labels as running sums (-1: when H > 32)
	int trie_sh = 2;          // TD_SPEC_TRIE_SH: match columns HMMs of the first segment share in its backward sweep
	int profile = 0;          // TD_SPEC_PROFILE: TDS_PROFILE
	int prune_stats = -1;     // TD_SPEC_PRUNE_STATS: TDS_PRUNE_STATS (-1: the kernel's own default)
	std::string extra_opts;   // TD_SPEC_EXTRA_OPTS: further compiler options, space separated
};
TdSpecKnobs td_spec_knobs(void);

#define TD_PRUNE_TABLES 16   /* 8 position-pruning tables, then up to 4 + 4 impulse-response tables of the restarted sweeps */
#define TD_PRUNE_RESTART_MAX 4   /* leading / trailing segments a restart can bridge */

// What the kernel is for one model under one set of knobs: built once, read by the source generator, the workspace layout, the
// bound tables and the C-ABI layer alike.
struct TdSpecPlan {
	TdSpecKnobs k;
	int S = 0, H = 0, C = 0;
	std::vector<int> col_off, hmm_off;       // [S] first column / first HMM (label) of a segment
	std::vector<int> group, group_f;         // [S] HMMs swept together, backward / forward
	std::vector<int> pure_last, drop_m;      // [S] the last column is not spilled / the one before it spills I_backward only
	std::vector<int> bw_off;                 // [H] first stored half-column of an HMM
	int64_t halves = 0;                      // stored half-columns (4 B per lane and position)
	std::vector<int> rt, rt_b;               // [S] HMMs in the run-time loop of the sweeps / of the restarted sweeps' bridges
	std::vector<int> base;                   // [C] ... the base their match column expects
	std::vector<float> hi, lo, nv;           // [S] ... and its three emission values
	bool trie_on = false;                    // suffix order of the first segment's backward sweep
	int trie_sh = 1, trie_n_share = 0;
	std::vector<int> trie_ord;
	int first_n = 0;                         // labels whose posteriors the forward sweep sums up itself (0: none)
	int prune_segs = 0;                      // leading segments the forward sweep may cut short (0: none)
	int sfx_first = 0;                       // first trailing segment the backward sweep may cut short (S: none)
	float prune_z = 0.0f;                    // zero-posterior margin
	int restart = 0;                         // the kernel restarts the far sweeps of the pruned segments (TDS_RESTART)
};
TdSpecPlan td_spec_plan(const td_model_desc* m, const TdSpecKnobs& k);
// the plan and the model's parameters as constexpr source text; td_jit.hip puts it in front of td_spec_kernel.inc (lsum_oob, window: as
// td_spec_compile's)
TD_HIDDEN std::string td_spec_model_section(const td_model_desc* m, const TdSpecPlan& p, int lsum_oob, int window);

float td_spec_prune_z(const td_model_desc* m, int n_seg, int sfx_first);
void td_spec_prune_tables(const td_model_desc* m, const TdSpecPlan& p, int lcap, int stride, std::vector<float>& tab);
void td_spec_layout(TdSpecLayout& L, const TdSpecPlan& p, int lmax);
// lsum_oob: the logsum form (the plan's k.lsum_oob unless the context had to fall back); window: -start/-end support compiled in
// *key_out: the cache key of the code object (a hash of the full source, every compile option and the compiler's version);
// key_only: nothing else is done.  Safe to call from any host thread: it touches neither a context nor the device.
int td_spec_compile(const td_model_desc* m, const TdSpecPlan& p, int lsum_oob, int window, std::vector<char>& code, std::string& log,
                    uint64_t* key_out = nullptr, bool key_only = false);
int td_spec_compiles_started(void);   // hiprtc compiles this process has actually started (cache hits do not count)
