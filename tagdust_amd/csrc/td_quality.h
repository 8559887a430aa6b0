// td_quality.h -- the base-quality filter (include/tagdust_quality.h) inside a context: its state, and what td_api.hip and
// td_batch.hip call.  The judge kernel and every td_qual_* entry point that takes a context are in td_quality.hip; the plan both
// sides share and the pack of the quality bytes are td_quality_def.h's.  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "td_keytable.h"
#include "td_quality_def.h"

struct TdSlot;

// The device tallies, 64 bits each: QL_COPIES copies of them, QL_COPY_WORDS words (one 128-byte line) apart, a workgroup adds to
// copy blockIdx.x % QL_COPIES and td_qual_get sums the copies (passed = eligible - failed is made there).
enum { QL_ELIGIBLE = 0, QL_FAILED, QL_LOW_BASES, QL_TALLY_WORDS };
#define QL_COPIES 64
#define QL_COPY_WORDS 16
#define QL_TALLY_BYTES (sizeof(kt_u64) * QL_COPIES * QL_COPY_WORDS)

struct TdQualState {
	bool on = false;
	int32_t gen = 0;                  // counts the enables: a batch remembers the one it was staged under (TdStaged::qual_gen)
	TdQualPlan plan{};
	int32_t H = 0;
	int32_t last_judged = 0;          // the last judged segment where a path cannot come back to it, else TD_MAX_SEGMENTS (td_qual_enable)
	int32_t* d_label = nullptr;       // [H] model.label, the filter's own copy
	kt_u64* d_tallies = nullptr;      // [QL_COPIES][QL_COPY_WORDS]
	KtEventPair ev;                   // around the last judge launch
	// td_qual_next: the quality bytes of the next TD_MODE_GET_LABEL batch (read i's at qual + offs[i])
	const uint8_t* next_qual = nullptr;
	int64_t next_reads = 0;
	bool named = false;
};

struct TdQualArgs {
	const int8_t* __restrict__ labels;       // [n_tiles][lmax + 1][64]  the decode launch's labels, device order
	const int32_t* __restrict__ lens;        // [n_tiles*64]
	int32_t* __restrict__ out_type;          // [n_tiles*64]  final outcomes of the decode launch, rewritten
	const int64_t* __restrict__ offs;        // [n_reads + 1] the caller's order, offs[0] = 0: a read's first low flag
	const int32_t* __restrict__ read_at;     // [n_reads] the read of device position k (NULL: k itself)
	const uint32_t* __restrict__ words;      // [n_words] one low flag per base, the last word zero
	const int32_t* __restrict__ label;       // [H]
	kt_u64 judged;                           // bit j: the bases of segment j are judged
	int64_t n_reads, n_words;
	int32_t n_tiles, lmax, H, max_low;
	int32_t last_judged;                     // labels of a segment behind this one end a lane's walk (TD_MAX_SEGMENTS: none do)
	unsigned long long* __restrict__ tallies;
};

// Inside slot_stage: the named quality bytes packed into the slot's page-locked words on the context's workers and their upload
// queued on `up`; consumes the name.  qual_check: TD_FAIL with a message (`who` in it) unless qualities are named for n reads.
KT_HIDDEN int qual_check(td_ctx* c, int64_t n, const char* who);
KT_HIDDEN int qual_stage(td_ctx* c, TdSlot& s, const int64_t* offs, int64_t n, hipStream_t up);
// the verdicts of one decoded slot, queued on its compute stream (td_batch.hip's launch_end while the filter is on)
KT_HIDDEN int qual_slot(td_ctx* c, TdSlot& s, int32_t* out_type, const int8_t* labels);
// option "quality_kernel_us" of td_get_option: the kernel's time of the last batch (waits for it)
KT_HIDDEN int qual_last_kernel_us(td_ctx* c, int32_t* us);
// label copy, tallies and events freed, the filter off (the caller has made sure nothing of it is queued any more)
KT_HIDDEN void qual_release(td_ctx* c);
