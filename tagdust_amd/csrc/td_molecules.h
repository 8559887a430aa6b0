// td_molecules.h -- the molecule count (include/tagdust_molecules.h) inside a context: its state, and what td_api.hip and td_batch.hip call.  The
// kernels and every td_mol_* entry point that takes a context are in td_molecules.hip; the table is td_keytable.h's.  Nothing here
// is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tagdust_molecules.h"
#include "td_keytable.h"

struct td_ctx;
struct TdSlot;

// tallies of the device table, 64 bits each, in the order of td_mol_totals; behind them the compaction's cursor, then dedup's
// three in the order of td_mol_dedup_totals, then the collapse's: the cursor of its two gathers, its roots, its longest chain
enum { TDM_ELIGIBLE = 0, TDM_COUNTED, TDM_EMPTY, TDM_N, TDM_OVERFLOW, TDM_MOLECULES, TDM_CURSOR, TDM_KEPT, TDM_DUPLICATES, TDM_UNJUDGED,
       TDM_GATHERED, TDM_ROOTS, TDM_CHAIN, TDM_TALLY_WORDS };
// words of a barcode bin's summary row: reads, molecules, ten levels (td_mol_row)
#define TDM_ROW_WORDS 12

// The count's state, and inside it one group per stage behind the count.  A group is value-initialised as a whole by what ends its
// stage -- free what it owns, then group = Group() -- as TdSlot's groups are (td_ctx.h): "off" is never a set of fields nulled by hand.
// dedup (td_mol_dedup_enable): the first ordinal of every slot's key, and what orders the two passes of neighbouring batches
struct TdMolDedup {
	bool on = false;
	unsigned long long* d_first = nullptr;    // [2^log2_slots], all-ones = no read yet
	int64_t next_ordinal = 0;                 // reads submitted in TD_MODE_GET_LABEL since dedup was enabled, last reset or frozen
	hipEvent_t ev_p1[2] = { nullptr, nullptr };   // behind pass 1 of the last batch ([turn ^ 1]) and of the one before it ([turn])
	bool p1_queued[2] = { false, false };
	int turn = 0;
	KtEventPair ev;                           // around the two passes of the last batch (option "dedup_kernel_us")
	void start_over() { next_ordinal = 0; p1_queued[0] = p1_queued[1] = false; }   // ordinals from 0, nothing of pass 1 is queued
};
// collapse (td_mol_collapse_enable): the origin of every slot's key; what a collapse computes, allocated by the first one
struct TdMolCollapse {
	bool on = false;
	td_mol_origin* d_origin = nullptr;        // [2^log2_slots], n == 0 = no origin yet
	uint32_t* d_occ = nullptr;                // the occupied slots' indices, cap_occ bytes of them
	size_t cap_occ = 0;
	uint32_t* d_parent = nullptr;             // [2^log2_slots] the slot of every occupied slot's parent, its own for a root
	unsigned long long* d_collapsed = nullptr;   // [2^log2_slots] the count of a root's tree, 0 for every other slot
	KtEventPair ev;                           // around the origin pass of the last batch (option "collapse_origin_kernel_us")
};
// the frozen state (td_mol_dedup_freeze; count, dedup and collapse all on): the table is read-only and every batch is replayed
// against keeper[]; the first freeze allocates it and the pair, whatever ends dedup or the collapse ends this group
struct TdMolFrozen {
	bool on = false;
	unsigned long long* d_keeper = nullptr;   // [2^log2_slots] of an occupied slot: the first ordinal of its root's own key
	KtEventPair ev;                           // around the replay kernel of the last batch (option "dedup_replay_kernel_us")
};
// mate mode (td_mol_mate_enable): M, and the mate batch td_mol_mate_next named for the next TD_MODE_GET_LABEL staging (the caller's
// pointers, read by that staging alone)
struct TdMolMate {
	int32_t bases = 0;                        // M: the mate's bases that belong to the key (0 = off)
	bool named = false;
	const uint8_t* codes = nullptr;
	const int64_t* offs = nullptr;
	int64_t reads = 0;
	KtEventPair ev;                           // around the mate kernel of the last staged mate batch (option "mate_kernel_us")
	// the mate filter (td_mol_mate_filter_enable): the mates are judged as TD_MODE_RNA_DUST judges and the verdict joined to the read's
	bool filter = false;
	KtEventPair ev_filter;                    // around the filter kernel of the last staged mate batch (option "mate_filter_kernel_us")
	KtEventPair ev_join;                      // around the join kernel of the last decoded batch (option "mate_join_kernel_us")
};
struct TdMolState {
	bool on = false;
	int32_t prefix = 0;         // P: read bases that belong to the key
	uint64_t r_segs = 0;        // bit j: segment j is an 'R' segment
	TdCountTable table;         // td_keytable.h, TDM_TALLY_WORDS tallies; its pair is option "molecules_kernel_us"
	unsigned long long* d_rows = nullptr;     // [TD_NUM_BARCODE_BINS][TDM_ROW_WORDS] the summary sweep's result
	TdMolDedup dedup;
	TdMolCollapse collapse;
	TdMolFrozen frozen;
	TdMolMate mate;
};

struct TdMolArgs {
	TdTileView tile;                          // td_keytable.h
	const int32_t*  __restrict__ lens;        // [n_tiles*64]
	const int32_t*  __restrict__ out_type;    // [n_tiles*64]  final outcomes of the decode launch
	const int32_t*  __restrict__ out_barcode; // [n_tiles*64]
	const int32_t*  __restrict__ out_finger;  // [n_tiles*64]
	const int32_t*  __restrict__ label;       // [H] model.label
	int64_t n_reads;
	uint64_t r_segs;
	int32_t n_tiles, H, prefix;
	TdKeyTable table;
	unsigned long long* __restrict__ tallies;
	// mate mode (mate_bases > 0; with read_at: the mate kernel leaves both in the caller's order)
	const unsigned long long* __restrict__ mate_w;   // [n_reads] the mate's prefix word
	const uint8_t* __restrict__ mate_n;       // [n_reads] its length n2 in the low 7 bits, bit 7 = one of those bases is an N
	int32_t mate_bases;                       // M (0 = off: neither array is read)
	// dedup's pass 1, the replay and mate mode
	const int32_t* __restrict__ read_at;      // [n_reads] device position -> index in the caller's order (NULL: the same)
	unsigned long long* __restrict__ first;   // [slot_mask + 1] the smallest ordinal of every slot's key
	int32_t* __restrict__ judged;             // [n_tiles*64] the read's table slot, -1 = not judged
	int64_t ordinal_base;                     // the ordinal of the batch's first read in the caller's order
	// the collapse's origin pass alone
	td_mol_origin* origin;                    // [slot_mask + 1] (not __restrict__: lanes of other waves write the same words)
	// the replay kernel alone (with read_at and ordinal_base)
	const unsigned long long* __restrict__ keeper;   // [slot_mask + 1] the ordinal of the one read that a slot's tree keeps
};

// A decoded slot's launches, queued on its compute stream behind the decode launch (td_batch.hip calls it last behind a decode launch while
// the count is on): the count, the collapse's origin pass, dedup's two passes, each when it is on -- or, in the frozen state, the
// replay kernel alone.  Dedup's second pass and the replay rewrite out_type, so everything else that reads the decoded outcomes is
// queued in front of them.
__attribute__((visibility("hidden"))) int mol_slot_decoded(td_ctx* c, TdSlot& s, int32_t* out_type, const int32_t* out_barcode,
                                                           const int32_t* out_finger, const int8_t* labels);
// Mate mode, inside slot_stage.  mol_mate_stage: the mate batch td_mol_mate_next named goes into the slot with the batch's own input, its
// copies queued on `up` in front of the upload event (the named batch is consumed).  mol_mate_launch: the mate kernel over it on the
// slot's aux stream, behind the upload event and in front of ev_pack.  mol_mate_check: TD_FAIL with a message (`who` in it) unless a
// mate batch of n reads is named; a wrong one is dropped.  With the mate filter on mol_mate_launch queues the filter kernel
// (td_mate_filter.hip) behind the mate kernel when dust or artifacts are set, and mol_mate_join, called by launch_end in front of
// everything that reads a TD_MODE_GET_LABEL batch's outcomes, queues the join on the slot's compute stream.
__attribute__((visibility("hidden"))) int mol_mate_check(td_ctx* c, int64_t n, const char* who);
__attribute__((visibility("hidden"))) int mol_mate_stage(td_ctx* c, TdSlot& s, int64_t n, hipStream_t up);
__attribute__((visibility("hidden"))) int mol_mate_launch(td_ctx* c, TdSlot& s, int64_t n);
__attribute__((visibility("hidden"))) int mol_mate_join(td_ctx* c, TdSlot& s, int32_t* out_type);
// The "*_kernel_us" options of td_get_option that belong here -- molecules_, dedup_, collapse_origin_, dedup_replay_, mate_, mate_filter_ and mate_join_: the time
// between the stage's two events of the last batch (waits for it).  TD_OK, TD_FAIL with the message, or -1: `name` is none of them.
__attribute__((visibility("hidden"))) int mol_kernel_us(td_ctx* c, const char* name, int32_t* us);
// table and label copy freed, count off (the caller has made sure nothing of it is queued any more)
__attribute__((visibility("hidden"))) void mol_release(td_ctx* c);
