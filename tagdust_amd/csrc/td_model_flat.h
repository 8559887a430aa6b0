// td_model_flat.h -- from what the caller hands in to what the device receives, decided on the host: a model description checked and
// flattened into the generic kernel's tables, the -ref text checked and packed into 2-bit words, the logsum table.  No HIP header and
// nothing of the context comes with it: td_api.hip asks, reports `why` through the context and does the allocations and copies; the
// unit and the stand-alone program over it (tools/model_host_check.cpp) build with a plain C++ compiler.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/tagdust_hip.h"
#include "td_device.h"

#ifndef TD_HIDDEN
#define TD_HIDDEN __attribute__((visibility("hidden")))
#endif

struct TdFlatModel {
	TdModelHeader h;
	std::vector<TdCol> cols;                   // [C]
	std::vector<uint32_t> hinfo;               // [H] type | segment << 8 | HMM << 16 | decoy << 31
	std::vector<int32_t> pred_off, pred_idx;   // [H + 1], [pred_off[H]] (one 0 when no label has a predecessor)
};
// false: the description is rejected and `why` says so (the text td_model_upload / td_arch_scores report)
TD_HIDDEN bool td_flatten_model(const td_model_desc* m, TdFlatModel& out, std::string& why);

// The n_seq > 0 sequences string[s_index[j] .. s_index[j + 1]) as TD_MODE_RNA_DUST reads them: seq[2 j] = first word, seq[2 j + 1] =
// length of sequence j in pk, 16 two-bit codes per word, every sequence from a word boundary (pk has one word to spare).
// false: s_index is rejected and `why` says so (td_set_artifacts' text).
TD_HIDDEN bool td_pack_artifacts(const uint8_t* string, const int32_t* s_index, int32_t n_seq, std::vector<int32_t>& seq,
                                 std::vector<uint32_t>& pk, std::string& why);
