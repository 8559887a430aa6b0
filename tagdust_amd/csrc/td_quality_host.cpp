// td_quality_host.cpp -- the host side of the base-quality filter (include/tagdust_quality.h): the check of the parameters against a
// model and the plan they come to, td_qual_pack -- the one pass over a batch's quality bytes, which the staging (td_batch.hip),
// td_qual_host and the tests all use -- and td_qual_host, the definition the device's kernel (td_quality.hip) is held against, over
// host arrays.  Plain C++: no device is used and no HIP header read.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "td_quality_def.h"

#if defined(__SSE2__) && !defined(__HIP_DEVICE_COMPILE__)
#include <emmintrin.h>
#define QUAL_PACK_SSE2 1
#endif

int qual_plan_build(td_ctx* c, const char* who, const td_model_desc* m, const td_qual_params* p, TdQualPlan& out)
{
	if (!m || m->S < 1 || m->S > TD_MAX_SEGMENTS || m->H < 1 || m->H > TD_MAX_HMMS || !m->seg_type || !m->label) return fail(c, "%s: no model", who);
	if (!p) return fail(c, "%s: no parameters", who);
	if (p->min_quality < 1 || p->min_quality > 93) return fail(c, "%s: min_quality = %d (1..93 supported)", who, p->min_quality);
	if (p->offset != 33 && p->offset != 64) return fail(c, "%s: offset = %d (33 or 64)", who, p->offset);
	if (p->max_low < 0) return fail(c, "%s: max_low = %d (0 or more)", who, p->max_low);
	if (p->segments < 1 || (p->segments & ~(TD_QUAL_SEG_B | TD_QUAL_SEG_F)))
		return fail(c, "%s: segments = %d (TD_QUAL_SEG_B = 1, TD_QUAL_SEG_F = 2, or both)", who, p->segments);
	TdQualPlan q{};
	q.p = *p;
	q.thr = p->offset + p->min_quality;
	for (int j = 0; j < m->S; j++) {
		const bool b = m->seg_type[j] == 'B' && (p->segments & TD_QUAL_SEG_B), f = m->seg_type[j] == 'F' && (p->segments & TD_QUAL_SEG_F);
		if (b || f) q.judged |= 1ull << j;
	}
	if (q.judged == 0ull)
		return fail(c, "%s: the model has no %s segment: there is no base to judge", who,
		            p->segments == TD_QUAL_SEG_B ? "'B'" : (p->segments == TD_QUAL_SEG_F ? "'F'" : "'B' or 'F'"));
	out = q;
	return TD_OK;
}

void qual_pack_range(const uint8_t* qual, int64_t lo, int64_t hi, int32_t thr, uint32_t* words)
{
	int64_t g = lo;
	if (thr > 255) {                                  // every byte is below: whole words of ones, the tail below
		for (; g + 32 <= hi; g += 32) words[g >> 5] = 0xFFFFFFFFu;
	} else {
#ifdef QUAL_PACK_SSE2
		// q < thr, unsigned: max(q, thr) != q
		const __m128i t = _mm_set1_epi8((char)(uint8_t)(thr < 0 ? 0 : thr));
		for (; g + 32 <= hi; g += 32) {
			const __m128i a = _mm_loadu_si128((const __m128i*)(qual + g)), b = _mm_loadu_si128((const __m128i*)(qual + g + 16));
			const uint32_t ge_a = (uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_max_epu8(a, t), a));
			const uint32_t ge_b = (uint32_t)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_max_epu8(b, t), b));
			words[g >> 5] = ~(ge_a | (ge_b << 16));
		}
#endif
	}
	for (; g < hi; g += 32) {                         // the scalar tail (all of it without SSE2)
		uint32_t w = 0u;
		const int64_t end = g + 32 < hi ? g + 32 : hi;
		for (int64_t q = g; q < end; q++) w |= (uint32_t)((int32_t)qual[q] < thr) << (q - g);
		words[g >> 5] = w;
	}
}

extern "C" int td_qual_pack(const uint8_t* qual, int64_t n, int32_t thr, uint32_t* words)
{
	if (n < 0 || !words || (!qual && n > 0)) return fail(nullptr, "td_qual_pack: bad arguments");
	if (thr < 0 || thr > 256) return fail(nullptr, "td_qual_pack: thr = %d (0..256 supported)", thr);
	qual_pack_range(qual, 0, n, thr, words);
	words[(n + 31) / 32] = 0u;
	return TD_OK;
}

extern "C" int td_qual_host(const td_model_desc* model, const td_qual_params* params, const int64_t* offs, int64_t n_reads, td_read_result* res,
                            const int8_t* labels, const uint8_t* qual, td_qual_totals* totals)
{
	TdQualPlan plan;
	if (qual_plan_build(nullptr, "td_qual_host", model, params, plan) != TD_OK) return TD_FAIL;
	if (n_reads < 0 || (n_reads > 0 && (!offs || !res || !labels))) return fail(nullptr, "td_qual_host: bad arguments");
	for (int64_t i = 0; i < n_reads; i++)
		if (offs[i + 1] < offs[i]) return fail(nullptr, "td_qual_host: read %lld has length %lld", (long long)i, (long long)(offs[i + 1] - offs[i]));
	const int64_t base = n_reads > 0 ? offs[0] : 0, n_bases = n_reads > 0 ? offs[n_reads] - base : 0;
	if (n_bases > 0 && !qual) return fail(nullptr, "td_qual_host: bad arguments");
	// the low flags as the device gets them: one pass over the batch's bytes
	std::vector<uint32_t> words((size_t)((n_bases + 31) / 32 + 1));
	if (td_qual_pack(n_bases > 0 ? qual + base : nullptr, n_bases, plan.thr, words.data()) != TD_OK) return TD_FAIL;
	bool judged[128];
	for (int h = 0; h < 128; h++) {
		const int seg = h < model->H ? model->label[h] & 0xFFFF : model->S;
		judged[h] = seg < model->S && ((plan.judged >> seg) & 1ull) != 0ull;
	}
	td_qual_totals t{};
	for (int64_t i = 0; i < n_reads; i++) {
		if (res[i].read_type != TD_EXTRACT_SUCCESS) continue;
		t.eligible++;
		const int64_t len = offs[i + 1] - offs[i], g0 = offs[i] - base;
		const int8_t* lab = labels + offs[i] + i;
		int64_t n_low = 0;
		for (int64_t p = 0; p < len; p++) {
			const int l = lab[p + 1];
			if (l < 0 || !judged[l]) continue;
			n_low += (words[(size_t)((g0 + p) >> 5)] >> ((g0 + p) & 31)) & 1u;
		}
		t.low_bases += n_low;
		if (n_low > plan.p.max_low) { res[i].read_type = TD_EXTRACT_FAIL_LOW_BASE_QUALITY; t.failed++; }
		else t.passed++;
	}
	if (totals) *totals = t;
	return TD_OK;
}
