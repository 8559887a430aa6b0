// td_calibrate.cpp -- the two entry points of include/tagdust_model.h that drive a context: the threshold from simulated reads
// (td_estimate_threshold) and the choice among candidate architectures (td_compare_architectures).  Plain C++ over the C ABI; what
// they compute on the host themselves is td_model.cpp's (td_calibration_classes, td_arch_posteriors: td_model_inner.h), so that
// td_model.cpp links without a context.
#include <stdlib.h>

#include <string>
#include <thread>
#include <vector>

#include "../../include/tagdust_model.h"
#include "td_jit.h"
#include "td_model_inner.h"

extern "C" int td_estimate_threshold(td_ctx* ctx, const td_arch* a, const td_seq_stats* ssi, float d, uint32_t seed,
                                     int32_t n_reads, int32_t rng, float* threshold)
{
	if (!ctx || !threshold) return TD_FAIL;
	// The scoring model's kernel is compiled (seconds) while the host emits the reads (seconds, bound to one thread by the
	// rand() sequence): the compile only fills the code cache td_model_upload looks into.
	std::thread warm;
	td_model_tables* scoring = nullptr;
	int32_t specialize = 0;
	const bool overlap = getenv("TD_CAL_OVERLAP") ? atoi(getenv("TD_CAL_OVERLAP")) != 0 : true;
	if (overlap && td_get_option(ctx, "specialize", &specialize) == TD_OK && specialize &&
	    td_model_build(a, ssi, 0.05f, d, &scoring) == TD_OK) {
		warm = std::thread([scoring] {
			const TdSpecPlan plan = td_spec_plan(&scoring->desc, td_spec_knobs());
			std::vector<char> code; std::string log;
			(void)td_spec_compile(&scoring->desc, plan, plan.k.lsum_oob, 0, code, log);
		});
	}
	td_calibration* cal = nullptr;
	const int emitted = td_calibration_emit(a, ssi, d, seed, n_reads, rng, &cal);
	if (warm.joinable()) warm.join();
	td_model_tables_free(scoring);
	if (emitted != TD_OK) return TD_FAIL;
	int rc = TD_FAIL;
	const int64_t n = cal->n_reads;
	std::vector<float> q((size_t)n);
	bool ok = td_model_upload(ctx, &cal->scoring->desc) == TD_OK;
	if (ok) {
		for (const TdCalClass& k : td_calibration_classes(cal->codes, cal->offs, n)) {
			std::vector<td_read_result> res(k.idx.size());
			ok = td_batch_upload(ctx, k.codes.data(), k.offs.data(), (int64_t)k.idx.size()) == TD_OK && td_run(ctx, TD_MODE_GET_PROB) == TD_OK &&
			     td_batch_download(ctx, res.data(), nullptr, nullptr) == TD_OK;
			if (!ok) break;
			for (size_t j = 0; j < k.idx.size(); j++) q[(size_t)k.idx[j]] = res[j].mapq;
		}
	}
	if (ok) {
		*threshold = td_calibration_select(q.data(), cal->is_random, n);
		rc = TD_OK;
	}
	td_calibration_free(cal);
	return rc;
}

extern "C" int td_compare_architectures(td_ctx* ctx, const td_arch* const* archs, int32_t n_arch, const uint8_t* codes,
                                        const int64_t* offs, int64_t n_reads, float e, float d, int32_t n_threads,
                                        float* posterior, int32_t* best)
{
	if (!ctx || !archs || n_arch < 1 || !codes || !offs || !posterior || !best || n_reads < 1) return TD_FAIL;
	if (n_threads < 1) n_threads = 1;
	// test_architectures() sets num_query = 100 000 (:38-42): statistics then scan batches of 100 000 reads until more than
	// 1 000 000 were seen (1 100 000 reads), and the candidates are scored on the first batch only (:182-184)
	const int64_t n_score = n_reads < 100000 ? n_reads : 100000;
	// every candidate's own sequence statistics and model (test_architectures.c:60-170), then all of them over the first
	// batch in one launch of the generic kernel (td_arch_scores: no per-candidate compile, reads staged once)
	std::vector<td_model_tables*> tabs((size_t)n_arch, nullptr);
	std::vector<const td_model_desc*> descs((size_t)n_arch, nullptr);
	int rc = TD_OK;
	for (int k = 0; k < n_arch && rc == TD_OK; k++) {
		td_seq_stats st;
		if (sequence_stats_limit(archs[k], codes, offs, n_reads, &st, 1100000) != TD_OK || td_model_build(archs[k], &st, e, d, &tabs[(size_t)k]) != TD_OK) rc = TD_FAIL;
		else descs[(size_t)k] = &tabs[(size_t)k]->desc;
	}
	std::vector<float> b((size_t)n_arch * (size_t)n_score);
	if (rc == TD_OK && td_arch_scores(ctx, descs.data(), n_arch, codes, offs, n_score, b.data()) != TD_OK) rc = TD_FAIL;
	for (td_model_tables* t : tabs) td_model_tables_free(t);
	if (rc != TD_OK) return TD_FAIL;
	td_arch_posteriors(b.data(), n_arch, n_score, n_threads, posterior, best);
	return TD_OK;
}
