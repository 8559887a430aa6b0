// dedup_host_check.cpp -- td_mol_dedup_host (include/tagdust_molecules.h) as a stand-alone program, for running it under the host
// sanitizers: no GPU is used, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tagdust_amd/csrc/td_census_host.cpp tagdust_amd/csrc/td_molecules_host.cpp tools/dedup_host_check.cpp -o /tmp/dedup_host_check
//   /tmp/dedup_host_check                                        # (leak detection stays on)
//
// Generated reads (lengths 0..200, N bases, every outcome, barcodes -1..299, few fingerprints of either sign), generated labels
// over an F-B-R-S-R model; for prefixes of 1, 7, 16 and 32 bases the marks and totals are held against a restatement with
// std::map over td_mol_host's own keys of each single read, the identities against td_mol_host's totals, and the reversed batch
// must keep the last read of every key.  is_duplicate has exactly n_reads bytes.  Exit status 0 when all of it agrees.
#define HOST_CHECK_NAME "dedup_host_check"
#include "host_check.h"
#include "../include/tagdust_molecules.h"

struct Batch {
	std::vector<int64_t> offs{ 0 };
	std::vector<uint8_t> codes;
	std::vector<int8_t> labels;
	std::vector<td_read_result> res;
};

int main()
{
	// F(1 HMM) B(3) R(1) S(1) R(1): label = hmm << 16 | segment
	const int32_t n_hmm[5] = { 1, 3, 1, 1, 1 }, n_col[5] = { 4, 6, 1, 3, 1 }, finger_len[5] = { 4, 0, 0, 0, 0 };
	const int8_t seg_type[5] = { 'F', 'B', 'R', 'S', 'R' };
	const int32_t label[7] = { 0, 1, (1 << 16) | 1, (2 << 16) | 1, 2, 3, 4 };
	td_model_desc m{};
	m.S = 5; m.H = 7; m.n_hmm = n_hmm; m.n_col = n_col; m.seg_type = seg_type; m.finger_len = finger_len; m.label = label;

	uint32_t s = 815u;
	const int64_t n = 3000;
	std::vector<std::vector<uint8_t>> seqs((size_t)n);
	std::vector<std::vector<int8_t>> labs((size_t)n);
	std::vector<td_read_result> recs((size_t)n);
	for (int64_t i = 0; i < n; i++) {
		const int len = (int)(rnd(s) % 201u);
		int h = 0;
		labs[(size_t)i].push_back(0);
		for (int p = 0; p < len; p++) {
			seqs[(size_t)i].push_back((uint8_t)(rnd(s) % 60u == 0 ? 4 : rnd(s) % 2u));   // (two bases: equal prefixes are met)
			if (rnd(s) % 4u == 0 && h < 6) h++;
			labs[(size_t)i].push_back((int8_t)h);
		}
		td_read_result r{};
		r.read_type = (int32_t)(rnd(s) % 3u == 0 ? rnd(s) % 7u : 0u) | (rnd(s) % 5u == 0 ? 0x300 : 0);
		r.barcode = rnd(s) % 3u == 0 ? (int32_t)(rnd(s) % 301u) - 1 : (int32_t)(rnd(s) % 3u);
		r.fingerprint = rnd(s) % 4u == 0 ? -1 : (int32_t)((rnd(s) % 3u) * 0x3A5F1700u + 4u);
		recs[(size_t)i] = r;
	}
	auto batch_of = [&](bool reversed) {
		Batch b;
		for (int64_t q = 0; q < n; q++) {
			const size_t i = (size_t)(reversed ? n - 1 - q : q);
			b.codes.insert(b.codes.end(), seqs[i].begin(), seqs[i].end());
			b.labels.insert(b.labels.end(), labs[i].begin(), labs[i].end());
			b.offs.push_back(b.offs.back() + (int64_t)seqs[i].size());
			b.res.push_back(recs[i]);
		}
		if (b.codes.empty()) b.codes.push_back(0);
		return b;
	};
	const Batch fwd = batch_of(false), rev = batch_of(true);

	for (int32_t P : { 1, 7, 16, 32 }) {
		// the key of every read on its own, from td_mol_host over that read alone (0: not counted)
		std::vector<uint64_t> key((size_t)n, 0);
		std::vector<bool> elig((size_t)n, false);
		for (int64_t i = 0; i < n; i++) {
			const int64_t o[2] = { 0, fwd.offs[(size_t)i + 1] - fwd.offs[(size_t)i] };
			td_census_entry* e = nullptr;
			int64_t k = 0;
			td_mol_totals t{};
			CHECK(td_mol_host(&m, P, fwd.codes.data() + fwd.offs[(size_t)i], o, 1, &fwd.res[(size_t)i], fwd.labels.data() + fwd.offs[(size_t)i] + i, &e, &k, &t) == TD_OK);
			elig[(size_t)i] = t.eligible == 1;
			if (k == 1) key[(size_t)i] = e[0].key;
			td_census_free(e);
		}
		td_mol_totals mt{};
		{
			td_census_entry* e = nullptr;
			int64_t k = 0;
			CHECK(td_mol_host(&m, P, fwd.codes.data(), fwd.offs.data(), n, fwd.res.data(), fwd.labels.data(), &e, &k, &mt) == TD_OK);
			td_census_free(e);
		}
		uint8_t* dup = (uint8_t*)malloc((size_t)n);       // (exactly n bytes: the sanitizer sees one too many)
		uint8_t* rdup = (uint8_t*)malloc((size_t)n);
		CHECK(dup && rdup);
		td_mol_dedup_totals t{}, rt{};
		CHECK(td_mol_dedup_host(&m, P, fwd.codes.data(), fwd.offs.data(), n, fwd.res.data(), fwd.labels.data(), dup, &t) == TD_OK);
		CHECK(td_mol_dedup_host(&m, P, rev.codes.data(), rev.offs.data(), n, rev.res.data(), rev.labels.data(), rdup, &rt) == TD_OK);
		std::map<uint64_t, int64_t> first, last;
		td_mol_dedup_totals w{};
		for (int64_t i = 0; i < n; i++) {
			if (!elig[(size_t)i]) { CHECK(dup[i] == 0); continue; }
			if (key[(size_t)i] == 0) { w.unjudged++; w.kept++; CHECK(dup[i] == 0); continue; }
			if (!first.count(key[(size_t)i])) first[key[(size_t)i]] = i;
			last[key[(size_t)i]] = i;
			const bool d = first[key[(size_t)i]] != i;
			CHECK(dup[i] == (d ? 1 : 0));
			if (d) w.duplicates++; else w.kept++;
		}
		CHECK(memcmp(&w, &t, sizeof w) == 0 && memcmp(&rt, &t, sizeof t) == 0);
		CHECK(t.duplicates > 0 && t.unjudged > 0 && mt.eligible == t.kept + t.duplicates);
		CHECK(t.kept == mt.molecules + mt.skipped_empty + mt.skipped_n + mt.overflow && t.unjudged == mt.skipped_empty + mt.skipped_n);
		for (int64_t i = 0; i < n; i++)
			CHECK(rdup[n - 1 - i] == (key[(size_t)i] != 0 && last[key[(size_t)i]] != i ? 1 : 0));
		free(dup); free(rdup);
	}
	uint8_t one = 0;
	CHECK(td_mol_dedup_host(&m, 0, fwd.codes.data(), fwd.offs.data(), n, fwd.res.data(), fwd.labels.data(), &one, nullptr) == TD_FAIL);
	CHECK(td_mol_dedup_host(&m, 33, fwd.codes.data(), fwd.offs.data(), n, fwd.res.data(), fwd.labels.data(), &one, nullptr) == TD_FAIL);
	CHECK(td_mol_dedup_host(&m, 20, fwd.codes.data(), fwd.offs.data(), n, fwd.res.data(), fwd.labels.data(), nullptr, nullptr) == TD_FAIL);
	CHECK(td_mol_dedup_host(&m, 20, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == TD_OK);
	printf("dedup_host_check: ok\n");
	return 0;
}
