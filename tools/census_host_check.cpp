// census_host_check.cpp -- the host side of include/tagdust_census.h (td_census_host, td_census_merge, td_census_key_text) as a
// stand-alone program, for running it under the host sanitizers: no GPU, no HIP runtime, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tagdust_amd/csrc/td_census_host.cpp tools/census_host_check.cpp -o /tmp/census_host_check
//   /tmp/census_host_check                                       # (leak detection stays on)
//
// Generated reads (lengths 0..200, N bases, every outcome), generated labels over a B-S-B-R model; the census of each B segment
// and of -1 is held against a restatement with std::map, the census of two halves merged against the whole, every key through
// td_census_key_text and back.  Exit status 0 when all of it agrees.
#define HOST_CHECK_NAME "census_host_check"
#include "host_check.h"
#include "../include/tagdust_census.h"

int main()
{
	// B(3 HMMs) S(1) B(2) R(1): label = hmm << 16 | segment
	const int32_t n_hmm[4] = { 3, 1, 2, 1 }, n_col[4] = { 6, 3, 4, 1 }, finger_len[4] = { 0, 0, 0, 0 };
	const int8_t seg_type[4] = { 'B', 'S', 'B', 'R' };
	const int32_t label[7] = { 0, 1 << 16, 2 << 16, 1, 2, (1 << 16) | 2, 3 };
	td_model_desc m{};
	m.S = 4; m.H = 7; m.n_hmm = n_hmm; m.n_col = n_col; m.seg_type = seg_type; m.finger_len = finger_len; m.label = label;

	uint32_t s = 12345u;
	const int64_t n = 3000;
	std::vector<int64_t> offs(1, 0);
	std::vector<uint8_t> codes;
	std::vector<int8_t> labels;
	std::vector<td_read_result> res((size_t)n);
	for (int64_t i = 0; i < n; i++) {
		const int len = (int)(rnd(s) % 201u);
		int h = 0;
		labels.push_back(0);
		for (int p = 0; p < len; p++) {
			codes.push_back((uint8_t)(rnd(s) % 40u == 0 ? 4 : rnd(s) % 4u));
			if (rnd(s) % 5u == 0 && h < 6) h++;
			if (rnd(s) % 97u == 0) h = (int)(rnd(s) % 7u);      // (a path the decode kernels would not leave: the host scans to the end)
			labels.push_back((int8_t)h);
		}
		offs.push_back(offs.back() + len);
		res[(size_t)i] = td_read_result{};
		res[(size_t)i].read_type = (int32_t)(rnd(s) % 7u) | (rnd(s) % 3u == 0 ? 0x300 : 0);
	}
	if (codes.empty()) codes.push_back(0);

	auto census = [&](int32_t seg, uint32_t mask, int64_t lo, int64_t hi, std::vector<td_census_entry>& out, td_census_totals& t) {
		td_census_entry* e = nullptr;
		int64_t k = 0;
		std::vector<int64_t> o(offs.begin() + lo, offs.begin() + hi + 1);
		for (auto& v : o) v -= offs[(size_t)lo];
		const int rc = td_census_host(&m, seg, mask, codes.data() + offs[(size_t)lo], o.data(), hi - lo, res.data() + lo, labels.data() + offs[(size_t)lo] + lo, &e, &k, &t);
		if (rc == TD_OK) out.assign(e, e + k);
		td_census_free(e);
		return rc;
	};
	for (int32_t seg : { -1, 0, 2 }) {
		for (uint32_t mask : { TD_CENSUS_DEFAULT_MASK, 1u, 0xFFu }) {
			std::vector<td_census_entry> got;
			td_census_totals t{};
			CHECK(census(seg, mask, 0, n, got, t) == TD_OK);
			const int want_seg = seg == -1 ? 2 : seg;
			std::map<uint64_t, int64_t> ref;
			td_census_totals w{};
			for (int64_t i = 0; i < n; i++) {
				const uint32_t type = (uint32_t)res[(size_t)i].read_type & 0xFFu;
				if (!((mask >> type) & 1u)) continue;
				w.eligible++;
				std::vector<int> word;
				for (int64_t p = 0; p < offs[(size_t)i + 1] - offs[(size_t)i]; p++)
					if ((label[labels[(size_t)(offs[(size_t)i] + i + p + 1)]] & 0xFFFF) == want_seg) word.push_back(codes[(size_t)(offs[(size_t)i] + p)]);
				bool has_n = false;
				for (int b : word) has_n = has_n || b > 3;
				if (word.empty()) w.skipped_empty++;
				else if (word.size() > 28) w.skipped_long++;
				else if (has_n) w.skipped_n++;
				else {
					uint64_t key = (uint64_t)word.size() << 56, v = 0;
					for (int b : word) v = (v << 2) | (uint64_t)b;
					ref[key | v]++;
					w.counted++;
				}
			}
			w.distinct = (int64_t)ref.size();
			CHECK(memcmp(&w, &t, sizeof w) == 0);
			CHECK(got.size() == ref.size() && w.counted > 0 && w.skipped_empty > 0 && w.skipped_long > 0 && w.skipped_n > 0);
			for (size_t q = 0; q < got.size(); q++) {
				CHECK(ref.count(got[q].key) && ref[got[q].key] == got[q].count);
				CHECK(q == 0 || got[q - 1].count > got[q].count || (got[q - 1].count == got[q].count && got[q - 1].key < got[q].key));
				char text[32];
				CHECK(td_census_key_text(got[q].key, text) == TD_OK && strlen(text) == (size_t)(got[q].key >> 56));
				uint64_t back = (uint64_t)strlen(text) << 56, v = 0;
				for (const char* c = text; *c; c++) v = (v << 2) | (uint64_t)(strchr("ACGT", *c) - "ACGT");
				CHECK((back | v) == got[q].key);
			}
			// two halves merged are the whole
			std::vector<td_census_entry> a, b;
			td_census_totals ta{}, tb{};
			CHECK(census(seg, mask, 0, n / 3, a, ta) == TD_OK && census(seg, mask, n / 3, n, b, tb) == TD_OK);
			td_census_entry* merged = nullptr;
			int64_t nm = 0;
			CHECK(td_census_merge(a.data(), (int64_t)a.size(), b.data(), (int64_t)b.size(), &merged, &nm) == TD_OK);
			CHECK(nm == (int64_t)got.size() && (nm == 0 || memcmp(merged, got.data(), sizeof(td_census_entry) * (size_t)nm) == 0));
			td_census_free(merged);
			CHECK(ta.eligible + tb.eligible == t.eligible && ta.counted + tb.counted == t.counted);
		}
	}
	std::vector<td_census_entry> none;
	td_census_totals t{};
	CHECK(census(1, 1u, 0, n, none, t) == TD_FAIL && census(4, 1u, 0, n, none, t) == TD_FAIL && census(-1, 0u, 0, n, none, t) == TD_FAIL);
	char text[32];
	CHECK(td_census_key_text(0, text) == TD_FAIL && td_census_key_text(29ull << 56, text) == TD_FAIL);
	printf("census_host_check: ok\n");
	return 0;
}
