// samples_host_check.cpp -- the host side of include/tagdust_samples.h (td_samples_host, td_samples_key, td_samples_key_calls, the
// check of a sheet) as a stand-alone program: no HIP runtime, no Python.  Built under the sanitizers by tools/host_checks.sh:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tagdust_amd/csrc/td_census_host.cpp tagdust_amd/csrc/td_samples_host.cpp tools/samples_host_check.cpp -o /tmp/samples_host_check
//   /tmp/samples_host_check                                      # (leak detection stays on)
//
// Generated labels over a B-S-B-R model (paths the decode kernels would not leave among them: the host scans to the end), every
// outcome; the rewrite, the entries and the totals are held against a restatement with std::map, two parts merged against the
// whole, every key taken apart and put together again, every refusal of a sheet.  Exit status 0 when all of it agrees.
#define HOST_CHECK_NAME "samples_host_check"
#include "host_check.h"
#include "../include/tagdust_samples.h"

int main()
{
	// B(3 barcodes + decoy) S(1) B(2 + decoy) R(1): label = call << 16 | segment
	const int32_t n_hmm[4] = { 4, 1, 3, 1 }, n_col[4] = { 6, 3, 4, 1 }, finger_len[4] = { 0, 0, 0, 0 };
	const int8_t seg_type[4] = { 'B', 'S', 'B', 'R' };
	const int32_t label[9] = { 0, 1 << 16, 2 << 16, 3 << 16, 1, 2, (1 << 16) | 2, (2 << 16) | 2, 3 };
	td_model_desc m{};
	m.S = 4; m.H = 9; m.n_hmm = n_hmm; m.n_col = n_col; m.seg_type = seg_type; m.finger_len = finger_len; m.label = label;
	const int32_t sheet[4 * 2] = { 0, 0, 1, 1, 2, 0, 0, 1 };

	uint32_t s = 4242u;
	const int64_t n = 3000;
	std::vector<int64_t> offs(1, 0);
	std::vector<int8_t> labels;
	std::vector<td_read_result> res((size_t)n);
	for (int64_t i = 0; i < n; i++) {
		const int len = (int)(rnd(s) % 61u);
		const int first[5] = { 0, 4, 5, 8, 9 };      // HMMs of segment j: first[j] .. first[j + 1] - 1
		int seg = (int)(rnd(s) % 6u == 0), h = first[seg] + (int)(rnd(s) % (uint32_t)(first[seg + 1] - first[seg]));
		labels.push_back(0);
		for (int p = 0; p < len; p++) {
			if (rnd(s) % 4u == 0 && seg < 3) {           // the next segment (now and then the one behind it), one of its HMMs
				seg += seg < 2 && rnd(s) % 7u == 0 ? 2 : 1;
				h = first[seg] + (int)(rnd(s) % (uint32_t)(first[seg + 1] - first[seg]));
			}
			if (rnd(s) % 53u == 0) h = (int)(rnd(s) % 9u);   // (a path the decode kernels would not leave)
			labels.push_back((int8_t)h);
		}
		offs.push_back(offs.back() + len);
		res[(size_t)i] = td_read_result{};
		res[(size_t)i].barcode = -1;
		res[(size_t)i].read_type = rnd(s) % 3u ? 0 : (int32_t)(rnd(s) % 8u) | (rnd(s) % 2u ? 0x300 : 0);
	}

	auto run = [&](int64_t lo, int64_t hi, std::vector<td_read_result>& out, std::vector<td_census_entry>& ent, td_samples_totals& t) {
		td_census_entry* e = nullptr;
		int64_t k = 0;
		std::vector<int64_t> o(offs.begin() + lo, offs.begin() + hi + 1);
		for (auto& v : o) v -= offs[(size_t)lo];
		out.assign(res.begin() + lo, res.begin() + hi);
		const int rc = td_samples_host(&m, sheet, 4, o.data(), hi - lo, out.data(), labels.data() + offs[(size_t)lo] + lo, &e, &k, &t);
		if (rc == TD_OK) ent.assign(e, e + k);
		td_census_free(e);
		return rc;
	};
	std::vector<td_read_result> got;
	std::vector<td_census_entry> ent;
	td_samples_totals t{};
	CHECK(run(0, n, got, ent, t) == TD_OK);
	// the restatement
	td_samples_totals w{};
	std::map<uint64_t, int64_t> counts;
	for (int64_t i = 0; i < n; i++) {
		td_read_result want = res[(size_t)i];
		if (want.read_type == TD_EXTRACT_SUCCESS) {
			w.eligible++;
			int32_t calls[2] = { -1, -1 };
			for (int64_t p = 0; p < offs[(size_t)i + 1] - offs[(size_t)i]; p++) {
				const int32_t v = label[labels[(size_t)(offs[(size_t)i] + i + p + 1)]];
				if ((v & 0xFFFF) == 0) calls[0] = v >> 16;
				if ((v & 0xFFFF) == 2) calls[1] = v >> 16;
			}
			counts[((uint64_t)2 << 56) | (uint64_t)(calls[0] + 1) | ((uint64_t)(calls[1] + 1) << 8)]++;
			int row = -1;
			for (int q = 0; q < 4; q++) if (sheet[2 * q] == calls[0] && sheet[2 * q + 1] == calls[1]) row = q;
			if (calls[0] < 0 || calls[1] < 0 || calls[0] == 3 || calls[1] == 2) { w.incomplete++; want.read_type = TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND; }
			else if (row >= 0) { w.assigned++; want.barcode = (2 << 16) | row; }
			else { w.unlisted++; want.read_type = TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND; }
		}
		CHECK(memcmp(&want, &got[(size_t)i], sizeof want) == 0);
	}
	CHECK(memcmp(&w, &t, sizeof w) == 0 && w.assigned > 50 && w.unlisted > 50 && w.incomplete > 50 && t.overflow == 0);
	CHECK(ent.size() == counts.size());
	int64_t sum = 0;
	for (size_t q = 0; q < ent.size(); q++) {
		CHECK(counts.count(ent[q].key) && counts[ent[q].key] == ent[q].count);
		CHECK(q == 0 || ent[q - 1].count > ent[q].count || (ent[q - 1].count == ent[q].count && ent[q - 1].key < ent[q].key));
		sum += ent[q].count;
		int32_t calls[TD_SAMPLES_MAX_SEGMENTS], km = 0;
		CHECK(td_samples_key_calls(ent[q].key, calls, &km) == TD_OK && km == 2 && td_samples_key(calls, km) == ent[q].key);
	}
	CHECK(sum == t.eligible);
	// two parts merged are the whole
	std::vector<td_read_result> ra, rb;
	std::vector<td_census_entry> a, b;
	td_samples_totals ta{}, tb{};
	CHECK(run(0, n / 3, ra, a, ta) == TD_OK && run(n / 3, n, rb, b, tb) == TD_OK);
	td_census_entry* merged = nullptr;
	int64_t nm = 0;
	CHECK(td_census_merge(a.data(), (int64_t)a.size(), b.data(), (int64_t)b.size(), &merged, &nm) == TD_OK);
	CHECK(nm == (int64_t)ent.size() && memcmp(merged, ent.data(), sizeof(td_census_entry) * (size_t)nm) == 0);
	td_census_free(merged);
	CHECK(ta.eligible + tb.eligible == t.eligible && ta.assigned + tb.assigned == t.assigned && ta.unlisted + tb.unlisted == t.unlisted);
	ra.insert(ra.end(), rb.begin(), rb.end());
	CHECK(memcmp(ra.data(), got.data(), sizeof(td_read_result) * (size_t)n) == 0);
	// refusals
	td_census_entry* e = nullptr;
	int64_t k = 0;
	const int32_t decoy[2] = { 3, 0 }, twice[4] = { 1, 1, 1, 1 };
	CHECK(td_samples_host(&m, decoy, 1, offs.data(), n, got.data(), labels.data(), &e, &k, &t) == TD_FAIL && g_err.find("row 0") != std::string::npos);
	CHECK(td_samples_host(&m, twice, 2, offs.data(), n, got.data(), labels.data(), &e, &k, &t) == TD_FAIL && g_err.find("row 1 of the sheet repeats row 0") != std::string::npos);
	CHECK(td_samples_host(&m, sheet, 0, offs.data(), n, got.data(), labels.data(), &e, &k, &t) == TD_FAIL);
	CHECK(td_samples_host(&m, sheet, 256, offs.data(), n, got.data(), labels.data(), &e, &k, &t) == TD_FAIL);
	int32_t calls[TD_SAMPLES_MAX_SEGMENTS], km = 0;
	CHECK(td_samples_key(nullptr, 2) == 0 && td_samples_key(decoy, 5) == 0 && td_samples_key_calls(0, calls, &km) == TD_FAIL);
	CHECK(td_samples_key_calls(((uint64_t)1 << 56) | 0x100u, calls, &km) == TD_FAIL);
	printf("samples_host_check: ok\n");
	return 0;
}
