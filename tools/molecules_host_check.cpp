// molecules_host_check.cpp -- the host side of include/tagdust_molecules.h (td_mol_host, td_mol_summarise, td_mol_key) and
// td_fingerprint_text of include/tagdust_io.h as a stand-alone program, for running them under the host sanitizers: no GPU, no HIP
// runtime, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tagdust_amd/csrc/td_census_host.cpp tagdust_amd/csrc/td_molecules_host.cpp tagdust_amd/csrc/td_fastq.cpp \
//       tools/molecules_host_check.cpp -o /tmp/molecules_host_check -lpthread
//   /tmp/molecules_host_check                                    # (leak detection stays on)
//
// Generated reads (lengths 0..200, N bases, every outcome, barcodes -1..299, fingerprints of any sign), generated labels over an
// F-B-R-S-R model; the count for prefixes of 1, 7, 16, 31 and 32 bases is held against a restatement with std::map, the summary
// against a restatement, two parts merged against the whole, every fingerprint's text against get_finger_seq restated -- for the
// lengths 0..255 the low byte can name, whose last character is buf[255].  Exit status 0 when all of it agrees.
#define HOST_CHECK_NAME "molecules_host_check"
#include "host_check.h"
#include "../include/tagdust_io.h"
#include "../include/tagdust_molecules.h"

static uint64_t mix(uint64_t k)
{
	k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ull;
	k ^= k >> 27; k *= 0x94D049BB133111EBull;
	k ^= k >> 31;
	return k;
}

int main()
{
	// F(1 HMM) B(3) R(1) S(1) R(1): label = hmm << 16 | segment
	const int32_t n_hmm[5] = { 1, 3, 1, 1, 1 }, n_col[5] = { 4, 6, 1, 3, 1 }, finger_len[5] = { 4, 0, 0, 0, 0 };
	const int8_t seg_type[5] = { 'F', 'B', 'R', 'S', 'R' };
	const int32_t label[7] = { 0, 1, (1 << 16) | 1, (2 << 16) | 1, 2, 3, 4 };
	td_model_desc m{};
	m.S = 5; m.H = 7; m.n_hmm = n_hmm; m.n_col = n_col; m.seg_type = seg_type; m.finger_len = finger_len; m.label = label;

	uint32_t s = 4711u;
	const int64_t n = 4000;
	std::vector<int64_t> offs(1, 0);
	std::vector<uint8_t> codes;
	std::vector<int8_t> labels;
	std::vector<td_read_result> res((size_t)n);
	for (int64_t i = 0; i < n; i++) {
		const int len = (int)(rnd(s) % 201u);
		int h = 0;
		labels.push_back(0);
		for (int p = 0; p < len; p++) {
			codes.push_back((uint8_t)(rnd(s) % 60u == 0 ? 4 : rnd(s) % 4u));
			if (rnd(s) % 4u == 0 && h < 6) h++;
			if (rnd(s) % 97u == 0) h = (int)(rnd(s) % 7u);
			labels.push_back((int8_t)h);
		}
		offs.push_back(offs.back() + len);
		res[(size_t)i] = td_read_result{};
		res[(size_t)i].read_type = (int32_t)(rnd(s) % 3u == 0 ? rnd(s) % 7u : 0u) | (rnd(s) % 5u == 0 ? 0x300 : 0);
		res[(size_t)i].barcode = (int32_t)(rnd(s) % 301u) - 1;
		// few distinct values, so that equal keys are met; some negative, -1 among them
		res[(size_t)i].fingerprint = rnd(s) % 4u == 0 ? -1 : (int32_t)((rnd(s) % 6u) * 0x3A5F1700u + 4u);
		if (rnd(s) % 3u == 0) res[(size_t)i].barcode = (int32_t)(rnd(s) % 3u);
	}
	if (codes.empty()) codes.push_back(0);

	auto count = [&](int32_t P, int64_t lo, int64_t hi, std::vector<td_census_entry>& out, td_mol_totals& t) {
		td_census_entry* e = nullptr;
		int64_t k = 0;
		std::vector<int64_t> o(offs.begin() + lo, offs.begin() + hi + 1);
		for (auto& v : o) v -= offs[(size_t)lo];
		const int rc = td_mol_host(&m, P, codes.data() + offs[(size_t)lo], o.data(), hi - lo, res.data() + lo, labels.data() + offs[(size_t)lo] + lo, &e, &k, &t);
		if (rc == TD_OK) out.assign(e, e + k);
		td_census_free(e);
		return rc;
	};
	for (int32_t P : { 1, 7, 16, 31, 32 }) {
		std::vector<td_census_entry> got;
		td_mol_totals t{};
		CHECK(count(P, 0, n, got, t) == TD_OK);
		std::map<uint64_t, int64_t> ref;
		td_mol_totals w{};
		for (int64_t i = 0; i < n; i++) {
			if (((uint32_t)res[(size_t)i].read_type & 0xFFu) != 0u) continue;
			w.eligible++;
			std::vector<int> word;
			for (int64_t p = 0; p < offs[(size_t)i + 1] - offs[(size_t)i] && (int)word.size() < P; p++)
				if (seg_type[label[labels[(size_t)(offs[(size_t)i] + i + p + 1)]] & 0xFFFF] == 'R') word.push_back(codes[(size_t)(offs[(size_t)i] + p)]);
			bool has_n = false;
			for (int b : word) has_n = has_n || b > 3;
			if (word.empty()) w.skipped_empty++;
			else if (has_n) w.skipped_n++;
			else {
				uint64_t v = 0;
				for (int b : word) v = (v << 2) | (uint64_t)b;
				const uint64_t a = mix(((uint64_t)(uint32_t)res[(size_t)i].fingerprint << 8) | (uint64_t)word.size());
				uint64_t low = mix(v ^ a) & 0x00FFFFFFFFFFFFFFull;
				if (low == 0) low = 1;
				const int32_t bar = res[(size_t)i].barcode;
				const uint64_t key = ((uint64_t)(bar == -1 ? 0 : bar & 0xFF) << 56) | low;
				CHECK(key == td_mol_key(bar, res[(size_t)i].fingerprint, v, (int32_t)word.size()));
				ref[key]++;
				w.counted++;
			}
		}
		w.molecules = (int64_t)ref.size();
		CHECK(memcmp(&w, &t, sizeof w) == 0);
		CHECK(got.size() == ref.size() && w.counted > 0 && w.skipped_empty > 0 && w.skipped_n > 0 && w.molecules < w.counted);
		td_mol_row want[TD_NUM_BARCODE_BINS];
		memset(want, 0, sizeof want);
		for (size_t q = 0; q < got.size(); q++) {
			CHECK(ref.count(got[q].key) && ref[got[q].key] == got[q].count);
			CHECK(q == 0 || got[q - 1].count > got[q].count || (got[q - 1].count == got[q].count && got[q - 1].key < got[q].key));
			CHECK(td_mol_key_bin(got[q].key) == (int32_t)(got[q].key >> 56));
			td_mol_row& r = want[got[q].key >> 56];
			r.reads += got[q].count; r.molecules++;
			r.levels[(got[q].count < 10 ? got[q].count : 10) - 1]++;
		}
		td_mol_row rows[TD_NUM_BARCODE_BINS];
		CHECK(td_mol_summarise(got.data(), (int64_t)got.size(), rows) == TD_OK && memcmp(rows, want, sizeof rows) == 0);
		if (P == 1) CHECK(rows[0].levels[9] > 0 && rows[1].levels[9] > 0);   // (the last level is met: three barcodes, six fingerprints, four bases)
		// two parts merged are the whole
		std::vector<td_census_entry> a, b;
		td_mol_totals ta{}, tb{};
		CHECK(count(P, 0, n / 3, a, ta) == TD_OK && count(P, n / 3, n, b, tb) == TD_OK);
		td_census_entry* merged = nullptr;
		int64_t nm = 0;
		CHECK(td_census_merge(a.data(), (int64_t)a.size(), b.data(), (int64_t)b.size(), &merged, &nm) == TD_OK);
		CHECK(nm == (int64_t)got.size() && (nm == 0 || memcmp(merged, got.data(), sizeof(td_census_entry) * (size_t)nm) == 0));
		td_census_free(merged);
		CHECK(ta.eligible + tb.eligible == t.eligible && ta.counted + tb.counted == t.counted);
	}
	std::vector<td_census_entry> none;
	td_mol_totals t{};
	CHECK(count(0, 0, n, none, t) == TD_FAIL && count(33, 0, n, none, t) == TD_FAIL);
	td_mol_row rows[TD_NUM_BARCODE_BINS];
	CHECK(td_mol_summarise(nullptr, 0, rows) == TD_OK && rows[0].reads == 0 && td_mol_summarise(nullptr, 1, rows) == TD_FAIL);

	// td_fingerprint_text: every length the low byte can name, values of either sign
	for (int k = 0; k < 20000; k++) {
		const int32_t fp = k < 256 ? (int32_t)(0xDEADBE00u | (uint32_t)k) : (int32_t)((rnd(s) << 8) ^ rnd(s));
		char* buf = (char*)malloc(256);        // (exactly the documented size: the sanitizer sees one byte too many)
		CHECK(buf);
		const int len = td_fingerprint_text(fp, buf);
		CHECK(len == (fp & 0xFF) && strlen(buf) == (size_t)len);
		int key = fp >> 8;
		for (int i = 0; i < len; i++) { CHECK(buf[len - i - 1] == "ACGT"[key & 3]); key = key >> 2; }
		free(buf);
	}
	char text[256];
	CHECK(td_fingerprint_text((27 << 8) | 4, text) == 4 && !strcmp(text, "ACGT"));
	CHECK(td_fingerprint_text(-1253657586, text) == 14 && !strcmp(text, "TTGTCCCACGGTCA"));
	printf("molecules_host_check: ok\n");
	return 0;
}
