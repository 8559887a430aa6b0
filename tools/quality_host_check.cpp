// quality_host_check.cpp -- the host side of include/tagdust_quality.h (td_qual_pack, td_qual_host, the check of the parameters) as a
// stand-alone program: no HIP runtime, no Python.  Built under the sanitizers by tools/host_checks.sh:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tagdust_amd/csrc/td_quality_host.cpp tools/quality_host_check.cpp -o /tmp/quality_host_check
//   /tmp/quality_host_check                                      # (leak detection stays on)
//
// The pack over buffers of exactly n bytes (a read past the end is the sanitizer's to find) against a bit-by-bit restatement, every
// n up to 200 and every threshold class; ranges that meet on a multiple of 32 packed side by side against the whole; td_qual_host
// over generated labels of a B-F-S-R model, every outcome, against a restatement, for every choice of segments and two K, a batch
// in two parts against the whole; every refusal.  Exit status 0 when all of it agrees.
#define HOST_CHECK_NAME "quality_host_check"
#include "host_check.h"
#include "../tagdust_amd/csrc/td_quality_def.h"

int main()
{
	uint32_t s = 777u;
	// ---- td_qual_pack ----
	const int32_t thrs[] = { 0, 1, 53, 84, 128, 200, 255, 256 };
	for (int64_t n = 0; n <= 200; n++)
		for (const int32_t thr : thrs) {
			std::vector<uint8_t> q((size_t)n);                 // (exactly n bytes: nothing behind them may be read)
			for (auto& b : q) { const uint32_t r = rnd(s); b = (uint8_t)(r % 5u == 0 ? thr : (r % 5u == 1 ? thr - 1 : r >> 3)); }
			std::vector<uint32_t> w((size_t)((n + 31) / 32 + 1), 0xDEADBEEFu);
			CHECK(td_qual_pack(n ? q.data() : nullptr, n, thr, w.data()) == TD_OK);
			for (int64_t g = 0; g < (int64_t)w.size() * 32; g++) {
				const uint32_t want = g < n && (int32_t)q[(size_t)g] < thr ? 1u : 0u;
				CHECK(((w[(size_t)(g >> 5)] >> (g & 31)) & 1u) == want);
			}
		}
	{   // ranges side by side are the whole
		const int64_t n = 5000;
		std::vector<uint8_t> q((size_t)n);
		for (auto& b : q) b = (uint8_t)(33 + rnd(s) % 42u);
		std::vector<uint32_t> whole((size_t)((n + 31) / 32 + 1)), parts(whole.size(), 0xDEADBEEFu);
		CHECK(td_qual_pack(q.data(), n, 53, whole.data()) == TD_OK);
		const int64_t cuts[] = { 0, 32, 64, 1024, 4992, n };
		for (int k = 4; k >= 0; k--) qual_pack_range(q.data(), cuts[k], cuts[k + 1], 53, parts.data());
		parts.back() = 0u;
		CHECK(whole == parts);
	}
	CHECK(td_qual_pack(nullptr, 1, 53, nullptr) == TD_FAIL && td_qual_pack(nullptr, -1, 53, &s) == TD_FAIL);
	uint8_t one = 0;
	uint32_t two[2];
	CHECK(td_qual_pack(&one, 1, -1, two) == TD_FAIL && td_qual_pack(&one, 1, 257, two) == TD_FAIL);

	// ---- td_qual_host: B(2 barcodes + decoy) F(1) S(1) R(1): label = call << 16 | segment ----
	const int32_t n_hmm[4] = { 3, 1, 1, 1 }, n_col[4] = { 4, 6, 3, 1 }, finger_len[4] = { 0, 6, 0, 0 };
	const int8_t seg_type[4] = { 'B', 'F', 'S', 'R' };
	const int32_t label[6] = { 0, 1 << 16, 2 << 16, 1, 2, 3 };
	const int seg_of[6] = { 0, 0, 0, 1, 2, 3 };
	td_model_desc m{};
	m.S = 4; m.H = 6; m.n_hmm = n_hmm; m.n_col = n_col; m.seg_type = seg_type; m.finger_len = finger_len; m.label = label;
	const int64_t n = 2000, first = 11;                    // (offs[0] != 0: the first flag is not word-aligned)
	std::vector<int64_t> offs(1, first);
	std::vector<int8_t> labels((size_t)first, 0);          // (labels of read i at offs[i] + i)
	std::vector<uint8_t> qual((size_t)first, 0);
	std::vector<td_read_result> res((size_t)n);
	for (int64_t i = 0; i < n; i++) {
		const int len = (int)(rnd(s) % 70u);
		int h = (int)(rnd(s) % 3u);
		labels.push_back(0);
		for (int p = 0; p < len; p++) {
			if (rnd(s) % 5u == 0 && h < 5) h = h < 3 ? 3 : h + 1;
			if (rnd(s) % 61u == 0) h = (int)(rnd(s) % 6u);   // (a path the decode kernels would not leave)
			labels.push_back((int8_t)(rnd(s) % 97u == 0 ? -1 : h));
			qual.push_back((uint8_t)(rnd(s) % 12u == 0 ? 33 + rnd(s) % 20u : (rnd(s) % 50u == 0 ? 200 : 53 + rnd(s) % 22u)));
		}
		offs.push_back(offs.back() + len);
		res[(size_t)i] = td_read_result{};
		res[(size_t)i].barcode = -1;
		res[(size_t)i].read_type = rnd(s) % 4u ? 0 : (int32_t)(rnd(s) % 9u) | (rnd(s) % 2u ? 0x300 : 0);
	}
	auto run = [&](const td_qual_params& p, int64_t lo, int64_t hi, std::vector<td_read_result>& out, td_qual_totals& t) {
		out.assign(res.begin() + lo, res.begin() + hi);
		// (a sub-range keeps the batch's offsets: labels move by the reads in front)
		return td_qual_host(&m, &p, offs.data() + lo, hi - lo, out.data(), labels.data() + lo, qual.data(), &t);
	};
	for (int segs = 1; segs <= 3; segs++)
		for (const int K : { 0, 2 }) {
			const td_qual_params p{ 20, 33, K, segs };
			std::vector<td_read_result> got;
			td_qual_totals t{}, w{};
			CHECK(run(p, 0, n, got, t) == TD_OK);
			for (int64_t i = 0; i < n; i++) {
				td_read_result want = res[(size_t)i];
				if (want.read_type == TD_EXTRACT_SUCCESS) {
					w.eligible++;
					int64_t n_low = 0;
					for (int64_t q = 0; q < offs[(size_t)i + 1] - offs[(size_t)i]; q++) {
						const int l = labels[(size_t)(offs[(size_t)i] + i + q + 1)];
						if (l < 0) continue;
						const int8_t ty = seg_type[seg_of[l]];
						const bool judged = (ty == 'B' && (segs & TD_QUAL_SEG_B)) || (ty == 'F' && (segs & TD_QUAL_SEG_F));
						if (judged && qual[(size_t)(offs[(size_t)i] + q)] < 53) n_low++;
					}
					w.low_bases += n_low;
					if (n_low > K) { w.failed++; want.read_type = TD_EXTRACT_FAIL_LOW_BASE_QUALITY; } else w.passed++;
				}
				CHECK(memcmp(&want, &got[(size_t)i], sizeof want) == 0);
			}
			CHECK(memcmp(&w, &t, sizeof w) == 0 && t.eligible == t.passed + t.failed && t.failed > 20 && t.passed > 20);
			// two parts are the whole
			std::vector<td_read_result> ra, rb;
			td_qual_totals ta{}, tb{};
			CHECK(run(p, 0, n / 3, ra, ta) == TD_OK && run(p, n / 3, n, rb, tb) == TD_OK);
			ra.insert(ra.end(), rb.begin(), rb.end());
			CHECK(memcmp(ra.data(), got.data(), sizeof(td_read_result) * (size_t)n) == 0);
			CHECK(ta.eligible + tb.eligible == t.eligible && ta.failed + tb.failed == t.failed && ta.low_bases + tb.low_bases == t.low_bases);
		}
	// refusals
	std::vector<td_read_result> got;
	td_qual_totals t{};
	CHECK(run(td_qual_params{ 0, 33, 0, 3 }, 0, n, got, t) == TD_FAIL && g_err.find("min_quality") != std::string::npos);
	CHECK(run(td_qual_params{ 94, 33, 0, 3 }, 0, n, got, t) == TD_FAIL);
	CHECK(run(td_qual_params{ 20, 32, 0, 3 }, 0, n, got, t) == TD_FAIL && g_err.find("offset") != std::string::npos);
	CHECK(run(td_qual_params{ 20, 33, -1, 3 }, 0, n, got, t) == TD_FAIL && g_err.find("max_low") != std::string::npos);
	CHECK(run(td_qual_params{ 20, 33, 0, 0 }, 0, n, got, t) == TD_FAIL && run(td_qual_params{ 20, 33, 0, 4 }, 0, n, got, t) == TD_FAIL);
	const int8_t no_f[4] = { 'B', 'S', 'S', 'R' };
	m.seg_type = no_f;
	CHECK(run(td_qual_params{ 20, 33, 0, TD_QUAL_SEG_F }, 0, n, got, t) == TD_FAIL && g_err.find("no 'F' segment") != std::string::npos);
	CHECK(run(td_qual_params{ 20, 33, 0, 3 }, 0, n, got, t) == TD_OK);
	m.seg_type = seg_type;
	const td_qual_params ok{ 20, 33, 0, 3 };
	CHECK(td_qual_host(nullptr, &ok, offs.data(), n, got.data(), labels.data(), qual.data(), &t) == TD_FAIL);
	CHECK(td_qual_host(&m, nullptr, offs.data(), n, got.data(), labels.data(), qual.data(), &t) == TD_FAIL);
	CHECK(td_qual_host(&m, &ok, nullptr, n, got.data(), labels.data(), qual.data(), &t) == TD_FAIL);
	CHECK(td_qual_host(&m, &ok, offs.data(), n, got.data(), labels.data(), nullptr, &t) == TD_FAIL);
	CHECK(td_qual_host(&m, &ok, offs.data(), 0, nullptr, nullptr, nullptr, &t) == TD_OK && t.eligible == 0);
	printf("quality_host_check: ok\n");
	return 0;
}
