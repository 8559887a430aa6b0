// mate_host_check.cpp -- the four *_mated host functions (include/tagdust_molecules.h) as a stand-alone program, for running them
// under the host sanitizers: no GPU is used, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tagdust_amd/csrc/td_census_host.cpp tagdust_amd/csrc/td_molecules_host.cpp tools/mate_host_check.cpp -o /tmp/mate_host_check
//   /tmp/mate_host_check                                         # (leak detection stays on)
//
// Generated reads as tools/dedup_host_check.cpp makes them (lengths 0..200, N bases, every outcome, few fingerprints), generated
// labels over an F-B-R-S-R model, and a mate per read of 0..50 bases over two letters with an N now and then, the mate batch in a
// block of exactly offs[n] bytes whose last mates are shorter than M: a read past a mate's end that leaves the block is the
// sanitizer's to see, one that stays inside shows in the keys.  For several (P, M) every read's class, key and origin are restated
// from td_mol_host_origins over that read alone (its own prefix word) and the mate's bytes, and td_mol_host_origins_mated,
// td_mol_dedup_host_mated and td_mol_dedup_collapsed_host_mated over the whole batch are held against that; mate == NULL against the
// unmated functions; the refusals.  Exit status 0 when all of it agrees.
#define HOST_CHECK_NAME "mate_host_check"
#include "host_check.h"
#include "../include/tagdust_molecules.h"

int main()
{
	// F(1 HMM) B(3) R(1) S(1) R(1): label = hmm << 16 | segment
	const int32_t n_hmm[5] = { 1, 3, 1, 1, 1 }, n_col[5] = { 4, 6, 1, 3, 1 }, finger_len[5] = { 4, 0, 0, 0, 0 };
	const int8_t seg_type[5] = { 'F', 'B', 'R', 'S', 'R' };
	const int32_t label[7] = { 0, 1, (1 << 16) | 1, (2 << 16) | 1, 2, 3, 4 };
	td_model_desc m{};
	m.S = 5; m.H = 7; m.n_hmm = n_hmm; m.n_col = n_col; m.seg_type = seg_type; m.finger_len = finger_len; m.label = label;

	uint32_t s = 2718u;
	const int64_t n = 3000;
	std::vector<int64_t> offs{ 0 }, moffs{ 0 };
	std::vector<uint8_t> codes, mcodes;
	std::vector<int8_t> labels;
	std::vector<td_read_result> res;
	for (int64_t i = 0; i < n; i++) {
		const int len = (int)(rnd(s) % 201u);
		int h = rnd(s) % 3u == 0 ? 2 : 0;                 // (a third of the reads have no read base in front of label 4)
		labels.push_back(0);
		for (int p = 0; p < len; p++) {
			codes.push_back((uint8_t)(rnd(s) % 60u == 0 ? 4 : rnd(s) % 2u));   // (two bases: equal prefixes are met)
			if (rnd(s) % 4u == 0 && h < 6) h++;
			labels.push_back((int8_t)(rnd(s) % 7u == 0 ? 3 : h));            // (now and then a barcode label: no read base)
		}
		offs.push_back(offs.back() + len);
		td_read_result r{};
		r.read_type = (int32_t)(rnd(s) % 3u == 0 ? rnd(s) % 7u : 0u) | (rnd(s) % 5u == 0 ? 0x300 : 0);
		r.barcode = rnd(s) % 3u == 0 ? (int32_t)(rnd(s) % 301u) - 1 : (int32_t)(rnd(s) % 3u);
		r.fingerprint = rnd(s) % 4u == 0 ? -1 : (int32_t)((rnd(s) % 3u) * 0x3A5F1700u + 4u);
		res.push_back(r);
		int mlen = (int)(rnd(s) % 51u);
		if (rnd(s) % 6u == 0) mlen = 0;
		if (i >= n - 3) mlen = (int)(n - i);               // the block ends in mates of 3, 2 and 1 bases
		for (int p = 0; p < mlen; p++) mcodes.push_back((uint8_t)(rnd(s) % 40u == 0 ? 4 + rnd(s) % 250u : (p < 3 ? rnd(s) % 2u : 0u)));
		moffs.push_back(moffs.back() + mlen);
	}
	if (codes.empty()) codes.push_back(0);
	uint8_t* mblock = (uint8_t*)malloc(mcodes.size());   // (exactly offs[n] bytes)
	CHECK(mblock && !mcodes.empty());
	memcpy(mblock, mcodes.data(), mcodes.size());

	const int32_t pm[][2] = { { 1, 31 }, { 12, 20 }, { 8, 8 }, { 31, 1 }, { 5, 2 } };
	for (const auto& q : pm) {
		const int32_t P = q[0], M = q[1];
		const td_mol_mate mate{ mblock, moffs.data(), M };
		// every read on its own: its class, key and origin from its own prefix (td_mol_host_origins over that read) and the mate's bytes
		enum { NOT = 0, EMPTY, HAS_N, COUNTED };
		std::vector<int> cls((size_t)n, NOT);
		std::vector<uint64_t> key((size_t)n, 0);
		std::map<uint64_t, int64_t> count, first;
		std::map<uint64_t, td_mol_origin> origin;
		td_mol_totals want{};
		for (int64_t i = 0; i < n; i++) {
			const int64_t o[2] = { 0, offs[(size_t)i + 1] - offs[(size_t)i] };
			td_census_entry* e = nullptr;
			td_mol_origin* eo = nullptr;
			int64_t k = 0;
			td_mol_totals t{};
			CHECK(td_mol_host_origins(&m, P, codes.data() + offs[(size_t)i], o, 1, &res[(size_t)i], labels.data() + offs[(size_t)i] + i, &e, &eo, &k, &t) == TD_OK);
			uint64_t w = k == 1 ? eo[0].w : 0;
			int cnt = k == 1 ? eo[0].n : 0;
			td_census_free(e); free(eo);
			if (t.eligible == 0) continue;
			want.eligible++;
			bool has_n = t.skipped_n == 1;
			const int64_t mlen = moffs[(size_t)i + 1] - moffs[(size_t)i];
			for (int64_t p = 0; p < mlen && p < M; p++) {
				const uint8_t b = mcodes[(size_t)(moffs[(size_t)i] + p)];
				if (b > 3) has_n = true;
				w = (w << 2) | (uint64_t)(b & 3u);
				cnt++;
			}
			if (t.skipped_n == 1) { cls[(size_t)i] = HAS_N; want.skipped_n++; continue; }
			if (cnt == 0) { cls[(size_t)i] = EMPTY; want.skipped_empty++; continue; }
			if (has_n) { cls[(size_t)i] = HAS_N; want.skipped_n++; continue; }
			cls[(size_t)i] = COUNTED; want.counted++;
			key[(size_t)i] = td_mol_key(res[(size_t)i].barcode, res[(size_t)i].fingerprint, w, cnt);
			count[key[(size_t)i]]++;
			if (!first.count(key[(size_t)i])) { first[key[(size_t)i]] = i; origin[key[(size_t)i]] = td_mol_origin{ w, res[(size_t)i].fingerprint, cnt }; }
		}
		want.molecules = (int64_t)count.size();
		// the count and its origins
		td_census_entry* e = nullptr;
		td_mol_origin* eo = nullptr;
		int64_t k = 0;
		td_mol_totals t{};
		CHECK(td_mol_host_origins_mated(&m, P, codes.data(), offs.data(), n, res.data(), labels.data(), &mate, &e, &eo, &k, &t) == TD_OK);
		CHECK(memcmp(&t, &want, sizeof t) == 0 && k == (int64_t)count.size());
		CHECK(want.counted > 500 && want.skipped_empty > 10 && want.skipped_n > 50 && want.molecules < want.counted);
		for (int64_t j = 0; j < k; j++) {
			CHECK(count.count(e[j].key) && count[e[j].key] == e[j].count);
			const td_mol_origin& o = origin[e[j].key];
			CHECK(o.w == eo[j].w && o.fingerprint == eo[j].fingerprint && o.n == eo[j].n && o.n >= 1 && o.n <= P + M);
			if (j > 0) CHECK(e[j - 1].count > e[j].count || (e[j - 1].count == e[j].count && e[j - 1].key < e[j].key));
		}
		td_census_entry* e2 = nullptr;
		int64_t k2 = 0;
		td_mol_totals t2{};
		CHECK(td_mol_host_mated(&m, P, codes.data(), offs.data(), n, res.data(), labels.data(), &mate, &e2, &k2, &t2) == TD_OK);
		CHECK(k2 == k && memcmp(&t2, &t, sizeof t) == 0 && (k == 0 || memcmp(e, e2, sizeof(td_census_entry) * (size_t)k) == 0));
		td_census_free(e); td_census_free(e2); free(eo);
		// dedup: the first read of a key stays
		uint8_t* dup = (uint8_t*)malloc((size_t)n);       // (exactly n bytes)
		CHECK(dup);
		td_mol_dedup_totals d{}, wd{};
		CHECK(td_mol_dedup_host_mated(&m, P, codes.data(), offs.data(), n, res.data(), labels.data(), &mate, dup, &d) == TD_OK);
		for (int64_t i = 0; i < n; i++) {
			const bool is_dup = cls[(size_t)i] == COUNTED && first[key[(size_t)i]] != i;
			CHECK(dup[i] == (is_dup ? 1 : 0));
			if (cls[(size_t)i] == NOT) continue;
			if (cls[(size_t)i] != COUNTED) wd.unjudged++;
			if (is_dup) wd.duplicates++; else wd.kept++;
		}
		CHECK(memcmp(&d, &wd, sizeof d) == 0 && d.duplicates > 0);
		CHECK(t.eligible == d.kept + d.duplicates && d.kept == t.molecules + t.skipped_empty + t.skipped_n);
		// survey, freeze, replay: the identities, and every kept judged read is the first of its key
		td_mol_dedup_totals c{};
		td_mol_collapse_totals ct{};
		CHECK(td_mol_dedup_collapsed_host_mated(&m, P, codes.data(), offs.data(), n, res.data(), labels.data(), &mate, dup, &c, &ct) == TD_OK);
		CHECK(ct.molecules_before == t.molecules && ct.molecules_after + ct.absorbed == ct.molecules_before);
		CHECK(t.eligible == c.kept + c.duplicates && c.kept == ct.molecules_after + t.skipped_empty + t.skipped_n && c.unjudged == d.unjudged);
		int64_t kept_judged = 0;
		for (int64_t i = 0; i < n; i++) {
			if (cls[(size_t)i] != COUNTED) { CHECK(dup[i] == 0); continue; }
			if (dup[i] == 0) { kept_judged++; CHECK(first[key[(size_t)i]] == i); }
		}
		CHECK(kept_judged == ct.molecules_after);
		free(dup);
	}
	// mate == NULL is the unmated function
	{
		td_census_entry* a = nullptr, * b = nullptr;
		int64_t ka = 0, kb = 0;
		td_mol_totals ta{}, tb{};
		CHECK(td_mol_host(&m, 16, codes.data(), offs.data(), n, res.data(), labels.data(), &a, &ka, &ta) == TD_OK);
		CHECK(td_mol_host_mated(&m, 16, codes.data(), offs.data(), n, res.data(), labels.data(), nullptr, &b, &kb, &tb) == TD_OK);
		CHECK(ka == kb && ka > 0 && memcmp(&ta, &tb, sizeof ta) == 0 && memcmp(a, b, sizeof(td_census_entry) * (size_t)ka) == 0);
		td_census_free(a); td_census_free(b);
		std::vector<uint8_t> da((size_t)n), db((size_t)n);
		td_mol_dedup_totals xa{}, xb{};
		CHECK(td_mol_dedup_host(&m, 16, codes.data(), offs.data(), n, res.data(), labels.data(), da.data(), &xa) == TD_OK);
		CHECK(td_mol_dedup_host_mated(&m, 16, codes.data(), offs.data(), n, res.data(), labels.data(), nullptr, db.data(), &xb) == TD_OK);
		CHECK(da == db && memcmp(&xa, &xb, sizeof xa) == 0);
		CHECK(td_mol_dedup_collapsed_host(&m, 16, codes.data(), offs.data(), n, res.data(), labels.data(), da.data(), &xa, nullptr) == TD_OK);
		CHECK(td_mol_dedup_collapsed_host_mated(&m, 16, codes.data(), offs.data(), n, res.data(), labels.data(), nullptr, db.data(), &xb, nullptr) == TD_OK);
		CHECK(da == db && memcmp(&xa, &xb, sizeof xa) == 0);
	}
	// the refusals
	{
		td_census_entry* e = nullptr;
		int64_t k = 0;
		uint8_t one = 0;
		const td_mol_mate none{ mblock, moffs.data(), 0 }, wide{ mblock, moffs.data(), 21 }, fits{ mblock, moffs.data(), 20 };
		CHECK(td_mol_host_mated(&m, 12, codes.data(), offs.data(), n, res.data(), labels.data(), &none, &e, &k, nullptr) == TD_FAIL && !e);
		CHECK(g_err.find("mate bases = 0") != std::string::npos);
		CHECK(td_mol_host_mated(&m, 12, codes.data(), offs.data(), n, res.data(), labels.data(), &wide, &e, &k, nullptr) == TD_FAIL && !e);
		CHECK(g_err.find("12 + 21") != std::string::npos);
		CHECK(td_mol_dedup_host_mated(&m, 12, codes.data(), offs.data(), n, res.data(), labels.data(), &wide, &one, nullptr) == TD_FAIL);
		CHECK(td_mol_dedup_collapsed_host_mated(&m, 12, codes.data(), offs.data(), n, res.data(), labels.data(), &none, &one, nullptr, nullptr) == TD_FAIL);
		CHECK(td_mol_host_mated(&m, 12, codes.data(), offs.data(), n, res.data(), labels.data(), &fits, &e, &k, nullptr) == TD_OK && e);
		td_census_free(e);
		CHECK(td_mol_dedup_host_mated(&m, 12, nullptr, nullptr, 0, nullptr, nullptr, &fits, nullptr, nullptr) == TD_OK);
	}
	free(mblock);
	printf("mate_host_check: ok\n");
	return 0;
}
