// dedup_collapsed_host_check.cpp -- td_mol_dedup_collapsed_host (include/tagdust_molecules.h) as a stand-alone program, for running
// it under the host sanitizers: no GPU is used, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tagdust_amd/csrc/td_census_host.cpp tagdust_amd/csrc/td_molecules_host.cpp tools/dedup_collapsed_host_check.cpp -o /tmp/dedup_collapsed_host_check
//   /tmp/dedup_collapsed_host_check                              # (leak detection stays on)
//
// Generated reads (lengths 0..200, N bases, every outcome, a few barcodes, UMIs of 4 bases from a skewed handful so that
// neighbours with very different counts meet, some records without a fingerprint), generated labels over an F-B-R-S-R model; for
// prefixes of 1, 7, 16 and 32 bases the marks and totals are held against a restatement with std::map over td_mol_host_origins'
// own key and origin of each single read -- counts, parents by the directional rule through td_mol_key, roots, the first ordinal
// of the root's own key --, both identities against td_mol_host's totals, the kept judged reads against the roots of
// td_mol_collapse_host, and td_mol_dedup_host must mark fewer.  is_duplicate has exactly n_reads bytes.  Exit status 0 when all of
// it agrees.
#define HOST_CHECK_NAME "dedup_collapsed_host_check"
#include "host_check.h"
#include "../include/tagdust_molecules.h"

#include <set>

int main()
{
	// F(1 HMM) B(3) R(1) S(1) R(1): label = hmm << 16 | segment
	const int32_t n_hmm[5] = { 1, 3, 1, 1, 1 }, n_col[5] = { 4, 6, 1, 3, 1 }, finger_len[5] = { 4, 0, 0, 0, 0 };
	const int8_t seg_type[5] = { 'F', 'B', 'R', 'S', 'R' };
	const int32_t label[7] = { 0, 1, (1 << 16) | 1, (2 << 16) | 1, 2, 3, 4 };
	td_model_desc m{};
	m.S = 5; m.H = 7; m.n_hmm = n_hmm; m.n_col = n_col; m.seg_type = seg_type; m.finger_len = finger_len; m.label = label;

	uint32_t s = 4711u;
	const int64_t n = 3000;
	std::vector<int64_t> offs{ 0 };
	std::vector<uint8_t> codes;
	std::vector<int8_t> labels;
	std::vector<td_read_result> res;
	for (int64_t i = 0; i < n; i++) {
		const int len = (int)(rnd(s) % 201u);
		int h = 0;
		labels.push_back(0);
		for (int p = 0; p < len; p++) {
			codes.push_back((uint8_t)(rnd(s) % 90u == 0 ? 4 : rnd(s) % 2u));   // (two bases: equal prefixes are met)
			if (rnd(s) % 4u == 0 && h < 6) h++;
			labels.push_back((int8_t)h);
		}
		offs.push_back((int64_t)codes.size());
		td_read_result r{};
		r.read_type = (int32_t)(rnd(s) % 4u == 0 ? rnd(s) % 7u : 0u) | (rnd(s) % 5u == 0 ? 0x300 : 0);
		r.barcode = (int32_t)(rnd(s) % 3u) - (rnd(s) % 7u == 0 ? 1 : 0);
		const uint32_t a = rnd(s) % 16u, b = rnd(s) % 16u, c = rnd(s) % 16u;
		const uint32_t umi = a < b ? (a < c ? a : c) : (b < c ? b : c);                // skewed: the small values are the frequent ones
		r.fingerprint = rnd(s) % 9u == 0 ? -1 : (int32_t)((umi << 8) | 4u);
		res.push_back(r);
	}
	if (codes.empty()) codes.push_back(0);

	for (int32_t P : { 1, 7, 16, 32 }) {
		// key and origin of every read on its own, from td_mol_host_origins over that read alone (key 0: not counted)
		std::vector<uint64_t> key((size_t)n, 0);
		std::vector<bool> elig((size_t)n, false);
		std::map<uint64_t, td_mol_origin> origin;
		std::map<uint64_t, int64_t> count, first;
		for (int64_t i = 0; i < n; i++) {
			const int64_t o[2] = { 0, offs[(size_t)i + 1] - offs[(size_t)i] };
			td_census_entry* e = nullptr;
			td_mol_origin* eo = nullptr;
			int64_t k = 0;
			td_mol_totals t{};
			CHECK(td_mol_host_origins(&m, P, codes.data() + offs[(size_t)i], o, 1, &res[(size_t)i], labels.data() + offs[(size_t)i] + i, &e, &eo, &k, &t) == TD_OK);
			elig[(size_t)i] = t.eligible == 1;
			if (k == 1) {
				key[(size_t)i] = e[0].key;
				origin[e[0].key] = eo[0];
				count[e[0].key]++;
				if (!first.count(e[0].key)) first[e[0].key] = i;
			}
			td_census_free(e);
			free(eo);
		}
		// the forest, restated: the parent is the qualifying neighbour that comes first by (count descending, key ascending)
		auto before = [&](uint64_t x, uint64_t y) { return count[x] != count[y] ? count[x] > count[y] : x < y; };
		std::map<uint64_t, uint64_t> parent, root;
		for (auto& kv : count) {
			const uint64_t u = kv.first;
			const td_mol_origin& o = origin[u];
			const int bases = o.fingerprint == -1 ? 0 : ((o.fingerprint & 0xFF) < 12 ? (o.fingerprint & 0xFF) : 12);
			uint64_t best = u;
			for (int i = 0; i < bases; i++)
				for (uint32_t d = 1; d <= 3; d++) {
					const uint64_t v = td_mol_key((int32_t)(u >> 56), (int32_t)((uint32_t)o.fingerprint ^ (d << (8 + 2 * i))), o.w, o.n);
					if (!count.count(v) || count[v] < 2 * kv.second - 1 || !before(v, u)) continue;
					if (best == u || before(v, best)) best = v;
				}
			parent[u] = best;
		}
		int64_t n_roots = 0, absorbed = 0;
		for (auto& kv : count) {
			uint64_t r = kv.first;
			while (parent[r] != r) r = parent[r];
			root[kv.first] = r;
			if (r == kv.first) n_roots++; else absorbed++;
		}
		td_mol_totals mt{};
		td_census_entry* all = nullptr;
		td_mol_origin* all_o = nullptr;
		int64_t n_all = 0;
		CHECK(td_mol_host_origins(&m, P, codes.data(), offs.data(), n, res.data(), labels.data(), &all, &all_o, &n_all, &mt) == TD_OK);
		td_census_entry* roots = nullptr;
		td_mol_origin* roots_o = nullptr;
		int64_t n_r = 0;
		td_mol_collapse_totals ct{};
		CHECK(td_mol_collapse_host(all, all_o, n_all, &roots, &roots_o, &n_r, &ct) == TD_OK);
		std::multiset<uint64_t> root_keys, kept_keys;
		for (int64_t q = 0; q < n_r; q++) root_keys.insert(roots[q].key);
		td_census_free(all); free(all_o); td_census_free(roots); free(roots_o);

		uint8_t* dup = (uint8_t*)malloc((size_t)n);       // (exactly n bytes: the sanitizer sees one too many)
		uint8_t* exact = (uint8_t*)malloc((size_t)n);
		CHECK(dup && exact);
		td_mol_dedup_totals t{}, et{};
		td_mol_collapse_totals got_ct{};
		CHECK(td_mol_dedup_collapsed_host(&m, P, codes.data(), offs.data(), n, res.data(), labels.data(), dup, &t, &got_ct) == TD_OK);
		CHECK(td_mol_dedup_host(&m, P, codes.data(), offs.data(), n, res.data(), labels.data(), exact, &et) == TD_OK);
		td_mol_dedup_totals w{};
		for (int64_t i = 0; i < n; i++) {
			if (!elig[(size_t)i]) { CHECK(dup[i] == 0); continue; }
			if (key[(size_t)i] == 0) { w.unjudged++; w.kept++; CHECK(dup[i] == 0); continue; }
			const bool d = first[root[key[(size_t)i]]] != i;
			CHECK(dup[i] == (d ? 1 : 0));
			if (!d) CHECK(exact[i] == 0);                  // the one read a tree keeps is the first of its own key
			if (d) w.duplicates++; else { w.kept++; kept_keys.insert(key[(size_t)i]); }
		}
		CHECK(memcmp(&w, &t, sizeof w) == 0);
		CHECK(memcmp(&ct, &got_ct, sizeof ct) == 0 && ct.molecules_after == n_roots && ct.absorbed == absorbed && ct.molecules_before == mt.molecules);
		CHECK(kept_keys == root_keys);
		CHECK(mt.eligible == t.kept + t.duplicates && t.kept == ct.molecules_after + mt.skipped_empty + mt.skipped_n + mt.overflow);
		CHECK(t.unjudged == mt.skipped_empty + mt.skipped_n && t.unjudged > 0 && t.duplicates > 0);
		CHECK(et.duplicates + ct.absorbed == t.duplicates);
		if (P <= 16) CHECK(ct.absorbed > 0 && et.duplicates < t.duplicates);
		// NULL totals are allowed
		CHECK(td_mol_dedup_collapsed_host(&m, P, codes.data(), offs.data(), n, res.data(), labels.data(), exact, nullptr, nullptr) == TD_OK);
		CHECK(memcmp(dup, exact, (size_t)n) == 0);
		free(dup); free(exact);
	}
	uint8_t one = 0;
	CHECK(td_mol_dedup_collapsed_host(&m, 0, codes.data(), offs.data(), n, res.data(), labels.data(), &one, nullptr, nullptr) == TD_FAIL);
	CHECK(td_mol_dedup_collapsed_host(&m, 33, codes.data(), offs.data(), n, res.data(), labels.data(), &one, nullptr, nullptr) == TD_FAIL);
	CHECK(td_mol_dedup_collapsed_host(&m, 20, codes.data(), offs.data(), n, res.data(), labels.data(), nullptr, nullptr, nullptr) == TD_FAIL);
	CHECK(td_mol_dedup_collapsed_host(nullptr, 20, codes.data(), offs.data(), n, res.data(), labels.data(), &one, nullptr, nullptr) == TD_FAIL);
	td_mol_dedup_totals zt{ 1, 1, 1 };
	CHECK(td_mol_dedup_collapsed_host(&m, 20, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &zt, nullptr) == TD_OK && zt.kept == 0 && zt.duplicates == 0);
	printf("dedup_collapsed_host_check: ok\n");
	return 0;
}
