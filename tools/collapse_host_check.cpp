// collapse_host_check.cpp -- td_mol_host_origins and td_mol_collapse_host (include/tagdust_molecules.h) as a stand-alone program, for
// running them under the host sanitizers: no GPU, no HIP runtime, no Python.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tagdust_amd/csrc/td_census_host.cpp tagdust_amd/csrc/td_molecules_host.cpp tools/collapse_host_check.cpp -o /tmp/collapse_host_check
//   /tmp/collapse_host_check                                     # (leak detection stays on)
//
// Generated reads (lengths 0..200, N bases, every outcome, barcodes -1..299, 4-nt fingerprints from a small alphabet so that
// neighbours meet, some -1), generated labels over an F-B-R-S-R model; for prefixes of 1, 2 and 32 bases td_mol_host_origins is held
// against td_mol_host and against td_mol_key of its own origins, td_mol_collapse_host against a restatement with std::map, both
// identities included; the two halves' results concatenated -- keys repeat -- must collapse to the whole's.  Inputs are handed over
// in blocks of exactly their size.  Exit status 0 when all of it agrees.
#define HOST_CHECK_NAME "collapse_host_check"
#include "host_check.h"
#include "../include/tagdust_molecules.h"

struct Batch {
	std::vector<int64_t> offs{ 0 };
	std::vector<uint8_t> codes;
	std::vector<int8_t> labels;
	std::vector<td_read_result> res;
};

struct Result {
	td_census_entry* e = nullptr;
	td_mol_origin* o = nullptr;
	int64_t n = 0;
	void clear() { td_census_free(e); free(o); e = nullptr; o = nullptr; n = 0; }
};

// the definition, restated: parents by the order of td_census_get among the neighbours the map holds, counts summed under roots
static bool restated(const Result& in, std::map<uint64_t, int64_t>& collapsed, td_mol_collapse_totals& t)
{
	std::map<uint64_t, int64_t> count;
	std::map<uint64_t, td_mol_origin> origin;
	for (int64_t i = 0; i < in.n; i++) {
		count[in.e[i].key] += in.e[i].count;
		origin.emplace(in.e[i].key, in.o[i]);
	}
	auto before = [&](uint64_t a, uint64_t b) { return count[a] != count[b] ? count[a] > count[b] : a < b; };
	std::map<uint64_t, uint64_t> parent;
	for (auto& kv : count) {
		const uint64_t u = kv.first;
		const td_mol_origin o = origin[u];
		const int L = o.fingerprint & 0xFF, m = o.fingerprint == -1 ? 0 : (L < 12 ? L : 12);
		uint64_t best = u;
		for (int i = 0; i < m; i++)
			for (uint32_t d = 1; d <= 3; d++) {
				const uint64_t v = td_mol_key(td_mol_key_bin(u), (int32_t)((uint32_t)o.fingerprint ^ (d << (8 + 2 * i))), o.w, o.n);
				if (!count.count(v) || count[v] < 2 * count[u] - 1 || !before(v, u)) continue;
				if (best == u || before(v, best)) best = v;
			}
		parent[u] = best;
	}
	t = td_mol_collapse_totals{};
	for (auto& kv : count) {
		uint64_t r = kv.first;
		int64_t steps = 0;
		while (parent[r] != r) { r = parent[r]; steps++; if (steps > (int64_t)count.size()) return false; }
		collapsed[r] += kv.second;
		if (steps > t.longest_chain) t.longest_chain = steps;
	}
	t.molecules_before = (int64_t)count.size(); t.molecules_after = (int64_t)collapsed.size(); t.absorbed = t.molecules_before - t.molecules_after;
	return true;
}

int main()
{
	// F(1 HMM) B(3) R(1) S(1) R(1): label = hmm << 16 | segment
	const int32_t n_hmm[5] = { 1, 3, 1, 1, 1 }, n_col[5] = { 4, 6, 1, 3, 1 }, finger_len[5] = { 4, 0, 0, 0, 0 };
	const int8_t seg_type[5] = { 'F', 'B', 'R', 'S', 'R' };
	const int32_t label[7] = { 0, 1, (1 << 16) | 1, (2 << 16) | 1, 2, 3, 4 };
	td_model_desc m{};
	m.S = 5; m.H = 7; m.n_hmm = n_hmm; m.n_col = n_col; m.seg_type = seg_type; m.finger_len = finger_len; m.label = label;

	uint32_t s = 1609u;
	const int64_t n = 4000;
	Batch all, half[2];
	for (int64_t i = 0; i < n; i++) {
		Batch* into[2] = { &all, &half[i < n / 2 ? 0 : 1] };
		const int len = (int)(rnd(s) % 201u);
		std::vector<uint8_t> seq;
		std::vector<int8_t> lab{ 0 };
		int h = 0;
		for (int p = 0; p < len; p++) {
			seq.push_back((uint8_t)(rnd(s) % 60u == 0 ? 4 : rnd(s) % 2u));   // (two bases: equal prefixes are met)
			if (rnd(s) % 4u == 0 && h < 6) h++;
			lab.push_back((int8_t)h);
		}
		td_read_result r{};
		r.read_type = (int32_t)(rnd(s) % 5u == 0 ? rnd(s) % 7u : 0u) | (rnd(s) % 5u == 0 ? 0x300 : 0);
		r.barcode = rnd(s) % 8u == 0 ? (int32_t)(rnd(s) % 301u) - 1 : (int32_t)(rnd(s) % 2u);
		// a 4-nt fingerprint of two letters per base, drawn unevenly so that counts differ; one in ten has none
		uint32_t bases = 0;
		for (int q = 0; q < 4; q++) bases = (bases << 2) | (rnd(s) % 4u == 0 ? 1u : 0u);
		r.fingerprint = rnd(s) % 10u == 0 ? -1 : (int32_t)((bases << 8) | 4u);
		for (Batch* b : into) {
			b->codes.insert(b->codes.end(), seq.begin(), seq.end());
			b->labels.insert(b->labels.end(), lab.begin(), lab.end());
			b->offs.push_back(b->offs.back() + (int64_t)seq.size());
			b->res.push_back(r);
		}
	}

	for (int32_t P : { 1, 2, 32 }) {
		auto origins_of = [&](const Batch& b, Result& out, td_mol_totals& t) {
			return td_mol_host_origins(&m, P, b.codes.data(), b.offs.data(), (int64_t)b.res.size(), b.res.data(), b.labels.data(), &out.e, &out.o, &out.n, &t);
		};
		Result whole, part[2];
		td_mol_totals t{}, tp[2] = {}, plain_t{};
		CHECK(origins_of(all, whole, t) == TD_OK);
		CHECK(origins_of(half[0], part[0], tp[0]) == TD_OK && origins_of(half[1], part[1], tp[1]) == TD_OK);
		td_census_entry* plain = nullptr;
		int64_t n_plain = 0;
		CHECK(td_mol_host(&m, P, all.codes.data(), all.offs.data(), n, all.res.data(), all.labels.data(), &plain, &n_plain, &plain_t) == TD_OK);
		CHECK(n_plain == whole.n && memcmp(&plain_t, &t, sizeof t) == 0 && (whole.n == 0 || memcmp(plain, whole.e, sizeof(td_census_entry) * (size_t)whole.n) == 0));
		td_census_free(plain);
		for (int64_t i = 0; i < whole.n; i++)
			CHECK(whole.o[i].n >= 1 && whole.o[i].n <= P && td_mol_key(td_mol_key_bin(whole.e[i].key), whole.o[i].fingerprint, whole.o[i].w, whole.o[i].n) == whole.e[i].key);

		Result col;
		td_mol_collapse_totals ct{}, want_t{};
		CHECK(td_mol_collapse_host(whole.e, whole.o, whole.n, &col.e, &col.o, &col.n, &ct) == TD_OK);
		std::map<uint64_t, int64_t> want;
		CHECK(restated(whole, want, want_t));
		CHECK(memcmp(&ct, &want_t, sizeof ct) == 0 && col.n == (int64_t)want.size());
		int64_t sum = 0;
		for (int64_t i = 0; i < col.n; i++) {
			CHECK(want.count(col.e[i].key) && want[col.e[i].key] == col.e[i].count);
			CHECK(td_mol_key(td_mol_key_bin(col.e[i].key), col.o[i].fingerprint, col.o[i].w, col.o[i].n) == col.e[i].key);
			if (i > 0) CHECK(col.e[i - 1].count > col.e[i].count || (col.e[i - 1].count == col.e[i].count && col.e[i - 1].key < col.e[i].key));
			sum += col.e[i].count;
		}
		CHECK(sum == t.counted && ct.molecules_after + ct.absorbed == ct.molecules_before && ct.molecules_before == t.molecules);
		if (P <= 2) CHECK(ct.absorbed > 0 && ct.longest_chain >= 1);

		// the halves concatenated, keys repeated, in blocks of exactly their size
		const int64_t nc = part[0].n + part[1].n;
		td_census_entry* ce = (td_census_entry*)malloc(sizeof(td_census_entry) * (size_t)(nc ? nc : 1));
		td_mol_origin* co = (td_mol_origin*)malloc(sizeof(td_mol_origin) * (size_t)(nc ? nc : 1));
		CHECK(ce && co);
		for (int h = 0, at = 0; h < 2; h++)
			for (int64_t i = 0; i < part[h].n; i++, at++) { ce[at] = part[h].e[i]; co[at] = part[h].o[i]; }
		Result both;
		td_mol_collapse_totals bt{};
		CHECK(td_mol_collapse_host(ce, co, nc, &both.e, &both.o, &both.n, &bt) == TD_OK);
		CHECK(nc > whole.n && both.n == col.n && memcmp(&bt, &ct, sizeof ct) == 0);
		CHECK(both.n == 0 || (memcmp(both.e, col.e, sizeof(td_census_entry) * (size_t)col.n) == 0 && memcmp(both.o, col.o, sizeof(td_mol_origin) * (size_t)col.n) == 0));
		free(ce); free(co);
		whole.clear(); part[0].clear(); part[1].clear(); col.clear(); both.clear();
	}
	Result r;
	td_mol_collapse_totals ct{};
	CHECK(td_mol_collapse_host(nullptr, nullptr, 0, &r.e, &r.o, &r.n, &ct) == TD_OK && r.n == 0 && ct.molecules_before == 0);
	r.clear();
	CHECK(td_mol_collapse_host(nullptr, nullptr, 1, &r.e, &r.o, &r.n, &ct) == TD_FAIL);
	CHECK(td_mol_collapse_host(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == TD_FAIL);
	td_mol_totals t{};
	CHECK(td_mol_host_origins(&m, 33, all.codes.data(), all.offs.data(), n, all.res.data(), all.labels.data(), &r.e, &r.o, &r.n, &t) == TD_FAIL);
	CHECK(td_mol_host_origins(&m, 20, all.codes.data(), all.offs.data(), n, all.res.data(), all.labels.data(), &r.e, nullptr, &r.n, &t) == TD_FAIL);
	printf("collapse_host_check: ok\n");
	return 0;
}
