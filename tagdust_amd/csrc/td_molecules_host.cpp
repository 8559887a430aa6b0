// td_molecules_host.cpp -- the host side of the molecule count (include/tagdust_molecules.h): the definitions the device
// (td_molecules.hip) is held against, over host arrays -- td_mol_host and td_mol_host_origins (one walk over the reads, the second
// keeps what every key was made of), td_mol_dedup_host, td_mol_collapse_host, td_mol_dedup_collapsed_host, each over reads also as
// *_mated with the mate batch joined into the key (the unmated name is the call with no mate) --, td_mol_summarise,
// which a run over several devices calls on merged entries, and the key itself.  Plain C++: no device is used and no HIP header read.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "td_count_key.h"

void mol_emit_ordered(const td_census_entry* e, const td_mol_origin* o, int64_t n, int64_t take, td_census_entry* out_e, td_mol_origin* out_o)
{
	std::vector<int64_t> order((size_t)n);
	for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
	std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return kt_entry_before(e[x], e[y]); });
	for (int64_t q = 0; q < take && q < n; q++) { out_e[q] = e[order[(size_t)q]]; out_o[q] = o[order[(size_t)q]]; }
}

namespace {

// what read i is to the count on the host: not eligible, or one of the three classes; *key and *origin of a counted read
enum { MOL_NOT_ELIGIBLE = 0, MOL_EMPTY, MOL_HAS_N, MOL_COUNTED };
// (mate: NULL, or the mate batch whose first min(len(mate i), bases) bases follow the read's own prefix in the word)
int host_read_class(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t i,
                    const td_read_result* res, const int8_t* labels, const td_mol_mate* mate, uint64_t* key, td_mol_origin* origin)
{
	if (((uint32_t)res[i].read_type & 0xFFu) != (uint32_t)TD_EXTRACT_SUCCESS) return MOL_NOT_ELIGIBLE;
	const int64_t len = offs[i + 1] - offs[i];
	const int8_t* lab = labels + offs[i] + i;
	const uint8_t* seq = codes + offs[i];
	uint64_t w = 0;
	int cnt = 0;
	bool has_n = false;
	for (int64_t p = 0; p < len && cnt < prefix_bases; p++) {
		const int l = lab[p + 1];
		if (l < 0 || l >= m->H) continue;
		const int seg = m->label[l] & 0xFFFF;
		if (seg >= m->S || m->seg_type[seg] != 'R') continue;
		cnt++;
		if (seq[p] > 3) has_n = true;
		w = (w << 2) | (uint64_t)(seq[p] & 3u);
	}
	if (mate) {                                       // the mate's prefix behind the read's own: never past the mate's own end
		const int64_t mlen = mate->offs[i + 1] - mate->offs[i];
		const uint8_t* ms = mate->codes + mate->offs[i];
		for (int64_t p = 0; p < mlen && p < mate->bases; p++) {
			cnt++;
			if (ms[p] > 3) has_n = true;
			w = (w << 2) | (uint64_t)(ms[p] & 3u);
		}
	}
	if (cnt == 0) return MOL_EMPTY;
	if (has_n) return MOL_HAS_N;
	*key = mol_key(res[i].barcode, res[i].fingerprint, w, cnt);
	*origin = td_mol_origin{ w, res[i].fingerprint, cnt };
	return MOL_COUNTED;
}

// what opens every *_host function over reads (`who`, for its messages; args_ok: its own pointers and sizes)
int host_checks(const char* who, const td_model_desc* m, int32_t prefix_bases, const td_mol_mate* mate, int64_t n_reads, bool args_ok)
{
	if (!m || m->S < 1 || m->H < 1 || !m->seg_type || !m->label) return fail(nullptr, "%s: no model", who);
	if (!mol_prefix_ok(prefix_bases)) return fail(nullptr, "%s: prefix_bases = %d (1..%d supported)", who, prefix_bases, TD_MOL_MAX_PREFIX);
	if (!args_ok) return fail(nullptr, "%s: bad arguments", who);
	if (mate) {
		if (mate->bases < 1) return fail(nullptr, "%s: mate bases = %d (at least 1)", who, mate->bases);
		if (prefix_bases + mate->bases > TD_MOL_MAX_PREFIX)
			return fail(nullptr, "%s: prefix_bases + mate bases = %d + %d (at most %d together: they share one 64-bit word)", who, prefix_bases,
			            mate->bases, TD_MOL_MAX_PREFIX);
		if (n_reads > 0 && (!mate->offs || !mate->codes)) return fail(nullptr, "%s: bad arguments (the mate batch)", who);
		for (int64_t i = 0; i < n_reads; i++)
			if (mate->offs[i + 1] < mate->offs[i]) return fail(nullptr, "%s: mate %lld has a negative length", who, (long long)i);
	}
	return TD_OK;
}

// entries with repeated keys (any order) and their origins -> one entry per key, in the order of td_census_get
void host_add_repeated(const td_census_entry* entries, const td_mol_origin* origins, int64_t n, std::vector<td_census_entry>& v,
                       std::vector<td_mol_origin>& vo)
{
	std::vector<int64_t> order((size_t)n);
	for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
	std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return entries[x].key < entries[y].key; });
	std::vector<td_census_entry> e;
	std::vector<td_mol_origin> eo;
	for (int64_t i : order) {
		if (entries[i].count <= 0) continue;
		if (!e.empty() && e.back().key == entries[i].key) e.back().count += entries[i].count;
		else { e.push_back(entries[i]); eo.push_back(origins[i]); }
	}
	v.resize(e.size()); vo.resize(e.size());
	mol_emit_ordered(e.data(), eo.data(), (int64_t)e.size(), (int64_t)e.size(), v.data(), vo.data());
}

// The collapse's forest over v, one entry per key in the order of td_census_get, with its origins: parent and root of every entry
// (indices into v; a root is its own), the count of every root's tree (0 elsewhere) and the totals.  td_mol_collapse_host and
// td_mol_dedup_collapsed_host both stand on this one copy.
struct HostForest {
	std::vector<size_t> parent, root;
	std::vector<int64_t> collapsed;
	td_mol_collapse_totals totals{};
};
void host_forest(const std::vector<td_census_entry>& v, const std::vector<td_mol_origin>& vo, HostForest& f)
{
	const size_t N = v.size();
	std::unordered_map<uint64_t, size_t> at;
	for (size_t u = 0; u < N; u++) at[v[u].key] = u;
	// v is in the order of td_census_get: "v comes before u" is "its index is smaller", and the first qualifying neighbour the smallest
	f.parent.assign(N, 0);
	for (size_t u = 0; u < N; u++) {
		f.parent[u] = u;
		const int m = vo[u].n > 0 ? mol_umi_bases(vo[u].fingerprint) : 0;
		for (int i = 0; i < m; i++)
			for (uint32_t d = 1; d <= 3; d++) {
				const auto g = at.find(mol_neighbour_key(v[u].key, vo[u], i, d));
				if (g == at.end()) continue;
				const size_t q = g->second;
				if (v[q].count >= 2 * v[u].count - 1 && q < f.parent[u]) f.parent[u] = q;
			}
	}
	// a parent has a smaller index: roots and depths in one pass from the front
	f.root.assign(N, 0);
	f.collapsed.assign(N, 0);
	std::vector<int64_t> depth(N);
	td_mol_collapse_totals t{};
	for (size_t u = 0; u < N; u++) {
		f.root[u] = f.parent[u] == u ? u : f.root[f.parent[u]];
		depth[u] = f.parent[u] == u ? 0 : depth[f.parent[u]] + 1;
		f.collapsed[f.root[u]] += v[u].count;
		t.longest_chain = std::max(t.longest_chain, depth[u]);
		t.molecules_after += f.root[u] == u;
	}
	t.molecules_before = (int64_t)N; t.absorbed = t.molecules_before - t.molecules_after;
	f.totals = t;
}

td_mol_origin* copy_origins(const std::vector<td_mol_origin>& v)
{
	td_mol_origin* p = (td_mol_origin*)malloc(sizeof(td_mol_origin) * (v.size() ? v.size() : 1));
	if (p && !v.empty()) memcpy(p, v.data(), sizeof(td_mol_origin) * v.size());
	return p;
}

// td_mol_host_mated (with_origins false: they are dropped) and td_mol_host_origins_mated, `who` in the messages: the walk over the reads, the
// entries in the order of td_census_get
int host_count(const char* who, bool with_origins, const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs,
               int64_t n_reads, const td_read_result* res, const int8_t* labels, const td_mol_mate* mate, td_census_entry** entries,
               td_mol_origin** origins, int64_t* n, td_mol_totals* totals)
{
	if (entries) *entries = nullptr;
	if (origins) *origins = nullptr;
	if (n) *n = 0;
	const bool args_ok = entries && (origins || !with_origins) && n && n_reads >= 0 && (n_reads == 0 || (offs && res && labels && codes));
	if (host_checks(who, m, prefix_bases, mate, n_reads, args_ok) != TD_OK) return TD_FAIL;
	td_mol_totals t{};
	std::vector<td_census_entry> each;                // one entry of count 1 per counted read
	std::vector<td_mol_origin> each_o;
	for (int64_t i = 0; i < n_reads; i++) {
		uint64_t key = 0;
		td_mol_origin o{};
		const int cls = host_read_class(m, prefix_bases, codes, offs, i, res, labels, mate, &key, &o);
		if (cls == MOL_NOT_ELIGIBLE) continue;
		t.eligible++;
		if (cls == MOL_EMPTY) t.skipped_empty++;
		else if (cls == MOL_HAS_N) t.skipped_n++;
		else { each.push_back(td_census_entry{ key, 1 }); each_o.push_back(o); t.counted++; }
	}
	std::vector<td_census_entry> v;
	std::vector<td_mol_origin> vo;
	host_add_repeated(each.data(), each_o.data(), (int64_t)each.size(), v, vo);
	t.molecules = (int64_t)v.size();
	td_census_entry* pe = kt_copy_entries(v);
	td_mol_origin* po = with_origins ? copy_origins(vo) : nullptr;
	if (!pe || (with_origins && !po)) { free(pe); free(po); return fail(nullptr, "%s: out of memory", who); }
	*entries = pe; *n = (int64_t)v.size();
	if (with_origins) *origins = po;
	if (totals) *totals = t;
	return TD_OK;
}

}   // namespace

extern "C" int td_mol_host_mated(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                                 const td_read_result* res, const int8_t* labels, const td_mol_mate* mate, td_census_entry** entries, int64_t* n,
                                 td_mol_totals* totals)
{
	return host_count(mate ? "td_mol_host_mated" : "td_mol_host", false, m, prefix_bases, codes, offs, n_reads, res, labels, mate, entries, nullptr, n, totals);
}

extern "C" int td_mol_host(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                           const td_read_result* res, const int8_t* labels, td_census_entry** entries, int64_t* n, td_mol_totals* totals)
{
	return td_mol_host_mated(m, prefix_bases, codes, offs, n_reads, res, labels, nullptr, entries, n, totals);
}

extern "C" int td_mol_host_origins_mated(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                                         const td_read_result* res, const int8_t* labels, const td_mol_mate* mate, td_census_entry** entries,
                                         td_mol_origin** origins, int64_t* n, td_mol_totals* totals)
{
	return host_count(mate ? "td_mol_host_origins_mated" : "td_mol_host_origins", true, m, prefix_bases, codes, offs, n_reads, res, labels, mate, entries,
	                  origins, n, totals);
}

extern "C" int td_mol_host_origins(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                                   const td_read_result* res, const int8_t* labels, td_census_entry** entries, td_mol_origin** origins, int64_t* n,
                                   td_mol_totals* totals)
{
	return td_mol_host_origins_mated(m, prefix_bases, codes, offs, n_reads, res, labels, nullptr, entries, origins, n, totals);
}

extern "C" int td_mol_dedup_host(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                                 const td_read_result* res, const int8_t* labels, uint8_t* is_duplicate, td_mol_dedup_totals* totals)
{
	return td_mol_dedup_host_mated(m, prefix_bases, codes, offs, n_reads, res, labels, nullptr, is_duplicate, totals);
}

extern "C" int td_mol_dedup_host_mated(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                                       const td_read_result* res, const int8_t* labels, const td_mol_mate* mate, uint8_t* is_duplicate,
                                       td_mol_dedup_totals* totals)
{
	if (host_checks(mate ? "td_mol_dedup_host_mated" : "td_mol_dedup_host", m, prefix_bases, mate, n_reads, n_reads >= 0 && (n_reads == 0 || (offs && res && labels && codes && is_duplicate))) != TD_OK) return TD_FAIL;
	td_mol_dedup_totals t{};
	std::unordered_set<uint64_t> seen;                // the keys of the reads so far: a read's ordinal is its index, the first one stays
	for (int64_t i = 0; i < n_reads; i++) {
		is_duplicate[i] = 0;
		uint64_t key = 0;
		td_mol_origin o{};
		const int cls = host_read_class(m, prefix_bases, codes, offs, i, res, labels, mate, &key, &o);
		if (cls == MOL_NOT_ELIGIBLE) continue;
		if (cls != MOL_COUNTED) { t.unjudged++; t.kept++; continue; }
		if (seen.insert(key).second) t.kept++;
		else { is_duplicate[i] = 1; t.duplicates++; }
	}
	if (totals) *totals = t;
	return TD_OK;
}

extern "C" int td_mol_dedup_collapsed_host(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs, int64_t n_reads,
                                           const td_read_result* res, const int8_t* labels, uint8_t* is_duplicate, td_mol_dedup_totals* totals,
                                           td_mol_collapse_totals* collapse_totals)
{
	return td_mol_dedup_collapsed_host_mated(m, prefix_bases, codes, offs, n_reads, res, labels, nullptr, is_duplicate, totals, collapse_totals);
}

extern "C" int td_mol_dedup_collapsed_host_mated(const td_model_desc* m, int32_t prefix_bases, const uint8_t* codes, const int64_t* offs,
                                                 int64_t n_reads, const td_read_result* res, const int8_t* labels, const td_mol_mate* mate,
                                                 uint8_t* is_duplicate, td_mol_dedup_totals* totals, td_mol_collapse_totals* collapse_totals)
{
	if (host_checks(mate ? "td_mol_dedup_collapsed_host_mated" : "td_mol_dedup_collapsed_host", m, prefix_bases, mate, n_reads, n_reads >= 0 && (n_reads == 0 || (offs && res && labels && codes && is_duplicate))) != TD_OK)
		return TD_FAIL;
	// the survey: every counted read's key and origin, and the first ordinal of every key (a read's ordinal is its index)
	std::vector<uint64_t> key_of((size_t)n_reads, 0);
	std::vector<int> cls_of((size_t)n_reads, MOL_NOT_ELIGIBLE);
	std::vector<td_census_entry> each;
	std::vector<td_mol_origin> each_o;
	std::unordered_map<uint64_t, int64_t> first;
	for (int64_t i = 0; i < n_reads; i++) {
		td_mol_origin o{};
		cls_of[(size_t)i] = host_read_class(m, prefix_bases, codes, offs, i, res, labels, mate, &key_of[(size_t)i], &o);
		if (cls_of[(size_t)i] != MOL_COUNTED) continue;
		each.push_back(td_census_entry{ key_of[(size_t)i], 1 });
		each_o.push_back(o);
		first.emplace(key_of[(size_t)i], i);              // (the first one stays)
	}
	// the freeze: the collapse, and for every key the first ordinal of its root's own key
	std::vector<td_census_entry> v;
	std::vector<td_mol_origin> vo;
	host_add_repeated(each.data(), each_o.data(), (int64_t)each.size(), v, vo);
	HostForest f;
	host_forest(v, vo, f);
	std::unordered_map<uint64_t, int64_t> keeper;
	for (size_t u = 0; u < v.size(); u++) keeper[v[u].key] = first[v[f.root[u]].key];
	// the replay of the same reads
	td_mol_dedup_totals t{};
	for (int64_t i = 0; i < n_reads; i++) {
		is_duplicate[i] = 0;
		if (cls_of[(size_t)i] == MOL_NOT_ELIGIBLE) continue;
		if (cls_of[(size_t)i] != MOL_COUNTED) { t.unjudged++; t.kept++; continue; }
		if (keeper[key_of[(size_t)i]] == i) t.kept++;
		else { is_duplicate[i] = 1; t.duplicates++; }
	}
	if (totals) *totals = t;
	if (collapse_totals) *collapse_totals = f.totals;
	return TD_OK;
}

extern "C" int td_mol_collapse_host(const td_census_entry* entries, const td_mol_origin* origins, int64_t n, td_census_entry** out_entries,
                                    td_mol_origin** out_origins, int64_t* out_n, td_mol_collapse_totals* totals)
{
	if (out_entries) *out_entries = nullptr;
	if (out_origins) *out_origins = nullptr;
	if (out_n) *out_n = 0;
	if (!out_entries || !out_origins || !out_n || n < 0 || (n > 0 && (!entries || !origins))) return fail(nullptr, "td_mol_collapse_host: bad arguments");
	std::vector<td_census_entry> v;
	std::vector<td_mol_origin> vo;
	host_add_repeated(entries, origins, n, v, vo);
	HostForest f;
	host_forest(v, vo, f);
	std::vector<td_census_entry> r;                   // the roots with their collapsed counts, then in the order of td_census_get
	std::vector<td_mol_origin> r_o;
	for (size_t u = 0; u < v.size(); u++) if (f.root[u] == u) { r.push_back(td_census_entry{ v[u].key, f.collapsed[u] }); r_o.push_back(vo[u]); }
	std::vector<td_census_entry> re(r.size());
	std::vector<td_mol_origin> ro(r.size());
	mol_emit_ordered(r.data(), r_o.data(), (int64_t)r.size(), (int64_t)r.size(), re.data(), ro.data());
	td_census_entry* pe = kt_copy_entries(re);
	td_mol_origin* po = copy_origins(ro);
	if (!pe || !po) { free(pe); free(po); return fail(nullptr, "td_mol_collapse_host: out of memory"); }
	*out_entries = pe; *out_origins = po; *out_n = (int64_t)re.size();
	if (totals) *totals = f.totals;
	return TD_OK;
}

extern "C" int td_mol_summarise(const td_census_entry* entries, int64_t n, td_mol_row rows[TD_NUM_BARCODE_BINS])
{
	if (!rows || n < 0 || (n > 0 && !entries)) return fail(nullptr, "td_mol_summarise: bad arguments");
	memset(rows, 0, sizeof(td_mol_row) * TD_NUM_BARCODE_BINS);
	for (int64_t i = 0; i < n; i++) {
		if (entries[i].count <= 0) continue;
		td_mol_row& r = rows[td_mol_key_bin(entries[i].key)];
		r.reads += entries[i].count;
		r.molecules++;
		r.levels[std::min<int64_t>(entries[i].count, TD_MOL_LEVELS) - 1]++;
	}
	return TD_OK;
}

extern "C" uint64_t td_mol_key(int32_t barcode, int32_t fingerprint, uint64_t w, int32_t n) { return mol_key(barcode, fingerprint, w, n); }
extern "C" int32_t td_mol_key_bin(uint64_t key) { return (int32_t)(key >> 56); }
