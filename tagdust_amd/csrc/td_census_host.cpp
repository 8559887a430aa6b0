// td_census_host.cpp -- the host side of the census (include/tagdust_census.h): td_census_host, the definition the device's count
// (td_census.hip) is held against, over host arrays; td_census_merge, which adds two results; td_census_key_text; and the host
// helpers of every td_census_entry result, the molecule count's included.  Plain C++: no device is used and no HIP header read.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "td_count_key.h"

bool kt_entry_before(const td_census_entry& x, const td_census_entry& y) { return x.count != y.count ? x.count > y.count : x.key < y.key; }

td_census_entry* kt_copy_entries(const std::vector<td_census_entry>& v)
{
	td_census_entry* p = (td_census_entry*)malloc(sizeof(td_census_entry) * (v.size() ? v.size() : 1));
	if (p && !v.empty()) memcpy(p, v.data(), sizeof(td_census_entry) * v.size());
	return p;
}

void kt_tally_keys(std::vector<uint64_t>& keys, std::vector<td_census_entry>& out)
{
	std::sort(keys.begin(), keys.end());
	for (size_t i = 0; i < keys.size();) {
		size_t j = i;
		while (j < keys.size() && keys[j] == keys[i]) j++;
		out.push_back(td_census_entry{ keys[i], (int64_t)(j - i) });
		i = j;
	}
	std::sort(out.begin(), out.end(), kt_entry_before);
}

int census_pick_segment(td_ctx* c, const char* who, const td_model_desc* m, int32_t segment, int32_t* out)
{
	if (!m || m->S < 1 || !m->seg_type || !m->label) return fail(c, "%s: no model", who);
	int last = -1;
	for (int j = 0; j < m->S; j++) if (m->seg_type[j] == 'B') last = j;
	if (last < 0) return fail(c, "%s: the model has no 'B' segment: there is no barcode to take a census of", who);
	if (segment == -1) { *out = last; return TD_OK; }
	if (segment < 0 || segment >= m->S) return fail(c, "%s: segment %d is out of range (0..%d, or -1 for the last 'B' segment)", who, segment, m->S - 1);
	if (m->seg_type[segment] != 'B') return fail(c, "%s: segment %d is a '%c' segment, not a 'B' segment", who, segment, (char)m->seg_type[segment]);
	*out = segment;
	return TD_OK;
}

bool census_mask_ok(uint32_t mask) { return mask != 0u && mask <= 0xFFu; }

extern "C" int td_census_host(const td_model_desc* m, int32_t segment, uint32_t outcome_mask, const uint8_t* codes, const int64_t* offs,
                              int64_t n_reads, const td_read_result* res, const int8_t* labels,
                              td_census_entry** entries, int64_t* n, td_census_totals* totals)
{
	if (entries) *entries = nullptr;
	if (n) *n = 0;
	int32_t seg = -1;
	if (census_pick_segment(nullptr, "td_census_host", m, segment, &seg) != TD_OK) return TD_FAIL;
	if (!census_mask_ok(outcome_mask)) return fail(nullptr, "td_census_host: outcome_mask 0x%x is not a non-empty subset of bits 0..7", outcome_mask);
	if (!entries || !n || n_reads < 0 || (n_reads > 0 && (!offs || !res || !labels))) return fail(nullptr, "td_census_host: bad arguments");
	td_census_totals t{};
	std::vector<uint64_t> keys;
	for (int64_t i = 0; i < n_reads; i++) {
		const uint32_t type = (uint32_t)res[i].read_type & 0xFFu;
		if (type >= 8u || !((outcome_mask >> type) & 1u)) continue;
		t.eligible++;
		const int64_t len = offs[i + 1] - offs[i];
		const int8_t* lab = labels + offs[i] + i;
		const uint8_t* seq = codes + offs[i];
		uint64_t w = 0;
		int cnt = 0;
		bool has_n = false;
		for (int64_t p = 0; p < len; p++) {
			const int l = lab[p + 1];
			if (l < 0 || l >= m->H || (m->label[l] & 0xFFFF) != seg) continue;
			cnt++;
			if (cnt <= TD_CENSUS_MAX_WORD) {
				if (seq[p] > 3) has_n = true;
				w = (w << 2) | (uint64_t)(seq[p] & 3u);
			}
		}
		if (cnt == 0) t.skipped_empty++;
		else if (cnt > TD_CENSUS_MAX_WORD) t.skipped_long++;
		else if (has_n) t.skipped_n++;
		else { keys.push_back(((uint64_t)cnt << 56) | w); t.counted++; }
	}
	std::vector<td_census_entry> v;
	kt_tally_keys(keys, v);
	t.distinct = (int64_t)v.size();
	if (!(*entries = kt_copy_entries(v))) return fail(nullptr, "td_census_host: out of memory");
	*n = (int64_t)v.size();
	if (totals) *totals = t;
	return TD_OK;
}

// (the molecule count's entries go through these two as well)
extern "C" int td_census_merge(const td_census_entry* a, int64_t na, const td_census_entry* b, int64_t nb, td_census_entry** out, int64_t* n)
{
	if (!out || !n || na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b)) return fail(nullptr, "td_census_merge: bad arguments");
	std::vector<td_census_entry> all;
	all.insert(all.end(), a, a + na);
	all.insert(all.end(), b, b + nb);
	std::sort(all.begin(), all.end(), [](const td_census_entry& x, const td_census_entry& y) { return x.key < y.key; });
	std::vector<td_census_entry> v;
	for (const td_census_entry& e : all) {
		if (!v.empty() && v.back().key == e.key) v.back().count += e.count;
		else v.push_back(e);
	}
	std::sort(v.begin(), v.end(), kt_entry_before);
	if (!(*out = kt_copy_entries(v))) return fail(nullptr, "td_census_merge: out of memory");
	*n = (int64_t)v.size();
	return TD_OK;
}

extern "C" void td_census_free(td_census_entry* entries) { free(entries); }

extern "C" int td_census_key_text(uint64_t key, char buf[32])
{
	if (!buf) return TD_FAIL;
	buf[0] = 0;
	const int len = (int)(key >> 56);
	if (len < 1 || len > TD_CENSUS_MAX_WORD) return fail(nullptr, "td_census_key_text: 0x%llx is no key (length %d)", (unsigned long long)key, len);
	if (len < TD_CENSUS_MAX_WORD && ((key & KEY_LOW_MASK) >> (2 * len)) != 0) return fail(nullptr, "td_census_key_text: 0x%llx is no key (bits beyond its %d bases)", (unsigned long long)key, len);
	for (int i = 0; i < len; i++) buf[i] = "ACGT"[(key >> (2 * (len - 1 - i))) & 3u];
	buf[len] = 0;
	return TD_OK;
}
