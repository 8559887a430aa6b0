// td_samples_host.cpp -- the host side of sample assignment (include/tagdust_samples.h): the check of a sheet against a model and the
// plan it comes to, the keys in both directions, and td_samples_host, the definition the device's kernel (td_samples.hip) is held
// against, over host arrays.  A read's class and key are td_samples_def.h's, the text the kernel compiles too.  Plain C++: no
// device is used and no HIP header read.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "td_samples_def.h"

// The columns of a plan: the model's own 'B' segments stand at columns first_column.. of m_total (column_hmms: every column's
// n_hmm, NULL when all columns are the model's own), their labels in tc; seg[] = the segments of the own columns.
static int smp_columns_build(td_ctx* c, const char* who, const td_model_desc* m, int32_t m_total, int32_t first_column, const int32_t* column_hmms,
                             TdSamplePlan& p, int seg[TD_SAMPLES_MAX_SEGMENTS], int& n_own)
{
	if (!m || m->S < 1 || m->H < 1 || !m->seg_type || !m->label || !m->n_hmm) return fail(c, "%s: no model", who);
	if (m->H > 127) return fail(c, "%s: the model has %d HMMs (at most 127)", who, m->H);
	memset(&p, 0, sizeof p);
	int n_b = 0;
	for (int t = 0; t < TD_SAMPLES_MAX_SEGMENTS; t++) seg[t] = 0;
	for (int j = 0; j < m->S; j++) {
		if (m->seg_type[j] != 'B') continue;
		if (n_b < TD_SAMPLES_MAX_SEGMENTS) seg[n_b] = j;
		n_b++;
	}
	if (n_b == 0) return fail(c, "%s: the model has no 'B' segment: there is no barcode to assign a sample by", who);
	if (n_b > TD_SAMPLES_MAX_SEGMENTS) return fail(c, "%s: the model has %d 'B' segments (at most %d)", who, n_b, TD_SAMPLES_MAX_SEGMENTS);
	if (!column_hmms) { m_total = n_b; first_column = 0; }
	if (m_total < 1 || m_total > TD_SAMPLES_MAX_SEGMENTS) return fail(c, "%s: m_total = %d (1..%d columns supported)", who, m_total, TD_SAMPLES_MAX_SEGMENTS);
	if (first_column < 0 || first_column + n_b > m_total)
		return fail(c, "%s: the model's %d 'B' segments from column %d on do not fit into %d columns", who, n_b, first_column, m_total);
	for (int t = 0; t < n_b; t++)
		if (m->n_hmm[seg[t]] < 2 || m->n_hmm[seg[t]] > 127) return fail(c, "%s: 'B' segment %d has %d HMMs (a barcode and the decoy at least, 127 at most)", who, seg[t], m->n_hmm[seg[t]]);
	for (int t = 0; t < m_total; t++) {
		const bool own = t >= first_column && t < first_column + n_b;
		const int32_t n = column_hmms ? column_hmms[t] : m->n_hmm[seg[t]];
		if (own && n != m->n_hmm[seg[t - first_column]])
			return fail(c, "%s: column_hmms[%d] = %d, 'B' segment %d of the model (that column) has %d HMMs", who, t, n, seg[t - first_column], m->n_hmm[seg[t - first_column]]);
		if (n < 2 || n > 127) return fail(c, "%s: column_hmms[%d] = %d (a barcode and the decoy at least, 127 at most)", who, t, n);
		p.decoy |= (uint32_t)n << (8 * t);
	}
	p.m = m_total; p.last_seg = seg[n_b - 1];
	p.ordered = 1;
	for (int h = 0; h + 1 < m->H; h++) if ((m->label[h] & 0xFFFF) > (m->label[h + 1] & 0xFFFF)) p.ordered = 0;
	for (int h = 0; h < m->H; h++) {
		const int s = m->label[h] & 0xFFFF, call = (m->label[h] >> 16) & 0x7FFF;
		uint16_t e = s > p.last_seg ? (uint16_t)SMP_TC_BEHIND : (uint16_t)0;
		for (int t = 0; t < n_b; t++) {
			if (s != seg[t]) continue;
			if (call > 126) return fail(c, "%s: HMM %d is call %d of 'B' segment %d (at most 126)", who, h, call, s);
			e = (uint16_t)(SMP_TC_CHOSEN | (uint32_t)((first_column + t) << 8) | (uint32_t)(call + 1));
		}
		p.tc[h + 1] = e;
	}
	n_own = n_b;
	return TD_OK;
}

// ... and its rows: inside their columns, the decoy excluded, pairwise different
static int smp_rows_build(td_ctx* c, const char* who, const int32_t* tuples, int32_t n_samples, int32_t first_column, const int seg[TD_SAMPLES_MAX_SEGMENTS],
                          int n_own, TdSamplePlan& p)
{
	if (n_samples < 1 || n_samples > TD_SAMPLES_MAX) return fail(c, "%s: n_samples = %d (1..%d supported)", who, n_samples, TD_SAMPLES_MAX);
	if (!tuples) return fail(c, "%s: no sheet", who);
	p.n_samples = n_samples;
	std::vector<std::pair<uint32_t, int>> rows;
	for (int s = 0; s < n_samples; s++) {
		uint32_t w = 0;
		for (int t = 0; t < p.m; t++) {
			const int32_t b = tuples[(size_t)s * p.m + t], n = (int32_t)((p.decoy >> (8 * t)) & 0xFFu);
			const bool own = t >= first_column && t < first_column + n_own;
			if (b < 0 || b >= n - 1) {   // (an own column is named by its segment, a partner's by its number alone)
				if (own) return fail(c, "%s: row %d of the sheet: barcode %d of 'B' segment %d (column %d) is out of range (0..%d; the last HMM is the all-N decoy)", who,
				                     s, b, seg[t - first_column], t, n - 2);
				return fail(c, "%s: row %d of the sheet: barcode %d of column %d (another file's) is out of range (0..%d; the last HMM is the all-N decoy)", who,
				            s, b, t, n - 2);
			}
			w |= (uint32_t)(b + 1) << (8 * t);
		}
		rows.push_back({ w, s });
	}
	std::sort(rows.begin(), rows.end());
	for (size_t k = 0; k + 1 < rows.size(); k++)
		if (rows[k].first == rows[k + 1].first) return fail(c, "%s: row %d of the sheet repeats row %d", who, rows[k + 1].second, rows[k].second);
	for (size_t k = 0; k < rows.size(); k++) { p.row[k] = rows[k].first; p.sample[k] = (uint8_t)rows[k].second; }
	return TD_OK;
}

int smp_plan_build(td_ctx* c, const char* who, const td_model_desc* m, const int32_t* tuples, int32_t n_samples, TdSamplePlan& out)
{
	TdSamplePlan p;
	int seg[TD_SAMPLES_MAX_SEGMENTS], n_own = 0;
	if (smp_columns_build(c, who, m, 0, 0, nullptr, p, seg, n_own) != TD_OK) return TD_FAIL;
	if (smp_rows_build(c, who, tuples, n_samples, 0, seg, n_own, p) != TD_OK) return TD_FAIL;
	out = p;
	return TD_OK;
}

int smp_join_plan_build(td_ctx* c, const char* who, const td_model_desc* m, const int32_t* tuples, int32_t n_samples, int32_t m_total,
                        int32_t first_column, const int32_t* column_hmms, TdSamplePlan& out)
{
	TdSamplePlan p;
	int seg[TD_SAMPLES_MAX_SEGMENTS], n_own = 0;
	if (!column_hmms) return fail(c, "%s: no column_hmms", who);
	if (m_total < 2 || m_total > TD_SAMPLES_MAX_SEGMENTS) return fail(c, "%s: m_total = %d (2..%d columns supported)", who, m_total, TD_SAMPLES_MAX_SEGMENTS);
	if (smp_columns_build(c, who, m, m_total, first_column, column_hmms, p, seg, n_own) != TD_OK) return TD_FAIL;
	if (smp_rows_build(c, who, tuples, n_samples, first_column, seg, n_own, p) != TD_OK) return TD_FAIL;
	out = p;
	return TD_OK;
}

int smp_export_plan_build(td_ctx* c, const char* who, const td_model_desc* m, int32_t first_column, TdSamplePlan& out)
{
	TdSamplePlan p;
	int seg[TD_SAMPLES_MAX_SEGMENTS], n_own = 0;
	if (first_column < 0 || first_column >= TD_SAMPLES_MAX_SEGMENTS) return fail(c, "%s: first_column = %d (0..%d)", who, first_column, TD_SAMPLES_MAX_SEGMENTS - 1);
	// (every column the exporter does not fill counts as another's: only the own ones are looked at)
	int32_t hmms[TD_SAMPLES_MAX_SEGMENTS] = { 2, 2, 2, 2 };
	int n_b = 0;
	if (m && m->seg_type && m->n_hmm)
		for (int j = 0; j < m->S; j++)
			if (m->seg_type[j] == 'B') { if (first_column + n_b < TD_SAMPLES_MAX_SEGMENTS) hmms[first_column + n_b] = m->n_hmm[j]; n_b++; }
	if (smp_columns_build(c, who, m, TD_SAMPLES_MAX_SEGMENTS, first_column, hmms, p, seg, n_own) != TD_OK) return TD_FAIL;
	out = p;
	return TD_OK;
}

int smp_names_check(td_ctx* c, const char* who, const char* const* names, int32_t n_samples, std::vector<std::string>& out)
{
	std::vector<std::string> v;
	std::set<std::string> seen;
	for (int s = 0; s < n_samples; s++) {
		std::string name = names && names[s] ? std::string(names[s]) : "S" + std::to_string(s + 1);
		if (name.empty() || name.size() > TD_SAMPLES_MAX_NAME) return fail(c, "%s: row %d of the sheet: a name has 1..%d characters, this one %zu", who, s, TD_SAMPLES_MAX_NAME, name.size());
		for (const char ch : name) {
			const bool ok = (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '.' || ch == '_' || ch == '-';
			if (!ok) return fail(c, "%s: row %d of the sheet: the name '%s' holds a character outside [A-Za-z0-9._-]", who, s, name.c_str());
		}
		if (!seen.insert(name).second) return fail(c, "%s: row %d of the sheet: the name '%s' is taken by an earlier row", who, s, name.c_str());
		v.push_back(name);
	}
	out.swap(v);
	return TD_OK;
}

extern "C" uint64_t td_samples_key(const int32_t* calls, int32_t m)
{
	if (!calls || m < 1 || m > TD_SAMPLES_MAX_SEGMENTS) return 0;
	uint32_t w = 0;
	for (int t = 0; t < m; t++) {
		if (calls[t] < -1 || calls[t] > 126) return 0;
		w |= (uint32_t)(calls[t] + 1) << (8 * t);
	}
	return smp_key(w, m);
}

extern "C" int td_samples_key_calls(uint64_t key, int32_t calls[TD_SAMPLES_MAX_SEGMENTS], int32_t* m)
{
	const int k = (int)(key >> 56);
	if (!calls || !m) return fail(nullptr, "td_samples_key_calls: bad arguments");
	if (k < 1 || k > TD_SAMPLES_MAX_SEGMENTS) return fail(nullptr, "td_samples_key_calls: 0x%llx is no key (%d segments)", (unsigned long long)key, k);
	if ((key & KEY_LOW_MASK) >> (8 * k) != 0) return fail(nullptr, "td_samples_key_calls: 0x%llx is no key (bits beyond its %d calls)", (unsigned long long)key, k);
	for (int t = 0; t < TD_SAMPLES_MAX_SEGMENTS; t++) {
		const int b = (int)((key >> (8 * t)) & 0xFFu);
		if (b > 127) return fail(nullptr, "td_samples_key_calls: 0x%llx is no key (call %d of segment %d)", (unsigned long long)key, b - 1, t);
		calls[t] = t < k ? b - 1 : -1;
	}
	*m = k;
	return TD_OK;
}

// a read's own calls word under plan p, from its labels (the last position of a segment wins)
static uint32_t own_calls(const TdSamplePlan& p, int H, const int8_t* lab, int64_t len)
{
	uint32_t calls = 0;
	for (int64_t q = 0; q < len; q++) {
		const int l = lab[q + 1];
		if (l < 0 || l >= H) continue;
		const uint32_t e = p.tc[l + 1];
		if (e & SMP_TC_CHOSEN) calls = smp_take(calls, e);
	}
	return calls;
}

// The definition over host arrays under a built plan; words = the partners' export words of a join (NULL: no join).
static int assign_host(const char* who, const TdSamplePlan& p, int H, const uint32_t* words, const int64_t* offs, int64_t n_reads, td_read_result* res,
                       const int8_t* labels, td_census_entry** entries, int64_t* n, td_samples_join_totals* totals)
{
	td_samples_join_totals t{};
	std::vector<uint64_t> keys;
	for (int64_t i = 0; i < n_reads; i++) {
		if (res[i].read_type != TD_EXTRACT_SUCCESS) continue;
		if (words && words[i] == SMP_PARTNER_FAILED) { t.partner_failed++; continue; }
		t.t.eligible++;
		const uint32_t calls = own_calls(p, H, labels + offs[i] + i, offs[i + 1] - offs[i]) | (words ? words[i] : 0u);
		keys.push_back(smp_key(calls, p.m));
		const int s = smp_incomplete(calls, p.decoy, p.m) ? -2 : smp_find(p.row, p.sample, p.n_samples, calls);
		if (s >= 0) { res[i].barcode = (p.last_seg << 16) | s; t.t.assigned++; }
		else { res[i].read_type = TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND; if (s == -2) t.t.incomplete++; else t.t.unlisted++; }
	}
	std::vector<td_census_entry> v;
	kt_tally_keys(keys, v);
	if (!(*entries = kt_copy_entries(v))) return fail(nullptr, "%s: out of memory", who);
	*n = (int64_t)v.size();
	if (totals) *totals = t;
	return TD_OK;
}

extern "C" int td_samples_host(const td_model_desc* model, const int32_t* tuples, int32_t n_samples, const int64_t* offs, int64_t n_reads,
                               td_read_result* res, const int8_t* labels, td_census_entry** entries, int64_t* n, td_samples_totals* totals)
{
	if (entries) *entries = nullptr;
	if (n) *n = 0;
	TdSamplePlan p;
	if (smp_plan_build(nullptr, "td_samples_host", model, tuples, n_samples, p) != TD_OK) return TD_FAIL;
	if (!entries || !n || n_reads < 0 || (n_reads > 0 && (!offs || !res || !labels))) return fail(nullptr, "td_samples_host: bad arguments");
	td_samples_join_totals t{};
	if (assign_host("td_samples_host", p, model->H, nullptr, offs, n_reads, res, labels, entries, n, &t) != TD_OK) return TD_FAIL;
	if (totals) *totals = t.t;
	return TD_OK;
}

extern "C" int td_samples_export_host(const td_model_desc* model, int32_t first_column, const int64_t* offs, int64_t n_reads,
                                      const td_read_result* res, const int8_t* labels, uint32_t* words)
{
	TdSamplePlan p;
	if (smp_export_plan_build(nullptr, "td_samples_export_host", model, first_column, p) != TD_OK) return TD_FAIL;
	if (n_reads < 0 || (n_reads > 0 && (!offs || !res || !labels || !words))) return fail(nullptr, "td_samples_export_host: bad arguments");
	for (int64_t i = 0; i < n_reads; i++) {
		const bool extracted = res[i].read_type == TD_EXTRACT_SUCCESS;
		words[i] = smp_export_word(extracted, extracted ? own_calls(p, model->H, labels + offs[i] + i, offs[i + 1] - offs[i]) : 0u);
	}
	return TD_OK;
}

extern "C" int td_samples_join_host(const td_model_desc* model, const int32_t* tuples, int32_t n_samples, int32_t m_total, int32_t first_column,
                                    const int32_t* column_hmms, const uint32_t* words, const int64_t* offs, int64_t n_reads, td_read_result* res,
                                    const int8_t* labels, td_census_entry** entries, int64_t* n, td_samples_join_totals* totals)
{
	if (entries) *entries = nullptr;
	if (n) *n = 0;
	TdSamplePlan p;
	if (smp_join_plan_build(nullptr, "td_samples_join_host", model, tuples, n_samples, m_total, first_column, column_hmms, p) != TD_OK) return TD_FAIL;
	if (!entries || !n || n_reads < 0 || (n_reads > 0 && (!offs || !res || !labels || !words))) return fail(nullptr, "td_samples_join_host: bad arguments");
	return assign_host("td_samples_join_host", p, model->H, words, offs, n_reads, res, labels, entries, n, totals);
}
