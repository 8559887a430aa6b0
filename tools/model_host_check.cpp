// model_host_check.cpp -- the path from an architecture to what the device receives, as far as the host decides it, as a stand-alone
// program for the host sanitizers: td_model.cpp (architecture, statistics, tables), td_model_flat.cpp (the generic kernel's tables,
// the -ref text in 2-bit words, the logsum table), td_spec_plan.cpp and td_spec_bounds.cpp (plan, model section, workspace layout,
// bound tables of the specialised kernel), and the host arithmetic of td_estimate_threshold / td_compare_architectures (td_model.cpp).
// No GPU is used, no HIP header, no Python, no stubs.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tagdust_amd/csrc/td_model.cpp tagdust_amd/csrc/td_model_flat.cpp tagdust_amd/csrc/td_spec_plan.cpp
//       tagdust_amd/csrc/td_spec_bounds.cpp tools/model_host_check.cpp -o /tmp/model_host_check
//   /tmp/model_host_check                                        # (leak detection stays on)
//
// (a) four architectures built from strings, each held against its own description; (b) descriptions and an index the library must
// reject, with the text it reports; (c) the two calibration functions against restatements written here.  Exit status 0 when all of
// it agrees.
#define HOST_CHECK_NAME "model_host_check"
#include "host_check.h"

#include <math.h>

#include <algorithm>

#include "../include/tagdust_model.h"
#include "../tagdust_amd/csrc/td_jit.h"
#include "../tagdust_amd/csrc/td_model_flat.h"
#include "../tagdust_amd/csrc/td_model_inner.h"

static uint32_t bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
static bool live(float v) { return !(v == -INFINITY); }

// a few dozen reads of 30..50 random bases, the first `stamp.size()` of every other read taken from `stamp`
static void make_reads(uint32_t seed, const std::string& stamp, std::vector<uint8_t>& codes, std::vector<int64_t>& offs)
{
	codes.clear(); offs.assign(1, 0);
	for (int i = 0; i < 48; i++) {
		const int len = 30 + (int)(rnd(seed) % 21);
		for (int q = 0; q < len; q++) {
			uint8_t b = (uint8_t)(rnd(seed) & 3);
			if (i % 2 == 0 && q < (int)stamp.size()) b = (uint8_t)std::string("ACGT").find(stamp[(size_t)q]);
			codes.push_back(b);
		}
		offs.push_back((int64_t)codes.size());
	}
}

// ---------------------------------------------------------------------------------------------------------
// (a) one architecture: description -> flat tables, plan, model section, layout, bound tables
// ---------------------------------------------------------------------------------------------------------
static int n_prune_runs = 0, n_rt_loops = 0, n_first_labels = 0;

// the literals of kCols in the model section, in the order they stand there
static bool section_cols(const std::string& sec, int C, std::vector<float>& out)
{
	const std::string head = "static constexpr GCol kCols[" + std::to_string(C) + "] = {\n";
	const size_t at = sec.find(head);
	if (at == std::string::npos) return false;
	const char* p = sec.c_str() + at + head.size();
	const char* const minus_inf = "(-__builtin_inff())";
	out.clear();
	while (strncmp(p, "};\n", 3) != 0) {
		if (!*p) return false;
		if (!strncmp(p, minus_inf, strlen(minus_inf))) { out.push_back(-INFINITY); p += strlen(minus_inf); continue; }
		if (*p == '-' || *p == '0') {
			char* end = nullptr;
			out.push_back(strtof(p, &end));   // a hex float: exact
			if (end == p || *end != 'f') return false;
			p = end + 1;
			continue;
		}
		if (!strchr(" {},\n", *p)) return false;
		p++;
	}
	return true;
}

static int check_architecture(const char* name, const std::vector<std::string>& segments, const std::string& stamp)
{
	g_err = name;
	std::vector<const char*> args;
	for (const std::string& s : segments) args.push_back(s.c_str());
	td_arch* a = nullptr;
	CHECK(td_arch_parse(args.data(), (int32_t)args.size(), &a) == TD_OK);
	std::vector<uint8_t> codes; std::vector<int64_t> offs;
	make_reads(12345u + (uint32_t)segments.size(), stamp, codes, offs);
	td_seq_stats st;
	CHECK(td_sequence_stats(a, codes.data(), offs.data(), (int64_t)offs.size() - 1, &st) == TD_OK);
	td_model_tables* tab = nullptr;
	CHECK(td_model_build(a, &st, 0.05f, 0.1f, &tab) == TD_OK);
	const td_model_desc* m = &tab->desc;
	const int S = m->S, H = m->H, C = m->C;
	CHECK(S == (int)segments.size());

	TdFlatModel f;
	std::string why;
	CHECK(td_flatten_model(m, f, why));
	CHECK(why.empty());
	// column and HMM offsets
	CHECK(f.h.S == S && f.h.H == H && f.h.C == C && f.h.avg_len == m->avg_len);
	int co = 0, ho = 0, req = 0, maxc = 0;
	for (int j = 0; j < S; j++) {
		const TdSeg& s = f.h.seg[j];
		CHECK(s.col_off == co && s.hmm_off == ho && s.n_hmm == m->n_hmm[j] && s.n_col == m->n_col[j]);
		CHECK(bits(s.skip) == bits(m->skip[j]) && s.skip_live == (int)live(m->skip[j]) && s.type == m->seg_type[j]);
		co += s.n_hmm * s.n_col; ho += s.n_hmm;
		if (m->seg_type[j] == 'F') req += a->seq_len[j];
		maxc = std::max(maxc, s.n_col);
	}
	CHECK(co == C && ho == H && f.h.required_finger_len == req && f.h.max_ncol == maxc);
	CHECK(bits(f.h.r_stay) == bits((float)log((double)(float)(1.0 - 1.0 / (double)(float)m->avg_len))));
	CHECK(bits(f.h.r_exit) == bits((float)log((double)(float)(1.0 / (double)(float)m->avg_len))));
	// columns: the description's bits, and a flag bit exactly where the parameter is not -inf
	CHECK((int)f.cols.size() == C);
	for (int k = 0; k < C; k++) {
		const TdCol& q = f.cols[(size_t)k];
		uint32_t fl = 0;
		for (int t = 0; t < 9; t++) { CHECK(bits(q.t[t]) == bits(m->trans[k * 9 + t])); fl |= (uint32_t)live(m->trans[k * 9 + t]) << t; }
		fl |= (uint32_t)live(m->sM[k]) << 9 | (uint32_t)live(m->sI[k]) << 10;
		CHECK(bits(q.sM) == bits(m->sM[k]) && bits(q.sI) == bits(m->sI[k]));
		for (int e = 0; e < 5; e++) CHECK(bits(q.eM[e]) == bits(m->eM[k * 5 + e]) && bits(q.eI[e]) == bits(m->eI[k * 5 + e]));
		CHECK(q.flags == fl && q.pad[0] == 0 && q.pad[1] == 0);
	}
	// hinfo: HMM f of segment j, in that order
	CHECK((int)f.hinfo.size() == H);
	for (int j = 0, h = 0; j < S; j++)
		for (int hm = 0; hm < m->n_hmm[j]; hm++, h++) {
			const uint32_t v = f.hinfo[(size_t)h];
			CHECK((int)(v & 0xFF) == m->seg_type[j] && (int)(v >> 8 & 0xFF) == j && (int)(v >> 16 & 0x7FFF) == hm);
			CHECK((v >> 31) == (uint32_t)(m->seg_type[j] == 'B' && hm == m->n_hmm[j] - 1));
		}
	// predecessor lists: the u < v with A[u][v] = 1, ascending
	CHECK((int)f.pred_off.size() == H + 1 && f.pred_off[0] == 0);
	for (int v = 0; v < H; v++) {
		int at = f.pred_off[(size_t)v];
		for (int u = 0; u < v; u++)
			if (m->A[u * H + v] == 1.0f) { CHECK(at < f.pred_off[(size_t)v + 1] && f.pred_idx[(size_t)at] == u); at++; }
		CHECK(at == f.pred_off[(size_t)v + 1]);
	}
	CHECK((int)f.pred_idx.size() == std::max(f.pred_off[(size_t)H], 1));

	// the plan and the model section
	const TdSpecPlan p = td_spec_plan(m, TdSpecKnobs());
	CHECK(p.S == S && p.H == H && p.C == C && (int)p.col_off.size() == S && (int)p.hmm_off.size() == S);
	for (int j = 0; j < S; j++) CHECK(p.col_off[(size_t)j] == f.h.seg[j].col_off && p.hmm_off[(size_t)j] == f.h.seg[j].hmm_off);
	for (int j = 0; j < S; j++) if (p.rt[(size_t)j] > 0) n_rt_loops++;
	if (p.first_n > 0) n_first_labels++;
	const std::string sec = td_spec_model_section(m, p, p.k.lsum_oob, 0);
	std::vector<float> lit;
	CHECK(section_cols(sec, C, lit));
	CHECK((int)lit.size() == 21 * C);
	for (int k = 0; k < C; k++) {
		const float* r = lit.data() + (size_t)k * 21;
		for (int t = 0; t < 9; t++) CHECK(bits(r[t]) == bits(m->trans[k * 9 + t]));
		CHECK(bits(r[9]) == bits(m->sM[k]) && bits(r[10]) == bits(m->sI[k]));
		for (int e = 0; e < 5; e++) CHECK(bits(r[11 + e]) == bits(m->eM[k * 5 + e]) && bits(r[16 + e]) == bits(m->eI[k * 5 + e]));
	}
	// the workspace layout: ascending, 256-byte aligned, the last array ends within the slot
	for (int lmax : { 1, 33, 1026 }) {
		TdSpecLayout L;
		td_spec_layout(L, p, lmax);
		const int64_t o[] = { L.codes, L.sb, L.sf, L.bw, L.dp, L.path, L.total, L.rs, L.bm, L.ba, L.acc, L.pmask, L.slot_bytes };
		CHECK(o[0] == 0);
		for (size_t i = 0; i < sizeof o / sizeof o[0]; i++) CHECK(o[i] % 256 == 0 && (i == 0 || o[i] > o[i - 1]));
		CHECK(L.bw - L.sf >= (int64_t)(S + 1) * (lmax + 2) * 64 * 4 && L.dp - L.bw >= p.halves * lmax * 64 * 4);
		CHECK(L.pmask + (int64_t)H * ((lmax + 31) / 32) * 4 <= L.slot_bytes);
	}
	// the bound tables, where the plan prunes
	if (p.prune_segs > 0 || p.sfx_first < S) {
		std::vector<float> t;
		td_spec_prune_tables(m, p, 40, 48, t);
		CHECK(t.size() == (size_t)TD_PRUNE_TABLES * 48);
		n_prune_runs++;
	}
	td_model_tables_free(tab);
	td_arch_free(a);
	return 0;
}

// ---------------------------------------------------------------------------------------------------------
// (b) rejections: B:ACGT,TTGA + R:N (S 2, H 4, C 13) with one thing wrong at a time
// ---------------------------------------------------------------------------------------------------------
static int check_rejections()
{
	const char* segs[] = { "B:ACGT,TTGA", "R:N" };
	td_arch* a = nullptr;
	CHECK(td_arch_parse(segs, 2, &a) == TD_OK);
	std::vector<uint8_t> codes; std::vector<int64_t> offs;
	make_reads(99u, "ACGT", codes, offs);
	td_seq_stats st;
	CHECK(td_sequence_stats(a, codes.data(), offs.data(), (int64_t)offs.size() - 1, &st) == TD_OK);
	td_model_tables* tab = nullptr;
	CHECK(td_model_build(a, &st, 0.05f, 0.1f, &tab) == TD_OK);
	const td_model_desc good = tab->desc;
	CHECK(good.S == 2 && good.H == 4 && good.C == 13);
	const std::vector<int32_t> n_col(good.n_col, good.n_col + 2), label(good.label, good.label + 4);
	const std::vector<float> A(good.A, good.A + 16);
	TdFlatModel f;
	std::string why;
	auto rejected = [&](const td_model_desc& m, const char* text) {
		why.clear();
		g_err = text;
		return !td_flatten_model(&m, f, why) && why == text;
	};
	{ td_model_desc m = good; m.S = 0; CHECK(rejected(m, "td_model_upload: 0 segments (1..64 supported)")); }
	{ td_model_desc m = good; m.H = TD_MAX_HMMS + 1; CHECK(rejected(m, "td_model_upload: 128 HMMs (1..127 supported)")); }
	{ td_model_desc m = good; m.sI = nullptr; CHECK(rejected(m, "td_model_upload: NULL table pointer")); }
	{ td_model_desc m = good; std::vector<int32_t> v = n_col; v[1] = 0; m.n_col = v.data(); CHECK(rejected(m, "td_model_upload: segment 1 has 1 HMMs x 0 columns")); }
	{ td_model_desc m = good; m.C = 14; CHECK(rejected(m, "td_model_upload: inconsistent sizes (columns 13 vs C 14, HMMs 4 vs H 4)")); }
	{ td_model_desc m = good; std::vector<int32_t> v = label; v[0] = 2; m.label = v.data(); CHECK(rejected(m, "td_model_upload: label[0] names segment 2")); }
	{ td_model_desc m = good; std::vector<float> v = A; v[0 * 4 + 1] = 0.5f; m.A = v.data(); CHECK(rejected(m, "td_model_upload: transition matrix entry [0][1] = 0.5 is not 0/1")); }
	{ td_model_desc m = good; std::vector<float> v = A; v[2 * 4 + 2] = 0.0f; m.A = v.data(); CHECK(rejected(m, "td_model_upload: transition matrix diagonal [2] must be 1")); }
	CHECK(td_flatten_model(&good, f, why));
	td_model_tables_free(tab);
	td_arch_free(a);

	// the -ref text: a descending index, then three sequences (17, 0 and 16 characters) against their packing spelled out
	const std::string text = "XACGTACGTACGTACGTTXTTTTGGGGCCCCAAA";
	std::vector<int32_t> seq; std::vector<uint32_t> pk;
	const int32_t down[] = { 0, 5, 3 };
	why.clear();
	g_err = "the -ref text";
	CHECK(!td_pack_artifacts((const uint8_t*)text.data(), down, 2, seq, pk, why));
	CHECK(why == "td_set_artifacts: s_index is not ascending at 1");
	const int32_t idx[] = { 0, 18, 18, 34 };
	CHECK((int)text.size() == 34);
	CHECK(td_pack_artifacts((const uint8_t*)text.data(), idx, 3, seq, pk, why));
	CHECK(seq == (std::vector<int32_t>{ 0, 18, 2, 0, 2, 16 }) && pk.size() == 4);
	for (int j = 0; j < 3; j++)
		for (int q = 0; q < idx[j + 1] - idx[j]; q++)
			CHECK((pk[(size_t)seq[(size_t)j * 2] + (size_t)q / 16] >> (2 * (q % 16)) & 3u) == ((uint32_t)text[(size_t)(idx[j] + q)] & 3u));
	CHECK(pk[1] >> 4 == 0 && pk[3] == 0);   // nothing behind a sequence's last character, nor in the spare word

	const float* T = td_logsum_table();
	CHECK(T == td_logsum_table() && bits(T[0]) == bits((float)log(2.0)) && bits(T[TD_LOGSUM_SIZE - 1]) == bits((float)log(1.0 + exp(-15.999))));
	return 0;
}

// ---------------------------------------------------------------------------------------------------------
// (c) the host arithmetic of the two calibration entry points
// ---------------------------------------------------------------------------------------------------------
// every read goes to the first of the three percentile cuts (75 %, 95 %, the longest) its length does not exceed
static int check_classes(const std::vector<int>& lens, size_t want_classes)
{
	const int64_t n = (int64_t)lens.size();
	std::vector<uint8_t> codes; std::vector<int64_t> offs(1, 0);
	uint32_t seed = 7;
	for (int l : lens) { for (int q = 0; q < l; q++) codes.push_back((uint8_t)(rnd(seed) % 5)); offs.push_back((int64_t)codes.size()); }
	if (codes.empty()) codes.push_back(9);   // (never read)
	const std::vector<TdCalClass> got = td_calibration_classes(codes.data(), offs.data(), n);
	std::vector<int> sorted = lens;
	std::sort(sorted.begin(), sorted.end());
	std::vector<int> cuts;
	for (int64_t r : { (n - 1) * 3 / 4, (n - 1) * 19 / 20, n - 1 }) if (cuts.empty() || sorted[(size_t)r] > cuts.back()) cuts.push_back(sorted[(size_t)r]);
	std::vector<TdCalClass> want(cuts.size());
	for (TdCalClass& w : want) w.offs.push_back(0);
	for (int64_t i = 0; i < n; i++) {
		size_t k = 0;
		while (lens[(size_t)i] > cuts[k]) k++;
		want[k].idx.push_back(i);
		for (int q = 0; q < lens[(size_t)i]; q++) want[k].codes.push_back(codes[(size_t)(offs[(size_t)i] + q)]);
		want[k].offs.push_back((int64_t)want[k].codes.size());
	}
	CHECK(got.size() == want_classes);
	size_t g = 0, reads = 0;
	for (const TdCalClass& w : want) {
		if (w.idx.empty()) continue;
		CHECK(g < got.size());
		CHECK(got[g].idx == w.idx && got[g].offs == w.offs);
		CHECK(w.codes.empty() ? got[g].codes == std::vector<uint8_t>(1, 0) : got[g].codes == w.codes);
		reads += w.idx.size();
		g++;
	}
	CHECK(g == got.size() && reads == (size_t)n);
	return 0;
}

static float logsum_here(float a, float b)
{
	const float mx = a > b ? a : b, mn = a > b ? b : a;
	if (mn == -INFINITY || mx - mn >= 15.7f) return mx;
	return mx + td_logsum_table()[(int)((mx - mn) * 1000.0f)];
}

static int check_posteriors(int n_arch, int n_threads, int64_t n_score)
{
	std::vector<float> b((size_t)n_arch * (size_t)n_score);
	uint32_t seed = 31u + (uint32_t)n_arch;
	for (int k = 0; k < n_arch; k++)
		for (int64_t i = 0; i < n_score; i++) b[(size_t)k * (size_t)n_score + (size_t)i] = -40.0f - 0.37f * (float)(rnd(seed) % 64) + 0.05f * (float)k;
	std::vector<float> got((size_t)n_arch, -1.0f), want((size_t)n_arch);
	int32_t best = -7;
	td_arch_posteriors(b.data(), n_arch, n_score, n_threads, got.data(), &best);
	// a thread's share of the reads is summed on its own, from log(1) = 0; the last thread takes what the division leaves over
	for (int k = 0; k < n_arch; k++) {
		float total = 0.0f;
		for (int t = 0; t < n_threads; t++) {
			float part = 0.0f;
			const int64_t share = n_score / n_threads, end = t + 1 == n_threads ? n_score : (t + 1) * share;
			for (int64_t i = t * share; i < end; i++) part += b[(size_t)k * (size_t)n_score + (size_t)i];
			total += part;
		}
		want[(size_t)k] = total;
	}
	int32_t want_best = 0;
	if (n_arch == 1) want[0] = 1.0f;
	else {
		float sum = want[0];
		for (int k = 1; k < n_arch; k++) sum = logsum_here(sum, want[(size_t)k]);
		for (float& w : want) w -= sum;
		sum = -INFINITY;
		for (float w : want) sum = logsum_here(sum, w);
		for (float& w : want) w = w - sum == -INFINITY ? 0.0f : (float)exp((double)(w - sum));
		for (int k = 1; k < n_arch; k++) if (want[(size_t)k] > want[(size_t)want_best]) want_best = k;
		float all = 0.0f;
		for (float w : want) all += w;
		CHECK(fabsf(all - 1.0f) < 1e-3f);
	}
	for (int k = 0; k < n_arch; k++) CHECK(bits(got[(size_t)k]) == bits(want[(size_t)k]));
	CHECK(best == want_best);
	return 0;
}

int main()
{
	// 96 distinct barcodes of six bases, so that the plan's run-time HMM loop (16 HMMs or more) and its H > 32 branches are taken
	std::string many = "B:";
	for (int i = 0; i < 96; i++) {
		if (i) many += ',';
		for (int q = 0, v = i * 37 + 11; q < 6; q++, v /= 4) many += "ACGT"[v % 4];
	}
	if (check_architecture("two barcodes", { "B:ACGT,TTGA", "R:N" }, "ACGT")) return 1;
	if (check_architecture("fingerprint, spacer, read", { "F:NNNN", "S:GTCA", "R:N" }, "ACGTGTCA")) return 1;
	if (check_architecture("every segment letter", { "P:AGGTCTAGCC", "B:ACGTAC,TTGACA,GGATCC", "F:NNNNN", "S:GTA", "O:NN", "G:GG", "R:N", "P:AGATCGGAAGAGC" },
	                       "CTAGCCACGTACAACCTGTA")) return 1;
	if (check_architecture("96 barcodes", { many, "R:N" }, "TGAAAA")) return 1;
	g_err = "what the four architectures reach";
	CHECK(n_prune_runs >= 2 && n_rt_loops >= 1 && n_first_labels >= 1);
	g_err.clear();
	if (check_rejections()) return 1;
	g_err = "length classes";
	if (check_classes(std::vector<int>(12, 40), 1)) return 1;
	if (check_classes(std::vector<int>(5, 0), 1)) return 1;
	{ std::vector<int> l(10, 30); l[3] = l[8] = 45; if (check_classes(l, 2)) return 1; }
	{ std::vector<int> l; for (int i = 0; i < 20; i++) l.push_back(30 + i * 7 % 20); l[11] = 380; if (check_classes(l, 3)) return 1; }
	g_err = "posteriors";
	for (int n_arch : { 1, 3 })
		for (int n_threads : { 1, 3 })
			if (check_posteriors(n_arch, n_threads, 10)) return 1;
	printf("model_host_check: ok\n");
	return 0;
}
