// td_spec_plan.cpp -- what the model-specialised kernel is for one model, decided on the host in plain C++: the TD_SPEC_* knobs, the
// plan, the model section (the plan and the model's parameters as constexpr source text) and the workspace layout.  No HIP header,
// no hiprtc and none of the kernel's own source text: td_jit.hip puts the section in front of that text and compiles it; the
// stand-alone program over this unit (tools/model_host_check.cpp) builds with a plain C++ compiler.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "td_jit.h"

static std::string flit(float v)
{
	if (isinf(v)) return v < 0 ? "(-__builtin_inff())" : "__builtin_inff()";
	if (v != v) return "__builtin_nanf(\"\")";
	char buf[64];
	snprintf(buf, sizeof buf, "%af", (double)v); // hex float: exact
	return buf;
}

// Every TD_SPEC_* knob of the kernel, read here and nowhere else: when a model is uploaded, or for a context-free query, and
// then held in that model's plan.  (TD_SPEC_CACHE_DIR names a place, not a property of the kernel: td_spec_cache_dir.)
TdSpecKnobs td_spec_knobs(void)
{
	TdSpecKnobs k;
	auto num = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
	auto flag = [](const char* name, int unset) -> int { const char* e = getenv(name); return e ? atoi(e) != 0 : unset; };   // unset may be -1
	if (const int v = num("TD_SPEC_BLOCK", 0); v >= 64 && v <= 1024 && v % 64 == 0) k.block = v;
	if (const int v = num("TD_SPEC_MINWAVES", 0); v >= 1 && v <= 8) k.min_waves = v;
	if (const int v = num("TD_SPEC_GROUPCOLS", 0); v > 0) k.groupcols = v;
	k.groupcols_fwd = num("TD_SPEC_GROUPCOLS_FWD", k.groupcols_fwd);
	k.rt_min = num("TD_SPEC_RT_MIN", k.rt_min);
	k.trie_sh = num("TD_SPEC_TRIE_SH", k.trie_sh);
	k.profile = num("TD_SPEC_PROFILE", k.profile);
	k.lsum_oob = flag("TD_SPEC_LSUM_OOB", k.lsum_oob);
	k.prune = flag("TD_SPEC_PRUNE", k.prune);
	k.prune_sfx = flag("TD_SPEC_PRUNE_SFX", k.prune_sfx);
	k.restart = flag("TD_SPEC_RESTART", k.restart);
	k.firstseg = flag("TD_SPEC_FIRSTSEG", k.firstseg);
	k.prune_stats = flag("TD_SPEC_PRUNE_STATS", k.prune_stats);
	if (const char* e = getenv("TD_SPEC_EXTRA_OPTS")) k.extra_opts = e;
	return k;
}

namespace {
// A last column whose backward values are just P[i+1] + MSKIP / P[i+1] + ISKIP (no live IM / II term, barcode_hmm.c:
// 3522-3534) is not spilled: the forward sweep recomputes it from the next segment's silent row.  Must hold for every
// HMM of the segment so that the spill layout stays regular.
int pure_last(const td_model_desc* m, int j, int col_off)
{
	for (int f = 0; f < m->n_hmm[j]; f++) {
		const int q = col_off + f * m->n_col[j] + m->n_col[j] - 1;
		if (!(m->trans[q * 9 + 4] == -INFINITY) || !(m->trans[q * 9 + 3] == -INFINITY)) return 0;
	}
	return 1;
}

// Run-time HMM loop eligibility of segment j: the longest prefix of HMMs that share every transition / entry / insert
// emission with HMM 0 and whose match columns are all "one base high, other three low, N separate" with the same three
// values.  Returns the prefix length (0 if the segment has fewer than min_hmms or is not of that shape); fills base codes and hi/lo/nv.
int rt_prefix(const td_model_desc* m, int j, int col_off, int* base /* [C] */, float* hi, float* lo, float* nv, int min_hmms)
{
	const int n = m->n_hmm[j], nc = m->n_col[j];
	if (n < min_hmms) return 0;
	auto match_type = [&](int q, int* b, float* h, float* l, float* v) -> bool {
		const float* e = m->eM + (size_t)q * 5;
		for (int x = 0; x < 4; x++) {
			const float other = e[(x + 1) & 3];
			bool ok = !(e[x] == other);
			for (int y = 0; y < 4 && ok; y++) if (y != x && !(e[y] == other)) ok = false;
			if (ok) { *b = x; *h = e[x]; *l = other; *v = e[4]; return true; }
		}
		return false;
	};
	int b0; float h0, l0, v0;
	if (!match_type(col_off, &b0, &h0, &l0, &v0)) return 0;
	int f = 0;
	for (; f < n; f++) {
		bool ok = true;
		for (int g = 0; g < nc && ok; g++) {
			const int q = col_off + f * nc + g, q0 = col_off + g;
			if (memcmp(m->trans + (size_t)q * 9, m->trans + (size_t)q0 * 9, 36) || memcmp(m->eI + (size_t)q * 5, m->eI + (size_t)q0 * 5, 20) ||
			    memcmp(&m->sM[q], &m->sM[q0], 4) || memcmp(&m->sI[q], &m->sI[q0], 4)) { ok = false; break; }
			int b; float h, l, v;
			if (!match_type(q, &b, &h, &l, &v) || memcmp(&h, &h0, 4) || memcmp(&l, &l0, 4) || memcmp(&v, &v0, 4)) { ok = false; break; }
			base[q] = b;
		}
		if (!ok) break;
	}
	*hi = h0; *lo = l0; *nv = v0;
	return f >= min_hmms ? f : 0;
}

// HMMs swept together per position pass, evenly sized groups of about `target` columns.
int group_size(int n_hmm, int n_col, int target)
{
	int maxf = target / n_col;
	if (maxf < 1) maxf = 1;
	if (maxf > n_hmm) maxf = n_hmm;
	const int groups = (n_hmm + maxf - 1) / maxf;
	return (n_hmm + groups - 1) / groups;
}

// Labels of the first segment when none of them has a predecessor and every later label has either all of them or
// none as predecessors (the usual case: barcodes first): their label-DP value is a plain running sum of their
// posteriors, kept in a register by the forward sweep; later labels only need the running maximum over them (one
// float + one byte per position, td_spec_kernel.inc), so their posteriors are never stored.
int first_labels(const td_model_desc* m, int firstseg)
{
	// Measured on MI355X: +26 % on config 5 (96 barcodes, H = 100: the label DP leaves the workspace for registers),
	// -1 % on config 3 (8 barcodes) and -10 % on config 2, where the extra row costs more than the posteriors it replaces
	// -- so it is used when the label DP would not fit the register path otherwise.  TD_SPEC_FIRSTSEG=0 / 1 forces it.
	const int H = m->H, n0 = m->n_hmm[0];
	const int mode = firstseg >= 0 ? firstseg : H > 32;
	if (!mode) return 0;
	if (n0 < 2 || n0 >= H) return 0;
	for (int v = 0; v < n0; v++)
		for (int u = 0; u < v; u++) if (m->A[u * H + v] == 1.0f) return 0;
	for (int w = n0; w < H; w++) {
		int c = 0;
		for (int u = 0; u < n0; u++) c += m->A[u * H + w] == 1.0f;
		if (c != 0 && c != n0) return 0;
	}
	return n0;
}

// A "read-like" segment: one HMM of one column whose match state cannot be entered or left (every transition but II and
// ISKIP is -inf), entered through its insert state, with an insert self-loop and an exit -- barcode_hmm.c:5042-5082 builds
// every R segment like that.
bool read_like(const td_model_desc* m, int j, int co)
{
	if (m->n_hmm[j] != 1 || m->n_col[j] != 1) return false;
	const float* t = m->trans + (size_t)co * 9;
	for (int k = 0; k < 9; k++) if (k != TD_II && k != TD_ISKIP && t[k] > -INFINITY) return false;
	return m->sM[co] == -INFINITY && m->sI[co] > -INFINITY && t[TD_II] > -INFINITY && t[TD_ISKIP] > -INFINITY;
}
}

// What the kernel is for this model under these knobs.  Everything that generates source, lays out the workspace, fills the
// bound tables or answers "prune_active" reads it from here.
TdSpecPlan td_spec_plan(const td_model_desc* m, const TdSpecKnobs& k)
{
	TdSpecPlan p;
	const int S = m->S, H = m->H, C = m->C;
	p.k = k; p.S = S; p.H = H; p.C = C;
	p.col_off.resize(S); p.hmm_off.resize(S);
	for (int j = 0, co = 0, ho = 0; j < S; co += m->n_hmm[j] * m->n_col[j], ho += m->n_hmm[j], j++) { p.col_off[j] = co; p.hmm_off[j] = ho; }
	// Group sizes.  Measured on MI355X (configs 2, 3, 5) at 4 waves/SIMD:
	// 18 columns in the backward sweep (fewer passes over the silent rows; its carried state is only Mn/In) and 12 in
	// the forward sweep (which also holds the reloaded backward rows) -- +2 % over 12/12; 8 and 24+/24+ are slower.
	p.group.resize(S); p.group_f.resize(S); p.pure_last.resize(S); p.drop_m.resize(S); p.bw_off.resize(H);
	for (int j = 0; j < S; j++) {
		p.group[j] = group_size(m->n_hmm[j], m->n_col[j], k.groupcols);
		p.group_f[j] = group_size(m->n_hmm[j], m->n_col[j], k.groupcols_fwd > 0 ? k.groupcols_fwd : k.groupcols);
		p.pure_last[j] = pure_last(m, j, p.col_off[j]);
	}
	// spill layout in half-columns (4 B per lane and position): a stored column is (M_backward, I_backward) = 2; the column
	// before a pure last column keeps only its I_backward (kDropM) -- its M_backward is one logsum chain over the next
	// position's I_backward of the same column and two silent-row values the forward sweep holds anyway
	int cols = 0;
	for (int j = 0; j < S; j++) {
		p.drop_m[j] = m->n_col[j] >= 2 && p.pure_last[j];
		for (int f = 0; f < m->n_hmm[j]; f++) { p.bw_off[p.hmm_off[j] + f] = cols; cols += 2 * (m->n_col[j] - p.pure_last[j]) - p.drop_m[j]; }
	}
	p.halves = cols;
	p.rt.assign(S, 0); p.rt_b.assign(S, 0); p.base.assign(C, 0);
	p.hi.assign(S, 0.0f); p.lo.assign(S, 0.0f); p.nv.assign(S, 0.0f);
	for (int j = 0; j < S; j++) {
		const int pre = rt_prefix(m, j, p.col_off[j], p.base.data(), &p.hi[j], &p.lo[j], &p.nv[j], k.rt_min);
		if (pre > 0) {
			p.group_f[j] = p.group[j];                       // one group size for both sweeps of a run-time-looped segment
			p.rt[j] = pre / p.group[j] * p.group[j];
			p.rt_b[j] = p.rt[j];
		} else {
			// the bridges of the restarted sweeps run one HMM at a time: any two HMMs of that shape share one loop body there
			p.rt_b[j] = rt_prefix(m, j, p.col_off[j], p.base.data(), &p.hi[j], &p.lo[j], &p.nv[j], 2);
		}
	}
	// Suffix ("trie") order of a run-time-looped FIRST segment's backward sweep (td_spec_kernel.inc, bwd_group): HMMs that expect the
	// same bases in their last SH match columns have the same floats in the rows of their last SH + 1 columns; groups of kGroup such
	// HMMs compute them once.  trie_ord: slot -> HMM, the sharing groups first (trie_n_share of them), the left-overs behind.
	{
		const int sh = k.trie_sh;
		bool on = p.rt[0] > 0 && sh >= 1 && m->n_col[0] >= sh + 2;
		std::vector<int> ord;
		int n_share = 0;
		if (on) {
			const int G = p.group[0], NC0 = m->n_col[0];
			std::map<std::vector<int>, std::vector<int>> cls;     // last sh bases -> HMMs (ascending)
			for (int f = 0; f < p.rt[0]; f++) {
				std::vector<int> key;
				for (int g = NC0 - sh; g < NC0; g++) key.push_back(p.base[(size_t)(p.col_off[0] + f * NC0 + g)]);
				cls[key].push_back(f);
			}
			std::vector<int> left;
			for (auto& kv : cls) {
				const std::vector<int>& v = kv.second;
				const size_t full = v.size() / (size_t)G * (size_t)G;
				for (size_t i = 0; i < full; i++) ord.push_back(v[i]);
				for (size_t i = full; i < v.size(); i++) left.push_back(v[i]);
			}
			n_share = (int)ord.size() / G;
			for (int f : left) ord.push_back(f);
			if (n_share == 0) on = false;
		}
		if (!on) { ord.assign(1, 0); n_share = 0; }
		p.trie_on = on; p.trie_sh = on ? sh : 1; p.trie_n_share = n_share; p.trie_ord = ord;
	}
	p.first_n = first_labels(m, k.firstseg);
	// Position pruning (td_spec_kernel.inc, "Position pruning").  prune_segs: the leading segments the forward sweep may cut short,
	// everything in front of the first read-like segment (0: none).  sfx_first: first of the trailing segments whose backward sweep
	// may stop early, everything behind the last read-like segment, if each of those segments has a single HMM (total_prob of a
	// multi-HMM segment would need its own argument; S: none).
	p.prune_segs = 0; p.sfx_first = S;
	if (k.prune && H - p.first_n <= 32) {   // the posterior-row bits (kMaskDP) say which rows exist
		int first = -1, last = -1;
		for (int j = 0; j < S; j++) if (read_like(m, j, p.col_off[j])) { if (first < 0) first = j; last = j; }
		if (first > 0) p.prune_segs = first;
		bool single = k.prune_sfx && last >= 0 && last < S - 1;
		for (int j = last + 1; single && j < S; j++) if (m->n_hmm[j] != 1) single = false;
		if (single) p.sfx_first = last + 1;
	}
	p.prune_z = td_spec_prune_z(m, p.prune_segs, p.sfx_first);
	// The restarted sweeps pay when the bridged segments are big (config 5: 97 barcode HMMs in a run-time loop, -9 %; config 3: nine
	// 6-column barcode HMMs and a 3-column spacer, 60 columns, 19.1 -> 18.7 ms per 2^20 reads); for config 2's eight 4-column HMMs
	// (32 columns, 100-base reads) the bridges -- one HMM at a time -- cost more than the dense positions they replace (13.1 -> 13.3).
	// TD_SPEC_RESTART=0 / 1 forces it.
	if (p.prune_segs <= 0 || p.prune_segs > TD_PRUNE_RESTART_MAX || (p.sfx_first < S && S - p.sfx_first > TD_PRUNE_RESTART_MAX)) p.restart = 0;
	else if (k.restart >= 0) p.restart = k.restart;
	else p.restart = p.col_off[p.prune_segs] >= 48;
	return p;
}

// The model section: the plan and the model's parameters, stated as constexpr data in front of td_spec_kernel.inc.
std::string td_spec_model_section(const td_model_desc* m, const TdSpecPlan& p, int lsum_oob, int window)
{
	std::string s;
	char buf[256];
	const int S = m->S, H = m->H, C = m->C;
	int req = 0;
	for (int j = 0; j < S; j++) if (m->seg_type[j] == 'F') req += m->finger_len[j];
	// 512 threads = 8 waves share one LDS copy of the logsum table; two such workgroups per CU = 4 waves per SIMD
	snprintf(buf, sizeof buf, "#define TDS_BLOCK %d\n#define TDS_MIN_WAVES %d\n", p.k.block, p.k.min_waves);
	s += buf;
	snprintf(buf, sizeof buf, "#define TDS_LSUM_OOB %d\n", lsum_oob != 0);
	s += buf;
	// -start / -end windows are rare: the window arithmetic is only compiled in for a context that has one set, so the
	// usual kernel keeps its register budget
	snprintf(buf, sizeof buf, "#define TDS_WINDOW %d\n", window != 0);
	s += buf;
	snprintf(buf, sizeof buf, "#define TDS_PROFILE %d\n", p.k.profile);
	s += buf;
	snprintf(buf, sizeof buf, "#define TD_S %d\n#define TD_H %d\n#define TD_C %d\n#define TD_REQ_FINGER %d\n", S, H, C, req);
	s += buf;
	s += "struct GCol { float t[9]; float sM, sI; float eM[5]; float eI[5]; };\n";
	auto int_array = [&](const char* name, const std::vector<int>& v) {
		s += std::string("static constexpr int ") + name + "[" + std::to_string(v.size()) + "] = {";
		for (size_t i = 0; i < v.size(); i++) { s += std::to_string(v[i]); if (i + 1 < v.size()) s += ","; }
		s += "};\n";
	};
	int_array("kNHmm", std::vector<int>(m->n_hmm, m->n_hmm + S)); int_array("kNCol", std::vector<int>(m->n_col, m->n_col + S));
	int_array("kColOff", p.col_off); int_array("kHmmOff", p.hmm_off);
	int_array("kRtB", p.rt_b);
	s += std::string("static constexpr bool kTrieOn = ") + (p.trie_on ? "true" : "false") + ";\n";
	s += "static constexpr int kTrieSH = " + std::to_string(p.trie_sh) + ";\n";
	s += "static constexpr int kTrieNShare = " + std::to_string(p.trie_n_share) + ";\n";
	int_array("kTrieOrd", p.trie_ord);
	int_array("kGroup", p.group); int_array("kGroupF", p.group_f); int_array("kPureLast", p.pure_last); int_array("kDropM", p.drop_m); int_array("kBwOff", p.bw_off);
	int_array("kRt", p.rt); int_array("kBase", p.base);
	auto float_array = [&](const char* name, const std::vector<float>& v) {
		s += std::string("static constexpr float ") + name + "[" + std::to_string(v.size()) + "] = {";
		for (size_t i = 0; i < v.size(); i++) { s += flit(v[i]); if (i + 1 < v.size()) s += ","; }
		s += "};\n";
	};
	float_array("kHi", p.hi); float_array("kLo", p.lo); float_array("kNv", p.nv);
	s += "static constexpr float kSkip[" + std::to_string(S) + "] = {";
	for (int j = 0; j < S; j++) { s += flit(m->skip[j]); if (j + 1 < S) s += ","; }
	s += "};\n";
	s += "static constexpr float kBg[5] = {";
	for (int i = 0; i < 5; i++) { s += flit(m->bg[i]); if (i < 4) s += ","; }
	s += "};\n";
	// random model constants, barcode_hmm.c:4520,4523 (float/double mix exactly as written there)
	const float stay_arg = (float)(1.0 - (1.0 / (double)(float)m->avg_len));
	const float exit_arg = (float)(1.0 / (double)(float)m->avg_len);
	s += "static constexpr float kRStay = " + flit(stay_arg == 0.0f ? -INFINITY : (float)log((double)stay_arg)) + ";\n";
	s += "static constexpr float kRExit = " + flit(exit_arg == 0.0f ? -INFINITY : (float)log((double)exit_arg)) + ";\n";
	s += "static constexpr GCol kCols[" + std::to_string(C) + "] = {\n";
	for (int k = 0; k < C; k++) {
		s += " {{";
		for (int t = 0; t < 9; t++) { s += flit(m->trans[k * 9 + t]); if (t < 8) s += ","; }
		s += "}," + flit(m->sM[k]) + "," + flit(m->sI[k]) + ",{";
		for (int e = 0; e < 5; e++) { s += flit(m->eM[k * 5 + e]); if (e < 4) s += ","; }
		s += "},{";
		for (int e = 0; e < 5; e++) { s += flit(m->eI[k * 5 + e]); if (e < 4) s += ","; }
		s += "}},\n";
	}
	s += "};\n";
	s += "static constexpr unsigned kHinfo[" + std::to_string(H) + "] = {";
	for (int h = 0; h < H; h++) {
		const int seg = m->label[h] & 0xFFFF, f = (m->label[h] >> 16) & 0x7FFF;
		unsigned v = (unsigned)(unsigned char)m->seg_type[seg] | ((unsigned)seg << 8) | ((unsigned)f << 16);
		if (m->seg_type[seg] == 'B' && f == m->n_hmm[seg] - 1) v |= 0x80000000u;
		snprintf(buf, sizeof buf, "0x%08xu%s", v, h + 1 < H ? "," : "");
		s += buf;
	}
	s += "};\n";
	std::vector<int> poff(H + 1, 0), pidx;
	for (int v = 0; v < H; v++) {
		poff[v] = (int)pidx.size();
		for (int u = 0; u < v; u++) if (m->A[u * H + v] == 1.0f) pidx.push_back(u);
	}
	poff[H] = (int)pidx.size();
	if (pidx.empty()) pidx.push_back(0);
	int_array("kPredOff", poff); int_array("kPredIdx", pidx);
	// the predecessor lists without the first segment's labels (first_labels): kPredFirst says which labels had them
	const int first_n = p.first_n;
	std::vector<int> pfirst(H, 0), poff2(H + 1, 0), pidx2;
	for (int v = 0; v < H; v++) {
		poff2[v] = (int)pidx2.size();
		for (int i = poff[v]; i < poff[v + 1]; i++) {
			if (pidx[i] < first_n) pfirst[v] = 1; else pidx2.push_back(pidx[i]);
		}
	}
	poff2[H] = (int)pidx2.size();
	if (pidx2.empty()) pidx2.push_back(0);
	s += "static constexpr int kFirstN = " + std::to_string(first_n) + ";\n";
	int_array("kPredFirst", pfirst); int_array("kPredOff2", poff2); int_array("kPredIdx2", pidx2);
	// runs of consecutive labels (from first_n on) with one and the same predecessor set: the many-label path of the
	// label DP finds the best predecessor once per run
	std::vector<int> runs;
	for (int v = first_n; v < H; v++) {
		bool same = v > first_n && pfirst[v] == pfirst[v - 1] && poff2[v + 1] - poff2[v] == poff2[v] - poff2[v - 1];
		for (int k = 0; same && k < poff2[v + 1] - poff2[v]; k++) same = pidx2[poff2[v] + k] == pidx2[poff2[v - 1] + k];
		if (!same) runs.push_back(v - first_n);
	}
	runs.push_back(H - first_n);
	s += "static constexpr int kPruneSegs = " + std::to_string(p.prune_segs) + ";\n";
	s += "static constexpr int kSfxFirst = " + std::to_string(p.sfx_first) + ";\n";
	s += "static constexpr float kPruneZ = " + flit(p.prune_z) + ";\n";
	if (p.k.prune_stats >= 0) s += std::string("#define TDS_PRUNE_STATS ") + (p.k.prune_stats ? "1" : "0") + "\n";
	s += std::string("#ifndef TDS_RESTART\n#define TDS_RESTART ") + (p.restart ? "1" : "0") + "\n#endif\n";
	s += "static constexpr int kNRuns = " + std::to_string((int)runs.size() - 1) + ";\n";
	int_array("kRunOff", runs);
	return s;
}

void td_spec_layout(TdSpecLayout& L, const TdSpecPlan& p, int lmax)
{
	auto al = [](int64_t v) { return (v + 255) & ~(int64_t)255; };
	int64_t o = 0;
	L.codes = o; o = al(o + (int64_t)(lmax + 2) * TD_WAVE);
	L.sb = o;    o = al(o + (int64_t)(p.S + 1) * (lmax + 2) * TD_WAVE * 4);
	L.sf = o;    o = al(o + (int64_t)(p.S + 1) * (lmax + 2) * TD_WAVE * 4);
	L.bw = o;    o = al(o + p.halves * lmax * TD_WAVE * 4 + 1024);
	L.dp = o;    o = al(o + (int64_t)lmax * p.H * TD_WAVE * 4);
	L.path = o;  o = al(o + (int64_t)lmax * ((p.H + 3) / 4) * TD_WAVE * 4);
	L.total = o; o = al(o + (int64_t)p.H * TD_WAVE * 4);
	L.rs = o;    o = al(o + (int64_t)2 * p.C * TD_WAVE * 4);   // hand-over rows of the restarted sweeps (position pruning)
	L.bm = o;    o = al(o + (int64_t)(lmax + 2) * TD_WAVE * 4);   // running maximum over the first segment's label sums
	L.ba = o;    o = al(o + (int64_t)(lmax + 2) * TD_WAVE);       // and the label that holds it
	L.acc = o;   o = al(o + (int64_t)2 * p.H * TD_WAVE * 4);   // two label-DP rows (previous / current position)
	L.pmask = o; o = al(o + (int64_t)p.H * ((lmax + 31) / 32) * 4);   // which posterior rows were stored
	L.slot_bytes = o;
}
