// td_model_flat.cpp -- see td_model_flat.h.  Plain C++: caller tables in, device tables out.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "td_model_flat.h"
#include "td_model_inner.h"

static bool reject(std::string& why, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	why = buf;
	return false;
}

extern "C" const float* td_logsum_table(void)
{
	// init_logsum(), src/misc.c:57-63: (float) log(1. + exp((double) -i / SCALE)), SCALE = 1000.0f
	struct Table {
		float v[TD_LOGSUM_SIZE];
		Table() { for (int i = 0; i < TD_LOGSUM_SIZE; i++) v[i] = (float)log(1.0 + exp((double)-i / (double)1000.0f)); }
	};
	static const Table t;   // built by the first caller, whichever thread that is
	return t.v;
}

bool td_flatten_model(const td_model_desc* m, TdFlatModel& out, std::string& why)
{
	if (m->S < 1 || m->S > TD_MAX_SEGMENTS) return reject(why, "td_model_upload: %d segments (1..%d supported)", m->S, TD_MAX_SEGMENTS);
	if (m->H < 1 || m->H > TD_MAX_HMMS) return reject(why, "td_model_upload: %d HMMs (1..%d supported)", m->H, TD_MAX_HMMS);
	if (!m->n_hmm || !m->n_col || !m->skip || !m->seg_type || !m->finger_len || !m->trans || !m->eM || !m->eI ||
	    !m->sM || !m->sI || !m->label || !m->A)
		return reject(why, "td_model_upload: NULL table pointer");
	TdModelHeader h{};
	h.S = m->S; h.H = m->H; h.C = m->C; h.avg_len = m->avg_len;
	for (int i = 0; i < 5; i++) h.bg[i] = m->bg[i];
	// random model constants, barcode_hmm.c:4520,4523 (float/double mix exactly as written there)
	h.r_stay = p2sp((float)(1.0 - (1.0 / (double)(float)m->avg_len)));
	h.r_exit = p2sp((float)(1.0 / (double)(float)m->avg_len));
	int co = 0, ho = 0, req = 0, maxc = 0;
	for (int j = 0; j < m->S; j++) {
		if (m->n_hmm[j] < 1 || m->n_col[j] < 1) return reject(why, "td_model_upload: segment %d has %d HMMs x %d columns", j, m->n_hmm[j], m->n_col[j]);
		TdSeg& s = h.seg[j];
		s.n_hmm = m->n_hmm[j]; s.n_col = m->n_col[j]; s.col_off = co; s.hmm_off = ho;
		s.skip = m->skip[j]; s.skip_live = !(m->skip[j] == -INFINITY); s.type = m->seg_type[j];
		co += s.n_hmm * s.n_col; ho += s.n_hmm;
		if (m->seg_type[j] == 'F') req += m->finger_len[j];
		if (s.n_col > maxc) maxc = s.n_col;
	}
	if (co != m->C || ho != m->H) return reject(why, "td_model_upload: inconsistent sizes (columns %d vs C %d, HMMs %d vs H %d)", co, m->C, ho, m->H);
	h.required_finger_len = req;
	h.max_ncol = maxc;

	std::vector<TdCol> cols(m->C);
	for (int k = 0; k < m->C; k++) {
		TdCol& q = cols[k];
		memset(&q, 0, sizeof q);
		uint32_t fl = 0;
		for (int t = 0; t < 9; t++) { q.t[t] = m->trans[k * 9 + t]; if (!(q.t[t] == -INFINITY)) fl |= 1u << t; }
		q.sM = m->sM[k]; if (!(q.sM == -INFINITY)) fl |= TDF_SM;
		q.sI = m->sI[k]; if (!(q.sI == -INFINITY)) fl |= TDF_SI;
		for (int e = 0; e < 5; e++) { q.eM[e] = m->eM[k * 5 + e]; q.eI[e] = m->eI[k * 5 + e]; }
		q.flags = fl;
	}
	// per-HMM info for extract_reads (barcode_hmm.c:3205-3226): type | segment | hmm | decoy
	std::vector<uint32_t> hinfo(m->H);
	for (int hh = 0; hh < m->H; hh++) {
		const int seg = m->label[hh] & 0xFFFF, f = (m->label[hh] >> 16) & 0x7FFF;
		if (seg >= m->S) return reject(why, "td_model_upload: label[%d] names segment %d", hh, seg);
		uint32_t v = (uint32_t)(uint8_t)m->seg_type[seg] | ((uint32_t)seg << 8) | ((uint32_t)f << 16);
		if (m->seg_type[seg] == 'B' && f == m->n_hmm[seg] - 1) v |= 0x80000000u; // all-N decoy, interface.c:521-527
		hinfo[hh] = v;
	}
	// label transition matrix -> predecessor lists (only u < v; staying in v is handled in the kernel)
	std::vector<int32_t> poff(m->H + 1, 0), pidx;
	for (int v = 0; v < m->H; v++) {
		poff[v] = (int32_t)pidx.size();
		for (int u = 0; u < v; u++) {
			const float a = m->A[u * m->H + v];
			if (a != 0.0f && a != 1.0f) return reject(why, "td_model_upload: transition matrix entry [%d][%d] = %g is not 0/1", u, v, a);
			if (a == 1.0f) pidx.push_back(u);
		}
		if (m->A[v * m->H + v] != 1.0f) return reject(why, "td_model_upload: transition matrix diagonal [%d] must be 1", v);
	}
	poff[m->H] = (int32_t)pidx.size();
	if (pidx.empty()) pidx.push_back(0);

	out.h = h;
	out.cols.swap(cols); out.hinfo.swap(hinfo); out.pred_off.swap(poff); out.pred_idx.swap(pidx);
	return true;
}

bool td_pack_artifacts(const uint8_t* string, const int32_t* s_index, int32_t n_seq, std::vector<int32_t>& seq, std::vector<uint32_t>& pk,
                       std::string& why)
{
	for (int32_t j = 0; j < n_seq; j++)
		if (s_index[j + 1] < s_index[j] || s_index[j] < 0) return reject(why, "td_set_artifacts: s_index is not ascending at %d", j);
	// TD_MODE_RNA_DUST reads the text as 2-bit codes (only the low two bits are looked at; the leading 'X' is 'X' & 3 = 0),
	// 16 per dword, every sequence from a dword boundary: one wave-uniform load per 16 characters
	seq.assign((size_t)n_seq * 2, 0);
	size_t words = 0;
	for (int32_t j = 0; j < n_seq; j++) {
		seq[(size_t)j * 2] = (int32_t)words;
		seq[(size_t)j * 2 + 1] = s_index[j + 1] - s_index[j];
		words += (size_t)(s_index[j + 1] - s_index[j] + 15) / 16;
	}
	pk.assign(words + 1, 0u);
	for (int32_t j = 0; j < n_seq; j++)
		for (int32_t q = 0; q < seq[(size_t)j * 2 + 1]; q++)
			pk[(size_t)seq[(size_t)j * 2] + (size_t)(q >> 4)] |= (uint32_t)(string[s_index[j] + q] & 3u) << (2 * (q & 15));
	return true;
}
