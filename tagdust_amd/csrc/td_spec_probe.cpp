// td_spec_probe.cpp -- the probe reads a freshly loaded model-specialised kernel is checked with (td_spec_host.hip, probe_spec_kernel):
// TD_PROBE_READS reads made from the model description alone, decoded by the new kernel and by the generic ahead-of-time kernel;
// the new kernel takes over only when every byte a caller could see agrees.  Host only, no GPU.
//
// The reads follow the architecture (so that barcodes are found, fingerprints read and reads extracted), leave it (substitutions,
// single-base insertions and deletions, N) or ignore it (one read in eight is uniformly random), and their lengths are ragged
// inside every tile of 64 -- between them they reach the outcomes of extract_reads and the long and the short side of every sweep.
// The numbers come from a private integer generator with a fixed seed, never from the C library's rand(): threshold calibration is
// bound to that sequence (include/tagdust_model.h) and a model upload in the middle of it must not move it.
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/tagdust_hip.h"

namespace {
struct Lcg {
	uint64_t s;
	uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); }   // 31 bits
	uint32_t below(uint32_t n) { return n > 1 ? next() % n : 0; }
	bool one_in(uint32_t n) { return below(n) == 0; }
};

constexpr int kReadSegCap = 256;   // a read segment of the probe has at most this many bases, however long the model's average read

// the base a match column expects, or -1 where its emission says nothing about A, C, G, T (N columns, read segments)
int column_base(const float* e)
{
	int best = 0;
	bool flat = true;
	for (int x = 1; x < 4; x++) {
		if (e[x] != e[0]) flat = false;
		if (e[x] > e[best]) best = x;
	}
	return flat ? -1 : best;
}
}

extern "C" void td_spec_probe_params(float* threshold, int32_t* minlen, int32_t* dust, int32_t* matchstart, int32_t* matchend)
{
	if (threshold) *threshold = TD_PROBE_THRESHOLD;
	if (minlen) *minlen = TD_PROBE_MINLEN;
	if (dust) *dust = TD_PROBE_DUST;
	if (matchstart) *matchstart = TD_PROBE_WIN_START;
	if (matchend) *matchend = TD_PROBE_WIN_END;
}

extern "C" int64_t td_spec_probe(const td_model_desc* m, uint8_t* codes, int64_t cap, int64_t* offs)
{
	if (!m || m->S < 1 || m->S > TD_MAX_SEGMENTS || !m->n_hmm || !m->n_col || !m->seg_type || !m->eM || !m->skip) return -1;
	Lcg g{ 0x7461676475737432ULL };
	std::vector<int> col_off((size_t)m->S);
	int first_read_seg = m->S;
	for (int j = 0, co = 0; j < m->S; co += m->n_hmm[j] * m->n_col[j], j++) {
		if (m->n_hmm[j] < 1 || m->n_col[j] < 1) return -1;
		col_off[(size_t)j] = co;
		if (m->seg_type[j] == 'R' && first_read_seg == m->S) first_read_seg = j;
	}
	int read_cap = m->avg_len < 1 ? 1 : m->avg_len;
	if (read_cap > kReadSegCap) read_cap = kReadSegCap;
	int typical = 0;       // bases of a read that follows the architecture (for the length of the random ones)
	for (int j = 0; j < m->S; j++) typical += m->seg_type[j] == 'R' ? read_cap / 2 + 1 : m->n_col[j];

	std::vector<uint8_t> all;
	std::vector<int64_t> off(TD_PROBE_READS + 1, 0);
	std::vector<uint8_t> rd;
	int n_model = 0;
	for (int r = 0; r < TD_PROBE_READS; r++) {
		rd.clear();
		if ((r & 7) == 7) {
			// uniformly random, now and then with an N
			const int len = 4 + (int)g.below((uint32_t)(2 * typical));
			for (int p = 0; p < len; p++) rd.push_back(g.one_in(50) ? 4 : (uint8_t)g.below(4));
		} else {
			const int k = n_model++;
			int earlier = 1;   // product of the sizes of the barcode segments in front of segment j
			for (int j = 0; j < m->S; j++) {
				const int nh = m->n_hmm[j], nc = m->n_col[j];
				if (!(m->skip[j] == -INFINITY) && g.one_in(4)) continue;   // a segment the model may skip is skipped now and then
				if (m->seg_type[j] == 'R') {
					const int len = 1 + (int)g.below((uint32_t)read_cap);
					for (int p = 0; p < len; p++) rd.push_back((uint8_t)g.below(4));
					continue;
				}
				// every HMM of every multi-HMM segment gets its turn: k % nh.  A second barcode segment would only ever meet the
				// first one's HMM of the same number that way (extract_reads reports the LAST barcode segment), so barcode segments
				// step through their combinations: the first takes k % nh, a later one (k / product of the earlier sizes) % nh
				const bool bseg = m->seg_type[j] == 'B' && nh > 1;
				const int f = (bseg ? k / earlier : k) % nh;
				if (bseg && earlier <= TD_PROBE_READS) earlier *= nh;
				int g0 = 0, g1 = nc;
				if (m->seg_type[j] == 'P' && nc > 1 && g.one_in(2)) {   // a partial segment loses its far end: the 5' one its start
					if (j < first_read_seg) g0 = (int)g.below((uint32_t)nc); else g1 = 1 + (int)g.below((uint32_t)nc);
				}
				for (int c = g0; c < g1; c++) {
					const int b = column_base(m->eM + (size_t)(col_off[(size_t)j] + f * nc + c) * 5);
					rd.push_back(b >= 0 ? (uint8_t)b : (uint8_t)g.below(4));
				}
			}
			// sequencing errors: substitutions, single-base insertions and deletions, N -- three reads in four; the others stay clean
			if ((k & 3) != 0) {
				std::vector<uint8_t> mu;
				for (uint8_t b : rd) {
					const uint32_t u = g.below(200);
					if (u < 4) mu.push_back((uint8_t)((b + 1 + g.below(3)) & 3));       // substitution
					else if (u < 6) { mu.push_back((uint8_t)g.below(4)); mu.push_back(b); }   // insertion
					else if (u < 8) { }                                                  // deletion
					else if (u < 10) mu.push_back(4);                                    // N
					else mu.push_back(b);
				}
				rd.swap(mu);
			}
		}
		while (rd.size() < 4) rd.push_back((uint8_t)g.below(4));   // (every read reaches into the window variant's fixed window)
		if (r == 1) rd[rd.size() / 2] = 4;   // at least one N, whatever the generator drew
		all.insert(all.end(), rd.begin(), rd.end());
		off[(size_t)r + 1] = (int64_t)all.size();
	}
	// ragged inside every tile: a tile whose reads all came out one length gets one base more on its first read
	{
		std::vector<uint8_t> fixed;
		std::vector<int64_t> noff(TD_PROBE_READS + 1, 0);
		for (int t = 0; t < TD_PROBE_READS / 64; t++) {
			bool same = true;
			const int64_t l0 = off[(size_t)t * 64 + 1] - off[(size_t)t * 64];
			for (int q = 1; q < 64; q++) if (off[(size_t)t * 64 + q + 1] - off[(size_t)t * 64 + q] != l0) same = false;
			for (int q = 0; q < 64; q++) {
				const int r = t * 64 + q;
				fixed.insert(fixed.end(), all.begin() + off[(size_t)r], all.begin() + off[(size_t)r + 1]);
				if (same && q == 0) fixed.push_back((uint8_t)g.below(4));
				noff[(size_t)r + 1] = (int64_t)fixed.size();
			}
		}
		all.swap(fixed); off.swap(noff);
	}
	if (offs) memcpy(offs, off.data(), sizeof(int64_t) * (TD_PROBE_READS + 1));
	if (codes && cap >= (int64_t)all.size()) memcpy(codes, all.data(), all.size());
	return (int64_t)all.size();
}
