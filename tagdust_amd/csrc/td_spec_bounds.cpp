// td_spec_bounds.cpp -- the bound tables of the model-specialised kernel's position pruning and restarted sweeps
// (td_spec_kernel.inc, "Position pruning" / "Restarted sweeps"): plain host arithmetic in double, no device code.
#include <math.h>

#include <algorithm>
#include <vector>

#include "td_jit.h"

namespace {
// Spacing of the floats around v (the binade |v| lies in): what one float addition whose result is near v can be off by is half of it.
// The kernel's additions are monotone (v <= B  =>  fl(v + c) <= fl(B + c) <= B + c + ulp32(B + c) / 2), so the rounding a bound has to
// absorb is that of the BOUND's own magnitude, whatever the magnitude of the value below it.
inline double ulp32(double v)
{
	const double a = fabs(v);
	if (!(a >= 1.17549435e-38)) return 1.4012984643e-45;
	if (!(a < 3.0e38)) return 0.0;          // (-inf / the -3e38 floor of an unreachable state)
	int e;
	(void)frexp(a, &e);                     // a = m * 2^e, m in [0.5, 1)
	return ldexp(1.0, e - 24);
}
// Float rounding of the (up to four) additions that form a row value around a fold, for a row whose bound is v: a fixed part that
// covers short reads many times over, plus two spacings of v -- scores grow by ~1.4 nats per base, so beyond ~1500 bases half a
// spacing per addition (2.4e-4 at |v| = 4096) is more than any fixed number of this size covers.
inline double row_slack(double v) { return 2.0e-4 + 2.0 * ulp32(v); }
// log(e^a + e^b) plus what the reference's table form can add to it.  The table is indexed with the truncated difference
// (src/misc.c:72-78): its entry exceeds the exact term by < 5e-4, by < 1e-3 when the rounding of a - b moves the index down one
// more step.  On top of that the float rounding of the result's own addition (max + entry) and of the additions that formed the
// two operands: each operand's error enters with its weight in the sum, 1 for the larger, e^-d for the smaller.
inline double lse_up(double a, double b)
{
	if (a == -INFINITY) return b;
	if (b == -INFINITY) return a;
	const double mx = a > b ? a : b, mn = a > b ? b : a, d = mx - mn;
	const double wsm = d > 50.0 ? 0.0 : exp(-d);
	return mx + (d > 50.0 ? 0.0 : log1p(wsm)) + 1.0e-3 + 2.0 * ulp32(mx) + 2.0 * ulp32(mn) * wsm;
}
inline double emax(const float* e) { double v = e[0]; for (int x = 1; x < 5; x++) if (e[x] > v) v = e[x]; return v; }
// double -> float, rounded UP: every table entry is an upper bound or a threshold a value has to reach
inline float clampf(double v)
{
	if (!(v > -3.0e38)) return -3.0e38f;
	float f = (float)v;
	if ((double)f < v) f = nextafterf(f, INFINITY);
	return f;
}
inline double T(const td_model_desc* m, int q, int k) { return (double)m->trans[(size_t)q * 9 + k]; }

// The two recurrences, one segment at a time: the reference's (forward: barcode_hmm.c:4213-4344, backward: :3505-3607, as the
// kernel folds them) with every emission at its maximum over the five base codes and lse_up() for logsum.  co = the segment's
// first column, run = the skips accumulated up to and including segment j, L = positions.  peak, if given, is raised to every
// M / I value of the segment.

// Forward: P bounds the silent row the segment is entered from, Pn receives the row it leaves; peak is indexed by position.
void fwd_sweep(const td_model_desc* m, int j, int co, double run, int L, const std::vector<double>& P, std::vector<double>& Pn, double* peak)
{
	const int NC = m->n_col[j], NH = m->n_hmm[j];
	std::fill(Pn.begin(), Pn.end(), -INFINITY);
	Pn[0] = run;
	std::vector<double> Mp((size_t)NH * NC, -INFINITY), Ip((size_t)NH * NC, -INFINITY), Mc(NC), Ic(NC);
	for (int i = 1; i <= L; i++) {
		const double Pm = P[i - 1], Pi = P[i];
		double cs = -INFINITY;
		for (int f = 0; f < NH; f++) {
			const int q0 = co + f * NC;
			double* mp = &Mp[(size_t)f * NC]; double* ip = &Ip[(size_t)f * NC];
			double Dc = -INFINITY;
			for (int g = 0; g < NC; g++) {
				const int q = q0 + g, qp = q - 1;
				double M = Pm + m->sM[q], I = Pm + m->sI[q];
				if (g > 0) {
					M = lse_up(M, mp[g - 1] + T(m, qp, TD_MM));
					M = lse_up(M, ip[g - 1] + T(m, qp, TD_IM));
					const double D = lse_up(Mc[g - 1] + T(m, qp, TD_MD), Dc + T(m, qp, TD_DD));
					M = lse_up(M, Dc + T(m, qp, TD_DM));
					Dc = D;
				}
				I = lse_up(I, ip[g] + T(m, q, TD_II));
				I = lse_up(I, mp[g] + T(m, q, TD_MI));
				M += emax(m->eM + (size_t)q * 5); M += row_slack(M); I += emax(m->eI + (size_t)q * 5); I += row_slack(I);
				Mc[g] = M; Ic[g] = I;
				cs = lse_up(cs, M + T(m, q, TD_MSKIP));
				cs = lse_up(cs, I + T(m, q, TD_ISKIP));
				if (peak) { if (M > peak[i]) peak[i] = M; if (I > peak[i]) peak[i] = I; }
			}
			cs = lse_up(cs, Pi + (double)m->skip[j]);
			for (int g = 0; g < NC; g++) { mp[g] = Mc[g]; ip[g] = Ic[g]; }
		}
		Pn[i] = cs + row_slack(cs);
	}
}

// Backward, for a read of L bases: Q bounds the silent row the segment leaves into (Q[L + 1] = behind the read), Qn receives the
// row in front of it; a value at position i has L - i bases to go, which is what peak is indexed by.
void bwd_sweep(const td_model_desc* m, int j, int co, double run, int L, const std::vector<double>& Q, std::vector<double>& Qn, double* peak)
{
	const int NC = m->n_col[j], NH = m->n_hmm[j], K = NC - 1;
	std::fill(Qn.begin(), Qn.end(), -INFINITY);
	Qn[L + 1] = run;
	std::vector<double> Mn((size_t)NH * NC, -INFINITY), In((size_t)NH * NC, -INFINITY), Mc(NC), Ic(NC);
	for (int i = L; i >= 1; i--) {
		const double Pnx = Q[i + 1], Pi = Q[i];
		double cs = -INFINITY;
		for (int f = 0; f < NH; f++) {
			const int q0 = co + f * NC;
			double* mn = &Mn[(size_t)f * NC]; double* in = &In[(size_t)f * NC];
			auto EM = [&](int g) { return emax(m->eM + (size_t)(q0 + g) * 5); };
			auto EI = [&](int g) { return emax(m->eI + (size_t)(q0 + g) * 5); };
			double Dp = -INFINITY;
			{
				const int q = q0 + K;
				Mc[K] = Pnx + T(m, q, TD_MSKIP); Mc[K] += row_slack(Mc[K]);
				double I = Pnx + T(m, q, TD_ISKIP);
				I = lse_up(I, mn[K] + T(m, q, TD_IM) + EM(K));
				I = lse_up(I, in[K] + T(m, q, TD_II) + EI(K));
				Ic[K] = I + row_slack(I);
			}
			for (int g = K - 1; g >= 0; g--) {
				const int q = q0 + g;
				const double epc = EM(g + 1), eic = EI(g);
				double M = mn[g + 1] + epc + T(m, q, TD_MM);
				double I = in[g] + T(m, q, TD_II) + eic;
				M = lse_up(M, Pnx + T(m, q, TD_MSKIP)); I = lse_up(I, Pnx + T(m, q, TD_ISKIP));
				M = lse_up(M, in[g] + eic + T(m, q, TD_MI)); I = lse_up(I, mn[g + 1] + T(m, q, TD_IM) + epc);
				double D = Dp + T(m, q, TD_DD);
				M = lse_up(M, Dp + T(m, q, TD_MD));
				D = lse_up(D, Mc[g + 1] + EM(g + 1) + T(m, q, TD_DM));
				Mc[g] = M + row_slack(M); Ic[g] = I + row_slack(I); Dp = D + row_slack(D);
			}
			for (int g = K; g >= 0; g--) {
				const int q = q0 + g;
				cs = lse_up(cs, Mc[g] + (double)m->sM[q] + EM(g));
				cs = lse_up(cs, Ic[g] + (double)m->sI[q] + EI(g));
				if (peak) { if (Mc[g] > peak[L - i]) peak[L - i] = Mc[g]; if (Ic[g] > peak[L - i]) peak[L - i] = Ic[g]; }
			}
			cs = lse_up(cs, Pi + (double)m->skip[j]);
			for (int g = 0; g < NC; g++) { mn[g] = Mc[g]; in[g] = Ic[g]; }
		}
		Qn[i] = cs + row_slack(cs);
	}
}
}

// Zero-posterior bound: every term of a posterior fold is below -kPruneZ, the fold of 2 * columns terms then below -103.98
float td_spec_prune_z(const td_model_desc* m, int n_seg, int sfx_first)
{
	int ncmax = 1;
	for (int j = 0; j < m->S; j++) if ((j < n_seg || j >= sfx_first) && m->n_col[j] > ncmax) ncmax = m->n_col[j];
	return (float)(103.98 + log(2.0 * ncmax) + 2.0e-3 * 2.0 * ncmax + 0.25);
}

// TD_PRUNE_TABLES tables of `stride` floats (stride >= lcap + 2), for positions / distances up to lcap.
// Leading segments j < n_seg = p.prune_segs (forward sweep cut short):
//   fb[i]   >= every forward value (M, I of every column) of those segments at position i, for ANY read
//   bwb[m]  >= every backward value of those segments with m bases to go (position len - m), for ANY read
//   wa[i]   = 15.75 + bound on P[i-1] + sI of segment n_seg (a read segment): its entry term at position i
//   wb[i]   = 15.75 + bound on P[i] + skip of that segment                      (-FLT_MAX if it has no skip)
// Trailing segments j >= sfx_first = p.sfx_first (backward sweep cut short):
//   fbs[i], bws[m]   the same two bounds for those segments
//   wc[m]   = 15.75 + bound on P_next[i+1] + ISKIP of segment sfx_first - 1 (a read segment) with m = len - i - 1: its exit
//             term at position i
//   wd[m]   = 15.75 + bound on P_next[i] + skip of that segment with m = len - i   (-FLT_MAX if it has no skip)
// The bounds are the reference's recurrences (fwd_sweep, bwd_sweep): monotone in every operand, so by induction over the
// recurrence each bound dominates the value the kernel (or the reference) computes in float for any read.
void td_spec_prune_tables(const td_model_desc* m, const TdSpecPlan& p, int lcap, int stride, std::vector<float>& tab)
{
	const int S = m->S, L = lcap, n_seg = p.prune_segs, sfx_first = p.sfx_first;
	const std::vector<int>& col_off = p.col_off;
	tab.assign((size_t)TD_PRUNE_TABLES * stride, -3.0e38f);
	float* fbt = tab.data(); float* bwt = fbt + stride; float* wa = bwt + stride; float* wb = wa + stride;
	float* fbs = wb + stride; float* bws = fbs + stride; float* wc = bws + stride; float* wd = wc + stride;
	// ---- forward bounds ----
	std::vector<double> P(L + 2, -INFINITY), Pn(L + 2, -INFINITY), fb(L + 2, -INFINITY), fs(L + 2, -INFINITY);
	P[0] = 0.0;
	double run = 0.0;
	const int jf_end = sfx_first < S ? S : n_seg;   // segments the forward bound has to walk through
	auto entry_thresholds = [&]() {   // P bounds the silent row segment n_seg is entered from
		const int q = col_off[n_seg];
		for (int i = 1; i <= L; i++) {
			wa[i] = clampf(P[i - 1] + (double)m->sI[q] + 15.75);
			wb[i] = m->skip[n_seg] > -INFINITY ? clampf(P[i] + (double)m->skip[n_seg] + 15.75) : -3.0e38f;
		}
		wa[0] = wb[0] = 3.0e38f;
	};
	for (int j = 0; j < jf_end; j++) {
		if (j == n_seg && n_seg > 0) entry_thresholds();
		run += (double)m->skip[j];
		fwd_sweep(m, j, col_off[j], run, L, P, Pn, j < n_seg ? fb.data() : j >= sfx_first ? fs.data() : nullptr);
		P.swap(Pn);
	}
	if (jf_end == n_seg && n_seg > 0) entry_thresholds();
	for (int i = 1; i <= L; i++) { fbt[i] = clampf(fb[i] + 1.0e-3); fbs[i] = clampf(fs[i] + 1.0e-3); }
	fbt[0] = fbs[0] = 3.0e38f;   // (position 0 does not exist)
	// ---- backward bounds: a read of L bases; a value at position i has m = L - i bases to go ----
	std::vector<double> bw(L + 2, -INFINITY), bs(L + 2, -INFINITY);
	std::vector<double> Q(L + 3, -INFINITY), Qn(L + 3, -INFINITY);
	Q[L + 1] = 0.0;   // previous_silent, barcode_hmm.c:3476-3479
	run = 0.0;
	for (int j = S - 1; j >= 0; j--) {
		if (j == sfx_first - 1 && sfx_first < S) {   // Q bounds the silent row segment sfx_first - 1 leaves into
			const int q = col_off[j];
			for (int mm = 0; mm < L; mm++) {
				wc[mm] = clampf(Q[L - mm] + T(m, q, TD_ISKIP) + 15.75);
				wd[mm] = m->skip[j] > -INFINITY ? clampf(Q[L - mm] + (double)m->skip[j] + 15.75) : -3.0e38f;
			}
		}
		run += (double)m->skip[j];
		bwd_sweep(m, j, col_off[j], run, L, Q, Qn, j < n_seg ? bw.data() : j >= sfx_first ? bs.data() : nullptr);
		Q.swap(Qn);
	}
	for (int mm = 0; mm <= L; mm++) { bwt[mm] = clampf(bw[mm] + 1.0e-3); bws[mm] = clampf(bs[mm] + 1.0e-3); }

	// ---- restarted sweeps: impulse responses (tables 8.. and 12..) ----
	// A backward value of leading segment j at position i is a sum over the position at which the path reaches the silent state
	// in front of the first unpruned segment (a read segment, swept densely: the kernel has that row, Q, exactly):
	//     B_s(i) = sum_k w_s,k(read) * Q[i + 1 + k].
	// gq_j[k] bounds w_s,k from above for every state s of segment j and every read: the recurrences of segments n_seg - 1 .. j
	// (same folds, lse_up, every emission at its maximum) driven by an impulse -- a row Q that is 0 right behind the read and
	// -inf elsewhere -- so that a row k positions before the end holds the weight of emitting exactly k more bases before
	// reaching that silent state.  By induction over the recurrence (each lse_up fold dominates the table fold, sums distribute
	// over k), for any read
	//     B_s(i)  <=  log sum_k exp(gq_j[k] + Q[i + 1 + k])  <=  max_k (gq_j[k] + Q[i + 1 + k]) + log(number of k),
	// which is where a restarted sweep starts its upper ends (td_spec_kernel.inc "Restarted sweeps").  Forward mirror image for
	// the trailing segments: F_s(i) = sum_k w'_s,k * P[i - 1 - k], P = the silent row the last read segment leaves (dense,
	// exact); gf_j[k] from the recurrences of segments sfx_first .. j driven by an impulse at position 0.
	std::vector<double> peak(L + 2);
	if (n_seg > 0 && n_seg <= TD_PRUNE_RESTART_MAX) {
		std::fill(Q.begin(), Q.end(), -INFINITY);
		Q[L + 1] = 0.0;
		run = 0.0;
		for (int j = n_seg - 1; j >= 0; j--) {
			float* gq = tab.data() + (size_t)(8 + j) * stride;
			run += (double)m->skip[j];
			std::fill(peak.begin(), peak.end(), -INFINITY);
			bwd_sweep(m, j, col_off[j], run, L, Q, Qn, peak.data());
			for (int mm = 0; mm < L; mm++) gq[mm] = clampf(peak[mm] + 1.0e-3);
			Q.swap(Qn);
		}
	}
	if (sfx_first < S && S - sfx_first <= TD_PRUNE_RESTART_MAX) {
		std::fill(P.begin(), P.end(), -INFINITY);
		P[0] = 0.0;
		run = 0.0;
		for (int j = sfx_first; j < S; j++) {
			float* gf = tab.data() + (size_t)(12 + j - sfx_first) * stride;
			run += (double)m->skip[j];
			std::fill(peak.begin(), peak.end(), -INFINITY);
			fwd_sweep(m, j, col_off[j], run, L, P, Pn, peak.data());
			for (int i = 1; i <= L; i++) gf[i] = clampf(peak[i] + 1.0e-3);      // a value at position i = the impulse i positions back
			gf[0] = -3.0e38f;
			P.swap(Pn);
		}
	}
}
