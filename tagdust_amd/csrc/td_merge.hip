// td_merge.hip -- the merge kernel (gfx950) and its host side: overlap_reads() (src/merge.c:399-688) for a batch of pairs.
//
// Mapping: one pair per wave, four waves per block, blocks striding over the batch.
//   staging   both reads once into the wave's LDS, one number per base: 5 q + x (q the dense quality index, x the base code; a byte
//             when 5 nq <= 256, else 16 bits).  Read 2 is reverse-complemented and its qualities reversed while staging.
//   scores    a lane walks one candidate diagonal: two LDS reads (consecutive lanes, consecutive elements), one gather from T
//             (LDS when it fits the budget, else global memory, where L2 holds it), one float add -- an ordered chain from 0.0f.
//             Candidates are taken in pairs: lane task t is the t-th candidate of the first sweep (read 1 from t, the longest
//             first) and the t-th last of the second (read 2 from nB-1-t, the shortest first), so that for reads of about equal
//             length every lane walks about len + min_overlap cells and the wave's lanes finish together.
//   best      per lane, then across lanes by comparisons only: the largest score, among equal scores the smallest d.
//   consensus position-parallel over the output: head, aligned part, tail; id by a ballot count.
// No atomics, no workspace: inputs, T, outputs.  A pair with a read longer than TD_MERGE_STAGE_BASES is skipped (the host does it).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>

#include "td_merge_internal.h"

namespace {

constexpr int kWaves = 4;                       // pairs per block
constexpr int kStage = TD_MERGE_STAGE_BASES;
constexpr size_t kTableLdsBudget = 32 * 1024;   // T in LDS up to here (dim <= 90: 18 quality characters); beyond it occupancy would pay

struct MergeArgs {
	int64_t n;
	const uint8_t* codes1; const uint8_t* qual1; const int64_t* offs1;
	const uint8_t* codes2; const uint8_t* qual2; const int64_t* offs2;
	const float* T; const float* profile; const int16_t* qindex; const uint8_t* qchar;
	int32_t nq, dim, min_overlap;
	float threshold;
	td_merge_record* rec; char* seq; char* qual;
	uint32_t off_qindex, off_qchar, off_T, off_stage;   // LDS layout in bytes (profile at 0)
};

template <typename E, bool TLDS>
__global__ __launch_bounds__(kWaves * 64) void td_merge_kernel(const MergeArgs a)
{
	extern __shared__ __align__(16) unsigned char smem[];
	float* s_profile = (float*)smem;
	uint16_t* s_qindex = (uint16_t*)(smem + a.off_qindex);
	uint8_t* s_qchar = smem + a.off_qchar;
	float* s_T = (float*)(smem + a.off_T);
	const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
	E* F = (E*)(smem + a.off_stage) + (size_t)wave * 2 * kStage;
	E* R = F + kStage;
	const int nq = a.nq, dim = a.dim, m = a.min_overlap;

	for (int k = tid; k < 2 * nq; k += kWaves * 64) s_profile[k] = a.profile[k];
	for (int k = tid; k < 256; k += kWaves * 64) {
		const int q = a.qindex[k];
		s_qindex[k] = (uint16_t)(q < 0 || q >= nq ? 0 : q);         // (a character outside the tables cannot occur: they were built from this batch)
		s_qchar[k] = k < nq ? a.qchar[k] : (uint8_t)'!';
	}
	if (TLDS) for (int k = tid; k < dim * dim; k += kWaves * 64) s_T[k] = a.T[k];
	const float* T = TLDS ? s_T : a.T;
	__syncthreads();

	// (every wave of a block makes the same number of trips: the barriers below are block-wide)
	for (int64_t base = (int64_t)blockIdx.x * kWaves; base < a.n; base += (int64_t)gridDim.x * kWaves) {
		const int64_t p = base + wave;
		int lf = 0, lr = 0;
		int64_t o1 = 0, o2 = 0;
		bool mine = p < a.n;
		if (mine) {
			o1 = a.offs1[p]; o2 = a.offs2[p];
			lf = (int)(a.offs1[p + 1] - o1); lr = (int)(a.offs2[p + 1] - o2);
			mine = lf <= kStage && lr <= kStage;
		}
		if (mine) {
			for (int i = lane; i < lf; i += 64) {
				const int x = a.codes1[o1 + i];
				F[i] = (E)(5 * s_qindex[a.qual1[o1 + i]] + (x > 4 ? 4 : x));
			}
			for (int j = lane; j < lr; j += 64) {
				const int64_t s = o2 + (lr - 1 - j);
				const int x = a.codes2[s];
				R[j] = (E)(5 * s_qindex[a.qual2[s]] + td_merge_rc(x > 4 ? 4 : x));
			}
		}
		__syncthreads();
		if (mine) {
			// candidates: first sweep i = 0 .. nA-1 (d = i), second sweep j = 0 .. nB-1 (d = lf + j)
			const int nA = lr > m ? (lf - m > 0 ? lf - m : 0) : 0;
			const int nB = lf > m ? (lr - m > 0 ? lr - m : 0) : 0;
			const int nt = nA > nB ? nA : nB;
			float bs = -INFINITY;
			int bd = -1;
			for (int t = lane; t < nt; t += 64) {
				if (t < nA) {
					const int len = lf - t < lr ? lf - t : lr;
					const E* f = F + t;
					float s = 0.0f;
					for (int k = 0; k < len; k++) s = s + T[(int)f[k] * dim + (int)R[k]];
					if (td_merge_better(s, t, bs, bd)) { bs = s; bd = t; }
				}
				if (t < nB) {
					const int j = nB - 1 - t;
					const int len = lr - j < lf ? lr - j : lf;
					const E* r = R + j;
					float s = 0.0f;
					for (int k = 0; k < len; k++) s = s + T[(int)F[k] * dim + (int)r[k]];
					if (td_merge_better(s, lf + j, bs, bd)) { bs = s; bd = lf + j; }
				}
			}
			for (int w = 32; w >= 1; w >>= 1) {        // comparisons only
				const float os = __shfl_xor(bs, w, 64);
				const int od = __shfl_xor(bd, w, 64);
				if (od >= 0 && (bd < 0 || td_merge_better(os, od, bs, bd))) { bs = os; bd = od; }
			}
			td_merge_record rec;
			rec.best_d = bd;
			if (bd < 0) { rec.out_len = 0; rec.id = 0; rec.aligned = 0; rec.status = TD_MERGE_NO_CANDIDATE; }
			else {
				const int i0 = bd < lf ? bd : 0, j0 = bd < lf ? 0 : bd - lf;
				const int head = i0 + j0;
				const int aligned = lf - i0 < lr - j0 ? lf - i0 : lr - j0;
				const int out_len = lf + lr - aligned;
				char* seq = a.seq + (o1 + o2);
				char* qual = a.qual + (o1 + o2);
				int id = 0;
				for (int pos0 = 0; pos0 < out_len; pos0 += 64) {
					const int pos = pos0 + lane;
					bool same = false;
					if (pos < out_len) {
						int x, q;
						if (pos >= head && pos < head + aligned) {
							const int k = pos - head;
							const int ef = F[i0 + k], er = R[j0 + k];
							const int xf = ef % 5, qf = ef / 5, xr = er % 5, qr = er / 5;
							same = xf == xr;
							x = same ? xf : td_merge_pick(s_profile, qf, xf, qr, xr);
							q = qf > qr ? qf : qr;
						} else {
							int e;
							if (pos < head) e = bd < lf ? F[pos] : R[pos];
							else {
								const int k = pos - head - aligned;
								e = i0 + aligned < lf ? F[i0 + aligned + k] : R[j0 + aligned + k];
							}
							x = e % 5; q = e / 5;
						}
						seq[pos] = x == 0 ? 'A' : x == 1 ? 'C' : x == 2 ? 'G' : x == 3 ? 'T' : 'C';     // "ACGTC"[x]
						qual[pos] = (char)s_qchar[q];
					}
					id += __popcll(__ballot(same));
				}
				rec.id = id;
				rec.aligned = aligned;
				const bool pass = td_merge_passes(id, aligned, a.threshold);
				rec.out_len = pass ? out_len : 0;
				rec.status = pass ? TD_MERGE_WRITTEN : TD_MERGE_BELOW;
			}
			if (lane == 0) a.rec[p] = rec;
		}
		__syncthreads();      // the next trip's staging overwrites F and R
	}
}

#define MERGE_HIP(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { err = std::string("td_merge_device: ") + #call + ": " + hipGetErrorString(e_); (void)hipGetLastError(); return false; } } while (0)

struct Buf {
	void* p = nullptr;
	size_t cap = 0;
};

} // namespace

struct TdMergeDevice {
	int device = 0, n_cu = 256;
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	Buf codes1, qual1, offs1, codes2, qual2, offs2, T, small, rec, seq, qual;
	bool room(Buf& b, size_t bytes, std::string& err)
	{
		if (b.cap >= bytes && b.p) return true;
		if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
		const size_t want = bytes + bytes / 4 + 4096;
		MERGE_HIP(hipMalloc(&b.p, want));
		b.cap = want;
		return true;
	}
};

TdMergeDevice* td_merge_device_open(int device, std::string& err)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n < 1) { (void)hipGetLastError(); err = "td_merge_device: no HIP device (there is no quiet fall-back: ask for the host path with device = -1 / --host)"; return nullptr; }
	if (device < 0 || device >= n) { err = "td_merge_device: no device " + std::to_string(device) + " (" + std::to_string(n) + " present)"; return nullptr; }
	TdMergeDevice* d = new TdMergeDevice();
	d->device = device;
	auto open = [&]() -> bool {
		MERGE_HIP(hipSetDevice(device));
		hipDeviceProp_t prop;
		MERGE_HIP(hipGetDeviceProperties(&prop, device));
		if (prop.multiProcessorCount > 0) d->n_cu = prop.multiProcessorCount;
		MERGE_HIP(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
		MERGE_HIP(hipEventCreate(&d->ev0));
		MERGE_HIP(hipEventCreate(&d->ev1));
		return true;
	};
	if (!open()) { td_merge_device_close(d); return nullptr; }
	return d;
}

void td_merge_device_close(TdMergeDevice* d)
{
	if (!d) return;
	(void)hipSetDevice(d->device);
	for (Buf* b : { &d->codes1, &d->qual1, &d->offs1, &d->codes2, &d->qual2, &d->offs2, &d->T, &d->small, &d->rec, &d->seq, &d->qual })
		if (b->p) (void)hipFree(b->p);
	if (d->ev0) (void)hipEventDestroy(d->ev0);
	if (d->ev1) (void)hipEventDestroy(d->ev1);
	if (d->stream) (void)hipStreamDestroy(d->stream);
	delete d;
}

bool td_merge_device_run(TdMergeDevice* d, const TdMergeView& v, const td_merge_tables& t, int min_overlap, float threshold,
                         int placement, td_merge_record* rec, char* seq, char* qual, int* table_in_lds, float* kernel_ms, std::string& err)
{
	if (table_in_lds) *table_in_lds = 0;
	if (kernel_ms) *kernel_ms = 0.0f;
	const size_t t_bytes = sizeof(float) * (size_t)t.dim * (size_t)t.dim;
	const bool fits = t_bytes <= kTableLdsBudget;
	if (placement == TD_MERGE_TABLE_LDS && !fits) {
		err = "td_merge_device: the table of " + std::to_string(t.nq) + " quality characters (" + std::to_string(t_bytes) + " bytes) does not fit the LDS budget of " + std::to_string(kTableLdsBudget) + " bytes";
		return false;
	}
	if (placement != TD_MERGE_TABLE_AUTO && placement != TD_MERGE_TABLE_LDS && placement != TD_MERGE_TABLE_GLOBAL) { err = "td_merge_device: unknown table placement"; return false; }
	const bool tlds = placement == TD_MERGE_TABLE_GLOBAL ? false : fits;
	if (v.n == 0) return true;
	MERGE_HIP(hipSetDevice(d->device));
	const int64_t n = v.n;
	const size_t nb1 = (size_t)v.offs1[n], nb2 = (size_t)v.offs2[n];
	// profile, qindex, qchar in one small buffer
	const size_t sm_profile = 0, sm_qindex = sizeof(float) * 2 * (size_t)t.nq, sm_qchar = sm_qindex + sizeof(int16_t) * 256, sm_bytes = sm_qchar + 256;
	if (!d->room(d->codes1, nb1 + 1, err) || !d->room(d->qual1, nb1 + 1, err) || !d->room(d->offs1, sizeof(int64_t) * (size_t)(n + 1), err) ||
	    !d->room(d->codes2, nb2 + 1, err) || !d->room(d->qual2, nb2 + 1, err) || !d->room(d->offs2, sizeof(int64_t) * (size_t)(n + 1), err) ||
	    !d->room(d->T, t_bytes, err) || !d->room(d->small, sm_bytes, err) || !d->room(d->rec, sizeof(td_merge_record) * (size_t)n, err) ||
	    !d->room(d->seq, nb1 + nb2 + 1, err) || !d->room(d->qual, nb1 + nb2 + 1, err)) return false;
	unsigned char small[sizeof(float) * 2 * 256 + sizeof(int16_t) * 256 + 256];
	memcpy(small + sm_profile, t.profile, sizeof(float) * 2 * (size_t)t.nq);
	memcpy(small + sm_qindex, t.qindex, sizeof(int16_t) * 256);
	memcpy(small + sm_qchar, t.qchar, 256);
	hipStream_t st = d->stream;
	MERGE_HIP(hipMemcpyAsync(d->codes1.p, v.codes1, nb1, hipMemcpyHostToDevice, st));
	MERGE_HIP(hipMemcpyAsync(d->qual1.p, v.qual1, nb1, hipMemcpyHostToDevice, st));
	MERGE_HIP(hipMemcpyAsync(d->offs1.p, v.offs1, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
	MERGE_HIP(hipMemcpyAsync(d->codes2.p, v.codes2, nb2, hipMemcpyHostToDevice, st));
	MERGE_HIP(hipMemcpyAsync(d->qual2.p, v.qual2, nb2, hipMemcpyHostToDevice, st));
	MERGE_HIP(hipMemcpyAsync(d->offs2.p, v.offs2, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
	MERGE_HIP(hipMemcpyAsync(d->T.p, t.T, t_bytes, hipMemcpyHostToDevice, st));
	MERGE_HIP(hipMemcpyAsync(d->small.p, small, sm_bytes, hipMemcpyHostToDevice, st));
	// (pairs the kernel skips keep a defined record until the host path fills them in)
	MERGE_HIP(hipMemsetAsync(d->rec.p, 0, sizeof(td_merge_record) * (size_t)n, st));

	MergeArgs a;
	a.n = n;
	a.codes1 = (const uint8_t*)d->codes1.p; a.qual1 = (const uint8_t*)d->qual1.p; a.offs1 = (const int64_t*)d->offs1.p;
	a.codes2 = (const uint8_t*)d->codes2.p; a.qual2 = (const uint8_t*)d->qual2.p; a.offs2 = (const int64_t*)d->offs2.p;
	a.T = (const float*)d->T.p;
	a.profile = (const float*)((const unsigned char*)d->small.p + sm_profile);
	a.qindex = (const int16_t*)((const unsigned char*)d->small.p + sm_qindex);
	a.qchar = (const uint8_t*)d->small.p + sm_qchar;
	a.nq = t.nq; a.dim = t.dim; a.min_overlap = min_overlap; a.threshold = threshold;
	a.rec = (td_merge_record*)d->rec.p; a.seq = (char*)d->seq.p; a.qual = (char*)d->qual.p;
	const bool wide = t.dim > 256;
	auto up16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
	a.off_qindex = (uint32_t)up16(sizeof(float) * 2 * (size_t)t.nq);
	a.off_qchar = a.off_qindex + 512;
	a.off_T = a.off_qchar + 256;
	a.off_stage = (uint32_t)up16(a.off_T + (tlds ? t_bytes : 0));
	const size_t lds = a.off_stage + (size_t)kWaves * 2 * kStage * (wide ? 2 : 1);     // <= 3 KB + 32 KB + 8 KB
	const int64_t want_blocks = (n + kWaves - 1) / kWaves;
	const int64_t max_blocks = (int64_t)d->n_cu * 8;
	const unsigned grid = (unsigned)(want_blocks < max_blocks ? want_blocks : max_blocks);
	MERGE_HIP(hipEventRecord(d->ev0, st));
	if (wide) {
		if (tlds) hipLaunchKernelGGL((td_merge_kernel<uint16_t, true>), dim3(grid), dim3(kWaves * 64), lds, st, a);
		else hipLaunchKernelGGL((td_merge_kernel<uint16_t, false>), dim3(grid), dim3(kWaves * 64), lds, st, a);
	} else {
		if (tlds) hipLaunchKernelGGL((td_merge_kernel<uint8_t, true>), dim3(grid), dim3(kWaves * 64), lds, st, a);
		else hipLaunchKernelGGL((td_merge_kernel<uint8_t, false>), dim3(grid), dim3(kWaves * 64), lds, st, a);
	}
	MERGE_HIP(hipGetLastError());
	MERGE_HIP(hipEventRecord(d->ev1, st));
	MERGE_HIP(hipMemcpyAsync(rec, d->rec.p, sizeof(td_merge_record) * (size_t)n, hipMemcpyDeviceToHost, st));
	MERGE_HIP(hipMemcpyAsync(seq, d->seq.p, nb1 + nb2, hipMemcpyDeviceToHost, st));
	MERGE_HIP(hipMemcpyAsync(qual, d->qual.p, nb1 + nb2, hipMemcpyDeviceToHost, st));
	MERGE_HIP(hipStreamSynchronize(st));
	float ms = 0.0f;
	MERGE_HIP(hipEventElapsedTime(&ms, d->ev0, d->ev1));
	if (kernel_ms) *kernel_ms = ms;
	if (table_in_lds) *table_in_lds = tlds ? 1 : 0;
	return true;
}
