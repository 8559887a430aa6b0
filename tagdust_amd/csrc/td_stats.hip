// td_stats.hip -- the counting half of get_sequence_stats() (src/io.c:125-188) on the device: the base histogram, the sum and
// the maximum of the read lengths and, for a leading / trailing 'P' segment, s0 / s1 / s2 of the linker match lengths.
//
// Two kernels over buffers of the call's own (nothing of a context is touched):
//   td_stats_hist_kernel   the histogram does not depend on read boundaries: it streams codes[offs[0] .. offs[n]) with 16-byte
//                          loads, one launch per uploaded piece, so that the kernel of one piece runs beside the copy of the next;
//   td_stats_reads_kernel  one lane per read: its length, and the two linker scans, which read only the first / last
//                          linker-length bytes of the read.
// Everything is summed as 64-bit integers -- per lane, then per wave (shuffles), then per workgroup (LDS), then ONE integer
// atomic per counter per workgroup -- so the result is exact and independent of the launch geometry.  No float atomics.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "td_stats.h"

#define ST_BLOCK 256
#define ST_WAVE 64
#define ST_PIECE ((int64_t)32 << 20)   // bytes per uploaded piece (a multiple of 16)

enum { ST_BASE = 0 /* .. 4 */, ST_LEN_SUM = 5, ST_LEN_MAX = 6, ST_FIVE = 7 /* s0 s1 s2 */, ST_THREE = 10 /* s0 s1 s2 */, ST_WORDS = 13 };

typedef unsigned long long u64;

// the value of lane (this ^ o), moved as two dwords
__device__ inline u64 shfl_xor_u64(u64 v, int o)
{
	const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o);
	return ((u64)hi << 32) | lo;
}

__device__ inline u64 wave_sum(u64 v)
{
#pragma unroll
	for (int o = ST_WAVE / 2; o >= 1; o >>= 1) v += shfl_xor_u64(v, o);
	return v;
}

__device__ inline u64 wave_max(u64 v)
{
#pragma unroll
	for (int o = ST_WAVE / 2; o >= 1; o >>= 1) { const u64 w = shfl_xor_u64(v, o); v = w > v ? w : v; }
	return v;
}

// v[0 .. N) of every lane of the workgroup -> one atomic per counter on out[first + i]; i == max_at is a maximum, the others sums
template <int N>
__device__ inline void block_commit(u64* v, u64* __restrict__ out, int first, int max_at)
{
	__shared__ u64 part[ST_BLOCK / ST_WAVE][N];
	const int lane = threadIdx.x & (ST_WAVE - 1), wave = threadIdx.x / ST_WAVE;
#pragma unroll
	for (int i = 0; i < N; i++) {
		const u64 r = i == max_at ? wave_max(v[i]) : wave_sum(v[i]);
		if (lane == 0) part[wave][i] = r;
	}
	__syncthreads();
	if (threadIdx.x < N) {
		const int i = threadIdx.x;
		u64 r = part[0][i];
		for (int w = 1; w < ST_BLOCK / ST_WAVE; w++) r = i == max_at ? (part[w][i] > r ? part[w][i] : r) : r + part[w][i];
		if (r) { if (i == max_at) atomicMax(out + first + i, r); else atomicAdd(out + first + i, r); }
	}
}

// bytes of w equal to k (k < 128): exact per byte, no carries between bytes
__device__ inline uint32_t bytes_equal(uint32_t w, uint32_t k)
{
	const uint32_t x = w ^ (k * 0x01010101u);
	const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);   // 0x80 in every byte of x that is 0
	return (uint32_t)__popc(z);
}

// codes: 16-byte aligned, n_bytes of them.  Codes 0..3 are counted; everything else is slot 4 = bytes seen - those.
__global__ __launch_bounds__(ST_BLOCK) void td_stats_hist_kernel(const uint8_t* __restrict__ codes, int64_t n_bytes, u64* __restrict__ out)
{
	u64 v[5] = { 0, 0, 0, 0, 0 };
	const int64_t n16 = n_bytes >> 4;
	const int64_t tid = (int64_t)blockIdx.x * ST_BLOCK + threadIdx.x, step = (int64_t)gridDim.x * ST_BLOCK;
	const uint4* p = (const uint4*)codes;
	uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
	int64_t seen = 0;
	for (int64_t i = tid; i < n16; i += step) {
		const uint4 q = p[i];
		const uint32_t w[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
		for (int j = 0; j < 4; j++) {
			c0 += bytes_equal(w[j], 0); c1 += bytes_equal(w[j], 1); c2 += bytes_equal(w[j], 2); c3 += bytes_equal(w[j], 3);
		}
		seen += 16;
		if ((seen & 0x3FFFFFFF) == 0) { v[0] += c0; v[1] += c1; v[2] += c2; v[3] += c3; c0 = c1 = c2 = c3 = 0; }   // (long before 32 bits run out)
	}
	const int64_t t = (n16 << 4) + tid;   // the up to 15 bytes behind the last whole 16
	if (t < n_bytes) {
		const uint32_t b = codes[t];
		c0 += b == 0; c1 += b == 1; c2 += b == 2; c3 += b == 3;
		seen += 1;
	}
	v[0] += c0; v[1] += c1; v[2] += c2; v[3] += c3;
	v[4] = (u64)seen - v[0] - v[1] - v[2] - v[3];
	block_commit<5>(v, out, ST_BASE, -1);
}

// codes = the bytes from offs[0] on; offs[0 .. n]; five / three: the linkers' base codes (length 0: none)
__global__ __launch_bounds__(ST_BLOCK) void td_stats_reads_kernel(const uint8_t* __restrict__ codes, const int64_t* __restrict__ offs, int64_t n,
                                                                  const uint8_t* __restrict__ five, int five_len,
                                                                  const uint8_t* __restrict__ three, int three_len, u64* __restrict__ out)
{
	u64 v[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };   // len_sum, len_max, five s0 s1 s2, three s0 s1 s2
	const int64_t base = offs[0];
	const int64_t step = (int64_t)gridDim.x * ST_BLOCK;
	for (int64_t r = (int64_t)blockIdx.x * ST_BLOCK + threadIdx.x; r < n; r += step) {
		const int64_t o = offs[r] - base;
		const int len = (int)(offs[r + 1] - offs[r]);
		const uint8_t* seq = codes + o;
		v[0] += (u64)len;
		if ((u64)len > v[1]) v[1] = (u64)len;
		if (five_len) {
			// the longest linker suffix of m > 3 bases that equals the read's first m; position len reads as the loader's 0
			// terminator (io.c:1759, the code of 'A'), anything further out matches nothing -- so m <= len + 1
			for (int m = five_len < len + 1 ? five_len : len + 1; m > 3; m--) {
				const uint8_t* lk = five + (five_len - m);
				int c = 0;
				for (; c < m; c++) {
					const int b = c < len ? (int)seq[c] : 0;
					if (b != (int)lk[c]) break;
				}
				if (c == m) { v[2] += 1; v[3] += (u64)m; v[4] += (u64)m * (u64)m; break; }
			}
		}
		if (three_len) {
			// the longest linker prefix of m > 3 bases that equals the read's last m; positions before the read match nothing
			for (int m = three_len < len ? three_len : len; m > 3; m--) {
				const uint8_t* tail = seq + (len - m);
				int c = 0;
				for (; c < m; c++)
					if ((int)tail[c] != (int)three[c]) break;
				if (c == m) { v[5] += 1; v[6] += (u64)m; v[7] += (u64)m * (u64)m; break; }
			}
		}
	}
	block_commit<8>(v, out, ST_LEN_SUM, 1);
}

namespace {
struct Buffers {   // everything the call owns on the device, released on every way out
	uint8_t* codes = nullptr; int64_t* offs = nullptr; uint8_t* link = nullptr; u64* out = nullptr; hipStream_t stream = nullptr;
	~Buffers()
	{
		if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
		void* p[] = { codes, offs, link, out };
		for (void* q : p) if (q) (void)hipFree(q);
	}
};
}

#define ST_CHK(call)                                                                                     \
	do {                                                                                                 \
		hipError_t e_ = (call);                                                                          \
		if (e_ != hipSuccess) { snprintf(err, errcap, "td_sequence_stats_device: %s failed: %s", #call, hipGetErrorString(e_)); return TD_FAIL; } \
	} while (0)

int td_stats_count_device(int device, const std::vector<uint8_t>& five, const std::vector<uint8_t>& three, const uint8_t* codes,
                          const int64_t* offs, int64_t n_reads, int64_t scan_limit, TdSeqCounts* k, char* err, size_t errcap)
{
	*k = TdSeqCounts();
	const int64_t n = n_reads < scan_limit ? n_reads : scan_limit;
	// the kernels index with these: nothing reaches the device that would make them read outside the uploaded bytes
	for (int64_t r = 0; r < n; r++) {
		const int64_t len = offs[r + 1] - offs[r];
		if (len < 0 || len > 0x7FFFFFFF) { snprintf(err, errcap, "td_sequence_stats_device: offs is not ascending at read %lld (or the read has 2^31 bases or more)", (long long)r); return TD_FAIL; }
	}
	const int64_t n_bytes = offs[n] - offs[0];
	ST_CHK(hipSetDevice(device));
	Buffers b;
	ST_CHK(hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking));
	ST_CHK(hipMalloc((void**)&b.codes, (size_t)(n_bytes > 0 ? n_bytes : 1)));
	ST_CHK(hipMalloc((void**)&b.offs, sizeof(int64_t) * (size_t)(n + 1)));
	ST_CHK(hipMalloc((void**)&b.link, five.size() + three.size() + 1));
	ST_CHK(hipMalloc((void**)&b.out, sizeof(u64) * ST_WORDS));
	ST_CHK(hipMemsetAsync(b.out, 0, sizeof(u64) * ST_WORDS, b.stream));
	ST_CHK(hipMemcpyAsync(b.offs, offs, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, b.stream));
	if (!five.empty()) ST_CHK(hipMemcpyAsync(b.link, five.data(), five.size(), hipMemcpyHostToDevice, b.stream));
	if (!three.empty()) ST_CHK(hipMemcpyAsync(b.link + five.size(), three.data(), three.size(), hipMemcpyHostToDevice, b.stream));
	for (int64_t at = 0; at < n_bytes; at += ST_PIECE) {
		const int64_t m = n_bytes - at < ST_PIECE ? n_bytes - at : ST_PIECE;
		ST_CHK(hipMemcpyAsync(b.codes + at, codes + offs[0] + at, (size_t)m, hipMemcpyHostToDevice, b.stream));
		int64_t blocks = ((m >> 4) + ST_BLOCK * 4 - 1) / (ST_BLOCK * 4);   // four 16-byte loads per lane
		if (blocks < 1) blocks = 1;
		if (blocks > 2048) blocks = 2048;
		hipLaunchKernelGGL(td_stats_hist_kernel, dim3((unsigned)blocks), dim3(ST_BLOCK), 0, b.stream, (const uint8_t*)(b.codes + at), m, b.out);
		ST_CHK(hipGetLastError());
	}
	if (n > 0) {
		int64_t blocks = (n + ST_BLOCK - 1) / ST_BLOCK;
		if (blocks > 4096) blocks = 4096;
		hipLaunchKernelGGL(td_stats_reads_kernel, dim3((unsigned)blocks), dim3(ST_BLOCK), 0, b.stream, (const uint8_t*)b.codes, (const int64_t*)b.offs, n,
		                   (const uint8_t*)b.link, (int)five.size(), (const uint8_t*)(b.link + five.size()), (int)three.size(), b.out);
		ST_CHK(hipGetLastError());
	}
	u64 w[ST_WORDS];
	ST_CHK(hipMemcpyAsync(w, b.out, sizeof w, hipMemcpyDeviceToHost, b.stream));
	ST_CHK(hipStreamSynchronize(b.stream));
	k->n_reads = n;
	for (int i = 0; i < 5; i++) k->base[i] = (int64_t)w[ST_BASE + i];
	k->len_sum = (int64_t)w[ST_LEN_SUM]; k->len_max = (int64_t)w[ST_LEN_MAX];
	for (int i = 0; i < 3; i++) { k->five[i] = (int64_t)w[ST_FIVE + i]; k->three[i] = (int64_t)w[ST_THREE + i]; }
	return TD_OK;
}
