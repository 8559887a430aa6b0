// workers_host_check.cpp -- the host worker pool and the two thread-count rules (tagdust_amd/csrc/td_workers.h) as a stand-alone
// program over that header alone: no GPU, no HIP runtime, no Python.  tools/host_checks.sh runs it under AddressSanitizer and UBSan,
// tools/tsan_stream.sh under ThreadSanitizer.
//
//   g++ -std=c++17 -O1 -g tools/workers_host_check.cpp -o /tmp/workers_host_check -lpthread && /tmp/workers_host_check
//
// Prints "workers_host_check: ok"; a hang (a lost wake-up) ends in SIGALRM after 120 s.
#include <stdio.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <utility>

#include "../tagdust_amd/csrc/td_workers.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "workers_host_check: %s:%d: %s failed\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// run(n): every index of [0, n) exactly once
static bool run_covers(TdWorkers& w, int64_t n)
{
	std::vector<std::atomic<int>> hit((size_t)(n > 0 ? n : 1));
	for (auto& h : hit) h = 0;
	std::atomic<int64_t> outside(0);
	w.run(n, [&](int64_t k) { if (k < 0 || k >= n) outside++; else hit[(size_t)k]++; });
	if (outside) return false;
	for (int64_t k = 0; k < n; k++) if (hit[(size_t)k] != 1) return false;
	return n > 0 || hit[0] == 0;
}

// ranges(n, nt): the ranges tile [0, n) exactly; there are as many as the grain allows (min(nt, n / 4096), at least one) and
// no more; the first one runs on the calling thread
static bool ranges_tile(TdWorkers& w, int64_t n, int nt)
{
	std::mutex mu;
	std::vector<std::pair<int64_t, int64_t>> got;
	bool first_on_caller = false;
	const std::thread::id me = std::this_thread::get_id();
	w.ranges(n, nt, [&](int64_t lo, int64_t hi) {
		std::lock_guard<std::mutex> lk(mu);
		got.push_back({ lo, hi });
		if (lo == 0) first_on_caller = std::this_thread::get_id() == me;
	});
	if (n <= 0) return got.empty();
	const int64_t most = std::max<int64_t>(1, std::min<int64_t>(nt, n / 4096));
	const int64_t per = (n + most - 1) / most;
	if ((int64_t)got.size() != (n + per - 1) / per || (int64_t)got.size() > most || !first_on_caller) return false;
	std::sort(got.begin(), got.end());
	int64_t at = 0;
	for (auto& r : got) { if (r.first != at || r.second <= r.first) return false; at = r.second; }
	return at == n;
}

// copy(bytes, nt): destination equals source, the byte either side of it untouched
static bool copy_exact(TdWorkers& w, size_t bytes, int nt)
{
	std::vector<unsigned char> src(bytes + 1), dst(bytes + 2, 0xA5);      // (+1: data() of an empty vector may be null)
	uint32_t s = (uint32_t)bytes * 2654435761u + 17u;
	for (size_t k = 0; k < bytes; k++) { s = s * 1664525u + 1013904223u; src[k] = (unsigned char)(s >> 24); }
	w.copy(dst.data() + 1, src.data(), bytes, nt);
	return dst[0] == 0xA5 && dst[bytes + 1] == 0xA5 && (bytes == 0 || !memcmp(dst.data() + 1, src.data(), bytes));
}

int main()
{
	alarm(120);
	{ TdWorkers idle(4); }                                   // made and gone without work
	{ TdWorkers none; CHECK(none.size() == 1); CHECK(run_covers(none, 100)); }
	{
		TdWorkers w(4);
		CHECK(w.size() == 4);
		for (int64_t n : { (int64_t)0, (int64_t)1, (int64_t)3, (int64_t)10007 }) CHECK(run_covers(w, n));
		CHECK(run_covers(w, -5));
	}
	for (int nt : { 1, 2, 3, 16 }) {
		TdWorkers w;                                          // grown by the calls, as a context's pool is
		for (int64_t n : { (int64_t)0, (int64_t)4095, (int64_t)8192, (int64_t)100003 }) CHECK(ranges_tile(w, n, nt));
		CHECK(w.size() <= std::max(nt, 1));
	}
	for (int nt : { 3, 16 }) {
		TdWorkers w;
		const size_t mib = (size_t)1 << 20;
		for (size_t bytes : { (size_t)0, (size_t)1, 4 * mib }) CHECK(copy_exact(w, bytes, nt));
		CHECK(w.size() == 1);                                 // up to 4 chunks: a plain memcpy, no thread was started
		CHECK(copy_exact(w, 4 * mib + 1, nt));
		CHECK(w.size() == std::min(nt, 5));                   // 5 chunks: one thread per share, at most one share per chunk
		CHECK(copy_exact(w, 37 * mib + 13, nt));
		CHECK(w.size() == nt);
	}
	{   // a pool grows between calls
		TdWorkers w(2);
		CHECK(run_covers(w, 1000));
		w.grow(5);
		CHECK(w.size() == 5);
		CHECK(run_covers(w, 1000));
		w.grow(3);
		CHECK(w.size() == 5);
		CHECK(ranges_tile(w, 100003, 5));
	}
	{   // back-to-back small runs: the wake-up of every one must arrive
		TdWorkers w(4);
		std::atomic<int64_t> sum(0);
		for (int r = 0; r < 1000; r++) w.run(1 + r % 7, [&](int64_t k) { sum += k + 1; });
		int64_t want = 0;
		for (int r = 0; r < 1000; r++) { const int64_t n = 1 + r % 7; want += n * (n + 1) / 2; }
		CHECK(sum == want);
	}
	// the count rules
	CHECK(td_stage_threads(5, 32) == 5 && td_stage_threads(40, 32) == 32 && td_stage_threads(40, 64) == 40 && td_stage_threads(100, 64) == 64);
	{
		int hw = (int)std::thread::hardware_concurrency();
		if (hw < 1) hw = 1;
		const int want = hw >= 16 ? 8 : (hw >= 4 ? hw / 2 : 1);
		CHECK(td_stage_threads(0, 32) == want && td_stage_threads(-1, 64) == want);
		unsetenv("TD_HOST_THREADS");
		CHECK(td_context_threads() == std::min(hw, 16));
		setenv("TD_HOST_THREADS", "3", 1);  CHECK(td_context_threads() == 3);
		setenv("TD_HOST_THREADS", "99", 1); CHECK(td_context_threads() == 16);
		setenv("TD_HOST_THREADS", "0", 1);  CHECK(td_context_threads() == 1);
	}
	printf("workers_host_check: ok\n");
	return 0;
}
