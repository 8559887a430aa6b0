// td_workers.h -- the host side's one way of running a loop on several threads, and its two rules for how many.  Plain C++17, no
// HIP: the streaming pipeline's stages, the merger, the whole-text parser / writer and a context's copies all work on a TdWorkers.
//
// The contract: ONE caller at a time per pool.  run / ranges / copy / grow come from one thread at a time (the stage that owns
// the pool); stages that run side by side have a pool each (the writer has a second one for its appender thread for exactly this
// reason).  The threads are persistent: started by the constructor or by grow(), joined by the destructor.  The calling thread
// takes work itself in every call, so a pool of n runs n - 1 threads of its own.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

class TdWorkers {
public:
	explicit TdWorkers(int n_threads = 1) { grow(n_threads); }
	TdWorkers(const TdWorkers&) = delete;
	TdWorkers& operator=(const TdWorkers&) = delete;
	~TdWorkers()
	{
		{ std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
		cv_.notify_all();
		for (auto& t : th_) t.join();
	}
	int size() const { return (int)th_.size() + 1; }
	// at least n_threads from now on, the caller included (a context's "host_threads" may rise after the pool was made)
	void grow(int n_threads)
	{
		while (size() < n_threads) th_.emplace_back([this] { worker(); });
	}
	// task(k) for every k in [0, n), each exactly once; the indices are handed out one by one to whichever thread is free
	void run(int64_t n, const std::function<void(int64_t)>& task)
	{
		if (n <= 0) return;
		if (th_.empty() || n == 1) { for (int64_t k = 0; k < n; k++) task(k); return; }
		{
			std::lock_guard<std::mutex> lk(mu_);
			task_ = &task; n_ = n; next_ = 1; gen_++;
		}
		cv_.notify_all();
		task(0);                               // the calling thread takes the first index, then whatever is next
		take(task, n);
		std::unique_lock<std::mutex> lk(mu_);  // every index has been taken: wait for the threads that are still at theirs
		done_.wait(lk, [this] { return active_ == 0; });
		task_ = nullptr;
	}
	// fn(lo, hi) over [0, n) in at most nt contiguous ranges, the first on the calling thread; fewer than 4096 items per thread
	// lowers nt.  A range is one index of run(): as a rule one per thread, but a thread that is free takes the next one, so
	// which thread gets which range (beyond the first) is not fixed.  Every thread of the pool is woken for a call, also where nt
	// is smaller than the pool (a context's "host_threads" lowered after it grew); the ones that find nothing go back to sleep.
	void ranges(int64_t n, int nt, const std::function<void(int64_t, int64_t)>& fn)
	{
		if (n <= 0) return;
		if (nt > n / 4096) nt = (int)(n / 4096);
		if (nt <= 1) { fn(0, n); return; }
		grow(nt);
		const int64_t per = (n + nt - 1) / nt;
		run((n + per - 1) / per, [&](int64_t k) { fn(k * per, (k + 1) * per < n ? (k + 1) * per : n); });
	}
	// memcpy(dst, src, bytes) in at most nt contiguous shares of whole 1 MiB chunks, handed out like ranges; up to 4 chunks are
	// not worth a hand-off
	void copy(void* dst, const void* src, size_t bytes, int nt)
	{
		const size_t chunk = (size_t)1 << 20;
		const size_t nchunks = (bytes + chunk - 1) / chunk;
		if ((size_t)nt > nchunks) nt = (int)nchunks;
		if (nchunks <= 4 || nt <= 1) { memcpy(dst, src, bytes); return; }
		grow(nt);
		const size_t per = (nchunks + (size_t)nt - 1) / (size_t)nt * chunk;
		run((int64_t)((bytes + per - 1) / per), [&](int64_t k) {
			const size_t lo = (size_t)k * per;
			memcpy((char*)dst + lo, (const char*)src + lo, lo + per < bytes ? per : bytes - lo);
		});
	}

private:
	// Takes indices until none is left, without the mutex: a thread that loses the processor while it holds a lock that every
	// other one needs for its next index holds all of them up.
	void take(const std::function<void(int64_t)>& task, int64_t n)
	{
		for (;;) {
			const int64_t k = next_.fetch_add(1, std::memory_order_relaxed);
			if (k >= n) return;
			task(k);
		}
	}
	// A thread joins a run under the mutex (active_) and leaves it under the mutex: run() returns, and the next run is set up,
	// only when none is left inside take() with this run's task.
	void worker()
	{
		uint64_t seen = 0;
		std::unique_lock<std::mutex> lk(mu_);
		for (;;) {
			cv_.wait(lk, [&] { return stop_ || (gen_ != seen && task_); });
			if (stop_) return;
			seen = gen_;
			const std::function<void(int64_t)>* t = task_;
			const int64_t n = n_;
			active_++;
			lk.unlock();
			take(*t, n);
			lk.lock();
			if (--active_ == 0) done_.notify_all();
		}
	}
	std::vector<std::thread> th_;
	std::mutex mu_;
	std::condition_variable cv_, done_;
	const std::function<void(int64_t)>* task_ = nullptr;
	std::atomic<int64_t> next_{ 0 };
	int64_t n_ = 0;
	int active_ = 0;
	uint64_t gen_ = 0;
	bool stop_ = false;
};

// Threads of a context (option "host_threads") and of the whole-text writer: TD_HOST_THREADS, else the machine's, 1..16.
inline int td_context_threads()
{
	int nt = (int)std::thread::hardware_concurrency();
	if (const char* e = getenv("TD_HOST_THREADS")) nt = atoi(e);
	if (nt > 16) nt = 16;
	if (nt < 1) nt = 1;
	return nt;
}

// Threads of a pipeline stage (td_stream_opts / td_merge_opts n_threads): what was asked for, at most cap; nothing asked for: 8
// on a machine of 16 or more, half of a smaller one's, 1 below four.
inline int td_stage_threads(int requested, int cap)
{
	if (requested > 0) return requested > cap ? cap : requested;
	int hw = (int)std::thread::hardware_concurrency();
	if (hw < 1) hw = 1;
	return hw >= 16 ? 8 : (hw >= 4 ? hw / 2 : 1);
}
