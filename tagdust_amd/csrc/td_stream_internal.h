// td_stream_internal.h -- what the units of the streaming pipeline share: td_stream_reader.cpp (input side), td_stream_writer.cpp
// (output side), td_stream.cpp (the stages and the decode entry points) and td_merge_stream.cpp (the `merge` controller on the same
// readers).  Only per-batch and per-run calls cross a unit boundary -- Reader::start / stop / release, Writer::open / write_batch /
// finish / close, queue push / pop; what a hot loop calls per record or per byte (Bytes::room) is inline here or lies beside it.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tagdust_io.h"
#include "td_io_internal.h"
#include "td_workers.h"

namespace tdstream {

inline double now_s()
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- bounded FIFO between the stages ----
template <typename T>
class Queue {
public:
	explicit Queue(size_t cap) : cap_(cap) {}
	bool push(T v)          // false: the pipeline was aborted
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [&] { return abort_ || q_.size() < cap_; });
		if (abort_) return false;
		q_.push_back(std::move(v));
		cv_.notify_all();
		return true;
	}
	bool pop(T& v)          // false: closed and empty, or aborted
	{
		std::unique_lock<std::mutex> lk(mu_);
		cv_.wait(lk, [&] { return abort_ || closed_ || !q_.empty(); });
		if (abort_ || q_.empty()) return false;
		v = std::move(q_.front());
		q_.pop_front();
		cv_.notify_all();
		return true;
	}
	int try_pop(T& v)       // 1: got one; 0: nothing there right now; -1: closed and empty, or aborted
	{
		std::lock_guard<std::mutex> lk(mu_);
		if (abort_) return -1;
		if (q_.empty()) return closed_ ? -1 : 0;
		v = std::move(q_.front());
		q_.pop_front();
		cv_.notify_all();
		return 1;
	}
	void close() { std::lock_guard<std::mutex> lk(mu_); closed_ = true; cv_.notify_all(); }
	void abort() { std::lock_guard<std::mutex> lk(mu_); abort_ = true; cv_.notify_all(); }

private:
	std::mutex mu_;
	std::condition_variable cv_;
	std::deque<T> q_;
	size_t cap_;
	bool closed_ = false, abort_ = false;
};

// ---- the error of a run: the first message stays, and failing ends the run by aborting every queue between its stages ----
class RunError {
public:
	template <typename Q>
	void watch(Q* q)        // q->abort() when the run fails (at once when it already has); q outlives the run's threads
	{
		std::lock_guard<std::mutex> lk(mu_);
		if (!msg_.empty()) q->abort();
		aborts_.push_back([q] { q->abort(); });
	}
	void fail(const std::string& m)
	{
		std::lock_guard<std::mutex> lk(mu_);
		if (msg_.empty()) msg_ = m;
		for (auto& a : aborts_) a();
	}
	bool failed() { std::lock_guard<std::mutex> lk(mu_); return !msg_.empty(); }
	std::string message() { std::lock_guard<std::mutex> lk(mu_); return msg_; }

private:
	std::mutex mu_;
	std::string msg_;
	std::vector<std::function<void()>> aborts_;
};

// ---- input text: one mapping of a plain file, or blocks read from a pipe ----
struct Block {
	const char* data = nullptr;
	int64_t len = 0;
	char* owned = nullptr;          // malloc'ed (pipe input); a mapped file is owned by the Source
	~Block() { free(owned); }
};

class Source {
public:
	~Source();
	bool open(const char* path, int64_t block_bytes, std::string& err);
	// the next block of whole records (nullptr at the end); *read_s += time spent waiting for bytes
	std::shared_ptr<Block> next(double* read_s, std::string& err);

private:
	std::shared_ptr<Block> sam_block(std::shared_ptr<Block> b, int64_t have, const bool end_of_input, std::string& err);

	int fd_ = -1, fd_in_ = -1;
	std::string cmd_;
	bool sam_ = false;
	FILE* pipe_ = nullptr;
	void* map_ = nullptr;
	int64_t map_len_ = 0, map_pos_ = 0, block_ = 0;
	bool eof_ = false, fasta_ = false, first_block_ = true;
	std::vector<char> carry_;
};

// ---- a decode batch: exactly batch_reads records (fewer at the end), device-ready buffers in page-locked memory ----
struct Piece {                      // records [lo, hi) of one parsed chunk of a block
	std::shared_ptr<Block> blk;
	std::shared_ptr<std::vector<TdRec>> recs;
	int64_t lo = 0, hi = 0;
	int64_t first = 0;              // index of record lo within the batch
};

struct Batch {
	int64_t n = 0, n_bases = 0;
	uint8_t* codes = nullptr;  size_t cap_codes = 0;
	uint8_t* seq_out = nullptr; size_t cap_seq = 0;
	uint8_t* qual = nullptr;   size_t cap_qual = 0;   // the records' quality lines, read i's at offs[i]: only for a file whose
	                                                  // context has the base-quality filter on (Reader::want_qual)
	int64_t* offs = nullptr;
	td_read_result* res = nullptr;
	std::vector<Piece> pieces;
	int64_t cap_reads = 0;     // offs / res hold this many reads
	const uint8_t* seq_src = nullptr;   // what the writer prints: seq_out, or codes for a file that is not decoded (run_rna_dust)
};

// a growing byte buffer without the zero-fill of std::string::resize
struct Bytes {
	char* p = nullptr;
	size_t n = 0, cap = 0;
	Bytes() = default;
	Bytes(const Bytes&) = delete;
	Bytes& operator=(const Bytes&) = delete;
	Bytes(Bytes&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
	~Bytes() { free(p); }
	char* room(size_t more)
	{
		if (n + more > cap) {
			size_t c = cap ? cap * 2 : (size_t)1 << 16;
			while (c < n + more) c *= 2;
			p = (char*)realloc(p, c);
			cap = c;
		}
		return p + n;
	}
};

// ---- stage 1 of one input file: its source, the batches it owns, an allocator thread and a producer thread with a parse pool ----
struct Reader {
	RunError& err;
	const td_stream_opts o;
	const bool dry;            // batch buffers in plain memory: a file that no device sees
	const bool want_seq;       // page-locked room for rewritten sequences (not for a file that goes through TD_MODE_RNA_DUST)
	const int parse_threads;
	bool want_qual = false;    // the base-quality filter is on in the file's context (tagdust_quality.h): batches carry the quality
	                           // lines, and a record without one (FASTA) ends the run; set before start()
	std::string path;          // ... the file's name for that message
	Source src;
	std::unique_ptr<TdWorkers> parse_pool;
	std::unique_ptr<Queue<Batch*>> ready, free_list;
	std::vector<Batch*> all;
	int64_t bytes_in = 0;
	double read_s = 0, parse_s = 0;
	double dbg_pass1 = 0, dbg_grow = 0, dbg_encode = 0;
	size_t batch_hint = 0;
	std::mutex all_mu;
	std::condition_variable hint_cv;
	bool hint_ready = false, stop_alloc = false;
	std::thread t_alloc, t_prod;

	Reader(RunError& e, const td_stream_opts& opts, bool dry_, bool want_seq_, int parse_threads_)
		: err(e), o(opts), dry(dry_), want_seq(want_seq_), parse_threads(parse_threads_) {}
	~Reader() { stop(); release(false); }

	// the queues (n_batches: `depth` on the device, one being filled, one being written, one spare on either side), the first
	// two batches, the two threads; false: not even those two batches could be had (nothing was started)
	bool start(int n_batches);
	// ends the two threads: once the input has been read to its end or the run has failed (the producer leaves a wait on an
	// aborted queue), also when start() failed or was never called
	void stop();
	// the batches of a finished run: kept for the next one (page-locked, within the cache's size) or freed
	void release(bool keep);

	Batch* new_batch();
	void allocator(int n_more);
	void producer();
};

// ---- the output side of stage 3: the output files, a pool that formats a batch's records, an appender thread that writes them ----
struct OutBufs;      // a sub-range's formatted text, one buffer per output file (td_stream_writer.cpp)

struct Writer {
	RunError& err;
	TdWorkers pool;
	const int num_alternatives;
	bool fingerprint_text = false;      // td_stream_opts.fingerprint_text: ";FP:ACGT" instead of ";FP:27"
	std::vector<int> fds;
	std::vector<int64_t> file_off;
	int64_t bytes_out = 0;
	double dbg_format = 0, dbg_pwrite = 0;
	// Appends run beside the formatting of the next batch: every append is a pwrite at an offset fixed when the batch was
	// formatted, so the order in which they reach the files is free.  Two sets of formatted text; a set is reused once its
	// appends have been written (append_wait).
	struct Wr { size_t file, k0, k1; int64_t at; };
	struct AppendJob { int set; std::vector<Wr> wr; };
	std::unique_ptr<TdWorkers> append_pool;
	std::thread appender;
	std::mutex ap_mu;
	std::condition_variable ap_cv;
	std::deque<AppendJob> ap_jobs;
	bool ap_busy[2] = { false, false }, ap_stop = false, ap_started = false;
	int ap_errno = 0, ap_set = 0;
	std::vector<OutBufs> ap_bufs[2];

	Writer(RunError& e, int n_threads, int num_alternatives_);
	~Writer();

	// creates the output files; false: `why` says which one could not be created, and none of them stays open
	bool open(const std::vector<std::string>& names, std::string& why);
	// format the records of one batch per output file (on the pool) and hand the appends (in input order per file) to the
	// appender thread; finish() before the files are closed
	bool write_batch(Batch* b, const int32_t* ctype, const int32_t* cbar, size_t file_base);
	// waits for the appends of every batch written; false if one of them failed
	bool finish() { return append_wait(-1); }
	// stops the appender (after a failure appends may still be queued: none may outlive the descriptors) and closes the files;
	// the errno of the first close that failed, 0 if none did
	int close();

	void append_loop();
	// waits until the appends of `set` (-1: of every set) are in the files; false if one of them failed
	bool append_wait(int set);
	void append_stop();
};

// td_stream_opts as the run uses them (the defaults of include/tagdust_io.h); td_stream.cpp
td_stream_opts resolve_opts(const td_stream_opts* opts, bool reference_batches);

// ---- what a run over several files in lock-step shares with the next such run (td_stream_reader.cpp) ----
// compare_read_names(), src/io.c:2128-2393: the same place on the flow cell (CASAVA 1.8 / <= 1.7 names), else the same name up
// to the first blank or ';'.  The format is taken from the first name seen (`detected`, like the reference's static).
bool names_differ(const std::string& a, const std::string& b, int& detected);
// name of record i of a batch
std::string record_name(const Batch& b, int64_t i);
// The lock-step check (barcode_hmm.c:257-289, merge.c:164-193): batch j of each of the K files holds the same number of records (a
// missing batch, b[k] == NULL: that file has ended, counts as a different number), and in the first batches (`first`, cleared here)
// the first 1000 names of every file name the same reads as file 0's (`name_format`: names_differ's state, -1 before the first
// call).  The objection, starting with `prefix`, or empty.  Not every b[k] may be NULL.
std::string lockstep_objection(const std::string& prefix, Batch* const* b, const char* const* paths, int K, bool& first, int& name_format);
// The end of a run's readers, the same after a failure: both queues of every reader aborted (a producer still at work leaves
// its wait; after a run that read its input to the end nothing waits on them any more), the threads ended, what they counted
// added to the caller's sums, the batches released (keep: into the cache for the next run).
void finish_readers(const std::vector<std::unique_ptr<Reader>>& readers, bool keep, int64_t& bytes_in, double& parse_s, double& read_s);

} // namespace tdstream
