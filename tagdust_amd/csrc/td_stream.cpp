// td_stream.cpp -- input files of any size through the decode path as a pipeline (include/tagdust_io.h): td_stream_run, one
// input file on one device (td_stream_survey: the same without a write stage), and td_stream_run_multi, the K input files of a paired / multi-read run in lock-step on N devices.
//
//   reader / parser thread (per file) caller's thread                     writer thread
//   block k+1: read or map, find      batch k: td_submit ... td_wait      batch k-1: format per output file, append
//   records, base-code them into      (several batches in flight on the
//   the next batch's pinned buffers   devices)
//
// It replaces the reference's batch loop around run_pHMM (src/barcode_hmm.c:244-385): read_fasta_fastq() of <= 1 000 001
// records of every file (io.c:1684-1815, through popen("cat|zcat|bzcat"), io.c:382-608) -> run_pHMM -> print_all() appending
// to the per-barcode files (io.c:757-1016) -- with the three steps of consecutive batches running side by side, each of the
// two host steps on several threads.  Batches hold exactly `batch_reads` records like the reference's (the -ref artifact
// filter's per-thread read ranges are taken over a batch, barcode_hmm.c:2478-2583, so the boundaries are part of the result).
//
// The pieces: a Reader per input file (Source, parse pool, the batches it owns, its allocator and producer threads), one
// run_stages() for both entry points (the device stage over tuples of one batch per file, the write-stage thread, the
// teardown), one Writer (output files, format pool, appender thread) and one RunError that all of them share: the first
// failure anywhere is the run's message and ends every stage.  An entry point validates its arguments, sets these up and
// gives run_stages what is its own: the check of a tuple and what the write stage does with a finished one.
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <math.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/tagdust_io.h"
#include "../../include/tagdust_molecules.h"   // td_mol_mate_next: pair mode of td_stream_run_multi
#include "td_io_internal.h"
#include "td_merge_internal.h"
#include "td_workers.h"

namespace {

double now_s()
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

// ---- input text: one mapping of a plain file, or blocks read from a pipe ----
struct Block {
	const char* data = nullptr;
	int64_t len = 0;
	char* owned = nullptr;          // malloc'ed (pipe input); a mapped file is owned by the Source
	~Block() { free(owned); }
};

class Source {
public:
	~Source()
	{
		if (map_ && map_ != MAP_FAILED) munmap(map_, (size_t)map_len_);
		if (pipe_) pclose(pipe_);
		if (fd_ >= 0) close(fd_);
	}
	bool open(const char* path, int64_t block_bytes, std::string& err)
	{
		block_ = block_bytes;
		const std::string p = path;
		auto ends = [&](const char* sfx) { const size_t n = strlen(sfx); return p.size() >= n && p.compare(p.size() - n, n, sfx) == 0; };
		struct stat st;
		if (p != "-" && stat(path, &st) != 0) { err = "td_stream_run: cannot find input file " + p; return false; }
		std::string q;
		for (char ch : p) { if (ch == '\'') q += "'\\''"; else q += ch; }
		const bool sam = ends(".sam") || ends(".sam.gz"), bam = ends(".bam") || ends(".bam.gz");
		if (sam || bam) {
			// io_handler(), io.c:467-575: alignments come as text from `samtools view` (-S for SAM text), secondary and
			// QC-failed records dropped (-F 768); a .gz of either goes through zcat first.  read_sam_chunk (io.c:1498-1660) takes
			// QNAME, SEQ and QUAL of every line that does not start with '@'.
			const std::string view = std::string("samtools view ") + (sam ? "-SF 768 " : "-F 768 ");
			cmd_ = ends(".gz") ? "zcat -- '" + q + "' | " + view + "-" : view + "'" + q + "'";
			if (p == "-") { err = "td_stream_run: SAM/BAM input from stdin is not supported"; return false; }
			pipe_ = popen(cmd_.c_str(), "r");
			if (!pipe_) { err = "td_stream_run: cannot start " + cmd_; return false; }
			fd_in_ = fileno(pipe_);
			sam_ = true;
			return true;
		}
		if (ends(".gz") || ends(".bz2")) {             // io_handler(), io.c:382-608: zcat / bzcat through popen
			cmd_ = std::string(ends(".gz") ? "zcat" : "bzcat") + " -- '" + q + "'";
			pipe_ = popen(cmd_.c_str(), "r");
			if (!pipe_) { err = "td_stream_run: cannot start " + cmd_; return false; }
			fd_in_ = fileno(pipe_);
			return true;
		}
		if (p == "-") { fd_in_ = 0; return true; }
		fd_ = ::open(path, O_RDONLY);
		if (fd_ < 0) { err = "td_stream_run: cannot open " + p + ": " + strerror(errno); return false; }
		if (S_ISREG(st.st_mode)) {
			map_len_ = st.st_size;
			if (map_len_ == 0) { eof_ = true; return true; }
			map_ = mmap(nullptr, (size_t)map_len_, PROT_READ, MAP_PRIVATE, fd_, 0);
			if (map_ != MAP_FAILED) {
				(void)madvise(map_, (size_t)map_len_, MADV_SEQUENTIAL);
				fasta_ = ((const char*)map_)[0] == '>';
				return true;
			}
			map_ = nullptr;                            // fall back to read()
		}
		fd_in_ = fd_;
		return true;
	}
	// the next block of whole records (nullptr at the end); *read_s += time spent waiting for bytes
	std::shared_ptr<Block> next(double* read_s, std::string& err)
	{
		if (eof_) return nullptr;
		auto b = std::make_shared<Block>();
		if (map_) {
			const char* text = (const char*)map_;
			int64_t end = map_pos_ + block_;
			end = end >= map_len_ ? map_len_ : td_next_record_start(text, map_len_, end, fasta_);
			b->data = text + map_pos_; b->len = end - map_pos_;
			(void)madvise((void*)((uintptr_t)(text + map_pos_) & ~(uintptr_t)4095), (size_t)(b->len + 4096), MADV_WILLNEED);
			map_pos_ = end;
			if (map_pos_ >= map_len_) eof_ = true;
			return b;
		}
		// pipe / stdin: fill a buffer, cut it at the last record start found in its tail, carry the rest over
		const double t0 = now_s();
		const int64_t cap = block_ + (int64_t)carry_.size() + 1;
		b->owned = (char*)malloc((size_t)cap);
		if (!b->owned) { err = "td_stream_run: out of memory"; return nullptr; }
		int64_t have = (int64_t)carry_.size();
		if (have) memcpy(b->owned, carry_.data(), (size_t)have);
		carry_.clear();
		bool end_of_input = false;
		while (have < cap - 1) {
			const ssize_t r = read(fd_in_, b->owned + have, (size_t)(cap - 1 - have));
			if (r < 0) { if (errno == EINTR) continue; err = std::string("td_stream_run: read failed: ") + strerror(errno); return nullptr; }
			if (r == 0) { end_of_input = true; break; }
			have += r;
		}
		if (end_of_input && pipe_) {
			// the decompressor's verdict: a truncated or corrupt .gz / .bz2 ends the stream early with a non-zero status -- an error,
			// not the end of the input (io_handler's pclose, io.c:382-608, ignores it; a partial set of output files helps nobody)
			const int status = pclose(pipe_);
			pipe_ = nullptr;
			if (status != 0) {
				err = "td_stream_run: `" + cmd_ + "` failed (status " + std::to_string(status) + "): truncated or corrupt input" + (sam_ ? ", or no samtools on PATH" : "");
				return nullptr;
			}
		}
		*read_s += now_s() - t0;
		if (sam_) {
			std::shared_ptr<Block> r = sam_block(b, have, end_of_input, err);
			if (r && r->len == 0) return eof_ ? nullptr : next(read_s, err);   // header lines only
			return r;
		}
		if (first_block_) { fasta_ = have > 0 && b->owned[0] == '>'; first_block_ = false; }
		int64_t cut = have;
		if (!end_of_input) {
			// the last record start in the buffer: search forward from ever earlier points of the tail
			cut = -1;
			for (int64_t back = 1 << 16; cut < 0; back *= 4) {
				int64_t from = have - back;
				if (from < 1) from = 1;
				int64_t p = td_next_record_start(b->owned, have, from, fasta_), last = -1;
				while (p < have) { last = p; p = td_next_record_start(b->owned, have, p + 1, fasta_); }
				if (last > 0) cut = last;
				else if (from == 1) { err = "td_stream_run: no record boundary within a block of input (raise block_bytes)"; return nullptr; }
			}
			carry_.assign(b->owned + cut, b->owned + have);
		} else {
			eof_ = true;
		}
		b->data = b->owned; b->len = cut;
		if (cut == 0 && eof_) return nullptr;
		return b;
	}

private:
	// Alignment text -> the four-line records the parser takes: '@' QNAME, SEQ, '+', QUAL (fields 1, 10 and 11 of every line that
	// is not a header line, read_sam_chunk, io.c:1498-1660).  Whole lines only; the rest is carried over to the next block.
	std::shared_ptr<Block> sam_block(std::shared_ptr<Block> b, int64_t have, const bool end_of_input, std::string& err)
	{
		int64_t cut = have;
		if (!end_of_input) {
			while (cut > 0 && b->owned[cut - 1] != '\n') --cut;
			if (cut == 0) { err = "td_stream_run: no line end within a block of SAM input (raise block_bytes)"; return nullptr; }
			carry_.assign(b->owned + cut, b->owned + have);
		} else {
			eof_ = true;
		}
		auto out = std::make_shared<Block>();
		out->owned = (char*)malloc((size_t)cut + 8);      // a record shrinks: 11+ tab-separated fields against 3 of them and 5 bytes
		if (!out->owned) { err = "td_stream_run: out of memory"; return nullptr; }
		char* o = out->owned;
		const char* t = b->owned;
		const char* const end = t + cut;
		auto blank = [](const char ch) { return ch == ' ' || ch == '\t' || ch == '\r' || ch == '\v' || ch == '\f'; };
		while (t < end) {
			const char* nl = (const char*)memchr(t, '\n', (size_t)(end - t));
			const char* le = nl ? nl : end;
			if (le > t && t[0] != '@') {
				const char* f[12];
				int nf = 0;
				const char* c = t;
				f[nf++] = c;
				while (c < le && nf < 12) { if (blank(*c)) f[nf++] = c + 1; ++c; }
				if (nf < 11) { err = "td_stream_run: SAM line with fewer than 11 fields: " + std::string(t, (size_t)std::min<int64_t>(le - t, 60)); return nullptr; }
				auto field_end = [&](const char* s) { while (s < le && !blank(*s)) ++s; return s; };
				const char* n1 = field_end(f[0]);
				const char* s1 = field_end(f[9]);
				const char* q1 = field_end(f[10]);
				if (q1 - f[10] != s1 - f[9]) { err = "td_stream_run: SAM record without one quality per base: " + std::string(f[0], (size_t)(n1 - f[0])); return nullptr; }
				*o++ = '@'; memcpy(o, f[0], (size_t)(n1 - f[0])); o += n1 - f[0]; *o++ = '\n';
				memcpy(o, f[9], (size_t)(s1 - f[9])); o += s1 - f[9]; *o++ = '\n';
				*o++ = '+'; *o++ = '\n';
				memcpy(o, f[10], (size_t)(q1 - f[10])); o += q1 - f[10]; *o++ = '\n';
			}
			t = nl ? nl + 1 : end;
		}
		out->data = out->owned; out->len = o - out->owned;
		return out;
	}

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
	int64_t* offs = nullptr;
	td_read_result* res = nullptr;
	std::vector<Piece> pieces;
	int64_t cap_reads = 0;     // offs / res hold this many reads
	const uint8_t* seq_src = nullptr;   // what the writer prints: seq_out, or codes for a file that is not decoded (run_rna_dust)
};

// Page-locked batch buffers outlive a run: page-locking runs at about 1 GB/s, which is most of what a short file costs.  The
// buffers of the last run (up to 1 GiB) wait here for the next one of the same process; td_stream_release frees them.
std::mutex g_cache_mu;
std::vector<Batch*> g_cache;
const size_t kCacheBytes = (size_t)1 << 30;

size_t batch_bytes(const Batch* b)
{
	return b->cap_codes + b->cap_seq + (size_t)b->cap_reads * (sizeof(int64_t) + sizeof(td_read_result));
}

// batch buffers: page-locked for the device; plain memory for a parse-only run (no GPU runtime needed then)
void* buf_alloc(bool dry, size_t bytes) { return dry ? malloc(bytes ? bytes : 1) : td_host_alloc(bytes); }
void buf_free(bool dry, void* p) { if (dry) free(p); else td_host_free(p); }

bool grow_buf(bool dry, uint8_t** p, size_t* cap, size_t need, size_t keep, size_t hint)
{
	if (*cap >= need) return true;
	size_t want = need + need / 4 + 4096;
	if (want < hint) want = hint;          // what a whole batch is expected to need: allocated once, reused by later batches
	uint8_t* q = (uint8_t*)buf_alloc(dry, want);
	if (!q) return false;
	if (*p && keep) memcpy(q, *p, keep);
	if (*p) buf_free(dry, *p);
	*p = q; *cap = want;
	return true;
}

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

// "%d"
inline int put_int(char* w, int v)
{
	char tmp[16];
	int k = 0;
	unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
	do { tmp[k++] = (char)('0' + u % 10); u /= 10; } while (u);
	int o = 0;
	if (v < 0) w[o++] = '-';
	while (k) w[o++] = tmp[--k];
	return o;
}

// "%0.2f" of a float, digit for digit what printf prints: the float times 100 is exact in double (24 x 7 significant bits),
// nearbyint rounds it half-to-even like printf rounds the exact decimal expansion; anything unusual goes to snprintf
inline int put_q(char* w, float q)
{
	const double x = (double)q * 100.0;
	if (!(x >= 0.0 && x < 1.0e15) || (x == 0.0 && std::signbit(q))) return snprintf(w, 48, "%0.2f", (double)q);   // (at most 42 characters)
	unsigned long long u = (unsigned long long)nearbyint(x);
	char tmp[24];
	int k = 0;
	tmp[k++] = (char)('0' + u % 10); u /= 10;
	tmp[k++] = (char)('0' + u % 10); u /= 10;
	tmp[k++] = '.';
	do { tmp[k++] = (char)('0' + u % 10); u /= 10; } while (u);
	int o = 0;
	while (k) w[o++] = tmp[--k];
	return o;
}

// formats the records of one piece sub-range into one buffer per output file (print_all(), io.c:917-1001)
struct OutBufs { std::vector<Bytes> file; };

// The rewritten sequence of a read is base codes 0..4 with removed positions as 65: the stretches of kept bases become the
// records.  Sixteen bytes at a time where the host has SSE2 (every x86-64 has): the write stage is the slower host stage of the
// pipeline, and these two loops were half of its formatting time.
#if defined(__SSE2__)
// number of leading bytes of s[0, n) that are >= 5 (GE = true) / < 5 (GE = false)
template <bool GE>
inline int64_t span_of(const uint8_t* s, int64_t n)
{
	int64_t g = 0;
	const __m128i five = _mm_set1_epi8(5);
	for (; g + 16 <= n; g += 16) {
		const __m128i v = _mm_loadu_si128((const __m128i*)(s + g));
		const unsigned ge = (unsigned)_mm_movemask_epi8(_mm_cmpeq_epi8(_mm_max_epu8(v, five), v));   // bit k: s[g + k] >= 5
		const unsigned stop = GE ? (~ge & 0xFFFFu) : ge;   // first byte that ends the span
		if (stop) return g + __builtin_ctz(stop);
	}
	while (g < n && ((s[g] >= 5) == GE)) g++;
	return g;
}
// w[k] = "ACGTN"[s[k]] for codes 0..4
inline void codes_to_text(char* w, const uint8_t* s, size_t n)
{
	size_t k = 0;
	const __m128i a = _mm_set1_epi8('A'), c1 = _mm_set1_epi8(1), c2 = _mm_set1_epi8(2), c3 = _mm_set1_epi8(3), c4 = _mm_set1_epi8(4);
	const __m128i d1 = _mm_set1_epi8('C' - 'A'), d2 = _mm_set1_epi8('G' - 'A'), d3 = _mm_set1_epi8('T' - 'A'), d4 = _mm_set1_epi8('N' - 'A');
	for (; k + 16 <= n; k += 16) {
		const __m128i v = _mm_loadu_si128((const __m128i*)(s + k));
		__m128i o = a;
		o = _mm_add_epi8(o, _mm_and_si128(_mm_cmpeq_epi8(v, c1), d1));
		o = _mm_add_epi8(o, _mm_and_si128(_mm_cmpeq_epi8(v, c2), d2));
		o = _mm_add_epi8(o, _mm_and_si128(_mm_cmpeq_epi8(v, c3), d3));
		o = _mm_add_epi8(o, _mm_and_si128(_mm_cmpeq_epi8(v, c4), d4));
		_mm_storeu_si128((__m128i*)(w + k), o);
	}
	static const char alphabet[] = "ACGTNN";
	for (; k < n; k++) w[k] = alphabet[s[k]];
}
#else
template <bool GE>
inline int64_t span_of(const uint8_t* s, int64_t n) { int64_t g = 0; while (g < n && ((s[g] >= 5) == GE)) g++; return g; }
inline void codes_to_text(char* w, const uint8_t* s, size_t n) { static const char alphabet[] = "ACGTNN"; for (size_t k = 0; k < n; k++) w[k] = alphabet[s[k]]; }
#endif

// ctype / cbar: read_type and barcode of the record as the controller combines them over the input files of a run
// (barcode_hmm.c:329-351; NULL: this file's own); file_base: index of this input file's first output file (io.c:917-1001: c)
void format_records(const Batch& b, const Piece& pc, int64_t lo, int64_t hi, int num_alternatives, OutBufs& out,
                    const int32_t* ctype = nullptr, const int32_t* cbar = nullptr, size_t file_base = 0, bool fingerprint_text = false)
{
	const char* text = pc.blk->data;
	const std::vector<TdRec>& recs = *pc.recs;
	char head[352];                                        // (";FP:" + up to 255 bases + ";RQ:" + the quality)
	const size_t n_files = out.file.size();
	for (int64_t r = lo; r < hi; r++) {
		const TdRec& rec = recs[(size_t)r];
		const int64_t i = pc.first + (r - pc.lo);             // index in the batch
		const td_read_result& rr = b.res[i];
		size_t f;                                              // io.c:923-934
		const int32_t rtype = ctype ? ctype[i] : rr.read_type, rbar = cbar ? cbar[i] : rr.barcode;
		if ((rtype & 0xFF) == TD_EXTRACT_DUPLICATE) continue;  // dedup: not the first read of its molecule, and no failure either
		if (rtype == TD_EXTRACT_SUCCESS) f = (rbar != -1) ? (size_t)(rbar & 0xFF) : 0;
		else f = (size_t)num_alternatives - 1;
		f += file_base;
		const uint8_t* s = (b.seq_src ? b.seq_src : b.seq_out) + b.offs[i];
		const int64_t len = b.offs[i + 1] - b.offs[i];
		const char* q = rec.qual_off >= 0 ? text + rec.qual_off : nullptr;
		int head_len = -1;
		int64_t g = 0;
		while (g < len) {
			g += span_of<true>(s + g, len - g);                // removed positions (65) split the read into records
			const int64_t g0 = g;
			g += span_of<false>(s + g, len - g);
			if (g == g0) break;
			if (f < n_files) {                                 // io.c:955-975: "@<name>[;FP:%d];RQ:%0.2f"
				if (head_len < 0) {
					int k = 0;
					if (rr.fingerprint != -1) {
						memcpy(head, ";FP:", 4);
						if (fingerprint_text) { (void)td_fingerprint_text(rr.fingerprint, head + 4); k = 4 + (rr.fingerprint & 0xFF); }   // io.c:960-963
						else k = 4 + put_int(head + 4, rr.fingerprint);
					}
					memcpy(head + k, ";RQ:", 4); k += 4;
					k += put_q(head + k, rr.mapq);
					head[k++] = '\n';
					head_len = k;
				}
				const size_t run = (size_t)(g - g0);
				Bytes& o = out.file[f];
				const size_t total = 1 + (size_t)rec.name_len + (size_t)head_len + run + 3 + run + 1;
				char* w = o.room(total);
				*w++ = '@';
				memcpy(w, text + rec.name_off, (size_t)rec.name_len); w += rec.name_len;
				memcpy(w, head, (size_t)head_len); w += head_len;
				codes_to_text(w, s + g0, run);
				w += run;
				*w++ = '\n'; *w++ = '+'; *w++ = '\n';
				if (q) memcpy(w, q + g0, run); else memset(w, '.', run);
				w += run;
				*w++ = '\n';
				o.n += total;
			}
			f += (size_t)num_alternatives;
		}
	}
}

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

// ---- stage 1 of one input file: its source, the batches it owns, an allocator thread and a producer thread with a parse pool ----
struct Reader {
	RunError& err;
	const td_stream_opts o;
	const bool dry;            // batch buffers in plain memory: a file that no device sees
	const bool want_seq;       // page-locked room for rewritten sequences (not for a file that goes through TD_MODE_RNA_DUST)
	const int parse_threads;
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
	bool start(int n_batches)
	{
		parse_pool.reset(new TdWorkers(parse_threads));
		ready.reset(new Queue<Batch*>((size_t)n_batches));
		free_list.reset(new Queue<Batch*>((size_t)n_batches));
		err.watch(ready.get());
		err.watch(free_list.get());
		for (int k = 0; k < 2; k++) {
			Batch* b = new_batch();
			if (!b) return false;
			free_list->push(b);
		}
		t_alloc = std::thread([this, n_batches] { allocator(n_batches - 2); });
		t_prod = std::thread([this] { producer(); });
		return true;
	}

	// ends the two threads: once the input has been read to its end or the run has failed (the producer leaves a wait on an
	// aborted queue), also when start() failed or was never called
	void stop()
	{
		if (t_prod.joinable()) t_prod.join();
		{ std::lock_guard<std::mutex> lk(all_mu); stop_alloc = true; }
		hint_cv.notify_all();
		if (free_list) free_list->abort();          // (an allocator waiting to hand over a batch)
		if (t_alloc.joinable()) t_alloc.join();
	}

	// the batches of a finished run: kept for the next one (page-locked, within the cache's size) or freed
	void release(bool keep)
	{
		std::lock_guard<std::mutex> lk(g_cache_mu);
		size_t held = 0;
		for (const Batch* q : g_cache) held += batch_bytes(q);
		for (Batch* q : all) {
			if (!dry && keep && q->codes && held + batch_bytes(q) <= kCacheBytes) {
				q->pieces.clear(); q->n = 0; q->n_bases = 0; q->seq_src = nullptr;
				held += batch_bytes(q);
				g_cache.push_back(q);
				continue;
			}
			buf_free(dry, q->codes); buf_free(dry, q->seq_out); buf_free(dry, q->offs); buf_free(dry, q->res);
			delete q;
		}
		all.clear();
	}

	Batch* new_batch()
	{
		if (!dry) {   // one the last run left behind?
			std::lock_guard<std::mutex> lk(g_cache_mu);
			for (size_t k = 0; k < g_cache.size(); k++)
				if (g_cache[k]->cap_reads >= o.batch_reads) {
					Batch* b = g_cache[k];
					g_cache.erase(g_cache.begin() + (long)k);
					b->offs[0] = 0;
					std::lock_guard<std::mutex> lk2(all_mu);
					all.push_back(b);
					return b;
				}
		}
		Batch* b = new Batch();
		b->cap_reads = o.batch_reads;
		b->offs = (int64_t*)buf_alloc(dry, sizeof(int64_t) * ((size_t)o.batch_reads + 1));
		b->res = (td_read_result*)buf_alloc(dry, sizeof(td_read_result) * (size_t)o.batch_reads);
		if (!b->offs || !b->res) { buf_free(dry, b->offs); buf_free(dry, b->res); delete b; return nullptr; }
		b->offs[0] = 0;
		{ std::lock_guard<std::mutex> lk(all_mu); all.push_back(b); }
		return b;
	}

	// The batch buffers are page-locked, and page-locking runs at about 1 GB/s: the pipeline starts with two batches and this
	// thread adds the others, sized for a whole batch (known after the first block), while the first ones are already at work.
	void allocator(int n_more)
	{
		size_t hint = 0;
		{
			std::unique_lock<std::mutex> lk(all_mu);
			hint_cv.wait(lk, [&] { return hint_ready || stop_alloc; });
			if (stop_alloc) return;
			hint = batch_hint;
		}
		for (int k = 0; k < n_more; k++) {
			{ std::lock_guard<std::mutex> lk(all_mu); if (stop_alloc) return; }
			Batch* b = new_batch();
			if (!b || !grow_buf(dry, &b->codes, &b->cap_codes, hint, 0, hint) || (want_seq && !grow_buf(dry, &b->seq_out, &b->cap_seq, hint, 0, hint))) return;   // (the pipeline runs with what it has)
			if (!free_list->push(b)) return;
		}
	}

	// read / map a block, find its records, hand them out to batches, base-code them
	void producer()
	{
		Batch* cur = nullptr;
		const int P = parse_pool->size();
		for (;;) {
			std::string e;
			std::shared_ptr<Block> blk = src.next(&read_s, e);
			if (!blk) { if (!e.empty()) { err.fail(e); return; } break; }
			const double t0 = now_s();
			bytes_in += blk->len;
			// records: P chunks cut at record starts, each parsed by the reference's line state machine
			const bool fasta = blk->len > 0 && blk->data[0] == '>';
			std::vector<int64_t> cut(1, 0);
			const int nchunk_want = blk->len < (1 << 20) ? 1 : P * 4;
			for (int t = 1; t < nchunk_want; t++) {
				const int64_t p = td_next_record_start(blk->data, blk->len, blk->len / nchunk_want * t, fasta);
				if (p < blk->len && p > cut.back()) cut.push_back(p);
			}
			cut.push_back(blk->len);
			const int nchunk = (int)cut.size() - 1;
			std::vector<std::shared_ptr<std::vector<TdRec>>> recs((size_t)nchunk);
			for (auto& r : recs) r = std::make_shared<std::vector<TdRec>>();
			std::vector<int64_t> bad((size_t)nchunk, -1);
			parse_pool->run(nchunk, [&](int64_t k) {
				std::vector<TdRec>& v = *recs[(size_t)k];
				v.reserve((size_t)((cut[(size_t)k + 1] - cut[(size_t)k]) / 200 + 16));
				td_parse_range(blk->data, cut[(size_t)k], cut[(size_t)k + 1], v);
				// "Length of sequence and base qualities differ" ends the reference's run (io.c:1776-1781)
				for (size_t i = 0; i < v.size(); i++)
					if (v[i].qual_off >= 0 && v[i].qual_len != (v[i].seq_off >= 0 ? v[i].seq_len : 0)) { bad[(size_t)k] = (int64_t)i; break; }
			});
			dbg_pass1 += now_s() - t0;
			for (int k = 0; k < nchunk; k++)
				if (bad[(size_t)k] >= 0) {
					const TdRec& q = (*recs[(size_t)k])[(size_t)bad[(size_t)k]];
					char msg[256];
					snprintf(msg, sizeof msg, "td_stream_run: record \"%.*s\": sequence has %d characters, base qualities %d",
					         q.name_len < 60 ? q.name_len : 60, blk->data + q.name_off, q.seq_off >= 0 ? q.seq_len : 0, q.qual_len);
					err.fail(msg);
					return;
				}
			{   // bases a full batch of reads like this block's will hold (+6 %)
				int64_t nrec = 0, nb = 0;
				for (auto& r : recs) { nrec += (int64_t)r->size(); for (const TdRec& q : *r) nb += q.seq_off >= 0 ? q.seq_len : 0; }
				if (nrec > 0) {
					const size_t h = (size_t)((double)nb / (double)nrec * (double)o.batch_reads * 1.06) + 4096;
					std::lock_guard<std::mutex> lk(all_mu);
					if (h > batch_hint) batch_hint = h;
					hint_ready = true;
					hint_cv.notify_all();
				}
			}
			// hand the records out to batches of exactly batch_reads, in order (offsets by a running sum); the pieces handed out
			// are base-coded (init_nuc_code) in parallel and full batches passed on whenever two are waiting, and before this
			// thread might have to wait for a free batch
			struct Job { Batch* b; size_t piece; };
			std::vector<Job> jobs;
			std::vector<Batch*> full;
			double t_seg = t0;
			auto flush = [&]() -> bool {
				const double tf0 = now_s();
				std::vector<Batch*> touched = full;
				if (cur) touched.push_back(cur);
				for (Batch* b : touched) {
					// page-locked room for the codes going in and the rewritten sequences coming back (bases of earlier pieces of
					// a batch are already encoded: keep them)
					bool mine = false;
					size_t keep = 0;
					for (const Job& j : jobs) if (j.b == b) { keep = (size_t)b->offs[b->pieces[j.piece].first]; mine = true; break; }
					if (!mine) continue;
					if (!grow_buf(dry, &b->codes, &b->cap_codes, (size_t)b->n_bases + 1, keep, batch_hint) ||
					    (want_seq && !grow_buf(dry, &b->seq_out, &b->cap_seq, (size_t)b->n_bases + 1, 0, batch_hint))) { err.fail("td_stream_run: page-locked memory exhausted"); return false; }
				}
				dbg_grow += now_s() - tf0;
				const double tf1 = now_s();
				struct Sub { Batch* b; size_t piece; int64_t lo, hi; };
				std::vector<Sub> subs;
				for (const Job& j : jobs) {
					const Piece& pc = j.b->pieces[j.piece];
					for (int64_t a = pc.lo; a < pc.hi; a += 16384) subs.push_back(Sub{ j.b, j.piece, a, std::min<int64_t>(a + 16384, pc.hi) });
				}
				parse_pool->run((int64_t)subs.size(), [&](int64_t k) {
					const Sub& sb = subs[(size_t)k];
					const Piece& pc = sb.b->pieces[sb.piece];
					const std::vector<TdRec>& v = *pc.recs;
					for (int64_t r = sb.lo; r < sb.hi; r++) {
						const TdRec& q = v[(size_t)r];
						if (q.seq_off < 0) continue;
						uint8_t* dst = sb.b->codes + sb.b->offs[pc.first + (r - pc.lo)];
						const unsigned char* sq = (const unsigned char*)pc.blk->data + q.seq_off;
						td_encode_bases(sq, dst, q.seq_len);
					}
				});
				jobs.clear();
				dbg_encode += now_s() - tf1;
				parse_s += now_s() - t_seg;                             // (time spent waiting for a free batch is not parsing)
				for (Batch* b : full) if (!ready->push(b)) return false;
				full.clear();
				t_seg = now_s();
				return true;
			};
			for (int k = 0; k < nchunk; k++) {
				const std::vector<TdRec>& v = *recs[(size_t)k];
				int64_t lo = 0;
				while (lo < (int64_t)v.size()) {
					if (!cur) {
						if (!full.empty() && !flush()) return;
						parse_s += now_s() - t_seg;
						if (!free_list->pop(cur)) return;                  // aborted
						t_seg = now_s();
						cur->n = 0; cur->n_bases = 0; cur->pieces.clear();
					}
					const int64_t take = std::min<int64_t>((int64_t)v.size() - lo, (int64_t)o.batch_reads - cur->n);
					Piece pc; pc.blk = blk; pc.recs = recs[(size_t)k]; pc.lo = lo; pc.hi = lo + take; pc.first = cur->n;
					int64_t total = cur->n_bases;
					for (int64_t r = lo; r < lo + take; r++) {
						total += v[(size_t)r].seq_off >= 0 ? v[(size_t)r].seq_len : 0;
						cur->offs[cur->n + (r - lo) + 1] = total;
					}
					cur->n += take; cur->n_bases = total;
					cur->pieces.push_back(pc);
					jobs.push_back(Job{ cur, cur->pieces.size() - 1 });
					lo += take;
					if (cur->n == o.batch_reads) { full.push_back(cur); cur = nullptr; }
				}
			}
			if (!flush()) return;
		}
		if (getenv("TD_STREAM_DEBUG")) fprintf(stderr, "td_stream: records %.3f s, buffers %.3f s, base codes %.3f s (parse stage %.3f s)\n", dbg_pass1, dbg_grow, dbg_encode, parse_s);
		if (cur && cur->n > 0) { if (!ready->push(cur)) return; }
		else if (cur) free_list->push(cur);
		ready->close();
	}
};

// ---- the output side of stage 3: the output files, a pool that formats a batch's records, an appender thread that writes them ----
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

	Writer(RunError& e, int n_threads, int num_alternatives_) : err(e), pool(n_threads), num_alternatives(num_alternatives_) {}
	~Writer() { (void)close(); }

	// creates the output files; false: `why` says which one could not be created, and none of them stays open
	bool open(const std::vector<std::string>& names, std::string& why)
	{
		for (auto& nm : names) {
			const int fd = ::open(nm.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
			if (fd < 0) { why = nm + ": " + strerror(errno); (void)close(); return false; }
			fds.push_back(fd);
		}
		file_off.assign(fds.size(), 0);
		return true;
	}
	// waits for the appends of every batch written; false if one of them failed
	bool finish() { return append_wait(-1); }
	// stops the appender (after a failure appends may still be queued: none may outlive the descriptors) and closes the files;
	// the errno of the first close that failed, 0 if none did
	int close()
	{
		append_stop();
		int first = 0;
		for (int fd : fds) if (::close(fd) != 0 && !first) first = errno;
		fds.clear();
		return first;
	}

	void append_loop()
	{
		for (;;) {
			AppendJob job;
			{
				std::unique_lock<std::mutex> lk(ap_mu);
				ap_cv.wait(lk, [&] { return ap_stop || !ap_jobs.empty(); });
				if (ap_jobs.empty()) return;
				job = std::move(ap_jobs.front());
				ap_jobs.pop_front();
			}
			const double t0 = now_s();
			const std::vector<OutBufs>& bufs = ap_bufs[job.set];
			std::vector<int> wrc(job.wr.size(), 0);
			append_pool->run((int64_t)job.wr.size(), [&](int64_t t) {
				const Wr& w = job.wr[(size_t)t];
				int64_t at = w.at;
				for (size_t k = w.k0; k < w.k1; k++) {
					const Bytes& sb = bufs[k].file[w.file];
					size_t off = 0;
					while (off < sb.n) {
						const ssize_t r = pwrite(fds[w.file], sb.p + off, sb.n - off, (off_t)(at + (int64_t)off));
						if (r < 0) { if (errno == EINTR) continue; wrc[(size_t)t] = errno ? errno : EIO; return; }
						off += (size_t)r;
					}
					at += (int64_t)sb.n;
				}
			});
			std::lock_guard<std::mutex> lk(ap_mu);
			dbg_pwrite += now_s() - t0;
			for (int e : wrc) if (e && !ap_errno) ap_errno = e;
			ap_busy[job.set] = false;
			ap_cv.notify_all();
		}
	}
	// waits until the appends of `set` (-1: of every set) are in the files; false if one of them failed
	bool append_wait(int set)
	{
		std::unique_lock<std::mutex> lk(ap_mu);
		ap_cv.wait(lk, [&] { return set < 0 ? (!ap_busy[0] && !ap_busy[1]) : !ap_busy[set]; });
		if (ap_errno) { const int e = ap_errno; lk.unlock(); err.fail(std::string("td_stream_run: write failed: ") + strerror(e)); return false; }
		return true;
	}
	void append_stop()
	{
		{ std::lock_guard<std::mutex> lk(ap_mu); ap_stop = true; }
		ap_cv.notify_all();
		if (appender.joinable()) appender.join();
	}

	// format the records of one batch per output file (on the pool) and hand the appends (in input order per file) to the
	// appender thread; finish() before the files are closed
	bool write_batch(Batch* b, const int32_t* ctype, const int32_t* cbar, size_t file_base)
	{
		if (!ap_started) {
			ap_started = true;
			append_pool.reset(new TdWorkers(pool.size()));
			appender = std::thread([this] { append_loop(); });
		}
		const int set = ap_set;
		ap_set ^= 1;
		if (!append_wait(set)) return false;
		std::vector<OutBufs>& bufs = ap_bufs[set];
		const double t0 = now_s();
		const int W = pool.size();
		struct Sub { size_t piece; int64_t lo, hi; };
		std::vector<Sub> subs;
		const int64_t step = std::max<int64_t>(4096, (b->n + W * 4 - 1) / (W * 4));
		for (size_t p = 0; p < b->pieces.size(); p++)
			for (int64_t a = b->pieces[p].lo; a < b->pieces[p].hi; a += step)
				subs.push_back(Sub{ p, a, std::min<int64_t>(a + step, b->pieces[p].hi) });
		if (bufs.size() < subs.size()) bufs.resize(subs.size());
		for (size_t k = 0; k < subs.size(); k++) {
			if (bufs[k].file.size() != fds.size()) bufs[k].file.resize(fds.size());
			for (auto& s : bufs[k].file) s.n = 0;
		}
		pool.run((int64_t)subs.size(), [&](int64_t k) {
			const Sub& sb = subs[(size_t)k];
			format_records(*b, b->pieces[sb.piece], sb.lo, sb.hi, num_alternatives, bufs[(size_t)k], ctype, cbar, file_base, fingerprint_text);
		});
		dbg_format += now_s() - t0;
		// Appends.  Buffered writes to one file serialise on its inode lock (8 threads on one file: 8 GB/s; one thread on each of
		// nine files: 56 GB/s, tools/ubench/file_write.cpp), so a file gets one task that appends its share of every sub-range
		// in order -- or a few tasks over runs of sub-ranges when it takes most of the bytes (no barcode segment: two files)
		std::vector<Wr> wr;
		int64_t total_bytes = 0;
		std::vector<int64_t> per_file(fds.size(), 0);
		for (size_t f = 0; f < fds.size(); f++) {
			for (size_t k = 0; k < subs.size(); k++) per_file[f] += (int64_t)bufs[k].file[f].n;
			total_bytes += per_file[f];
		}
		for (size_t f = 0; f < fds.size(); f++) {
			if (!per_file[f]) continue;
			int parts = (int)((double)per_file[f] / (double)total_bytes * (double)W + 0.5);
			if (parts > 4) parts = 4;
			if (parts < 1) parts = 1;
			const int64_t target = (per_file[f] + parts - 1) / parts;
			int64_t at = file_off[f], acc = 0;
			size_t k0 = 0;
			for (size_t k = 0; k < subs.size(); k++) {
				acc += (int64_t)bufs[k].file[f].n;
				if (acc >= target || k + 1 == subs.size()) {
					if (acc > 0) wr.push_back(Wr{ f, k0, k + 1, at });
					at += acc; acc = 0; k0 = k + 1;
				}
			}
			file_off[f] += per_file[f];
			bytes_out += per_file[f];
		}
		{
			std::lock_guard<std::mutex> lk(ap_mu);
			ap_busy[set] = true;
			ap_jobs.push_back(AppendJob{ set, std::move(wr) });
		}
		ap_cv.notify_all();
		return true;
	}
};

// ---- td_stream_opts as the run uses them (the defaults of include/tagdust_io.h) ----
// The reference reads 1 000 001 records at a time (param->num_query, barcode_hmm.c:172).  Per-read results do not depend on how
// a file is cut into batches -- except through the -ref artifact filter, whose per-thread read ranges are taken over a batch:
// with a filter set (and in a parse-only run) the batches are the reference's (reference_batches), otherwise they are 2^18
// reads (one tile per wave slot of the device; a quarter of the page-locked memory and a pipeline that fills four times sooner).
td_stream_opts resolve_opts(const td_stream_opts* opts, bool reference_batches)
{
	td_stream_opts o{};
	if (opts) o = *opts;
	if (o.batch_reads <= 0) o.batch_reads = reference_batches ? 1000001 : (1 << 18);
	if (o.block_bytes <= 0) o.block_bytes = (int64_t)64 << 20;
	if (o.block_bytes < 4096) o.block_bytes = 4096;
	o.n_threads = td_stage_threads(o.n_threads, 32);
	return o;
}

// batches (record ranges of every file) in flight on the devices: the option of a context of the run, 3 when it has none
int pipeline_depth(td_ctx* ctx)
{
	int32_t depth = 3;
	if (ctx) (void)td_get_option(ctx, "pipeline_depth", &depth);
	return depth;
}

bool artifacts_active(td_ctx* ctx)
{
	int32_t art = 0;
	(void)td_get_option(ctx, "artifacts_active", &art);
	return art != 0;
}

// ---- the three stages of a run over K input files in lock-step and N devices (td_stream_run: K = 1, N = 1) ----
struct Tuple {                        // batch j of every input file: records [j * batch_reads, ...) of each
	std::vector<Batch*> b;            // [file]; the batches stay their readers'
	std::vector<int64_t> tickets;     // [file * N + device]; 0: nothing was submitted
	Tuple(int K, int N) : b((size_t)K, nullptr), tickets((size_t)(K * N), 0) {}
};

struct Target {                       // where the batches of one input file go
	td_ctx* const* ctx;               // its context on each of the N devices; NULL: no device sees this file
	bool rna;                         // run_rna_dust (TD_MODE_RNA_DUST: the reads come back unchanged) instead of the HMM
	int mate = -1;                    // pair mode: the file whose batch is this file's mate batch (td_mol_mate_next), else -1
};

// Starts the readers, runs the write stage on a thread of its own (`write` for every finished tuple in input order, then the
// wait for the writer's appends; writer == NULL: a parse-only run, no output files) and the device stage on the calling thread
// (a context is driven from one thread): a ready batch of every reader -> `check` (an error message, or empty) -> submit, at most
// `depth` tuples in flight, waited for in order.  Then the teardown, the same after a failure at any point: every ticket still
// outstanding waited for, write stage and appender ended, files closed, readers stopped, batches released.  The run's error, if
// any, is in `err`; `prefix` starts the messages of this function.
void run_stages(const std::string& prefix, RunError& err, const std::vector<std::unique_ptr<Reader>>& readers, const std::vector<Target>& dev,
                const int N, const int depth, Writer* writer, const std::function<std::string(const Tuple&)>& check,
                const std::function<bool(Tuple&)>& write, td_stream_stats& st)
{
	const int K = (int)readers.size();
	const int n_batches = depth + 4;
	Queue<std::unique_ptr<Tuple>> done((size_t)n_batches);      // (tuples left in it by a failed run are freed with it)
	err.watch(&done);
	for (auto& r : readers)
		if (!r->start(n_batches)) { err.fail(prefix + "page-locked memory exhausted"); break; }
	std::thread t_write([&] {
		std::unique_ptr<Tuple> t;
		while (done.pop(t)) {
			const double t0 = now_s();
			if (!write(*t)) return;
			st.n_reads += t->b[0]->n; st.n_batches++;
			for (Batch* b : t->b) b->pieces.clear();               // releases the blocks
			st.write_s += now_s() - t0;
			for (int k = 0; k < K; k++) if (!readers[(size_t)k]->free_list->push(t->b[(size_t)k])) return;
		}
		const double t0 = now_s();
		if (writer) (void)writer->finish();
		st.write_s += now_s() - t0;
	});
	std::deque<std::unique_ptr<Tuple>> flying;
	auto wait_for = [&](const Tuple& t) -> bool {   // every ticket of the tuple, also after one of them has failed
		bool ok = true;
		for (int k = 0; k < K; k++)
			for (int d = 0; d < N; d++) {
				const int64_t ticket = t.tickets[(size_t)(k * N + d)];
				if (dev[(size_t)k].ctx && ticket && td_wait(dev[(size_t)k].ctx[d], ticket) != TD_OK) {
					if (ok) err.fail(prefix + td_last_error(dev[(size_t)k].ctx[d]));
					ok = false;
				}
			}
		return ok;
	};
	auto retire = [&]() -> bool {
		std::unique_ptr<Tuple> t = std::move(flying.front());
		flying.pop_front();
		const double t0 = now_s();
		const bool ok = wait_for(*t);
		st.decode_s += now_s() - t0;
		return ok && done.push(std::move(t));
	};
	while (!err.failed()) {
		std::unique_ptr<Tuple> t(new Tuple(K, N));
		int n_closed = 0;
		bool bad = false;
		// With nothing ready from a reader and tuples in flight the oldest one is retired instead of waiting: the reader may be
		// waiting for exactly that tuple's buffers.  (The allocator thread "runs with what it has" when page-locking fails part-way
		// -- a memlock limit, a container -- and with fewer than depth + 2 batches in all a loop that only retires at full depth
		// leaves the reader waiting for a free batch, this thread for a ready one and the writer for a finished one, forever.)
		for (int k = 0; k < K && !bad; k++)
			for (;;) {
				const Reader& r = *readers[(size_t)k];
				Batch* b = nullptr;
				const int got = flying.empty() ? (r.ready->pop(b) ? 1 : -1) : r.ready->try_pop(b);
				if (got == 1) { t->b[(size_t)k] = b; break; }
				if (got < 0) { n_closed++; break; }
				if (!retire()) { bad = true; break; }
			}
		if (bad || n_closed == K) break;
		const std::string objection = check(*t);
		if (!objection.empty()) { err.fail(objection); break; }
		if ((int)flying.size() >= depth && !retire()) break;
		const double t0 = now_s();
		const int64_t n = t->b[0]->n;
		bool ok = true;
		for (int k = 0; k < K && ok; k++) {
			if (!dev[(size_t)k].ctx) continue;
			Batch* b = t->b[(size_t)k];
			for (int d = 0; d < N && ok; d++) {      // run_pHMM's contiguous ranges over the devices (barcode_hmm.c:1911-1922)
				td_ctx* ctx = dev[(size_t)k].ctx[d];
				const int64_t interval = n / N, lo = (int64_t)d * interval, hi = (d == N - 1) ? n : lo + interval;
				if (hi <= lo) continue;
				const bool r = dev[(size_t)k].rna;
				// (the window: the artifact filter's thread ranges are those of the whole batch, not of a device's range)
				// (pair mode, one device: the tuple's batch of the mate file goes up with this one, on the same upload stream)
				ok = (N == 1 || td_set_batch_window(ctx, lo, n) == TD_OK) &&
				     (dev[(size_t)k].mate < 0 || td_mol_mate_next(ctx, t->b[(size_t)dev[(size_t)k].mate]->codes, t->b[(size_t)dev[(size_t)k].mate]->offs, n) == TD_OK) &&
				     td_submit(ctx, b->codes, 0, b->offs + lo, hi - lo, r ? TD_MODE_RNA_DUST : TD_MODE_GET_LABEL, b->res + lo, nullptr,
				               r ? nullptr : b->seq_out + b->offs[lo], &t->tickets[(size_t)(k * N + d)]) == TD_OK;
				if (!ok) err.fail(prefix + td_last_error(ctx));
			}
		}
		st.decode_s += now_s() - t0;
		flying.push_back(std::move(t));     // (also after a failed submit: the ranges already on other devices are waited for below)
		if (!ok) break;
	}
	while (!flying.empty() && !err.failed()) if (!retire()) break;
	if (err.failed()) {                     // nothing of ours may stay queued on the devices
		for (auto& t : flying) (void)wait_for(*t);
		flying.clear();
	}
	done.close();
	t_write.join();
	if (writer) {
		const int e = writer->close();
		if (e) err.fail(prefix + "close failed: " + strerror(e));
	}
	if (N > 1) for (const Target& tg : dev) if (tg.ctx) for (int d = 0; d < N; d++) (void)td_set_batch_window(tg.ctx[d], 0, 0);
	for (auto& r : readers) r->stop();
	for (auto& r : readers) {
		st.bytes_in += r->bytes_in; st.parse_s += r->parse_s; st.read_s += r->read_s;
		r->release(!err.failed());
	}
	if (writer) st.bytes_out = writer->bytes_out;
}

} // namespace

extern "C" void td_stream_release(void)
{
	std::lock_guard<std::mutex> lk(g_cache_mu);
	for (Batch* q : g_cache) { td_host_free(q->codes); td_host_free(q->seq_out); td_host_free(q->offs); td_host_free(q->res); delete q; }
	g_cache.clear();
}

// the writer's "%0.2f" (tests compare it with printf digit for digit); returns the number of characters written to buf[48]
extern "C" int td_format_q(float q, char* buf) { return put_q(buf, q); }

extern "C" int td_stream_run(td_ctx* ctx, const char* in_path, const td_arch* arch, const char* out_prefix,
                             const td_stream_opts* opts, td_stream_stats* stats)
{
	if (!in_path) { td_io_set_error("td_stream_run: NULL input path"); return TD_FAIL; }
	if (ctx && (!arch || !out_prefix)) { td_io_set_error("td_stream_run: a decoding run needs the architecture and an output prefix"); return TD_FAIL; }
	const td_stream_opts o = resolve_opts(opts, !ctx || artifacts_active(ctx));
	const double t_start = now_s();
	RunError err;
	std::vector<std::unique_ptr<Reader>> readers;
	readers.emplace_back(new Reader(err, o, ctx == nullptr, true, o.n_threads));
	std::string why;
	if (!readers[0]->src.open(in_path, o.block_bytes, why)) { td_io_set_error(why); return TD_FAIL; }
	std::unique_ptr<Writer> w;
	if (ctx) {
		std::vector<std::string> names;
		int num_alternatives = 2;
		td_writer_file_names(out_prefix, arch, names, &num_alternatives);
		w.reset(new Writer(err, o.n_threads, num_alternatives));
		w->fingerprint_text = o.fingerprint_text != 0;
		if (!w->open(names, why)) { td_io_set_error("td_stream_run: cannot create " + why); return TD_FAIL; }
	}
	td_stream_stats st{};
	uint64_t fnv = 1469598103934665603ULL;
	std::function<bool(Tuple&)> write;
	if (ctx) write = [&](Tuple& t) { return w->write_batch(t.b[0], nullptr, nullptr, 0); };
	else write = [&](Tuple& t) {
		// parse-only run: a checksum over what would have gone to the device (lengths and codes, in order)
		const Batch* b = t.b[0];
		for (int64_t i = 0; i < b->n; i++) {
			const int64_t l = b->offs[i + 1] - b->offs[i];
			fnv = (fnv ^ (uint64_t)l) * 1099511628211ULL;
			const uint8_t* s = b->codes + b->offs[i];
			for (int64_t j = 0; j < l; j++) fnv = (fnv ^ s[j]) * 1099511628211ULL;
		}
		return true;
	};
	td_ctx* const one[1] = { ctx };
	run_stages("td_stream_run: ", err, readers, { Target{ ctx ? one : nullptr, false } }, 1, pipeline_depth(ctx), w.get(),
	           [](const Tuple&) { return std::string(); }, write, st);
	if (!err.failed() && getenv("TD_STREAM_DEBUG"))
		fprintf(stderr, "td_stream: formatting %.3f s, appends %.3f s beside it (write stage %.3f s)\n", w ? w->dbg_format : 0.0, w ? w->dbg_pwrite : 0.0, st.write_s);
	st.wall_s = now_s() - t_start;
	st.codes_fnv = ctx ? 0 : fnv;
	if (stats) *stats = st;
	if (err.failed()) { td_io_set_error(err.message()); return TD_FAIL; }
	return TD_OK;
}

// A decode-only run: reader, then submit and wait, no writer and no output files -- what the context accumulates (its counters, a
// census, the molecule count's survey) is the result.
extern "C" int td_stream_survey(td_ctx* ctx, const char* in_path, const td_stream_opts* opts, td_stream_stats* stats)
{
	if (!ctx || !in_path) { td_io_set_error("td_stream_survey: needs a context and an input path"); return TD_FAIL; }
	const td_stream_opts o = resolve_opts(opts, artifacts_active(ctx));
	const double t_start = now_s();
	RunError err;
	std::vector<std::unique_ptr<Reader>> readers;
	readers.emplace_back(new Reader(err, o, false, true, o.n_threads));
	std::string why;
	if (!readers[0]->src.open(in_path, o.block_bytes, why)) { td_io_set_error(why); return TD_FAIL; }
	td_stream_stats st{};
	td_ctx* const one[1] = { ctx };
	run_stages("td_stream_survey: ", err, readers, { Target{ one, false } }, 1, pipeline_depth(ctx), nullptr,
	           [](const Tuple&) { return std::string(); }, [](Tuple&) { return true; }, st);
	st.wall_s = now_s() - t_start;
	if (stats) *stats = st;
	if (err.failed()) { td_io_set_error(err.message()); return TD_FAIL; }
	return TD_OK;
}

// The head of a file as the run will read it, through the pipeline's own Source / Reader (plain memory, no GPU): plain, .gz, .bz2,
// FASTA and SAM / BAM heads need no second parser.  Records are taken until at least `limit` are there or the file ends; the
// producer is then told to stop and the source closed -- the run opens the file again, as the reference does.
int td_stream_head(const char* path, int64_t limit, int32_t n_threads, std::vector<uint8_t>& codes, std::vector<int64_t>& offs, std::string& why)
{
	td_stream_opts want{};
	want.n_threads = n_threads;
	want.batch_reads = 1 << 16;
	want.block_bytes = (int64_t)16 << 20;
	const td_stream_opts o = resolve_opts(&want, false);
	codes.clear();
	offs.assign(1, 0);
	RunError err;
	Reader rd(err, o, true, false, o.n_threads);
	if (!rd.src.open(path, o.block_bytes, why)) return TD_FAIL;
	if (!rd.start(3)) { why = "td_stream_head: out of memory"; return TD_FAIL; }
	Batch* b = nullptr;
	while ((int64_t)offs.size() - 1 < limit && rd.ready->pop(b)) {
		const int64_t take = std::min<int64_t>(b->n, limit - ((int64_t)offs.size() - 1));
		const int64_t base = offs.back();
		codes.insert(codes.end(), b->codes, b->codes + b->offs[take]);
		for (int64_t i = 1; i <= take; i++) offs.push_back(base + b->offs[i]);
		b->pieces.clear();
		if (!rd.free_list->push(b)) break;
	}
	const bool enough = (int64_t)offs.size() - 1 >= limit;
	rd.ready->abort();          // (the producer leaves whatever wait it is in)
	rd.free_list->abort();
	rd.stop();
	if (err.failed() && !enough) { why = err.message(); return TD_FAIL; }
	return TD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Several input files of one run, several devices: the controller's loop for paired / three-read data
// (hmm_controller_multiple, src/barcode_hmm.c:244-385).
// ---------------------------------------------------------------------------------------------------------
namespace {

// dust_sequences(), src/barcode_hmm.c:2407-2467, on a read that nothing was removed from (run_rna_dust: the read as it was read)
bool rna_dust_low(const uint8_t* s, int64_t len, int dust_cut)
{
	if (len < 1) return false;
	int trip[64];
	for (int j = 0; j < 64; j++) trip[j] = 0;
	auto at = [&](int64_t k) -> unsigned { return k < len ? (unsigned)s[k] : 0u; };   // (the reference's sequences end in a 0 byte)
	unsigned key = ((at(0) & 3u) << 2) | (at(1) & 3u);
	const int64_t n = len > 64 ? 64 : len;
	int64_t c = 2;
	for (int64_t j = 2; j < n; j++) {
		key = ((key << 2) | (at(j) & 3u)) & 0x3Fu;
		trip[key]++;
		c++;
	}
	double sc = 0.0;
	for (int j = 0; j < 64; j++) sc += (double)trip[j] * ((double)trip[j] - 1.0) / 2.0;
	sc = sc / (double)(c - 3) * 10.0;
	return sc > (double)dust_cut;
}

// compare_read_names(), src/io.c:2128-2393: the same place on the flow cell (CASAVA 1.8 / <= 1.7 names), else the same name up
// to the first blank or ';'.  The format is taken from the first name seen (`detected`, like the reference's static).
bool names_differ(const std::string& a, const std::string& b, int& detected)
{
	char i1[100], f1[100], i2[100], f2[100];
	int r1 = 0, l1 = 0, t1 = 0, x1 = 0, y1 = 0, r2 = 0, l2 = 0, t2 = 0, x2 = 0, y2 = 0;
	i1[0] = f1[0] = i2[0] = f2[0] = 0;
	if (detected == -1) {
		if (sscanf(a.c_str(), "%99[^:]:%d:%99[^:]:%d:%d:%d:%d ", i1, &r1, f1, &l1, &t1, &x1, &y1) == 7) detected = 1;
		else if (sscanf(a.c_str(), "%99[^:]:%d:%d:%d:%d", i1, &l1, &t1, &x1, &y1) == 5) detected = 2;
		else detected = 1000;
	}
	if (detected == 1) {
		if (sscanf(a.c_str(), "%99[^:]:%d:%99[^:]:%d:%d:%d:%d ", i1, &r1, f1, &l1, &t1, &x1, &y1) != 7) return true;
		if (sscanf(b.c_str(), "%99[^:]:%d:%99[^:]:%d:%d:%d:%d ", i2, &r2, f2, &l2, &t2, &x2, &y2) != 7) return true;
		return y1 != y2 || x1 != x2 || t1 != t2 || l1 != l2 || strcmp(f1, f2) != 0 || r1 != r2 || strcmp(i1, i2) != 0;
	}
	if (detected == 2) {
		if (sscanf(a.c_str(), "%99[^:]:%d:%d:%d:%d", i1, &l1, &t1, &x1, &y1) != 5) return true;
		if (sscanf(b.c_str(), "%99[^:]:%d:%d:%d:%d", i2, &l2, &t2, &x2, &y2) != 5) return true;
		return y1 != y2 || x1 != x2 || t1 != t2 || l1 != l2 || strcmp(i1, i2) != 0;
	}
	for (size_t i = 0; i < a.size(); i++) {
		if (isspace((unsigned char)a[i]) || a[i] == ';') break;
		if (i >= b.size() || a[i] != b[i]) return true;
	}
	return false;
}

// name of record i of a batch
std::string record_name(const Batch& b, int64_t i)
{
	for (const Piece& pc : b.pieces)
		if (i >= pc.first && i < pc.first + (pc.hi - pc.lo)) {
			const TdRec& r = (*pc.recs)[(size_t)(pc.lo + (i - pc.first))];
			return std::string(pc.blk->data + r.name_off, (size_t)r.name_len);
		}
	return std::string();
}

// what the architectures and contexts of the input files say about the run (barcode_hmm.c:105-153)
struct MultiPlan {
	int bar_file = -1;                // the file that holds the barcode (at most one may), -1: none
	int num_out_reads = 0;            // read segments over all files
	int n_art = 0;                    // files whose contexts have a -ref artifact filter: none or all
	std::vector<int> read_present;    // read segments of every file
	std::vector<char> rna;            // run_rna_dust on the file's devices (TD_MODE_RNA_DUST)
	// pair mode (tagdust_molecules.h, mate mode): the contexts of the one decoded file report mate_bases > 0
	int mol_file = -1, mate_file = -1;   // the decoded file and its mate: the first file in call order other than it (-1: no pair mode)
};

// false: the files cannot make a run (td_io_set_error says why)
bool plan_multi(const td_stream_file* files, const int K, const int N, const int32_t dust, MultiPlan& m)
{
	m.read_present.assign((size_t)K, 0);
	m.rna.assign((size_t)K, 0);
	for (int k = 0; k < K; k++) {
		const td_arch* a = files[k].arch;
		if (!files[k].path || !a || a->n_segments < 1) { td_io_set_error("td_stream_run_multi: every input file needs a path and an architecture"); return false; }
		bool has_bar = false;
		for (int j = 0; j < a->n_segments; j++) { if (a->type[j] == 'B') has_bar = true; if (a->type[j] == 'R') m.read_present[(size_t)k]++; }
		if (has_bar) {
			if (m.bar_file >= 0) { td_io_set_error("td_stream_run_multi: barcodes seem to be in both architectures (barcode_hmm.c:140-145)"); return false; }
			m.bar_file = k;
		}
		m.num_out_reads += m.read_present[(size_t)k];
		// run_rna_dust (barcode_hmm.c:315-319) is what the controller runs instead of the HMM for an architecture that is one read segment
		const bool one_read = a->n_segments == 1 && a->type[0] == 'R';
		if (!files[k].ctx) {
			if (!one_read) { td_io_set_error("td_stream_run_multi: a file without contexts must have the architecture R:N"); return false; }
		} else {
			for (int d = 0; d < N; d++) if (!files[k].ctx[d]) { td_io_set_error("td_stream_run_multi: NULL context"); return false; }
			m.rna[(size_t)k] = one_read;
			m.n_art += artifacts_active(files[k].ctx[0]);
			if (one_read) {   // the devices run the DUST of this call
				int32_t cd = 0;
				(void)td_get_option(files[k].ctx[0], "dust", &cd);
				if (cd != dust) {
					td_io_set_error(std::string("td_stream_run_multi: ") + files[k].path + " (R:N) has contexts with dust " + std::to_string(cd) +
					                ", the call has dust " + std::to_string(dust));
					return false;
				}
			}
		}
	}
	// -ref (hmm_controller_multiple, barcode_hmm.c:209-214, :313-325): the controller hands the one FASTA to every file's step
	if (m.n_art > 0) {
		for (int k = 0; k < K; k++) {
			if (!files[k].ctx) {
				td_io_set_error(std::string("td_stream_run_multi: a -ref artifact filter is set, but ") + files[k].path +
				                " (R:N) has no contexts: its reads must be filtered too (give it contexts: TD_MODE_RNA_DUST)");
				return false;
			}
			if (!artifacts_active(files[k].ctx[0])) { td_io_set_error(std::string("td_stream_run_multi: a -ref artifact filter is set for some files but not for ") + files[k].path); return false; }
		}
	}
	// pair mode: a decoded file whose contexts are in mate mode takes the first other file's batches as its mate batches
	int n_decoded = 0, decoded = -1;
	for (int k = 0; k < K; k++) {
		if (!files[k].ctx || m.rna[(size_t)k]) continue;
		n_decoded++;
		int32_t mb = 0;
		(void)td_get_option(files[k].ctx[0], "mate_bases", &mb);
		if (mb > 0 && decoded < 0) decoded = k;
	}
	if (decoded >= 0) {
		if (N > 1) { td_io_set_error("td_stream_run_multi: mate mode is on and " + std::to_string(N) + " devices are given: a mate batch travels with its reads to one context (one device)"); return false; }
		if (n_decoded != 1 || K < 2) {
			td_io_set_error("td_stream_run_multi: mate mode is on and " + std::to_string(n_decoded) + " of " + std::to_string(K) +
			                " files are decoded: exactly one may be, and every other file, at least one, must be R:N");
			return false;
		}
		for (int k = 0; k < K; k++) {
			const td_arch* a = files[k].arch;
			if (k != decoded && !(a->n_segments == 1 && a->type[0] == 'R')) {
				td_io_set_error(std::string("td_stream_run_multi: mate mode is on and ") + files[k].path + " is not R:N: every file but the decoded one must be");
				return false;
			}
		}
		int32_t cd = 0;
		(void)td_get_option(files[decoded].ctx[0], "dust", &cd);
		if (m.n_art > 0 || dust != 0 || cd != 0) {
			td_io_set_error("td_stream_run_multi: mate mode is on with a -ref filter or DUST: the mate's own outcome is not joined to the count, so a mate "
			                "that could fail would take a molecule's one kept read out of the files (run with dust 0 and without a filter)");
			return false;
		}
		m.mol_file = decoded;
		m.mate_file = decoded == 0 ? 1 : 0;
	}
	if (m.num_out_reads == 0) { td_io_set_error("td_stream_run_multi: no read segment in any architecture: no output files to create (io.c:846-852)"); return false; }
	return true;
}

} // namespace

extern "C" int td_stream_run_multi(const td_stream_file* files, int32_t n_files, int32_t n_devices, const char* out_prefix, int32_t dust,
                                   const td_stream_opts* opts, td_stream_stats* stats, int64_t* counts)
{
	return td_stream_run_multi_hits(files, n_files, n_devices, out_prefix, dust, opts, stats, counts, nullptr, 0);
}

extern "C" int td_stream_run_multi_hits(const td_stream_file* files, int32_t n_files, int32_t n_devices, const char* out_prefix, int32_t dust,
                                        const td_stream_opts* opts, td_stream_stats* stats, int64_t* counts, int64_t* artifact_hits,
                                        int32_t n_artifacts)
{
	if (!files || n_files < 1 || n_files > 8 || !out_prefix) { td_io_set_error("td_stream_run_multi: bad arguments (1..8 input files, an output prefix)"); return TD_FAIL; }
	if (n_devices < 1) n_devices = 1;
	const int K = n_files, N = n_devices;
	MultiPlan m;
	if (!plan_multi(files, K, N, dust, m)) return TD_FAIL;
	const td_stream_opts o = resolve_opts(opts, m.n_art > 0);
	td_ctx* first_ctx = nullptr;
	for (int k = 0; k < K && !first_ctx; k++) if (files[k].ctx) first_ctx = files[k].ctx[0];
	const double t_start = now_s();

	RunError err;
	// print_all() names its files after param->read_structure: the barcode file's architecture, else the last file's
	std::vector<std::string> names;
	int num_alternatives = 2;
	td_writer_file_names_n(out_prefix, files[m.bar_file >= 0 ? m.bar_file : K - 1].arch, m.num_out_reads, names, &num_alternatives);
	Writer w(err, o.n_threads, num_alternatives);
	w.fingerprint_text = o.fingerprint_text != 0;
	std::string why;
	if (!w.open(names, why)) { td_io_set_error("td_stream_run_multi: cannot create " + why); return TD_FAIL; }
	std::vector<size_t> file_base((size_t)K, 0);      // io.c:917-1001: c
	{ size_t c = 0; for (int k = 0; k < K; k++) { file_base[(size_t)k] = c; c += (size_t)num_alternatives * (size_t)m.read_present[(size_t)k]; } }
	std::vector<std::unique_ptr<Reader>> readers;
	std::vector<Target> dev;
	for (int k = 0; k < K; k++) {
		// (a file that is not decoded needs no page-locked buffers, nor does one whose reads come back unchanged need room for rewritten ones)
		// (... but the mate file of pair mode does: its batches are uploaded from where they lie)
		readers.emplace_back(new Reader(err, o, files[k].ctx == nullptr && k != m.mate_file, files[k].ctx != nullptr && !m.rna[(size_t)k], std::max(1, o.n_threads / K)));
		dev.push_back(Target{ files[k].ctx, m.rna[(size_t)k] != 0, k == m.mol_file ? m.mate_file : -1 });
		if (!readers.back()->src.open(files[k].path, o.block_bytes, why)) { td_io_set_error(why); return TD_FAIL; }
	}

	// barcode_hmm.c:257-289: the files hold the same number of records, and the first 1000 names of every pair of files name the same reads
	bool first = true;
	int name_format = -1;
	auto check = [&](const Tuple& t) -> std::string {
		for (int k = 0; k < K; k++)
			if (!t.b[(size_t)k] || t.b[(size_t)k]->n != t.b[0]->n)   // (the controller's own words behind ours, barcode_hmm.c:262)
				return std::string("td_stream_run_multi: the input files differ in their number of records: Input File:") + files[0].path + " and " +
				       files[k].path + " differ in number of entries.";
		if (!first) return std::string();
		first = false;
		for (int64_t i = 0; i < std::min<int64_t>(1000, t.b[0]->n); i++) {
			const std::string na = record_name(*t.b[0], i);
			for (int k = 1; k < K; k++) {
				const std::string nb = record_name(*t.b[(size_t)k], i);
				if (names_differ(na, nb, name_format)) return "td_stream_run_multi: the input files seem to contain reads in different order: " + na + " / " + nb;
			}
		}
		return std::string();
	};
	// the write stage: run_rna_dust for the files that no device sees, the per-record combination, print_all
	int64_t cnt[TD_NUM_COUNTERS];
	for (int q = 0; q < TD_NUM_COUNTERS; q++) cnt[q] = 0;
	if (artifact_hits) for (int32_t q = 0; q < n_artifacts; q++) artifact_hits[q] = 0;
	std::vector<int32_t> ctype, cbar;
	auto write = [&](Tuple& t) -> bool {
		const int64_t n = t.b[0]->n;
		for (int k = 0; k < K; k++) {
			Batch* b = t.b[(size_t)k];
			if (files[k].ctx && !m.rna[(size_t)k]) { b->seq_src = nullptr; continue; }
			b->seq_src = b->codes;
			if (files[k].ctx) continue;             // (TD_MODE_RNA_DUST ran on the file's devices)
			const int64_t chunk = 16384, nch = (n + chunk - 1) / chunk;
			w.pool.run(nch, [&](int64_t c) {        // do_rna_dust, barcode_hmm.c:2370-2395 (no -ref filter: a run with one has contexts here)
				for (int64_t i = c * chunk; i < std::min(n, (c + 1) * chunk); i++) {
					td_read_result& r = b->res[i];
					memset(&r, 0, sizeof r);
					r.mapq = -1.0f; r.barcode = -1; r.fingerprint = -1;        // read_fasta_fastq's defaults, io.c:1698-1702
					r.read_type = TD_EXTRACT_SUCCESS;
					if (dust && rna_dust_low(b->codes + b->offs[i], b->offs[i + 1] - b->offs[i], dust)) r.read_type = TD_EXTRACT_FAIL_LOW_COMPLEXITY;
				}
			});
		}
		ctype.resize((size_t)n); cbar.resize((size_t)n);
		for (int64_t i = 0; i < n; i++) {          // barcode_hmm.c:329-351
			int32_t c = -100000;
			for (int k = 0; k < K; k++) c = std::max(c, t.b[(size_t)k]->res[i].read_type);
			ctype[(size_t)i] = c;
			cbar[(size_t)i] = t.b[(size_t)(m.bar_file >= 0 ? m.bar_file : 0)]->res[i].barcode;
			// the controller's counting, :354-384; a duplicate (dedup, tagdust_molecules.h) counts as the extracted read it was decoded
			// as, under its barcode bin: what the single-file run's device counters do
			const int32_t cc = (c & 0xFF) == TD_EXTRACT_DUPLICATE ? TD_EXTRACT_SUCCESS : c;
			cnt[cc & (TD_NUM_OUTCOME_SLOTS - 1)]++;
			if (cc == TD_EXTRACT_SUCCESS && cbar[(size_t)i] >= 0) cnt[TD_NUM_OUTCOME_SLOTS + (cbar[(size_t)i] & 0xFF)]++;
			// reference_fasta->mer_hash (:381): on the combined outcome, which is the largest of the files' -- of two files' hits the later sequence
			if (artifact_hits && (c & 0xFF) == TD_EXTRACT_FAIL_MATCHES_ARTIFACTS && (c >> 8) >= 1 && (c >> 8) <= n_artifacts) artifact_hits[(c >> 8) - 1]++;
		}
		bool ok = true;
		for (int k = 0; k < K && ok; k++)
			if (m.read_present[(size_t)k] > 0) ok = w.write_batch(t.b[(size_t)k], ctype.data(), cbar.data(), file_base[(size_t)k]);
		for (Batch* b : t.b) b->seq_src = nullptr;
		return ok;
	};
	td_stream_stats st{};
	run_stages("td_stream_run_multi: ", err, readers, dev, N, pipeline_depth(first_ctx), &w, check, write, st);
	st.wall_s = now_s() - t_start;
	if (stats) *stats = st;
	if (counts) for (int q = 0; q < TD_NUM_COUNTERS; q++) counts[q] = cnt[q];
	if (err.failed()) { td_io_set_error(err.message()); return TD_FAIL; }
	return TD_OK;
}

// td_merge_stream: the `merge` controller on the same readers
#include "td_merge_stream.inc"
