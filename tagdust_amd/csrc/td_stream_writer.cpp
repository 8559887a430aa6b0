// td_stream_writer.cpp -- the output side of the streaming pipeline (td_stream_internal.h): format_records with the helpers its loop
// calls per record (put_int, put_q, span_of, codes_to_text; all in this unit, so that they inline), and Writer -- the output files,
// the pool that formats a batch's records, the appender thread that writes them.
#include <errno.h>
#include <fcntl.h>
#include <math.h>
#include <string.h>
#include <unistd.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include <algorithm>
#include <cmath>

#include "td_stream_internal.h"

namespace tdstream {

// the formatted records of one piece sub-range: one buffer per output file (print_all(), io.c:917-1001)
struct OutBufs { std::vector<Bytes> file; };

namespace {

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

} // namespace

Writer::Writer(RunError& e, int n_threads, int num_alternatives_) : err(e), pool(n_threads), num_alternatives(num_alternatives_) {}
Writer::~Writer() { (void)close(); }

bool Writer::open(const std::vector<std::string>& names, std::string& why)
{
	for (auto& nm : names) {
		const int fd = ::open(nm.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
		if (fd < 0) { why = nm + ": " + strerror(errno); (void)close(); return false; }
		fds.push_back(fd);
	}
	file_off.assign(fds.size(), 0);
	return true;
}

int Writer::close()
{
	append_stop();
	int first = 0;
	for (int fd : fds) if (::close(fd) != 0 && !first) first = errno;
	fds.clear();
	return first;
}

void Writer::append_loop()
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

bool Writer::append_wait(int set)
{
	std::unique_lock<std::mutex> lk(ap_mu);
	ap_cv.wait(lk, [&] { return set < 0 ? (!ap_busy[0] && !ap_busy[1]) : !ap_busy[set]; });
	if (ap_errno) { const int e = ap_errno; lk.unlock(); err.fail(std::string("td_stream_run: write failed: ") + strerror(e)); return false; }
	return true;
}

void Writer::append_stop()
{
	{ std::lock_guard<std::mutex> lk(ap_mu); ap_stop = true; }
	ap_cv.notify_all();
	if (appender.joinable()) appender.join();
}

bool Writer::write_batch(Batch* b, const int32_t* ctype, const int32_t* cbar, size_t file_base)
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

} // namespace tdstream

// the writer's "%0.2f" (tests compare it with printf digit for digit); returns the number of characters written to buf[48]
extern "C" int td_format_q(float q, char* buf) { return tdstream::put_q(buf, q); }
