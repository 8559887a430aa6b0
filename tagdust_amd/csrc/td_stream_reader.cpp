// td_stream_reader.cpp -- the input side of the streaming pipeline (td_stream_internal.h): Source (one mapping of a plain file, or
// blocks from a pipe: zcat / bzcat / samtools), the page-locked batch cache that outlives a run, and Reader -- stage 1 of one input
// file: its allocator thread and its producer thread, which finds the records of a block and base-codes them into batches on a
// parse pool.  Then what runs over several readers share (the lock-step check, the readers' epilogue) and td_stream_head.
#include <ctype.h>
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

#include "td_stream_internal.h"

namespace tdstream {

Source::~Source()
{
	if (map_ && map_ != MAP_FAILED) munmap(map_, (size_t)map_len_);
	if (pipe_) pclose(pipe_);
	if (fd_ >= 0) close(fd_);
}

bool Source::open(const char* path, int64_t block_bytes, std::string& err)
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

std::shared_ptr<Block> Source::next(double* read_s, std::string& err)
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

// Alignment text -> the four-line records the parser takes: '@' QNAME, SEQ, '+', QUAL (fields 1, 10 and 11 of every line that
// is not a header line, read_sam_chunk, io.c:1498-1660).  Whole lines only; the rest is carried over to the next block.
std::shared_ptr<Block> Source::sam_block(std::shared_ptr<Block> b, int64_t have, const bool end_of_input, std::string& err)
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

namespace {

// Page-locked batch buffers outlive a run: page-locking runs at about 1 GB/s, which is most of what a short file costs.  The
// buffers of the last run (up to 1 GiB) wait here for the next one of the same process; td_stream_release frees them.
std::mutex g_cache_mu;
std::vector<Batch*> g_cache;
const size_t kCacheBytes = (size_t)1 << 30;

size_t batch_bytes(const Batch* b)
{
	return b->cap_codes + b->cap_seq + b->cap_qual + (size_t)b->cap_reads * (sizeof(int64_t) + sizeof(td_read_result));
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

} // namespace

bool Reader::start(int n_batches)
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

void Reader::stop()
{
	if (t_prod.joinable()) t_prod.join();
	{ std::lock_guard<std::mutex> lk(all_mu); stop_alloc = true; }
	hint_cv.notify_all();
	if (free_list) free_list->abort();          // (an allocator waiting to hand over a batch)
	if (t_alloc.joinable()) t_alloc.join();
}

void Reader::release(bool keep)
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
		buf_free(dry, q->codes); buf_free(dry, q->seq_out); buf_free(dry, q->qual); buf_free(dry, q->offs); buf_free(dry, q->res);
		delete q;
	}
	all.clear();
}

Batch* Reader::new_batch()
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
void Reader::allocator(int n_more)
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
		if (!b || !grow_buf(dry, &b->codes, &b->cap_codes, hint, 0, hint) || (want_seq && !grow_buf(dry, &b->seq_out, &b->cap_seq, hint, 0, hint)) ||
		    (want_qual && !grow_buf(dry, &b->qual, &b->cap_qual, hint, 0, hint))) return;   // (the pipeline runs with what it has)
		if (!free_list->push(b)) return;
	}
}

// read / map a block, find its records, hand them out to batches, base-code them
void Reader::producer()
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
			// the base-quality filter has nothing to judge in a record without a quality line (FASTA)
			if (want_qual && bad[(size_t)k] < 0)
				for (size_t i = 0; i < v.size(); i++)
					if (v[i].qual_off < 0) { bad[(size_t)k] = (int64_t)i; break; }
		});
		dbg_pass1 += now_s() - t0;
		for (int k = 0; k < nchunk; k++)
			if (bad[(size_t)k] >= 0) {
				const TdRec& q = (*recs[(size_t)k])[(size_t)bad[(size_t)k]];
				if (q.qual_off < 0) {
					err.fail("td_stream_run: the base-quality filter is on and record \"" + std::string(blk->data + q.name_off, (size_t)(q.name_len < 60 ? q.name_len : 60)) +
					         "\" of " + path + " has no quality line (FASTA): there is nothing to judge (run without --min-base-quality, or give FASTQ)");
					return;
				}
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
				    (want_seq && !grow_buf(dry, &b->seq_out, &b->cap_seq, (size_t)b->n_bases + 1, 0, batch_hint)) ||
				    (want_qual && !grow_buf(dry, &b->qual, &b->cap_qual, (size_t)b->n_bases + 1, keep, batch_hint))) { err.fail("td_stream_run: page-locked memory exhausted"); return false; }
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
					// the base-quality filter: the quality line beside the codes (a record has one byte per base: checked above)
					if (want_qual && q.qual_off >= 0) memcpy(sb.b->qual + sb.b->offs[pc.first + (r - pc.lo)], pc.blk->data + q.qual_off, (size_t)q.seq_len);
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

std::string record_name(const Batch& b, int64_t i)
{
	for (const Piece& pc : b.pieces)
		if (i >= pc.first && i < pc.first + (pc.hi - pc.lo)) {
			const TdRec& r = (*pc.recs)[(size_t)(pc.lo + (i - pc.first))];
			return std::string(pc.blk->data + r.name_off, (size_t)r.name_len);
		}
	return std::string();
}

std::string lockstep_objection(const std::string& prefix, Batch* const* b, const char* const* paths, int K, bool& first, int& name_format)
{
	auto count = [&](int k) { return b[k] ? b[k]->n : (int64_t)-1; };
	for (int k = 1; k < K; k++)
		if (count(k) != count(0))   // (the controllers' own words behind ours, barcode_hmm.c:262, merge.c:164-174)
			return prefix + "the input files differ in their number of records: Input File:" + paths[0] + " and " + paths[k] + " differ in number of entries.";
	if (!first) return std::string();
	first = false;
	for (int64_t i = 0; i < std::min<int64_t>(1000, b[0]->n); i++) {
		const std::string na = record_name(*b[0], i);
		for (int k = 1; k < K; k++) {
			const std::string nb = record_name(*b[k], i);
			if (names_differ(na, nb, name_format)) return prefix + "the input files seem to contain reads in different order: " + na + " / " + nb;
		}
	}
	return std::string();
}

void finish_readers(const std::vector<std::unique_ptr<Reader>>& readers, bool keep, int64_t& bytes_in, double& parse_s, double& read_s)
{
	for (auto& r : readers) {                 // (a reader that was never started has no queues)
		if (r->ready) r->ready->abort();
		if (r->free_list) r->free_list->abort();
	}
	for (auto& r : readers) r->stop();
	for (auto& r : readers) {
		bytes_in += r->bytes_in; parse_s += r->parse_s; read_s += r->read_s;
		r->release(keep);
	}
}

} // namespace tdstream

using namespace tdstream;

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

extern "C" void td_stream_release(void)
{
	std::lock_guard<std::mutex> lk(g_cache_mu);
	for (Batch* q : g_cache) { td_host_free(q->codes); td_host_free(q->seq_out); td_host_free(q->qual); td_host_free(q->offs); td_host_free(q->res); delete q; }
	g_cache.clear();
}
