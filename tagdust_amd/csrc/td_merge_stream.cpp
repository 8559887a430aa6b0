// td_merge_stream.cpp -- the pipeline under td_merge_stream (include/tagdust_merge.h) on the decode pipeline's input side
// (td_stream_internal.h: Source / Reader / Queue / RunError, the lock-step check, the readers' epilogue): the controller of the
// reference's `merge` (src/merge.c:59-216) as a pipeline.
//
//   reader / parser thread per file      caller's thread                          writer thread
//   the next batch of each file          equal counts, first 1000 names, quality   "@name\nseq\n+\nqual\n" per written pair,
//                                        bytes packed, td_merge_batch (device or   formatted by a pool, appended in order
//                                        host)
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>

#include "td_merge_internal.h"
#include "td_stream_internal.h"

using namespace tdstream;

namespace {

struct MergeDone {
	Batch* b1 = nullptr;
	Batch* b2 = nullptr;
	td_merge_result res{};
	~MergeDone() { free(res.rec); free(res.out_off); free(res.seq); free(res.qual); }
};

// the quality bytes of a batch, contiguous under its offsets; false: a record without qualities (FASTA)
bool merge_pack_qual(const Batch& b, TdWorkers& pool, std::vector<uint8_t>& q)
{
	q.resize((size_t)b.n_bases + 1);
	std::vector<char> bad(b.pieces.size(), 0);
	pool.run((int64_t)b.pieces.size(), [&](int64_t k) {
		const Piece& pc = b.pieces[(size_t)k];
		for (int64_t r = pc.lo; r < pc.hi; r++) {
			const TdRec& rec = (*pc.recs)[(size_t)r];
			const int64_t i = pc.first + (r - pc.lo);
			const int64_t len = b.offs[i + 1] - b.offs[i];
			if (rec.qual_off < 0) { bad[(size_t)k] = 1; return; }
			if (len > 0) memcpy(q.data() + b.offs[i], pc.blk->data + rec.qual_off, (size_t)len);
		}
	});
	for (char c : bad) if (c) return false;
	return true;
}

bool write_all(int fd, const char* p, size_t n)
{
	while (n > 0) {
		const ssize_t w = write(fd, p, n);
		if (w < 0) { if (errno == EINTR) continue; return false; }
		p += w; n -= (size_t)w;
	}
	return true;
}

} // namespace

// The pipeline of td_merge_stream (td_merge.cpp): `merge_batch` is what the calling thread does with a batch of pairs (td_merge_batch
// on the device or on the host).  pinned: the readers' batch buffers are page-locked.  This unit knows nothing of the merger but
// its plain structs, so it links without td_merge.cpp, and the decode pipeline's units link without this one.
int td_merge_stream_run(const char* in1, const char* in2, const char* out_path, int n_threads, int batch_pairs, bool pinned,
                        const std::function<bool(const TdMergeView&, TdWorkers&, td_merge_result*, std::string&)>& merge_batch, td_merge_stats* stats, std::string& error)
{
	td_stream_opts want{};
	want.batch_reads = batch_pairs > 0 ? batch_pairs : (1 << 18);
	want.n_threads = n_threads;
	const td_stream_opts o = resolve_opts(&want, false);
	const double t_start = now_s();
	const char* paths[2] = { in1, in2 };
	RunError err;
	std::vector<std::unique_ptr<Reader>> readers;
	std::string why;
	for (int k = 0; k < 2; k++) {
		readers.emplace_back(new Reader(err, o, !pinned, false, std::max(1, o.n_threads / 2)));
		if (!readers.back()->src.open(paths[k], o.block_bytes, why)) { error = why; return TD_FAIL; }
	}
	const bool to_stdout = !strcmp(out_path, "-");
	const int fd = to_stdout ? 1 : open(out_path, O_WRONLY | O_CREAT | O_TRUNC, 0644);
	if (fd < 0) { error = std::string("td_merge_stream: cannot create ") + out_path + ": " + strerror(errno); return TD_FAIL; }

	td_merge_stats st{};
	const int n_batches = 6;      // per file: one being filled, one ready, one being merged, two finished, one being written
	Queue<std::unique_ptr<MergeDone>> done(2);
	err.watch(&done);
	for (auto& r : readers)
		if (!r->start(n_batches)) { err.fail("td_merge_stream: page-locked memory exhausted"); break; }
	TdWorkers write_pool(o.n_threads), pack_pool(o.n_threads), merge_pool(n_threads);      // (merge_pool: td_merge_batch's, on the calling thread)
	std::thread t_write([&] {
		std::unique_ptr<MergeDone> d;
		while (done.pop(d)) {
			const double t0 = now_s();
			const Batch& b = *d->b1;
			const td_merge_result& res = d->res;
			struct Sub { size_t piece; int64_t lo, hi; };
			std::vector<Sub> subs;
			for (size_t k = 0; k < b.pieces.size(); k++)
				for (int64_t a = b.pieces[k].lo; a < b.pieces[k].hi; a += 8192) subs.push_back(Sub{ k, a, std::min<int64_t>(a + 8192, b.pieces[k].hi) });
			std::vector<Bytes> text(subs.size());
			write_pool.run((int64_t)subs.size(), [&](int64_t k) {
				const Sub& sb = subs[(size_t)k];
				const Piece& pc = b.pieces[sb.piece];
				Bytes& out = text[(size_t)k];
				for (int64_t r = sb.lo; r < sb.hi; r++) {
					const int64_t i = pc.first + (r - pc.lo);
					const size_t len = (size_t)res.rec[i].out_len;
					if (!len) continue;
					const TdRec& rec = (*pc.recs)[(size_t)r];
					const size_t total = 1 + (size_t)rec.name_len + 1 + len + 3 + len + 1;      // merge.c:330
					char* w = out.room(total);
					*w++ = '@';
					memcpy(w, pc.blk->data + rec.name_off, (size_t)rec.name_len); w += rec.name_len;
					*w++ = '\n';
					memcpy(w, res.seq + res.out_off[i], len); w += len;
					*w++ = '\n'; *w++ = '+'; *w++ = '\n';
					memcpy(w, res.qual + res.out_off[i], len); w += len;
					*w++ = '\n';
					out.n += total;
				}
			});
			for (const Bytes& t : text)
				if (t.n) {
					if (!write_all(fd, t.p, t.n)) { err.fail(std::string("td_merge_stream: write failed: ") + strerror(errno)); return; }
					st.bytes_out += (int64_t)t.n;
				}
			st.n_pairs += res.n_pairs; st.n_written += res.n_written; st.n_below += res.n_below; st.n_too_short += res.n_too_short;
			st.n_batches++;
			Batch* b1 = d->b1; Batch* b2 = d->b2;
			d.reset();
			b1->pieces.clear(); b2->pieces.clear();           // releases the blocks
			st.write_s += now_s() - t0;
			if (!readers[0]->free_list->push(b1) || !readers[1]->free_list->push(b2)) return;
		}
	});

	bool first = true;
	int name_format = -1;
	std::vector<uint8_t> q1, q2;
	while (!err.failed()) {
		Batch* b1 = nullptr; Batch* b2 = nullptr;
		const bool got1 = readers[0]->ready->pop(b1), got2 = readers[1]->ready->pop(b2);
		if (err.failed() || (!got1 && !got2)) break;
		Batch* const pair[2] = { b1, b2 };                       // (NULL: that reader has ended)
		const std::string objection = lockstep_objection("td_merge_stream: ", pair, paths, 2, first, name_format);   // merge.c:164-193
		if (!objection.empty()) { err.fail(objection); break; }
		const double t0 = now_s();
		if (!merge_pack_qual(*b1, pack_pool, q1) || !merge_pack_qual(*b2, pack_pool, q2)) { err.fail("td_merge_stream: FASTA input: the reads have no base qualities"); break; }
		TdMergeView v;
		v.n = b1->n;
		v.codes1 = b1->codes; v.qual1 = q1.data(); v.offs1 = b1->offs;
		v.codes2 = b2->codes; v.qual2 = q2.data(); v.offs2 = b2->offs;
		std::unique_ptr<MergeDone> d(new MergeDone());
		d->b1 = b1; d->b2 = b2;
		std::string e;
		if (!merge_batch(v, merge_pool, &d->res, e)) { err.fail("td_merge_stream: " + e); break; }
		st.kernel_s += (double)d->res.kernel_ms * 1e-3;
		st.merge_s += now_s() - t0;
		if (!done.push(std::move(d))) break;
	}
	done.close();
	t_write.join();
	if (!to_stdout && close(fd) != 0) err.fail(std::string("td_merge_stream: close failed: ") + strerror(errno));
	finish_readers(readers, !err.failed(), st.bytes_in, st.parse_s, st.read_s);
	st.wall_s = now_s() - t_start;
	if (stats) *stats = st;
	if (err.failed()) { error = err.message(); return TD_FAIL; }
	return TD_OK;
}
