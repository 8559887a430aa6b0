// merge_host_check.cpp -- the host path of include/tagdust_merge.h (td_merge_tables_build, td_merge_host) as a stand-alone program,
// for running it under the host sanitizers: no GPU, no HIP runtime, no Python.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/merge_host_check.cpp tagdust_amd/csrc/td_merge.cpp -o /tmp/merge_host_check -lpthread
//   /tmp/merge_host_check tests/golden/merge/r1.fq tests/golden/merge/r2.fq tests/golden/merge/merged_default.fq 16 0
//   /tmp/merge_host_check tests/golden/merge/r1.fq tests/golden/merge/r2.fq tests/golden/merge/merged_Q0.9_minlen20.fq 20 0.9
//
// Reads two four-line FASTQ files, merges them on 3 threads and compares the records with the expected file; exit status 0 when
// they are equal.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../tagdust_amd/csrc/td_merge_internal.h"

// the kernel's host side is not part of this program
TdMergeDevice* td_merge_device_open(int, std::string& err) { err = "no device in this program"; return nullptr; }
void td_merge_device_close(TdMergeDevice*) {}
bool td_merge_device_run(TdMergeDevice*, const TdMergeView&, const td_merge_tables&, int, float, int, td_merge_record*, char*, char*, int*, float*, std::string& err)
{
	err = "no device in this program";
	return false;
}

// nor are the streaming pipeline's readers (td_merge_stream.cpp over td_stream_reader.cpp)
int td_merge_stream_run(const char*, const char*, const char*, int, int, bool, const std::function<bool(const TdMergeView&, TdWorkers&, td_merge_result*, std::string&)>&,
                        td_merge_stats*, std::string& err)
{
	err = "no stream in this program";
	return TD_FAIL;
}

namespace {
std::string slurp(const char* path)
{
	std::ifstream f(path, std::ios::binary);
	if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
	std::stringstream s;
	s << f.rdbuf();
	return s.str();
}

struct Reads {
	std::string text;
	std::vector<int64_t> name_off, qual_off, offs;
	std::vector<int32_t> name_len;
	std::vector<uint8_t> codes;
	td_reads view{};
	explicit Reads(const char* path) : text(slurp(path))
	{
		offs.push_back(0);
		size_t p = 0;
		while (p < text.size()) {
			size_t e[4], q = p;
			for (int k = 0; k < 4; k++) { e[k] = text.find('\n', q); if (e[k] == std::string::npos) { fprintf(stderr, "%s: truncated record\n", path); exit(2); } q = e[k] + 1; }
			name_off.push_back((int64_t)p + 1);
			name_len.push_back((int32_t)(e[0] - p - 1));
			for (size_t k = e[0] + 1; k < e[1]; k++) {
				const char c = text[k];
				codes.push_back(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : c == '.' ? 5 : 4);
			}
			offs.push_back((int64_t)codes.size());
			qual_off.push_back((int64_t)e[2] + 1);
			p = q;
		}
		view.n_reads = (int64_t)name_off.size();
		view.text = text.data();
		view.name_off = name_off.data(); view.name_len = name_len.data(); view.qual_off = qual_off.data();
		view.offs = offs.data(); view.codes = codes.data();
	}
};
}

int main(int argc, char** argv)
{
	if (argc != 6) { fprintf(stderr, "usage: merge_host_check r1.fq r2.fq expected.fq minlen threshold\n"); return 2; }
	Reads r1(argv[1]), r2(argv[2]);
	const std::string want = slurp(argv[3]);
	td_merge_opts o;
	td_merge_opts_default(&o);
	o.min_overlap = atoi(argv[4]);
	o.threshold = (float)atof(argv[5]);
	o.n_threads = 3;
	o.device = -1;
	// the tables on their own, over every quality byte of both files
	std::string quals;
	for (const Reads* r : { &r1, &r2 })
		for (int64_t i = 0; i < r->view.n_reads; i++) quals.append(r->text, (size_t)r->qual_off[(size_t)i], (size_t)(r->offs[(size_t)i + 1] - r->offs[(size_t)i]));
	td_merge_tables* t = nullptr;
	if (td_merge_tables_build((const uint8_t*)quals.data(), (int64_t)quals.size(), &t) != TD_OK) { fprintf(stderr, "%s\n", td_merge_last_error()); return 1; }
	printf("tables: %d quality characters, T %d x %d\n", t->nq, t->dim, t->dim);
	td_merge_tables_free(t);
	td_merge_result* res = nullptr;
	if (td_merge_host(&r1.view, &r2.view, &o, &res) != TD_OK) { fprintf(stderr, "%s\n", td_merge_last_error()); return 1; }
	std::string got;
	for (int64_t p = 0; p < res->n_pairs; p++) {
		const size_t n = (size_t)res->rec[p].out_len;
		if (!n) continue;
		got += "@" + r1.text.substr((size_t)r1.name_off[(size_t)p], (size_t)r1.name_len[(size_t)p]) + "\n";
		got.append(res->seq + res->out_off[p], n); got += "\n+\n";
		got.append(res->qual + res->out_off[p], n); got += "\n";
	}
	printf("%lld pairs: %lld written, %lld below the threshold, %lld too short; output %s the expected file\n", (long long)res->n_pairs,
	       (long long)res->n_written, (long long)res->n_below, (long long)res->n_too_short, got == want ? "equals" : "DIFFERS FROM");
	td_merge_result_free(res);
	return got == want ? 0 : 1;
}
