// run_host_check.cpp -- the device-free units of the whole-run driver (tagdust_amd/csrc/td_run_opts.cpp, td_run_plan.cpp,
// td_run_report.cpp over td_run_internal.h) as a stand-alone program: no HIP runtime, no Python.  Built under the sanitizers by
// tools/host_checks.sh:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tagdust_amd/csrc/td_run_opts.cpp
//       tagdust_amd/csrc/td_run_plan.cpp tagdust_amd/csrc/td_run_report.cpp tagdust_amd/csrc/td_model.cpp tagdust_amd/csrc/td_model_flat.cpp
//       tagdust_amd/csrc/td_fastq.cpp tagdust_amd/csrc/td_census_host.cpp tagdust_amd/csrc/td_samples_host.cpp
//       tagdust_amd/csrc/td_molecules_host.cpp tools/run_host_check.cpp -o /tmp/run_host_check -lpthread
//   /tmp/run_host_check                                          # (leak detection stays on)
//
// Options, copy_out, the sample sheet's refusals, which file plays which part, the plan's text, the bytes of the three report
// files and the summary block, each against a string written out here from the format strings.  Every file it makes is in a
// directory of its own under $TMPDIR (or /tmp), removed at the end.  Exit status 0 when all of it agrees.
#define HOST_CHECK_NAME "run_host_check"
#include "host_check.h"
#include <unistd.h>
#include "../tagdust_amd/csrc/td_run_internal.h"

using namespace tdrun;

static std::string g_dir;
static std::vector<std::string> g_made;

static std::string put(const std::string& name, const std::string& text)
{
	const std::string p = g_dir + "/" + name;
	FILE* f = fopen(p.c_str(), "w");
	if (f) { fwrite(text.data(), 1, text.size(), f); fclose(f); }
	if (std::find(g_made.begin(), g_made.end(), p) == g_made.end()) g_made.push_back(p);
	return p;
}

// a command line -> options (NULL: refused, the message in g_err)
static td_run_opts* parse(const std::vector<std::string>& words)
{
	std::vector<const char*> argv(1, "tagdust-hip");
	for (const std::string& w : words) argv.push_back(w.c_str());
	td_run_opts* o = nullptr;
	char err[512] = "";
	const int rc = td_run_parse_args((int)argv.size(), argv.data(), &o, err, sizeof err);
	g_err = err;
	if (rc != TD_OK && (o || g_err != td_run_last_error())) g_err = "td_run_parse_args: out and err disagree with the return value";
	return rc == TD_OK ? o : nullptr;
}
static std::string refused(const std::vector<std::string>& words)
{
	td_run_opts* o = parse(words);
	td_run_opts_free(o);
	return o ? "(accepted)" : g_err;
}

// decide_roles for a command line and one architecture per file ("B:ACGT,TTGA R:N"): "" or the message
static std::string roles(const std::vector<std::string>& words, const std::vector<std::string>& files, RunRoles& r)
{
	td_run_opts* o = parse(words);
	if (!o) return "parse: " + g_err;
	std::vector<ArchPtr> archs(files.size());
	std::vector<const td_arch*> view;
	std::string why;
	for (size_t k = 0; k < files.size(); k++) {
		std::vector<std::string> segs;
		for (size_t at = 0; at < files[k].size();) {
			const size_t e = std::min(files[k].find(' ', at), files[k].size());
			segs.push_back(files[k].substr(at, e - at));
			at = e + 1;
		}
		if (!parse_arch(segs, archs[k], why)) { td_run_opts_free(o); return "parse_arch: " + why; }
		view.push_back(archs[k].get());
	}
	const int rc = decide_roles(o, view, r);
	td_run_opts_free(o);
	return rc == TD_OK ? "" : td_run_last_error();
}

static std::string plan_text(const std::vector<std::string>& words, bool* all_known)
{
	td_run_opts* o = parse(words);
	if (!o) return "parse: " + g_err;
	td_run_plan_t* p = nullptr;
	std::string s;
	if (td_run_plan(o, &p) != TD_OK) s = std::string("plan: ") + td_run_last_error();
	else {
		s.resize((size_t)td_run_plan_describe(p, nullptr, 0));
		std::vector<char> buf(s.size() + 1);
		td_run_plan_describe(p, buf.data(), (int64_t)buf.size());
		s = buf.data();
		*all_known = p->all_known;
	}
	td_run_plan_free(p);
	td_run_opts_free(o);
	return s;
}

static uint64_t census_key(const char* word)
{
	uint64_t k = 0;
	for (const char* p = word; *p; p++) k = (k << 2) | (uint64_t)(strchr("ACGT", *p) - "ACGT");
	return k | ((uint64_t)strlen(word) << 56);
}

static int count(const std::string& text, const std::string& what)
{
	int n = 0;
	for (size_t at = text.find(what); at != std::string::npos; at = text.find(what, at + 1)) n++;
	return n;
}

static int checks()
{
	const std::string out = g_dir + "/out";

	// ---- options ----
	{
		td_run_opts* o = parse({});
		CHECK(o && o->num_threads == 8 && o->confidence_threshold == 0.0f && o->sequencer_error_rate == 0.05f && o->indel_frequency == 0.1f);
		CHECK(o->minlen == 16 && o->dust == 100 && o->filter_error == 2 && o->matchstart == -1 && o->matchend == -1 && o->seed == 0);
		CHECK(o->n_devices == 1 && o->devices[0] == 0 && o->unknown_slots_log2 == 20 && o->molecules_prefix == 20 && o->molecules_slots_log2 == 26);
		CHECK(o->quality_segments == (TD_QUAL_SEG_B | TD_QUAL_SEG_F) && o->quality_offset == 33 && o->max_low_bases == 0 && o->min_base_quality == 0);
		CHECK(o->n_infiles == 0 && o->argc == 1 && !o->outfile && !o->arch_file && !o->samples_file && !o->reference_fasta && !o->segments[0]);
		CHECK(!o->molecules && !o->dedup && !o->collapse_umis && !o->dedup_collapsed && !o->mate_bases && !o->mate_filter && !o->unknown_barcodes);
		CHECK(!o->flavour && !o->host_threads && !o->batch_reads && !o->sync_compile && !o->stats_on_host && !o->force && !o->dry_run && !o->fingerprint_seq);
		td_run_opts_free(o);
		// one spelling of each own option, every string member set: td_run_opts_free owns all of it
		o = parse({ "--devices", "0,1", "--rtest", "--host-threads", "3", "--batch-reads", "500", "--sync-compile", "--stats-on-host", "--force", "--dry-run",
		            "--unknown-barcodes", "7", "--unknown-barcodes-slots", "10", "--fingerprint-seq", "--molecules", "--molecules-prefix", "12",
		            "--molecules-slots", "18", "--dedup", "--collapse-umis", "--dedup-collapsed", "--mate-bases", "8", "--mate-filter", "--samples", "S",
		            "--min-base-quality", "20", "--max-low-bases", "2", "--quality-segments", "F", "--quality-offset", "64", "-1", "B:ACGT", "-1", "B:TTGA",
		            "-10", "R:N", "-arch", "A", "-o", "O1", "-out", "O2", "-ref", "REF", "-start", "5", "-end", "9", "-seed", "42", "in1.fq", "-", "in2.fq" });
		CHECK(o && o->n_devices == 2 && o->devices[0] == 0 && o->devices[1] == 1 && o->flavour == 1 && o->host_threads == 3 && o->batch_reads == 500);
		CHECK(o->sync_compile && o->stats_on_host && o->force && o->dry_run && o->unknown_barcodes == 7 && o->unknown_slots_log2 == 10 && o->fingerprint_seq);
		CHECK(o->molecules && o->molecules_prefix == 12 && o->molecules_slots_log2 == 18 && o->dedup && o->collapse_umis && o->dedup_collapsed);
		CHECK(o->mate_bases == 8 && o->mate_filter && !strcmp(o->samples_file, "S") && o->min_base_quality == 20 && o->max_low_bases == 2);
		CHECK(o->quality_segments == TD_QUAL_SEG_F && o->quality_offset == 64 && !strcmp(o->segments[0], "B:TTGA") && !o->segments[1] && !strcmp(o->segments[9], "R:N"));
		CHECK(!strcmp(o->arch_file, "A") && !strcmp(o->outfile, "O2") && !strcmp(o->reference_fasta, "REF") && o->seed == 42);
		CHECK(o->matchstart == 4 && o->matchend == 9);   // -start is stored as atoi - 1
		CHECK(o->n_infiles == 3 && !strcmp(o->infile[0], "in1.fq") && !strcmp(o->infile[1], "-") && !strcmp(o->infile[2], "in2.fq"));
		CHECK(o->argc == 61 && !strcmp(o->argv[0], "tagdust-hip") && !strcmp(o->argv[60], "in2.fq"));
		td_run_opts_free(o);
		// the four implications onto --molecules
		struct { const char* opt; const char* arg; int dedup, collapse; } imp[] = { { "--dedup-collapsed", nullptr, 1, 1 }, { "--dedup", nullptr, 1, 0 },
		                                                                             { "--collapse-umis", nullptr, 0, 1 }, { "--mate-bases", "4", 0, 0 } };
		for (auto& c : imp) {
			o = c.arg ? parse({ c.opt, c.arg }) : parse({ c.opt });
			CHECK(o && o->molecules == 1 && o->dedup == c.dedup && o->collapse_umis == c.collapse);
			td_run_opts_free(o);
		}
		CHECK(refused({ "--max-low-bases", "1" }) == "--max-low-bases / --quality-segments / --quality-offset need --min-base-quality: they say how it judges");
		CHECK(refused({ "--quality-segments", "B" }) == "--max-low-bases / --quality-segments / --quality-offset need --min-base-quality: they say how it judges");
		CHECK(refused({ "--quality-offset", "33" }) == "--max-low-bases / --quality-segments / --quality-offset need --min-base-quality: they say how it judges");
		CHECK(refused({ "--devices", "0," }) == "--devices: cannot read the device list \"0,\"");
		CHECK(refused({ "--devices", "," }) == "--devices: cannot read the device list \",\" (want e.g. 0,1)");
		CHECK(refused({ "--devices", "x" }) == "--devices: cannot read the device list \"x\" (want e.g. 0,1)");
		CHECK(refused({ "--devices", "0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15,16" }) == "--devices: more than 16 devices");
		CHECK(refused({ "--devices", "0,1,2,3,4,5,6,7,8,9,10,11,12,13,14,15" }) == "(accepted)");
		CHECK(refused({ "in.fq", "-o" }) == "option -o requires an argument");
		CHECK(refused({ "--samples" }) == "option --samples requires an argument");
	}

	// ---- copy_out: the whole length comes back, the buffer is terminated whenever it has room for that ----
	{
		const std::string s = "hello";
		char buf[8];
		memset(buf, 'x', sizeof buf);
		CHECK(copy_out(s, buf, 0) == 5 && buf[0] == 'x' && copy_out(s, nullptr, 8) == 5);
		CHECK(copy_out(s, buf, 1) == 5 && buf[0] == 0 && buf[1] == 'x');
		CHECK(copy_out(s, buf, 3) == 5 && !strcmp(buf, "he") && buf[3] == 'x');
		CHECK(copy_out(s, buf, 6) == 5 && !strcmp(buf, "hello") && buf[6] == 'x');
	}

	// ---- the sample sheet, for two B segments ----
	{
		ArchPtr a, wide;
		std::string why;
		CHECK(parse_arch({ "B:ACGT,TTGA", "S:GG", "B:CC,GG", "R:N" }, a, why));
		SampleSheet sh;
		auto sheet = [&](const std::string& text) { const std::string p = put("sheet.txt", text); return read_sample_sheet(p.c_str(), a.get(), sh) == TD_OK ? std::string() : std::string(td_run_last_error()); };
		const std::string at = "--samples: " + g_dir + "/sheet.txt";
		CHECK(sheet("s1 ACGT CC\ns.2_-\tTTGA \t GG\n") == "");
		CHECK(sh.n() == 2 && sh.segs == std::vector<int>({ 0, 2 }) && sh.names == std::vector<std::string>({ "s1", "s.2_-" }) && sh.tuples == std::vector<int32_t>({ 0, 0, 1, 1 }));
		CHECK(sheet("# name b1 b2\n\n   \ns1 TTGA CC\n#s2 ACGT GG\n") == "" && sh.n() == 1 && sh.tuples == std::vector<int32_t>({ 1, 0 }));
		CHECK(sheet("s1 ACGT CC\r\n\r\ns2 TTGA GG\r\n") == "" && sh.n() == 2 && sh.names[1] == "s2" && sh.tuples == std::vector<int32_t>({ 0, 0, 1, 1 }));
		CHECK(sheet("s1 ACGT CC\ns2 TTGA\n") == at + " line 2: 2 columns, need 3 (the name and one barcode per barcode segment).");
		CHECK(sheet("s1 ACGT CC GG\n") == at + " line 1: 4 columns, need 3 (the name and one barcode per barcode segment).");
		CHECK(sheet("s+1 ACGT CC\n") == at + " line 1: the name 's+1' is not 1..64 characters of [A-Za-z0-9._-].");
		const std::string longest(TD_SAMPLES_MAX_NAME, 'n');
		CHECK(sheet(longest + " ACGT CC\n") == "" && sh.names[0] == longest);
		CHECK(sheet("\n" + longest + "n ACGT CC\n") == at + " line 2: the name '" + longest + "n' is not 1..64 characters of [A-Za-z0-9._-].");
		CHECK(sheet("s1 ACGT CC\ns2 AAAA GG\n") == at + " line 2: 'AAAA' is not a barcode of segment 1.");
		CHECK(sheet("s1 ACGT GGG\n") == at + " line 1: 'GGG' is not a barcode of segment 3.");
		CHECK(sheet("s1 NNNN CC\n") == at + " line 1: 'NNNN' is not a barcode of segment 1.");   // (the all-N wildcard is no barcode to list)
		CHECK(sheet("s1 ACGT NN\n") == at + " line 1: 'NN' is not a barcode of segment 3.");
		CHECK(sheet("s1 ACGT CC\n# x\ns1 TTGA GG\n") == at + " line 3: the name 's1' is taken by line 1.");
		CHECK(sheet("\ns1 ACGT CC\ns2 TTGA CC\ns3 ACGT CC\n") == at + " line 4: the barcodes repeat those of line 2.");
		CHECK(sheet("# nothing\n\n") == at + " lists no sample." && sheet("") == at + " lists no sample.");
		CHECK(read_sample_sheet((g_dir + "/none.txt").c_str(), a.get(), sh) == TD_FAIL && td_run_last_error() == "--samples: cannot open the sample sheet " + g_dir + "/none.txt.");
		// TD_SAMPLES_MAX + 1 rows, all different: sixteen barcodes in each of two segments
		std::string all16, rows;
		std::vector<std::string> two;
		for (int q = 0; q < 16; q++) two.push_back({ "ACGT"[q >> 2], "ACGT"[q & 3] });
		for (int q = 0; q < 16; q++) all16 += (q ? "," : "") + two[(size_t)q];
		CHECK(parse_arch({ "B:" + all16, "B:" + all16, "R:N" }, wide, why));
		for (int q = 0; q < TD_SAMPLES_MAX + 1; q++) rows += "n" + std::to_string(q) + " " + two[(size_t)(q >> 4)] + " " + two[(size_t)(q & 15)] + "\n";
		const std::string p = put("sheet.txt", rows);
		CHECK(read_sample_sheet(p.c_str(), wide.get(), sh) == TD_FAIL && td_run_last_error() == at + " line 256: more than 255 samples.");
		put("sheet.txt", rows.substr(0, rows.rfind("n255")));
		CHECK(read_sample_sheet(p.c_str(), wide.get(), sh) == TD_OK && sh.n() == TD_SAMPLES_MAX && sh.tuples[2 * 254] == 15 && sh.tuples[2 * 254 + 1] == 14);
	}

	// ---- which file plays which part ----
	{
		RunRoles r;
		const std::vector<std::string> o = { "-o", out };
		auto with = [&](std::vector<std::string> more) { more.insert(more.end(), o.begin(), o.end()); return more; };
		CHECK(roles(o, { "B:ACGT,TTGA R:N" }, r) == "");
		CHECK(r.bar_file == 0 && r.num_out_reads == 1 && r.mol_file == 0 && r.mate_file == -1 && r.qual_file == -1 && r.sheet.n() == 0);
		CHECK(r.out_files == std::vector<std::string>({ out + "_BC_ACGT.fq", out + "_BC_TTGA.fq", out + "_un.fq" }));
		CHECK(roles(with({ "--unknown-barcodes", "3", "--min-base-quality", "20" }), { "R:N", "R:N", "B:ACGT,TTGA F:NNNN R:N" }, r) == "");
		CHECK(r.bar_file == 2 && r.num_out_reads == 3 && r.mol_file == 0 && r.mate_file == -1 && r.qual_file == 2 && r.out_files.size() == 10 && r.out_files[9] == out + "_unknown_barcodes.txt");
		// --mate-bases: the one decoded file counts, the first other file is its mate
		CHECK(roles(with({ "--mate-bases", "8", "--min-base-quality", "20" }), { "R:N", "B:ACGT,TTGA F:NNNN R:N" }, r) == "");
		CHECK(r.bar_file == 1 && r.num_out_reads == 2 && r.mol_file == 1 && r.mate_file == 0 && r.qual_file == 1);
		CHECK(r.out_files == std::vector<std::string>({ out + "_BC_ACGT_READ1.fq", out + "_BC_TTGA_READ1.fq", out + "_un_READ1.fq", out + "_BC_ACGT_READ2.fq",
		                                                out + "_BC_TTGA_READ2.fq", out + "_un_READ2.fq", out + "_molecules.txt" }));
		CHECK(roles(with({ "--mate-bases", "8" }), { "B:ACGT,TTGA R:N", "R:N", "R:N" }, r) == "" && r.mol_file == 0 && r.mate_file == 1);
		// two decoded files: each option refuses in its own words
		CHECK(roles(with({ "--mate-bases", "8" }), { "B:ACGT,TTGA R:N", "F:NNNN R:N" }, r) ==
		      "--mate-bases: exactly one input file may have an architecture other than R:N (2 have): barcode and fingerprint of a molecule come from one "
		      "decoded file, every other file gives reads.");
		CHECK(roles(with({ "--min-base-quality", "20" }), { "B:ACGT,TTGA R:N", "F:NNNN R:N" }, r) ==
		      "--min-base-quality: exactly one input file may have an architecture other than R:N (2 have): one file's verdicts are the run's.");
		CHECK(roles(with({ "--mate-bases", "8" }), { "R:N", "R:N" }, r) ==
		      "--mate-bases: exactly one input file may have an architecture other than R:N (0 have): barcode and fingerprint of a molecule come from one "
		      "decoded file, every other file gives reads.");
		CHECK(roles(with({ "--min-base-quality", "20" }), { "R:N" }, r) ==
		      "--min-base-quality: the architecture is a single read segment: there is no model whose labels mark a barcode or a fingerprint.");
		CHECK(roles(o, { "B:ACGT,TTGA R:N", "B:CC,GG R:N" }, r) == "Barcodes seem to be in both architectures... ");
		CHECK(roles(with({ "--samples", "S" }), { "B:ACGT,TTGA R:N", "B:CC,GG R:N" }, r) ==
		      "Barcodes seem to be in both architectures... (--samples: barcodes spread over several input files are not joined; the controller's rule of one "
		      "barcode file stays, and a sheet lists the barcode segments of that one file.)");
		CHECK(roles(o, { "B:ACGT,TTGA", "F:NNNN" }, r) == "No read segment in any architecture: there would be no output file.");
		CHECK(roles(with({ "--collapse-umis" }), { "B:ACGT,TTGA R:N" }, r) ==
		      "--collapse-umis: the architecture has no fingerprint (F) segment: there is no UMI whose neighbours could be collapsed.");
		CHECK(roles(with({ "--collapse-umis" }), { "F:NNNN R:N" }, r) == "" && r.bar_file == -1 && r.out_files == std::vector<std::string>({ out + ".fq", out + "_un.fq", out + "_molecules.txt" }));
		CHECK(roles(with({ "--min-base-quality", "20", "--quality-segments", "F" }), { "B:ACGT,TTGA R:N" }, r) ==
		      "--min-base-quality: the architecture has no segment of the types --quality-segments names: there is no base to judge.");
		CHECK(roles(with({ "--min-base-quality", "20", "--quality-segments", "B" }), { "B:ACGT,TTGA R:N" }, r) == "" && r.qual_file == 0);
		CHECK(roles(with({ "--samples", g_dir + "/none.txt" }), { "F:NNNN R:N" }, r) == "--samples: no input file's architecture has a barcode segment.");
		CHECK(roles(with({ "--unknown-barcodes", "3" }), { "F:NNNN R:N" }, r) == "--unknown-barcodes: no input file's architecture has a barcode segment.");
		CHECK(roles(with({ "--molecules" }), { "R:N" }, r) == "--molecules: the architecture is a single read segment: there is no model whose labels mark a barcode or a fingerprint.");
		// --samples: the files are named after the sheet, the sheet is the roles'
		const std::string sheet = put("roles_sheet.txt", "left ACGT\nright TTGA\n");
		CHECK(roles(with({ "--samples", sheet, "--molecules" }), { "B:ACGT,TTGA R:N" }, r) == "" && r.sheet.n() == 2 && r.sheet.segs == std::vector<int>({ 0 }));
		CHECK(r.out_files == std::vector<std::string>({ out + "_BC_left.fq", out + "_BC_right.fq", out + "_un.fq", out + "_samples.txt", out + "_molecules.txt" }));
		// --join-barcodes: every barcode file is collected, the first holds the sheet, the columns are the files' 'B' segments, files first
		const std::string joined = put("roles_joined.txt", "a ACGT CC TT\nb TTGA GG AA\n");
		CHECK(roles(with({ "--samples", joined, "--join-barcodes" }), { "R:N", "B:ACGT,TTGA", "B:CC,GG S:A B:TT,AA R:N" }, r) == "");
		CHECK(r.bar_file == 1 && r.bar_files == std::vector<int>({ 1, 2 }) && r.first_column == std::vector<int>({ 0, 1 }) && r.num_out_reads == 2);
		CHECK(r.column_hmms == std::vector<int32_t>({ 3, 3, 3 }) && r.sheet.n() == 2 && r.sheet.segs == std::vector<int>({ 0, 0, 2 }) && r.sheet.files == std::vector<int>({ 1, 2, 2 }));
		CHECK(r.sheet.tuples == std::vector<int32_t>({ 0, 0, 0, 1, 1, 1 }));
		CHECK(r.join_line == "join: files 1,2; columns 1 = segment 1 of file 1, 2 = segment 1 of file 2, 3 = segment 3 of file 2; file 1 holds the sheet, a read whose "
		                     "partner in another barcode file is not extracted goes to _un\n");
		CHECK(r.out_files == std::vector<std::string>({ out + "_BC_a_READ1.fq", out + "_BC_b_READ1.fq", out + "_un_READ1.fq", out + "_BC_a_READ2.fq", out + "_BC_b_READ2.fq",
		                                                out + "_un_READ2.fq", out + "_samples.txt" }));
		CHECK(roles(with({ "--samples", joined, "--join-barcodes" }), { "B:ACGT,TTGA R:N", "R:N" }, r) ==
		      "--join-barcodes: only one input file (-) has barcode segments: there is nothing to join, drop the option (--samples alone assigns by all barcode "
		      "segments of one file).");
		CHECK(roles(with({ "--samples", joined, "--join-barcodes" }), { "B:AC,GT S:A B:AC,GT S:A B:AC,GT", "B:AC,GT S:A B:AC,GT R:N" }, r) ==
		      "--join-barcodes: the barcode files have 5 barcode segments together (at most 4).");
		CHECK(roles(with({ "--samples", joined, "--join-barcodes" }), { "B:ACGT,TTGA", "B:CC,GG R:N" }, r) ==
		      "--samples: " + joined + " line 1: 4 columns, need 3 (the name and one barcode per barcode segment of every barcode file, files first).");
		const std::string wrong = put("roles_wrong.txt", "a ACGT CC TT\nb TTGA GG CC\n");
		CHECK(roles(with({ "--samples", wrong, "--join-barcodes" }), { "B:ACGT,TTGA", "B:CC,GG S:A B:TT,AA R:N" }, r) ==
		      "--samples: " + wrong + " line 2: 'CC' (column 3) is not a barcode of segment 3 of file 1 (-).");
		// an output file that exists
		put("out_BC_TTGA.fq", "");
		CHECK(roles(o, { "B:ACGT,TTGA R:N" }, r) == "Error: some output files already exists. (" + out + "_BC_TTGA.fq; --force overwrites)");
		CHECK(roles(with({ "--force" }), { "B:ACGT,TTGA R:N" }, r) == "" && r.out_files.size() == 3);
		put("out_un.fq", "");
		CHECK(roles(o, { "F:NNNN R:N" }, r) == "");   // (the check is made for a barcode file only)
		const char* arch[2] = { "-1 R:N", "-1 B:ACGT,TTGA -2 R:N" };
		td_run_opts* po = parse(with({ "--force" }));
		char buf[4096];
		CHECK(po && td_run_output_files_describe(po, arch, 2, buf, sizeof buf) > 0);
		CHECK(buf == out + "_BC_ACGT_READ1.fq\n" + out + "_BC_TTGA_READ1.fq\n" + out + "_un_READ1.fq\n" + out + "_BC_ACGT_READ2.fq\n" + out + "_BC_TTGA_READ2.fq\n" + out + "_un_READ2.fq\n");
		td_run_opts_free(po);
	}

	// ---- the plan's text ----
	{
		const std::string in = put("in.fq", "@r\nACGT\n+\nIIII\n"), sheet = put("plan_sheet.txt", "s1 ACGT\ns2 TTGA\n"), o2 = g_dir + "/plan";
		bool all_known = false;
		CHECK(plan_text({ "-1", "B:ACGT,TTGA", "-2", "F:NNNN", "-3", "R:N", "--dedup-collapsed", "--samples", sheet, "--min-base-quality", "20", in, "-o", o2 }, &all_known) ==
		      "file 0 architecture: command line: -1 B:ACGT,TTGA -2 F:NNNN -3 R:N\n"
		      "dust: 100\n"
		      "ref: off\n"
		      "dedup: one read per molecule is written (barcode, fingerprint and the start of the read)\n"
		      "collapse: fingerprints one mismatch apart are counted as one molecule (directional rule; the count and --dedup stay exact)\n"
		      "dedup-collapsed: the input is read twice, a survey and then the run: one read per collapsed molecule is written, the first that carries the root's barcode, fingerprint and start\n"
		      "samples: " + sheet + ": 2 samples by segment 1 of file 0; a read whose barcodes are incomplete or name no sample goes to _un\n"
		      "quality: an extracted read with more than 0 bases below Q20 (offset 33) in its barcode or fingerprint segments goes to _un and is neither assigned, counted nor kept by --dedup\n"
		      "barcode file: 0\n"
		      "output reads: 1\n"
		      "output file: " + o2 + "_BC_s1.fq\n"
		      "output file: " + o2 + "_BC_s2.fq\n"
		      "output file: " + o2 + "_un.fq\n"
		      "output file: " + o2 + "_samples.txt\n"
		      "output file: " + o2 + "_molecules.txt\n");
		CHECK(all_known);
		const std::string af = put("arch.txt", "# candidates\ntagdust -1 B:ACGT,TTGA -2 R:N\nnothing here\ntagdust -1 R:N\n");
		CHECK(plan_text({ "-arch", af, "--samples", sheet, in, "-o", o2 }, &all_known) ==
		      "file 0 architecture: arch file: best of 2 candidates\n"
		      "arch file candidate 0: -1 B:ACGT,TTGA -2 R:N\n"
		      "arch file candidate 1: -1 R:N\n"
		      "dust: 100\n"
		      "ref: off\n"
		      "samples: " + sheet + ": resolved once the arch file's choice is made\n"
		      "output files: named once the arch file's choice is made\n");
		CHECK(!all_known);
		CHECK(plan_text({ "-1", "R:N", "--mate-bases", "8", "--mate-filter", in, in, "-o", o2 }, &all_known) ==
		      "plan: --mate-bases: exactly one input file may have an architecture other than R:N (0 have): barcode and fingerprint of a molecule come from one "
		      "decoded file, every other file gives reads.");
	}

	ArchPtr one, two, none;
	std::string why;
	CHECK(parse_arch({ "B:ACGT,TTGA", "R:N" }, one, why) && parse_arch({ "B:ACGT,TTGA", "S:GG", "B:CC,GG", "R:N" }, two, why) && parse_arch({ "F:NNNN", "R:N" }, none, why));

	// ---- <out>_unknown_barcodes.txt ----
	{
		td_run_opts* o = parse({ "--unknown-barcodes", "2" });
		CHECK(o);
		td_census_entry e[4] = { { census_key("ACGA"), 5 }, { census_key("AAGA"), 3 }, { census_key("TTGG"), 3 }, { 0, 1 } };
		td_run_report r{};
		r.unknown = e; r.n_unknown = 3;
		r.unknown_totals = td_census_totals{ 20, 11, 4, 2, 3, 0, 3 };
		const std::string head = "# unknown barcodes: what the reads that were not extracted spell in segment 1 (B:ACGT,TTGA) of reads.fq\n"
		                         "# eligible reads\t20\n# counted\t11\n# distinct sequences\t3\n# no base in the segment\t4\n# more than 28 bases\t2\n# with N\t3\n";
		const std::string cols = "# count\tsequence\tnearest\tdistance\n", two_lines = "5\tACGA\tACGT\t1\n3\tAAGA\tACGT\t2\n";   // (AAGA is two from both: the lower index)
		std::string text;
		CHECK(unknown_barcodes_text(o, one.get(), { "B:ACGT,TTGA", "R:N" }, "reads.fq", r, text) && text == head + cols + two_lines);
		o->unknown_barcodes = 10;
		text.clear();
		CHECK(unknown_barcodes_text(o, one.get(), { "B:ACGT,TTGA", "R:N" }, "reads.fq", r, text) && text == head + cols + two_lines + "3\tTTGG\tTTGA\t1\n");
		r.unknown_totals.overflow = 7;
		text.clear();
		CHECK(unknown_barcodes_text(o, one.get(), { "B:ACGT,TTGA", "R:N" }, "reads.fq", r, text));
		CHECK(text == head + "# the counting table was too small: 7 reads were not counted (the counts below are exact; --unknown-barcodes-slots 21 or more)\n" + cols + two_lines + "3\tTTGG\tTTGA\t1\n");
		// the last 'B' segment is the one that is spelled; a value that is no key ends the text where it stands
		r.unknown_totals.overflow = 0; r.n_unknown = 4; e[0].key = census_key("CG");
		text.clear();
		CHECK(!unknown_barcodes_text(o, two.get(), { "B:ACGT,TTGA", "S:GG", "B:CC,GG", "R:N" }, "reads.fq", r, text) && g_err.find("is no key") != std::string::npos);
		CHECK(text == "# unknown barcodes: what the reads that were not extracted spell in segment 3 (B:CC,GG) of reads.fq\n" + head.substr(head.find("# eligible")) + cols +
		              "5\tCG\tCC\t1\n3\tAAGA\tGG\t3\n3\tTTGG\tGG\t2\n");
		td_run_opts_free(o);
	}

	// ---- <out>_samples.txt ----
	{
		td_run_opts* o = parse({ "--samples", "sheet.txt" });
		CHECK(o);
		SampleSheet sh;
		sh.segs = { 0, 2 }; sh.names = { "s1", "s2" }; sh.tuples = { 0, 0, 1, 1 };
		const int32_t s1[2] = { 0, 0 }, decoy[2] = { 0, 2 }, missing[2] = { -1, 1 };
		td_census_entry e[3] = { { td_samples_key(s1, 2), 6 }, { td_samples_key(decoy, 2), 2 }, { td_samples_key(missing, 2), 1 } };
		td_run_report r{};
		r.samples = e; r.n_sample_keys = 3;
		r.samples_totals = td_samples_totals{ 10, 6, 1, 3, 0 };
		const std::vector<std::string> segs = { "B:ACGT,TTGA", "S:GG", "B:CC,GG", "R:N" };
		const std::string head = "# samples: the extracted reads of reads.fq by all their barcodes\n# sheet\tsheet.txt\n# samples\t2\n# segments\t1 (B:ACGT,TTGA)\t3 (B:CC,GG)\n";
		const std::string cols = "# sample\tbarcode 1\tbarcode 2\treads\tshare\n";
		std::string text;
		CHECK(samples_text(o, two.get(), segs, "reads.fq", sh, r, text));
		CHECK(text == head + "# extracted reads\t10\n# assigned\t6\n# not in the sheet\t1\n# incomplete\t3\n# not counted\t0\n" + cols +
		              "s1\tACGT\tCC\t6\t0.6000\ns2\tTTGA\tGG\t0\t0.0000\n# combinations not in the sheet\nACGT\tNN\t2\t0.2000\n-\tGG\t1\t0.1000\n");
		r.samples_totals = td_samples_totals{ 0, 0, 0, 0, 4 };
		text.clear();
		CHECK(samples_text(o, two.get(), segs, "reads.fq", sh, r, text));
		const std::string empty = head + "# extracted reads\t0\n# assigned\t0\n# not in the sheet\t0\n# incomplete\t0\n# not counted\t4\n"
		                          "# the counting table was too small: the counts below are exact, 4 reads are in none of them\n" + cols +
		                          "s1\tACGT\tCC\t6\t0.0000\ns2\tTTGA\tGG\t0\t0.0000\n# combinations not in the sheet\nACGT\tNN\t2\t0.0000\n";
		CHECK(text == empty + "-\tGG\t1\t0.0000\n");
		e[2].key = td_samples_key(s1, 1);   // a key of one segment in a sheet of two: the text ends in front of it
		text.clear();
		CHECK(!samples_text(o, two.get(), segs, "reads.fq", sh, r, text) && td_run_last_error() == std::string("--samples: 0x100000000000001 is no key of 2 segments"));
		CHECK(text == empty);
		td_run_opts_free(o);
	}

	// ---- <out>_molecules.txt ----
	{
		const std::string levels0 = "\t0\t0\t0\t0\t0\t0\t0\t0", cols = "# barcode\treads\tmolecules\tduplication\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10+";
		const std::string head = "# molecules: the extracted reads of reads.fq by barcode, fingerprint and the first bases of the read\n# prefix bases\t20\n";
		const std::string sums = "# extracted reads\t16\n# counted\t14\n# molecules\t12\n# no read base\t1\n# N in the prefix\t1\n";
		const std::string collapse = "# UMI collapse\tfingerprints one mismatch apart, directional rule\n# molecules after collapse\t11\n# absorbed\t1\n";
		std::vector<td_mol_row> rows(TD_NUM_BARCODE_BINS), crows(TD_NUM_BARCODE_BINS);
		rows[0].reads = 10; rows[0].molecules = 8; rows[0].levels[0] = 6; rows[0].levels[1] = 2;
		rows[1].reads = 4; rows[1].molecules = 4; rows[1].levels[0] = 4;
		crows[0].molecules = 7; crows[1].molecules = 4;
		td_run_report r{};
		r.molecules = rows.data();
		r.molecules_totals = td_mol_totals{ 16, 14, 1, 1, 0, 12 };
		r.collapse_totals = td_mol_collapse_totals{ 12, 11, 1, 2 };
		r.dedup_totals = td_mol_dedup_totals{ 12, 2, 0 };
		SampleSheet sh, no_sheet;
		sh.segs = { 0 }; sh.names = { "left", "right" }; sh.tuples = { 0, 1 };
		td_run_opts* plain = parse({ "--molecules" });
		td_run_opts* coll = parse({ "--collapse-umis" });
		CHECK(plain && coll);
		const std::string total = "total\t14\t12\t0.1429\t10\t2" + levels0 + "\n", total_c = "total\t14\t12\t0.1429\t10\t2" + levels0 + "\t11\t0.2143\n";
		// rows by sheet name, by barcode spelling, the one "-" row: plain, then with the collapse columns
		CHECK(molecules_text(plain, one.get(), "reads.fq", nullptr, 100, false, sh, r) ==
		      head + sums + cols + "\nleft\t10\t8\t0.2000\t6\t2" + levels0 + "\nright\t4\t4\t0.0000\t4\t0" + levels0 + "\n" + total);
		CHECK(molecules_text(plain, one.get(), "reads.fq", nullptr, 100, false, no_sheet, r) ==
		      head + sums + cols + "\nACGT\t10\t8\t0.2000\t6\t2" + levels0 + "\nTTGA\t4\t4\t0.0000\t4\t0" + levels0 + "\n" + total);
		CHECK(molecules_text(plain, none.get(), "reads.fq", nullptr, 100, false, no_sheet, r) == head + sums + cols + "\n-\t10\t8\t0.2000\t6\t2" + levels0 + "\n" + total);
		CHECK(molecules_text(plain, none.get(), "reads.fq", nullptr, 100, false, sh, r) == head + sums + cols + "\n-\t10\t8\t0.2000\t6\t2" + levels0 + "\n" + total);
		r.molecules_collapsed = crows.data();
		const std::string cols_c = cols + "\tcollapsed\tduplication_collapsed\n";
		CHECK(molecules_text(coll, one.get(), "reads.fq", nullptr, 100, false, sh, r) ==
		      head + sums + collapse + cols_c + "left\t10\t8\t0.2000\t6\t2" + levels0 + "\t7\t0.3000\nright\t4\t4\t0.0000\t4\t0" + levels0 + "\t4\t0.0000\n" + total_c);
		CHECK(molecules_text(coll, one.get(), "reads.fq", nullptr, 100, false, no_sheet, r) ==
		      head + sums + collapse + cols_c + "ACGT\t10\t8\t0.2000\t6\t2" + levels0 + "\t7\t0.3000\nTTGA\t4\t4\t0.0000\t4\t0" + levels0 + "\t4\t0.0000\n" + total_c);
		CHECK(molecules_text(coll, none.get(), "reads.fq", nullptr, 100, false, no_sheet, r) == head + sums + collapse + cols_c + "-\t10\t8\t0.2000\t6\t2" + levels0 + "\t7\t0.3000\n" + total_c);
		// more listed barcodes than bins: a row per bin, and the total over all bins
		std::string many = "B:";
		for (int q = 0; q < TD_NUM_BARCODE_BINS + 44; q++) many += std::string(q ? "," : "") + "ACGT"[q >> 8] + "ACGT"[(q >> 6) & 3] + "ACGT"[(q >> 4) & 3] + "ACGT"[(q >> 2) & 3] + "ACGT"[q & 3];
		ArchPtr wide;
		CHECK(parse_arch({ many, "R:N" }, wide, why) && wide->n_seq[0] == TD_NUM_BARCODE_BINS + 45);
		rows[TD_NUM_BARCODE_BINS - 1].reads = 2; rows[TD_NUM_BARCODE_BINS - 1].molecules = 1; rows[TD_NUM_BARCODE_BINS - 1].levels[1] = 1;
		crows[TD_NUM_BARCODE_BINS - 1].molecules = 1;
		for (td_run_opts* o : { plain, coll }) {
			r.molecules_collapsed = o == coll ? crows.data() : nullptr;
			const std::string text = molecules_text(o, wide.get(), "reads.fq", nullptr, 100, false, no_sheet, r), c = o == coll ? "\t1\t0.5000" : "";
			CHECK(count(text, "\n") == (o == coll ? 11 : 8) + TD_NUM_BARCODE_BINS + 1 && count(text, "\nAAAAA\t10\t8\t") == 1 && count(text, "\nCAAAA\t") == 0);
			CHECK(text.find("\nAAAAC\t4\t4\t0.0000\t4\t0" + levels0) != std::string::npos);
			const std::string tail = "\nATTTG\t0\t0\t0.0000\t0\t0" + levels0 + (o == coll ? "\t0\t0.0000" : "") + "\nATTTT\t2\t1\t0.5000\t0\t1" + levels0 + c +
			                         "\ntotal\t16\t13\t0.1875\t10\t3" + levels0 + (o == coll ? "\t12\t0.2500" : "") + "\n";
			CHECK(text.size() > tail.size() && text.compare(text.size() - tail.size(), tail.size(), tail) == 0);
		}
		td_run_opts_free(plain);
		td_run_opts_free(coll);
		rows[TD_NUM_BARCODE_BINS - 1] = td_mol_row{};
		r.molecules_collapsed = nullptr;
		// every header line is there exactly when its option or condition is
		struct { std::vector<std::string> words; bool use_ref; int64_t overflow; const char* lines; } heads[] = {
			{ { "--molecules" }, false, 0, "" },
			{ { "--mate-bases", "8" }, false, 0, "# mate bases\t8\n# mate file\tmates.fq\n" },
			{ { "--mate-bases", "8", "--mate-filter" }, false, 0, "# mate bases\t8\n# mate file\tmates.fq\n# mate filter\tdust 100, -ref none\n" },
			{ { "--mate-bases", "8", "--mate-filter", "-ref", "artifacts.fa" }, true, 0, "# mate bases\t8\n# mate file\tmates.fq\n# mate filter\tdust 100, -ref artifacts.fa\n" },
			{ { "--dedup" }, false, 0, "# written\t12\n# duplicates removed\t2\n" },
			{ { "--dedup-collapsed" }, false, 0, "# dedup\tcollapsed molecules\n# written\t12\n# duplicates removed\t2\n" },
			{ { "--molecules", "--molecules-slots", "10" }, false, 5, "# the counting table was too small: 5 reads were not counted (the counts below are exact; --molecules-slots 11 or more)\n" },
		};
		for (auto& h : heads) {
			td_run_opts* o = parse(h.words);
			CHECK(o);
			r.molecules_totals.overflow = h.overflow;
			r.molecules_collapsed = o->collapse_umis ? crows.data() : nullptr;
			const std::string text = molecules_text(o, one.get(), "reads.fq", "mates.fq", 100, h.use_ref, no_sheet, r), lines = h.lines;
			const size_t split = lines.find("# mate") == 0 ? lines.size() : 0;   // (the mate's lines stand in front of the sums, the others behind them)
			CHECK(text.find(head + lines.substr(0, split) + sums + lines.substr(split) + (o->collapse_umis ? collapse : "") + cols) == 0);
			for (const char* key : { "# mate bases", "# mate file", "# mate filter", "# the counting table", "# dedup\t", "# written", "# duplicates removed", "# UMI collapse" })
				CHECK(count(text, key) == count(lines + (o->collapse_umis ? collapse : ""), key));
			td_run_opts_free(o);
		}
	}

	// ---- the summary block ----
	{
		td_run_opts* o = parse({ "reads.fq", "mates.fq" });
		CHECK(o);
		td_run_report r{};
		r.counts[TD_EXTRACT_SUCCESS] = 80; r.counts[TD_EXTRACT_FAIL_ARCHITECTURE_MISMATCH] = 5; r.counts[TD_EXTRACT_FAIL_BAR_FINGER_NOT_FOUND] = 6;
		r.counts[TD_EXTRACT_FAIL_READ_TOO_SHORT] = 4; r.counts[TD_EXTRACT_FAIL_LOW_COMPLEXITY] = 3; r.counts[TD_EXTRACT_FAIL_MATCHES_ARTIFACTS] = 2;
		r.counts[TD_NUM_OUTCOME_SLOTS] = 1000;   // (a barcode bin: no part of the total)
		r.selected_threshold = 20.5f;
		auto summary = [&]() { char buf[2048]; const int64_t n = td_run_format_summary(o, &r, buf, sizeof buf); return n == (int64_t)strlen(buf) ? std::string(buf) : std::string("(length)"); };
		const std::string files = "Done.\n\nreads.fq\tInput file 0.\nmates.fq\tInput file 1.\n";
		const std::string counts = "5\tproblems with architecture\n6\tbarcode / UMI not found\n4\ttoo short\n3\tlow complexity\n2\tmatch artifacts:\n";
		const std::string body = files + "100\ttotal input reads\n20.50\tselected threshold\n80\tsuccessfully extracted\n80.0%\textracted\n" + counts;
		CHECK(summary() == body);
		int64_t hits[3] = { 0, 2, 1 };
		char n0[] = "first", n2[] = "third";
		char* names[3] = { n0, nullptr, n2 };
		r.n_artifacts = 3; r.artifact_hits = hits; r.artifact_names = names;
		CHECK(summary() == body + "2\t\n1\tthird\n");
		r.n_artifacts = 0;
		r.quality = 1; r.quality_totals.failed = 9;
		CHECK(summary() == body);   // (the line belongs to the option, not to the report)
		o->min_base_quality = 20; o->max_low_bases = 1;
		CHECK(summary() == body + "9\tlow base quality in barcode / UMI (Q < 20, more than 1 bases)\n");
		r.quality = 0;
		CHECK(summary() == body);
		// no read at all: the share is 0 / 0 as a float, and is printed as that
		memset(r.counts, 0, sizeof r.counts);
		CHECK(summary() == files + "0\ttotal input reads\n20.50\tselected threshold\n0\tsuccessfully extracted\n-nan%\textracted\n" +
		                   "0\tproblems with architecture\n0\tbarcode / UMI not found\n0\ttoo short\n0\tlow complexity\n0\tmatch artifacts:\n");
		td_run_opts_free(o);
	}
	return 0;
}

int main()
{
	const char* tmp = getenv("TMPDIR");
	std::string dir = std::string(tmp && *tmp ? tmp : "/tmp") + "/run_host_check.XXXXXX";
	if (!mkdtemp(&dir[0])) { fprintf(stderr, HOST_CHECK_NAME ": cannot make a directory under %s\n", tmp && *tmp ? tmp : "/tmp"); return 1; }
	g_dir = dir;
	const int rc = checks();
	for (const std::string& p : g_made) unlink(p.c_str());
	if (rmdir(g_dir.c_str()) != 0) { fprintf(stderr, HOST_CHECK_NAME ": %s is not empty\n", g_dir.c_str()); return 1; }
	if (rc == 0) printf("run_host_check: ok\n");
	return rc;
}
