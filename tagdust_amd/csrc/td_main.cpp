// td_main.cpp -- `tagdust-hip`: the tagdust command line on libtagdust_hip.so (include/tagdust_run.h).  Exit status 0 on success,
// 1 on any error with the message on stderr -- a deliberate departure: the reference returns EXIT_SUCCESS on its error paths and
// writes the text to stdout (src/main.c:209-215).
#include <stdio.h>

#include "../../include/tagdust_run.h"

int main(int argc, char** argv)
{
	char err[1024] = "";
	td_run_opts* opts = nullptr;
	if (td_run_parse_args(argc, argv, &opts, err, sizeof err) != TD_OK) { fprintf(stderr, "tagdust-hip: %s\n", err); return 1; }
	int rc = 0;
	if (opts->help || argc < 2) fputs(td_run_usage(), stdout);
	else if (opts->version) fputs(td_run_version(), stdout);
	else if (opts->dry_run) {
		td_run_plan_t* plan = nullptr;
		if (td_run_plan(opts, &plan) != TD_OK) { fprintf(stderr, "tagdust-hip: %s\n", td_run_last_error()); rc = 1; }
		else {
			const int64_t n = td_run_plan_describe(plan, nullptr, 0);
			char* text = new char[(size_t)n + 1];
			td_run_plan_describe(plan, text, n + 1);
			fputs(text, stdout);
			delete[] text;
			td_run_plan_free(plan);
		}
	} else {
		opts->echo_log = 1;
		td_run_report report;
		if (td_run_execute(opts, &report) != TD_OK) { fprintf(stderr, "tagdust-hip: %s\n", report.error); rc = 1; }
		td_run_report_clear(&report);
	}
	td_run_opts_free(opts);
	return rc;
}
