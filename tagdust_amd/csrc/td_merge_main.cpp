// td_merge_main.cpp -- `tagdust-merge`: the reference's `merge` command line on libtagdust_hip.so (include/tagdust_merge.h).
// Exit status 0 on success, 1 on any error with the message on stderr.
#include <stdio.h>

#include "../../include/tagdust_merge.h"

int main(int argc, char** argv)
{
	char err[1024] = "";
	td_merge_args args;
	if (td_merge_parse_args(argc, argv, &args, err, sizeof err) != TD_OK) { fprintf(stderr, "tagdust-merge: %s\n", err); return 1; }
	if (args.help || argc < 2) { fputs(td_merge_usage(), stdout); return 0; }
	td_merge_stats st;
	if (td_merge_stream(args.in1, args.in2, args.out_path, &args.opts, &st) != TD_OK) { fprintf(stderr, "tagdust-merge: %s\n", td_merge_last_error()); return 1; }
	fprintf(stderr, "tagdust-merge: %lld pairs, %lld merged reads written, %lld below the threshold, %lld too short, %.2f s\n",
	        (long long)st.n_pairs, (long long)st.n_written, (long long)st.n_below, (long long)st.n_too_short, st.wall_s);
	return 0;
}
