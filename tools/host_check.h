// host_check.h -- what the stand-alone programs over the host units of the two counts (tools/census_host_check.cpp,
// molecules_host_check.cpp, dedup_host_check.cpp, collapse_host_check.cpp, dedup_collapsed_host_check.cpp, mate_host_check.cpp, samples_host_check.cpp, quality_host_check.cpp) share: the message sink td_api.hip would be, a
// generator, CHECK (tools/batch_plan_host_check.cpp, over the batch geometry unit, and tools/model_host_check.cpp, over the model path, take the last two; tools/run_host_check.cpp, over the whole-run driver's device-free units, the sink and CHECK).  The program defines HOST_CHECK_NAME, its name in the messages, before it includes this.  tools/host_checks.sh
// builds and runs them all.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../tagdust_amd/csrc/td_count_key.h"

// td_api.hip is not part of these programs: the message sink of the units under test
static std::string g_err;
int fail(td_ctx*, const char* fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	g_err = buf;
	return TD_FAIL;
}

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, HOST_CHECK_NAME ": %s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_err.c_str()); return 1; } } while (0)
