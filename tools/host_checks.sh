#!/bin/bash
# The thirteen stand-alone programs over the library's plain C++ host units (tools/*_host_check.cpp), built with the host compiler under
# AddressSanitizer and UBSan and run, leak detection on: no GPU, no HIP runtime, no Python.  Every step must succeed; the last line
# is "host_checks: ok".   usage: tools/host_checks.sh   (CXX: the compiler, default g++; OUT: where the programs go)
set -e
cd "$(dirname "$0")/.."
CXX=${CXX:-g++}
OUT=${OUT:-/tmp/td_host_checks}
SAN="-std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
C=tagdust_amd/csrc
G=tests/golden/merge
mkdir -p $OUT &&
$CXX $SAN $C/td_census_host.cpp tools/census_host_check.cpp -o $OUT/census_host_check &&
$CXX $SAN $C/td_census_host.cpp $C/td_molecules_host.cpp $C/td_fastq.cpp tools/molecules_host_check.cpp -o $OUT/molecules_host_check -lpthread &&
$CXX $SAN $C/td_census_host.cpp $C/td_molecules_host.cpp tools/dedup_host_check.cpp -o $OUT/dedup_host_check &&
$CXX $SAN $C/td_census_host.cpp $C/td_molecules_host.cpp tools/collapse_host_check.cpp -o $OUT/collapse_host_check &&
$CXX $SAN $C/td_census_host.cpp $C/td_molecules_host.cpp tools/dedup_collapsed_host_check.cpp -o $OUT/dedup_collapsed_host_check &&
$CXX $SAN $C/td_census_host.cpp $C/td_molecules_host.cpp tools/mate_host_check.cpp -o $OUT/mate_host_check &&
$CXX $SAN $C/td_census_host.cpp $C/td_samples_host.cpp tools/samples_host_check.cpp -o $OUT/samples_host_check &&
$CXX $SAN $C/td_quality_host.cpp tools/quality_host_check.cpp -o $OUT/quality_host_check &&
$CXX $SAN -ffp-contract=off tools/merge_host_check.cpp $C/td_merge.cpp -o $OUT/merge_host_check -lpthread &&
$CXX $SAN $C/td_batch_plan.cpp tools/batch_plan_host_check.cpp -o $OUT/batch_plan_host_check &&
$CXX $SAN tools/workers_host_check.cpp -o $OUT/workers_host_check -lpthread &&
$CXX $SAN $C/td_model.cpp $C/td_model_flat.cpp $C/td_spec_plan.cpp $C/td_spec_bounds.cpp tools/model_host_check.cpp -o $OUT/model_host_check &&
$CXX $SAN $C/td_run_opts.cpp $C/td_run_plan.cpp $C/td_run_report.cpp $C/td_model.cpp $C/td_model_flat.cpp $C/td_fastq.cpp $C/td_census_host.cpp $C/td_samples_host.cpp $C/td_molecules_host.cpp tools/run_host_check.cpp -o $OUT/run_host_check -lpthread &&
$OUT/census_host_check &&
$OUT/molecules_host_check &&
$OUT/dedup_host_check &&
$OUT/collapse_host_check &&
$OUT/dedup_collapsed_host_check &&
$OUT/mate_host_check &&
$OUT/samples_host_check &&
$OUT/quality_host_check &&
$OUT/batch_plan_host_check &&
$OUT/workers_host_check &&
$OUT/model_host_check &&
$OUT/run_host_check &&
$OUT/merge_host_check $G/r1.fq $G/r2.fq $G/merged_default.fq 16 0 &&
$OUT/merge_host_check $G/r1.fq $G/r2.fq $G/merged_Q0.9_minlen20.fq 20 0.9 &&
echo "host_checks: ok"
