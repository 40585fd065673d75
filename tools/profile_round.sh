set -e
R=$PWD; O=$R/profile_out/r2p; mkdir -p $O && cd /tmp && export TMPDIR=/tmp
export OTTI_ARMED=0   # armed launches wait for the host inside the kernel: switched off so that every kernel duration in the trace is the kernel alone
rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt -- python3 $R/bench.py --full --steps 10 --warmup 2 --in-flight -1 --no-cpu-baseline --no-e2e --no-snark > $O/bench_under_rocprof.json 2> $O/bench_under_rocprof.err
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --full --steps 1 --warmup 1 --in-flight -1 --no-cpu-baseline --no-e2e --no-snark > $O/pmc_fetch.json 2> $O/pmc_fetch.err
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -- python3 $R/bench.py --full --steps 1 --warmup 1 --in-flight -1 --no-cpu-baseline --no-e2e --no-snark > $O/pmc_write.json 2> $O/pmc_write.err
cd $R
find $O -name "*.csv" | head -20
