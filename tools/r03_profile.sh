set -x
O=${1:?usage: tools/r03_profile.sh OUTDIR}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
(timeout 900 python -m pytest tests -m gpu -q --tb=line 2>&1 | grep -v "^$" | tail -12) > $O/t_all.log
timeout 400 rocprofv3 --kernel-trace --stats -d $O/prof -o large -- python bench.py --steps 10 --warmup 2 --no-cpu-baseline --no-extras > $O/prof_bench.log 2>&1
python tools/rocprof_summary.py $(ls $O/prof/*results.db $O/prof/*/*results.db 2>/dev/null | head -1) > $O/kernel_stats.csv 2>$O/summary.err
timeout 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $O/pmc_fetch -o p -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_fetch.log 2>&1
timeout 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $O/pmc_write -o p -- python bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_write.log 2>&1
python tools/pmc_traffic.py $O/pmc_fetch $O/pmc_write > $O/pmc_traffic.json 2>$O/pmc.err
UNI_PROF_DUMP=$O/pd_b16.txt timeout 200 python bench.py --full --no-cpu-baseline --no-extras > $O/bench_b16.json 2>/dev/null
UNI_PROF_DUMP=$O/pd_b1.txt timeout 200 python bench.py --full --batch 1 --steps 40 --no-cpu-baseline --no-extras > $O/bench_b1.json 2>/dev/null
python tools/prof_shapes.py $O/pd_b16.txt 3 > $O/shapes_b16.txt
python tools/prof_shapes.py $O/pd_b1.txt 3 > $O/shapes_b1.txt
rm -rf $O/prof $O/pmc_fetch $O/pmc_write $O/pd_b16.txt $O/pd_b1.txt
cat $O/t_all.log; head -12 $O/kernel_stats.csv; cat $O/pmc_traffic.json | head -30
