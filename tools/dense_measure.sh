set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
bash tools/mode_pmc.sh dense "k_graph_wide<false" || exit 1
python3 tools/mode_pmc_summary.py dense gpurun_out/pmc_dense "k_graph_wide<false" profiles/r04f_ > gpurun_out/dense_summary.log 2>&1 || { tail -5 gpurun_out/dense_summary.log; exit 1; }
cp gpurun_out/pmc_dense/trace/*kernel_stats.csv profiles/r04f_dense_kernel_stats.csv
LOG=${OUT:-.}/dense_bench.log  # the bench line with its CPU baseline (--full); OUT = the folder for the log
timeout -k 10 600 python3 bench.py --full --mode dense > $LOG 2>&1 || { tail -5 $LOG; exit 1; }
tail -1 $LOG | cut -c1-400
