# End-of-round collection: counters, torch launch sites, the full benchmark record, the one-rank RCCL dry runs, host vs GPU.
#   bash benchmarks/final_collect.sh [output directory, default collect_out]   (step_sq_counters.sh writes where it always does)
set -u
cd "$(dirname "$0")/.."
OUT=${1:-collect_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
bash benchmarks/step_sq_counters.sh r06 c1
bash benchmarks/step_sq_counters.sh r06 c2
python3 benchmarks/torch_kernel_sites.py c1 > $OUT/r06_torch_kernel_sites_c1.txt 2>/dev/null
python3 benchmarks/torch_op_sites.py c1 > $OUT/r06_torch_op_sites_c1.txt 2>/dev/null
python3 benchmarks/torch_kernel_sites.py c2 > $OUT/r06_torch_kernel_sites_c2.txt 2>/dev/null
python3 bench.py --full > $OUT/r06_bench_default.json 2> $OUT/r06_bench_default.err
DWC_FORCE_DP=1 python3 bench.py --gpus 1 --config c3 --also "" --steps 6 --warmup 2 --no-cpu-baseline > $OUT/r06_dp_dry_c3_forced_one_rank_rccl.json 2> $OUT/dp3.err
DWC_FORCE_DP=1 python3 bench.py --gpus 1 --config c4 --scaling strong --also "" --steps 6 --warmup 2 --no-cpu-baseline > $OUT/r06_dp_dry_c4_strong_forced_one_rank_rccl.json 2> $OUT/dp4.err
for B in 16 8 2; do python3 benchmarks/host_vs_gpu.py $B 128; done > $OUT/r06_host_vs_gpu_final.txt 2>&1
OUT=$OUT python3 - <<'PY'
import json, os
d=json.load(open(os.path.join(os.environ["OUT"], "r06_bench_default.json")))
print("c1", d["value"], d["ms_per_step"], d["roofline"]["frac"], d["cpu_baseline"]["value"])
c2=d["also"]["c2"]
print("c2", c2["value"], c2["ms_per_step"], c2["decode_conv_stack"]["forward"]["frac_of_mfma_peak"], c2["decode_conv_stack"]["backward"]["frac_of_mfma_peak"])
for f in ("r06_dp_dry_c3_forced_one_rank_rccl.json","r06_dp_dry_c4_strong_forced_one_rank_rccl.json"):
    e=json.load(open(os.path.join(os.environ["OUT"], f))); print(f, e["value"], e["ms_per_step"])
PY
head -1 $OUT/r06_torch_kernel_sites_c1.txt $OUT/r06_torch_kernel_sites_c2.txt
cat $OUT/r06_host_vs_gpu_final.txt | tail -8
