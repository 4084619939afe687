cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${1:?usage: tools/pmc_mem.sh <output directory>}
mkdir -p "$OUT"
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_f" -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > /dev/null 2> "$OUT/pmc_f.err"
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_w" -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > /dev/null 2> "$OUT/pmc_w.err"
rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum TCC_REQ_sum TCC_EA0_RDREQ_sum --output-format csv -d "$OUT/pmc_t" -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > /dev/null 2> "$OUT/pmc_t.err"
rocprofv3 --pmc GRBM_GUI_ACTIVE GRBM_COUNT --output-format csv -d "$OUT/pmc_g" -- python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > /dev/null 2> "$OUT/pmc_g.err"
