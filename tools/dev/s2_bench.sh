cd $GRAFT_REPO_ROOT
OUT=${1:?usage: s2_bench.sh OUTPUT_DIR}
timeout -k 10 1100 python3 bench.py --full > $OUT/s2_bench.json 2> $OUT/s2_bench.err; echo "rc=$?"
tail -c 1500 $OUT/s2_bench.json
