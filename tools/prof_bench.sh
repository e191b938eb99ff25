#!/bin/bash
# rocprofv3 kernel trace of a short bench run; summaries are copied to profiles/ by hand afterwards
cd /tmp && export TMPDIR=/tmp
cd "$GRAFT_REPO_ROOT"
out=${PROF_OUT:-prof_out}/prof
rm -rf $out && mkdir -p $out
rocprofv3 --kernel-trace --stats --output-format csv -d $out -- python3 bench.py --steps "${1:-500}" --warmup 20 --profile-steps 0 --no-cpu-baseline --graph "${2:-0}" --full > $out/bench.json 2> $out/bench.err
echo "exit=$?"
find $out -name "*kernel_stats.csv" | head -1 | xargs -r head -20
cat $out/bench.json
