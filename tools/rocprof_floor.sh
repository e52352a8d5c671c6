#!/bin/bash
# GPU box: what rocprofv3 --kernel-trace itself costs per dispatch.  The do-nothing kernel (qr_touch: the step's bytes, no
# arithmetic), the product kernel at 65 536 envs (below the tool's floor) and at 131 072 envs (above it), each through bench.py
# under the tool; per-dispatch durations / start-to-start periods from the trace.  The empty-kernel floor itself is measured by
# vmem_width_microbench.hip.  (The recorded tables up to profiles/r05/rocprof_dispatch_floor.txt time q_floor, a build of the step
# kernel that returned at once, in place of qr_touch; that build is retired.)
#   tools/rocprof_floor.sh > gpurun_out/r02/rocprof_dispatch_floor.txt
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd /tmp && export TMPDIR=/tmp
run() {  # tag bench-args...
  tag=$1; shift
  echo "== $tag: bench.py $*"
  un=$(python3 "$ROOT/bench.py" --cpu-seconds 0 --extras 0 "$@" 2>/dev/null | grep -o '"ms_per_step": [0-9.e-]*')
  echo "   un-profiled            $un"
  rm -rf /tmp/floor_$tag
  pr=$(rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/floor_$tag -- python3 "$ROOT/bench.py" --cpu-seconds 0 --extras 0 "$@" 2>/dev/null | grep -o '"ms_per_step": [0-9.e-]*')
  echo "   under rocprofv3        $pr"
  python3 "$ROOT/tools/trace_periods.py" /tmp/floor_$tag | sed 's/^/   /'
  rm -rf /tmp/floor_$tag
}
run touch --workload touch --steps 500
run quad65536 --steps 500
run quad131072 --steps 500 --envs 131072
