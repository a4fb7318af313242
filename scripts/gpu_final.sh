# Final check of a round's library: GPU suite, smoke, full-frame JIT/generic comparison, default bench line.
# usage: bash scripts/gpu_final.sh [tag]; logs go to $NRT_OUT (default out/)
set -o pipefail
out=${NRT_OUT:-out}
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
tag=${1:-final}
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$out/${tag}_pytest.log" 2>&1 || { tail -30 "$out/${tag}_pytest.log"; exit 1; }
tail -1 "$out/${tag}_pytest.log"
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke()" > "$out/${tag}_smoke.log" 2>&1 || { tail -5 "$out/${tag}_smoke.log"; exit 1; }
tail -1 "$out/${tag}_smoke.log"
timeout -k 10 200 python scripts/jit_compare.py > "$out/${tag}_jit_compare.log" 2>&1; rc=$?; tail -3 "$out/${tag}_jit_compare.log"; [ $rc -le 1 ] || exit 1
timeout -k 10 300 python bench.py --full > "$out/${tag}_bench_default.json" 2> "$out/${tag}_bench_default.err" || exit 1
tail -c 400 "$out/${tag}_bench_default.json"
