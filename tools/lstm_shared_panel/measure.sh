#!/bin/bash
# The shared-panel LSTM form (option "lstm_x3" = 4) against the parent commit's build on one machine, alternating -> profiles/lstm_shared_panel_times.txt
#   PARENT=<directory with the parent commit's libl2s_hip.so and libl2s_diag.so> bash tools/lstm_shared_panel/measure.sh [section ...]
# Sections (default: all): stamps  the block-stamp log of three chains (tools/overlap_stamps.py): chip time per LSTM launch, block lifetime
#                          bench   python bench.py at its defaults, three alternating pairs: parent, this build with "lstm_x3" = 4 (and = 3 once)
#                          bench20 the same at --steps 20 --warmup 5
#                          alone   --full on this build with "lstm_x3" = 4: one chain at a time and the roofline entry's block form
#                          dump    bench.py --steps 8 --warmup 8 --dump-outputs on both builds, compared to the bit
# Every GPU step runs under its own time limit and the steps are chained: the script ends at the first one that fails.
set -o pipefail
cd "$(dirname "$0")/../.."
: "${PARENT:?directory of the parent build}"
OUT=${OUT:-/tmp/lstm_shared_panel}
mkdir -p "$OUT"
SECTIONS=${*:-stamps bench bench20 alone dump}
line() { python -c "import sys,json; d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); print('$1 value %.1f  ms_per_step %.4f' % (d['value'], d['ms_per_step']))"; }
bench_parent() { L2S_LIB=$PARENT/libl2s_hip.so timeout -k 10 240 python bench.py "$@" 2>/dev/null | line "parent build,            "; }
bench_new4() { timeout -k 10 240 python bench.py --opt lstm_x3=4 "$@" 2>/dev/null | line "this build, lstm_x3 = 4,"; }
bench_new3() { timeout -k 10 240 python bench.py --opt lstm_x3=3 "$@" 2>/dev/null | line "this build, lstm_x3 = 3,"; }
for sec in $SECTIONS; do
  case $sec in
    stamps)
      echo "== stamps: three chains, 256 rows, block-stamp log (tools/overlap_stamps.py)" &&
      echo "-- parent build, decode loop" && L2S_LIB=$PARENT/libl2s_diag.so CHAINS=3 MODE=decode timeout -k 10 200 python tools/overlap_stamps.py 8 &&
      echo "-- this build, lstm_x3 = 4, decode loop" && L2S_OPT=lstm_x3=4 CHAINS=3 MODE=decode timeout -k 10 200 python tools/overlap_stamps.py 8 &&
      echo "-- parent build, LSTM chains alone" && L2S_LIB=$PARENT/libl2s_diag.so CHAINS=3 MODE=lstm timeout -k 10 200 python tools/overlap_stamps.py 8 &&
      echo "-- this build, lstm_x3 = 4, LSTM chains alone" && L2S_OPT=lstm_x3=4 CHAINS=3 MODE=lstm timeout -k 10 200 python tools/overlap_stamps.py 8 || exit 1 ;;
    bench)
      echo "== bench: python bench.py at its defaults, in the order run" &&
      bench_parent && bench_new4 && bench_parent && bench_new4 && bench_parent && bench_new4 && bench_new3 || exit 1 ;;
    bench20)
      echo "== bench20: python bench.py --steps 20 --warmup 5, in the order run" &&
      bench_parent --steps 20 --warmup 5 && bench_new4 --steps 20 --warmup 5 && bench_parent --steps 20 --warmup 5 && bench_new4 --steps 20 --warmup 5 &&
      bench_parent --steps 20 --warmup 5 && bench_new4 --steps 20 --warmup 5 || exit 1 ;;
    alone)
      echo "== alone: bench.py --full --skip-cpu-baseline --skip-train-leg, one_chain_at_a_time and the roofline entry" &&
      for o in 3 4; do
        timeout -k 10 400 python bench.py --full --skip-cpu-baseline --skip-train-leg --opt lstm_x3=$o 2>/dev/null | python -c "
import sys, json
d = json.loads([l for l in sys.stdin if l.startswith('{')][-1])
r = d.get('roofline', {})
print('this build, lstm_x3 = $o: value %.1f  one_chain_at_a_time %s  roofline %s avg_us %s' % (d['value'], d.get('one_chain_at_a_time'), r.get('kernel'), r.get('avg_us')))" || exit 1
      done ;;
    dump)
      echo "== dump: bench.py --steps 8 --warmup 8 --dump-outputs, this build (lstm_x3 = 4) against the parent" &&
      L2S_LIB=$PARENT/libl2s_hip.so timeout -k 10 240 python bench.py --steps 8 --warmup 8 --dump-outputs "$OUT/parent" > /dev/null 2>&1 &&
      timeout -k 10 240 python bench.py --steps 8 --warmup 8 --opt lstm_x3=4 --dump-outputs "$OUT/new" > /dev/null 2>&1 &&
      python -c "
import numpy as np
for f in ('lengths.npy', 'mel_post.npy'):
    a, b = np.load('$OUT/parent/' + f), np.load('$OUT/new/' + f)
    print(f, 'shape', a.shape, 'bit-equal', bool(a.shape == b.shape and a.tobytes() == b.tobytes()))" || exit 1 ;;
  esac
done
