# in-situ timeline of a BASELINE config under two builds of the library, alternating:  bash tools/libab.sh <tag> <config> <libA> <libB>
# any other timed program under the two builds, alternating the same way (two rounds, A B A B; DCCN_LIB_ALLOW_MISSING: the older
# build may lack entry points):  bash tools/libab.sh <tag> --cmd "<command printing JSON lines>" <libA> <libB>
#   e.g.  bash tools/libab.sh clsrx --cmd "python tools/clsrxbench.py --variants one" abl/libdccn_parent.so dl_ofdm_amd/lib/libdccn.so
mkdir -p gpurun_out/$1
if [ "$2" = "--cmd" ]; then
  set -o pipefail           # a run that fails or times out ends the comparison: nothing more is started on the GPU behind it
  for r in 1 2; do
  for lib in $4 $5; do
    DCCN_LIB_PATH=$lib DCCN_LIB_ALLOW_MISSING=1 timeout -k 10 300 $3 2>/dev/null | sed "s|^|$lib round $r |" || exit 1          # (to stdout: the caller keeps it)
  done
  done
  exit 0
fi
for r in 1 2; do
for lib in $3 $4; do
  DCCN_LIB_PATH=$lib timeout 200 python tools/steptl.py --config $2 2>/dev/null | python -c "
import json,sys
for ln in sys.stdin:
    r=json.loads(ln); print('$lib', 'period_us', r.get('period_us'), [(l.get('name'), l['us'], l.get('gap_before_us')) for l in r['launches']])" | tee -a gpurun_out/$1/libab_$2.txt
done
done
