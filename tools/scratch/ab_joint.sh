O=${1:?usage: tools/scratch/ab_joint.sh OUTDIR}; mkdir -p $O
L=$PWD/ts-asr_amd/lib
for i in 1 2; do
  for v in base kb2o2 kb2o1; do
    if [ $v = base ]; then unset TSASR_HIP_LIB; else export TSASR_HIP_LIB=$L/libtsasr_hip_$v.so; fi
    python bench.py --full --no-cpu-baseline > $O/h_${v}_$i.json 2> $O/h_${v}_$i.err || exit 1
    python bench.py --config longform --steps 20 --warmup 5 --full --no-cpu-baseline > $O/l_${v}_$i.json 2> $O/l_${v}_$i.err || exit 1
  done
done
O=$O python - <<'PY'
import json, glob, os
for f in sorted(glob.glob(os.path.join(os.environ['O'], '*.json'))):
    d = json.loads(open(f).read().strip().splitlines()[-1])
    print(f.split('/')[-1], d['ms_per_step'], d.get('rnnt_joint_loss_ms'))
PY
