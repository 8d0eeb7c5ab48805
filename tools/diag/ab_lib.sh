# in-box A/B of builds of the library: VARIANTS="old new" (files lib/<name>.so), bench.py --full --no-extra <args>, alternating
L=multi-modal-multi-label-facial-action-unit-detection-with-transformer_amd/lib
V=${VARIANTS:-old new}
O=${AB_OUT:-${TMPDIR:-/tmp}/avf_ab_lib}; mkdir -p $O  # the bench lines (the summary goes to stdout)
for r in 1 2; do
  for v in $V; do
    cp $L/$v.so $L/libavformer_hip.so
    timeout -k 10 300 python bench.py --full --no-extra --no-cpu-baseline "$@" > $O/ab_$v$r.json 2>/dev/null || exit 1
    python - <<PY
import json
d=json.loads(open("$O/ab_$v$r.json").read().strip().splitlines()[-1])
k=d["kernel_classes"]
print("$v$r", d["value"], d["ms_per_step"], {c:k[c]["ms_per_step"] for c in k})
PY
  done
done
cp $L/new.so $L/libavformer_hip.so
