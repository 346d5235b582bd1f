#!/bin/bash
# Development tool (GPU box, one card): the N > 1 control flow of bench.py rehearsed with two gloo ranks sharing the card, and the
# in-library RCCL legs at world size 1 (SMI_BENCH_FORCE_DIST).
set -e
export TMPDIR=/tmp
J2=$(mktemp)
J1=$(mktemp)
SMI_BENCH_BACKEND=gloo SMI_BENCH_DEVICE=0 timeout -k 10 500 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 20 --warmup 5 > $J2 2> $J2.err || { tail -30 $J2.err; exit 1; }
python3 -c "
import json,sys
r=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k:r[k] for k in ('value','n_gpus','ms_per_step','scaling')}); print({k:(v if not isinstance(v,dict) else {a:b for a,b in list(v.items())[:8]}) for k,v in r.items() if 'mgpu' in k or 'self' in k or 'check' in k})
" $J2
SMI_BENCH_FORCE_DIST=1 timeout -k 10 400 python3 -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29518 bench.py --full --gpus 1 --steps 20 --warmup 5 > $J1 2> $J1.err || { tail -30 $J1.err; exit 1; }
python3 -c "
import json,sys
r=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print({k:(v if not isinstance(v,dict) else {a:b for a,b in list(v.items())[:10]}) for k,v in r.items() if 'mgpu' in k or 'self' in k or 'check' in k})
" $J1
