#!/usr/bin/env bash
# Same CLI as the reference's tools/dist_test.sh:  dist_test.sh <config> <checkpoint> <gpus> [test.py args]
# test.py args pass through, e.g.  --eval waymo_native --matcher hungarian
# One process per MI355X; each rank evaluates a contiguous shard of the tracklets, rank 0 gathers and evaluates.
CONFIG=$1
CHECKPOINT=$2
GPUS=$3
PORT=${PORT:-29501}
export HSA_ENABLE_IPC_MODE_LEGACY=0
PYTHONPATH="$(dirname $0)/..":$PYTHONPATH \
python -m torch.distributed.run --nnodes=1 --nproc-per-node=$GPUS --master-addr 127.0.0.1 --master-port $PORT \
    $(dirname "$0")/test.py $CONFIG $CHECKPOINT --launcher pytorch ${@:4}
