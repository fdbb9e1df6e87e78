#!/usr/bin/env bash
# One process per MI355X over RCCL/xGMI: tools/dist_test.sh CONFIG CHECKPOINT NGPUS [test.py options]
# (the reference's launcher interface: each rank predicts its shard, rank 0 evaluates the gathered detections on its GPU)
set -euo pipefail
if [ "$#" -lt 3 ]; then
    echo "usage: $0 CONFIG CHECKPOINT NGPUS [--cfg-options k=v ...] [--batch-size N] [--out FILE]" >&2
    exit 2
fi
cfg=$1
ckpt=$2
ngpus=$3
shift 3
here=$(cd "$(dirname "$0")" && pwd)
export HSA_ENABLE_IPC_MODE_LEGACY=${HSA_ENABLE_IPC_MODE_LEGACY:-0}    # dmabuf IPC: RCCL needs it on this driver
exec python -m torch.distributed.run \
    --nnodes="${NNODES:-1}" --node-rank="${NODE_RANK:-0}" \
    --master-addr="${MASTER_ADDR:-127.0.0.1}" --master-port="${PORT:-29500}" \
    --nproc-per-node="$ngpus" \
    "$here/test.py" "$cfg" "$ckpt" --launcher pytorch "$@"
