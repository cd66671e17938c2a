"""Cost of attention dropout in the SST window-attention kernels: training steps of the configs[4] per-GPU share (the
scene of bench.py --workload sst: 32 grids, windows 8x8x8, drop levels 30/60/100, 2 BasicShiftBlockV2 on the fused
encoder-layer kernels) with the given attention dropout.  Run it under
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/sst_dropout_cost.py --dropout 0.1
and compare the window_attn_block_{fwd,bwd}_kernel / window_attn_{fwd,bwd}_kernel rows with a --dropout 0 run."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dropout', type=float, default=0.1)
    ap.add_argument('--grids', type=int, default=32)
    ap.add_argument('--steps', type=int, default=10)
    args = ap.parse_args()
    from objectcentricocccompletion_amd.linear import Linear
    from objectcentricocccompletion_amd.occ_encoder import synthetic_object_grids
    from objectcentricocccompletion_amd.sst import sst_modules as sm
    from objectcentricocccompletion_amd.voxel import dynamic_scatter, voxelization
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    G, shape, rng = args.grids, (64, 80, 80), [-4, -4, -3.2, 4, 4, 3.2]
    drop = {0: dict(max_tokens=30, drop_range=(0, 30)), 1: dict(max_tokens=60, drop_range=(30, 60)),
            2: dict(max_tokens=100, drop_range=(60, 100000))}
    inp = sm.SSTInputLayerV2(drop, (8, 8, 8), (80, 80, 64), shuffle_voxels=False, debug=False, mute=True).to(dev)
    model = sm.SSTv2(d_model=[128] * 2, nhead=[8] * 2, num_blocks=2, dim_feedforward=[256] * 2, dropout=args.dropout,
                     activation='gelu', num_attached_conv=0, to_bev=False, debug=False,
                     layer_cfg=dict(compute_dtype=torch.bfloat16)).to(dev).train()
    embed = Linear(16, 128).to(dev)
    xyz, feats, bidx = synthetic_object_grids(G, 8200, seed=0, device=dev)
    xyz[:, 2] *= 0.8
    zyx = voxelization(xyz, [0.1, 0.1, 0.1], rng, -1, -1)
    coors = torch.cat([bidx.view(-1, 1).to(torch.int32), zyx], 1)
    vfeats, vcoors = dynamic_scatter(feats, coors, 'mean', grid_shape=[G] + list(shape))
    d_out = None
    for _ in range(args.steps):
        model.zero_grad(set_to_none=True)
        info = inp(embed(vfeats), vcoors.long(), batch_size=G)
        out = model(info)[0]['voxel_feats']
        if d_out is None:
            d_out = (torch.randn(out.shape, device=dev) / out.shape[0]).to(out.dtype)
        out.backward(d_out)
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    print(f'{args.steps} training steps, attention dropout {args.dropout}, {vfeats.shape[0]} voxels')


if __name__ == '__main__':
    main()
