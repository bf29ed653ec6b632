#!/usr/bin/env python3
"""Time one feature-volume step of DINOv2 ViT-S/14 against DINO ViT-S/8 on the benchmark's workload (one GPU).

    python tools/dinov2_step.py [--workload 512] [--steps 3] [--warmup 1] [--archs A B ...] [--repeats R]

Both models see the same volume at feature_output_size 64: 896 x 896 images at patch 14 and 512 x 512 at patch 8, both
64 x 64 tokens (N = 4097), 1536 slices per step for the 512^3 volume.  Seeded synthetic weights (the timing does not depend
on them).  Timed steps run without the profiler; one more step per model is run with vittf_profiler_* on, for the per-class
milliseconds.  Prints ONE JSON line: slices/s of each model, their ratio, per-class ms per step, and the patch embedding's
ms per 256 slices.

--archs picks the models (default: vits14 vits8), e.g. ``--archs vits14 vits14_reg`` for the cost of the four register
tokens (N = 4101 against 4097); the ratio on the line is first over second.  --repeats R runs the list R times in that
order, so the models alternate: the line then carries every run's slices/s under ``runs`` (the spread of repeated runs of
one model is the yardstick for a difference between two), and each model's entry is its last run.
``--archs dinov3_vits16 vits14_reg``: both run N = 4101 at D = 384, so the difference is DINOv3's rotation of q and k (inside
the ``gemm_qkv`` class) plus the patch-16 against the patch-14 embedding.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(arch, vol, fos, steps, warmup):
    import torch
    import vit_tf_amd as vt
    model = vt.HipViT(vt.synthetic_state_dict(arch, 0), arch, 'fp16')
    dvol = vt.DeviceVolume(vol, model.device)
    im_sz, feat_out = vt.sizing(dvol.shape, fos, model.patch_size)
    slices = sum(dvol.shape)                   # every slice of every axis runs through the ViT (pooled windows cover them)
    for _ in range(warmup):
        vt.feature_volume(None, model, fos, 'all', dvol=dvol)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = vt.feature_volume(None, model, fos, 'all', dvol=dvol)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / steps
    vt._lib.profiler_enable(True)
    try:
        vt.feature_volume(None, model, fos, 'all', dvol=dvol)
        torch.cuda.synchronize()
        prof = vt._lib.profiler_collect()
    finally:
        vt._lib.profiler_enable(False)
    ms = {k: round(v[0], 3) for k, v in prof.items() if v[1]}
    res = {'arch': arch, 'image': list(im_sz),
           'tokens': (im_sz[0] // model.patch_size) * (im_sz[1] // model.patch_size) + 1 + model.num_register_tokens,
           'slices_per_step': slices, 'ms_per_step': round(sec * 1e3, 2), 'slices_per_s': round(slices / sec, 1),
           'class_ms_per_step': ms, 'patch_embed_kernel': vt._lib.kernel_name('patch_embed'),
           'patch_embed_ms_per_256_slices': round(prof['patch_embed'][0] * 256 / slices, 3),
           'out_shape': list(out.shape)}
    del model, dvol, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--workload', default='512', choices=['64', '256', '512'])
    ap.add_argument('--fos', type=int, default=64)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--archs', nargs='+', default=['vits14', 'vits8'], help='models to time, in order (default: vits14 vits8)')
    ap.add_argument('--repeats', type=int, default=1, help='run the list this many times, alternating the models')
    args = ap.parse_args()
    if len(set(args.archs)) != len(args.archs) or len(args.archs) < 2:
        ap.error('--archs takes two or more different models')
    import torch
    import bench
    import vit_tf_amd as vt
    torch.cuda.set_device(0)
    vol, _, desc = bench.make_workload(args.workload, vt)
    res, runs = {}, {name: [] for name in args.archs}
    for _ in range(max(1, args.repeats)):
        for name in args.archs:
            res[name] = run(name, vol, args.fos, args.steps, args.warmup)
            runs[name].append(res[name]['slices_per_s'])
    a, b = args.archs[0], args.archs[1]
    line = {'tool': 'dinov2_step', 'workload': args.workload, 'fos': args.fos, 'steps': args.steps,
            'device': torch.cuda.get_device_name(0), **{name: res[name] for name in args.archs},
            f'{a}_over_{b}_slices_per_s': round(res[a]['slices_per_s'] / res[b]['slices_per_s'], 4)}
    if args.repeats > 1:
        line['runs'] = runs
    print(json.dumps(line))


if __name__ == '__main__':
    main()
