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

--facet {key,query,value,token} / --layer N (infer.py's flags; default key, -1): with a non-default value every model of the
list is run twice per repeat, at the default and at the chosen facet / layer, as ``<arch>`` and ``<arch>@<facet>[_L<N>]``; the
line then carries ``<arch>@..._over_<arch>_slices_per_s`` for every model, and one model is enough.  ``--archs vits14_reg
dinov3_vits16 --facet token``: the cost of the token facet (one more full block and the final-norm kernel for one small
GEMM less) beside the key facet.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(arch, vol, fos, steps, warmup, facet='key', layer=-1):
    import torch
    import vit_tf_amd as vt
    model = vt.HipViT(vt.synthetic_state_dict(arch, 0), arch, 'fp16', layer=layer)
    part = vt.extract.PARTS[facet[0]]
    dvol = vt.DeviceVolume(vol, model.device)
    im_sz, feat_out = vt.sizing(dvol.shape, fos, model.patch_size)
    slices = sum(dvol.shape)                   # every slice of every axis runs through the ViT (pooled windows cover them)
    for _ in range(warmup):
        vt.feature_volume(None, model, fos, 'all', dvol=dvol, part=part)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = vt.feature_volume(None, model, fos, 'all', dvol=dvol, part=part)
    torch.cuda.synchronize()
    sec = (time.perf_counter() - t0) / steps
    vt._lib.profiler_enable(True)
    try:
        vt.feature_volume(None, model, fos, 'all', dvol=dvol, part=part)
        torch.cuda.synchronize()
        prof = vt._lib.profiler_collect()
    finally:
        vt._lib.profiler_enable(False)
    ms = {k: round(v[0], 3) for k, v in prof.items() if v[1]}
    res = {'arch': arch, 'facet': facet, 'layer': model.layer, 'image': list(im_sz),
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
    ap.add_argument('--facet', default='key', choices=['key', 'query', 'value', 'token'], help='facet to time beside the key facet')
    ap.add_argument('--layer', type=int, default=-1, help='hooked block to time beside the last one (0-based, negatives from the end)')
    args = ap.parse_args()
    variant = args.facet != 'key' or args.layer != -1
    if len(set(args.archs)) != len(args.archs) or len(args.archs) < (1 if variant else 2):
        ap.error('--archs takes two or more different models (one or more with --facet / --layer)')
    import torch
    import bench
    import vit_tf_amd as vt
    torch.cuda.set_device(0)
    vol, _, desc = bench.make_workload(args.workload, vt)
    tag = '@' + args.facet + (f'_L{args.layer}' if args.layer != -1 else '')
    # (name on the line, model, facet, layer), in running order: with a variant every model runs at the default first
    plan = []
    for name in args.archs:
        plan.append((name, name, 'key', -1))
        if variant:
            plan.append((name + tag, name, args.facet, args.layer))
    res, runs = {}, {key: [] for key, *_ in plan}
    for _ in range(max(1, args.repeats)):
        for key, name, facet, layer in plan:
            res[key] = run(name, vol, args.fos, args.steps, args.warmup, facet, layer)
            runs[key].append(res[key]['slices_per_s'])
    line = {'tool': 'dinov2_step', 'workload': args.workload, 'fos': args.fos, 'steps': args.steps,
            'device': torch.cuda.get_device_name(0), **{key: res[key] for key, *_ in plan}}
    pairs = [(n + tag, n) for n in args.archs] if variant else [(args.archs[0], args.archs[1])]
    for a, b in pairs:
        line[f'{a}_over_{b}_slices_per_s'] = round(res[a]['slices_per_s'] / res[b]['slices_per_s'], 4)
    if args.repeats > 1:
        line['runs'] = runs
    print(json.dumps(line))


if __name__ == '__main__':
    main()
