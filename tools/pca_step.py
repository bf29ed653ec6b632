#!/usr/bin/env python3
"""Time the two PCA kernels (vittf_feature_gram, vittf_feature_project) beside stock PyTorch-ROCm doing the same work (one GPU).

    python tools/pca_step.py [--sizes 64 128] [--features 384] [--components 3 32 64] [--steps 10] [--warmup 3]
                             [--out profiles/pca_kernels.json]

For every size n a synthetic n^3 x F fp16 feature volume (normal values with a per-channel offset): the Gram call (both of
its launches), the projection at every K, and in the same process the stock expressions ``feat.float() @ feat.float().T`` and
``comp @ feat.float()`` (the widening included: stock PyTorch has no fp16-in / fp32-accumulate / fp64-out Gram).  Every figure is
the median over --steps of one HIP event pair around one call, after --warmup calls; nothing else runs on the GPU meanwhile.
Also recorded: the relative Frobenius error of the GPU Gram against an fp64 Gram (torch, on the GPU) on a REAL feature volume
-- ViT-S/8 on seeded synthetic weights over the benchmark's 64^3 torus, feature_output_size 64 -- and on the synthetic ones.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    """Median milliseconds of fn() over `steps` event pairs, after `warmup` calls."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4), [round(m, 4) for m in ms]


def gram_error(feat):
    """Relative Frobenius error of vittf_feature_gram against torch's fp64 Gram of the same fp16 values."""
    import vit_tf_amd as vt
    x = feat.reshape(feat.shape[0], -1)
    gram, sums = vt.feature_gram(feat)
    ref = torch_gram64(x)
    return {'gram_rel_fro': float((gram - ref).norm() / ref.norm()),
            'sums_rel': float((sums - x.double().sum(1)).norm() / x.double().sum(1).norm())}


def torch_gram64(x, chunk=1 << 16):
    import torch
    ref = torch.zeros((x.shape[0], x.shape[0]), dtype=torch.float64, device=x.device)
    for v in range(0, x.shape[1], chunk):                    # (chunks: an fp64 copy of a 128^3 volume would be 6.4 GB)
        xd = x[:, v:v + chunk].double()
        ref += xd @ xd.T
    return ref


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--features', type=int, default=384)
    ap.add_argument('--components', type=int, nargs='+', default=[3, 32, 64])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pca_kernels.json'))
    args = ap.parse_args()
    import torch
    import bench
    import vit_tf_amd as vt
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    f = args.features
    line = {'tool': 'pca_step', 'device': torch.cuda.get_device_name(0), 'features': f, 'steps': args.steps, 'warmup': args.warmup,
            'gram_run': vt._lib.GRAM_RUN, 'volumes': {}}
    g = torch.Generator(device=dev).manual_seed(0)
    for n in args.sizes:
        nvox = n ** 3
        feat = torch.empty((f, n, n, n), dtype=torch.float16, device=dev)
        for c in range(0, f, 32):                             # (filled in slabs: no fp32 copy of the whole volume)
            feat[c:c + 32] = (torch.randn((32, n, n, n), generator=g, device=dev) + torch.randn((32, 1, 1, 1), generator=g, device=dev)).half()
        x = feat.reshape(f, nvox)
        res = {'nvox': nvox, 'volume_mb': round(f * nvox * 2 / 1e6, 1),
               'gram_workspace_mb': round(vt._lib.load().vittf_feature_gram_workspace_bytes(f, nvox) / 1e6, 1)}
        res['gram_ms'], res['gram_ms_all'] = timed(lambda: vt.feature_gram(feat), args.steps, args.warmup)
        res['stock_gram_ms'], res['stock_gram_ms_all'] = timed(lambda: x.float() @ x.float().T, args.steps, args.warmup)
        xf = x.float()
        res['stock_gram_fp32_input_ms'], _ = timed(lambda: xf @ xf.T, args.steps, args.warmup)      # the widening taken out
        res['gram_gb_per_s'] = round(f * nvox * 2 / res['gram_ms'] / 1e6, 1)
        res['gram_triangle_tflops'] = round((f // 32) * (f // 32 + 1) / 2 * 2048 * nvox / res['gram_ms'] / 1e9, 1)
        res.update(gram_error(feat))
        basis = vt.basis_from_gram(*vt.feature_gram(feat), nvox, max(args.components))
        res['project'] = {}
        for k in args.components:
            b = vt.Basis(basis.components[:k].contiguous(), basis.mean, basis.explained_variance[:k], basis.total_variance,
                         basis.center, basis.offset[:k].contiguous())
            comp, off = b.components.to(dev), b.offset.to(dev)
            ours, ours_all = timed(lambda: vt.project(feat, b), args.steps, args.warmup)
            stock, _ = timed(lambda: (comp @ x.float() - off[:, None]).half(), args.steps, args.warmup)
            stock32, _ = timed(lambda: (comp @ xf - off[:, None]).half(), args.steps, args.warmup)
            res['project'][str(k)] = {'ms': ours, 'ms_all': ours_all, 'stock_ms': stock, 'stock_fp32_input_ms': stock32,
                                      'gb_per_s': round((f + k) * nvox * 2 / ours / 1e6, 1)}
        line['volumes'][f'{n}^3'] = res
        del feat, x, xf
        torch.cuda.empty_cache()
    # a real feature volume: ViT-S/8 on seeded synthetic weights over the benchmark's 64^3 volume
    vol, _, desc = bench.make_workload('64', vt)
    model = vt.HipViT(vt.synthetic_state_dict('vits8', 0), 'vits8', 'fp16')
    real = vt.feature_volume(vol, model, 64, 'all')
    line['real_volume'] = {'source': f'vits8, synthetic weights seed 0, workload 64 ({desc}), feature_output_size 64',
                           'shape': list(real.shape), **gram_error(real)}
    reduced, basis = vt.reduce_features(real, 32)
    line['real_volume']['variance_kept_by_32'] = float(basis.explained_variance.sum() / basis.total_variance)
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
