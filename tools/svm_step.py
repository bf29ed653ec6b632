#!/usr/bin/env python3
"""Time the two SVM decision entries (vittf_svm_rbf_decide, vittf_svm_linear_decide) beside stock PyTorch-ROCm doing the same
work (one GPU).

    python tools/svm_step.py [--sizes 64 128] [--features 384] [--sv 1024 4096] [--classes 6] [--steps 10] [--warmup 3]
                             [--out profiles/svm_kernels.json]

For every size n a synthetic n^3 x F fp16 feature volume (tools/pca_step.py's), and for every S a model whose support vectors
are S voxel columns of it, with random coefficients in the pairs of each vector's class and gamma = 1 / (F var): the raw
vittf_svm_rbf_decide call (all three launches: coefficient scale, support-vector images, decision) and the
vittf_svm_linear_decide call on preallocated buffers, with and without the decision output; and the same expression in stock
PyTorch on the same GPU, chunked over the voxels: ``coef @ exp(-gamma (|s|^2 + |x|^2 - 2 sv @ feat.float())) + b`` (or ``w @
feat.float() + b``), then the vote.  Also 64^3 x 32 (a ``_pca32`` file).  Every figure is the median over --steps of one HIP
event pair around one call, after --warmup calls; nothing else runs on the GPU meanwhile.  Algorithmic work of the RBF entry:
2 nvox F S FLOP, reported against the dense fp16 MFMA peak (2500 TFLOP/s).  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.pca_step import timed          # noqa: E402

PEAK_FP16_TFLOPS = 2500.0                 # dense MFMA peak, as bench.py has it


def stock_decide(x, sv, coef, b, gamma, pairs, classes, chunk=1 << 15):
    """The RBF decision and the vote in stock PyTorch, in voxel chunks (the S x nvox kernel matrix would not fit whole)."""
    import torch
    s2 = sv.float().square().sum(1)[:, None]
    svf = sv.float()
    labels = torch.empty(x.shape[1], dtype=torch.uint8, device=x.device)
    for v in range(0, x.shape[1], chunk):
        xf = x[:, v:v + chunk].float()
        dec = coef @ torch.exp(-gamma * (s2 + xf.square().sum(0)[None, :] - 2.0 * (svf @ xf))) + b[:, None]
        labels[v:v + chunk] = stock_vote(dec, pairs, classes)
    return labels


def stock_vote(dec, pairs, classes):
    import torch
    votes = torch.zeros((classes, dec.shape[1]), dtype=torch.int32, device=dec.device)
    for p, (i, j) in enumerate(pairs):
        pos = dec[p] > 0
        votes[i] += pos
        votes[j] += ~pos
    return votes.argmax(0).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--features', type=int, default=384)
    ap.add_argument('--sv', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--classes', type=int, default=6)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'svm_kernels.json'))
    args = ap.parse_args()
    import torch
    import vit_tf_amd as vt
    from vit_tf_amd import _lib
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lib = _lib.require_device()
    c = args.classes
    pairs = vt.svm.pair_list(c)
    line = {'tool': 'svm_step', 'device': torch.cuda.get_device_name(0), 'classes': c, 'steps': args.steps, 'warmup': args.warmup,
            'peak_fp16_tflops': PEAK_FP16_TFLOPS, 'volumes': {}}
    g = torch.Generator(device=dev).manual_seed(0)
    t = lambda fn: timed(fn, args.steps, args.warmup)          # noqa: E731
    for n, f in [(n, args.features) for n in args.sizes] + [(64, 32)]:
        nvox = n ** 3
        feat = torch.empty((f, n, n, n), dtype=torch.float16, device=dev)
        for c0 in range(0, f, 32):                            # (filled in slabs: no fp32 copy of the whole volume)
            feat[c0:c0 + 32] = (torch.randn((32, n, n, n), generator=g, device=dev) + torch.randn((32, 1, 1, 1), generator=g, device=dev)).half()
        x = feat.reshape(f, nvox)
        gamma = 1.0 / (f * float(x[:, :1 << 16].float().var()))
        res = {'nvox': nvox, 'features': f, 'volume_mb': round(f * nvox * 2 / 1e6, 1), 'gamma': gamma, 'sv': {}}
        labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
        dec = torch.empty((len(pairs), nvox), dtype=torch.float32, device=dev)
        b = torch.randn(len(pairs), generator=g, device=dev) * 0.1
        for s in args.sv:
            sv = x[:, torch.randperm(nvox, generator=g, device=dev)[:s]].T.contiguous()
            cls = torch.sort(torch.randint(0, c, (s,), generator=g, device=dev)).values
            coef = torch.zeros((len(pairs), s), device=dev)
            for p, (i, j) in enumerate(pairs):
                coef[p] = torch.where(cls == i, 1.0, 0.0) * torch.rand(s, generator=g, device=dev) - torch.where(cls == j, 1.0, 0.0) * torch.rand(s, generator=g, device=dev)
            w = (coef.double() @ sv.double()).float()
            ws_bytes = lib.vittf_svm_rbf_workspace_bytes(f, s, c)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            rbf = lambda d: _lib.check(lib.vittf_svm_rbf_decide(                                              # noqa: E731
                _lib.ptr(x), f, nvox, _lib.ptr(sv), _lib.ptr(coef), _lib.ptr(b), s, c, gamma, None, _lib.ptr(labels), _lib.ptr(d),
                _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
            lin = lambda d: _lib.check(lib.vittf_svm_linear_decide(                                           # noqa: E731
                _lib.ptr(x), f, nvox, _lib.ptr(w), _lib.ptr(b), c, None, _lib.ptr(labels), _lib.ptr(d), _lib.stream_ptr()))
            r = {'workspace_mb': round(ws_bytes / 1e6, 2)}
            r['rbf_ms'], r['rbf_ms_all'] = t(lambda: rbf(None))
            r['rbf_with_decision_ms'], _ = t(lambda: rbf(dec))
            flop = 2.0 * nvox * f * s
            r['rbf_tflops'] = round(flop / (r['rbf_ms'] * 1e-3) / 1e12, 1)
            r['rbf_frac_of_fp16_peak'] = round(r['rbf_tflops'] / PEAK_FP16_TFLOPS, 4)
            rbf(dec)
            mine = labels.clone()
            stock = stock_decide(x, sv, coef, b, gamma, pairs, c)
            r['rbf_labels_differing_from_stock'] = int((stock != mine).sum())
            r['stock_rbf_ms'], _ = t(lambda: stock_decide(x, sv, coef, b, gamma, pairs, c))
            r['linear_ms'], r['linear_ms_all'] = t(lambda: lin(None))
            r['linear_with_decision_ms'], _ = t(lambda: lin(dec))
            r['linear_gb_per_s'] = round((2 * f + 1) * nvox / r['linear_ms'] / 1e6, 1)
            lin(dec)
            mine = labels.clone()
            stock_lin = lambda: torch.cat([stock_vote(w @ x[:, v:v + (1 << 18)].float() + b[:, None], pairs, c)   # noqa: E731
                                           for v in range(0, nvox, 1 << 18)])
            r['linear_labels_differing_from_stock'] = int((stock_lin() != mine).sum())
            r['stock_linear_ms'], _ = t(stock_lin)
            res['sv'][str(s)] = r
            print(f'{n}^3 x {f} S={s}: ' + json.dumps({k: v for k, v in r.items() if not k.endswith('_all')}), file=sys.stderr, flush=True)
            del ws, stock
        line['volumes'][f'{n}^3x{f}'] = res
        del feat, x, dec, labels
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
