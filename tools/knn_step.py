#!/usr/bin/env python3
"""Time the k-NN decision entry (vittf_knn_decide) beside stock PyTorch-ROCm doing the same work and beside the RBF decision
of the same frame (one GPU).

    python tools/knn_step.py [--sizes 64 128] [--features 384] [--bank 1024 4096] [--k 1 20] [--classes 6] [--steps 10]
                             [--warmup 3] [--out profiles/knn_kernels.json]

For every size n a synthetic n^3 x F fp16 feature volume (tools/svm_step.py's), and for every S a bank of S voxel columns of it,
L2-normalised and rounded to fp16, with sorted random classes: the raw vittf_knn_decide call (both launches: bank images,
decision) on preallocated buffers with the voxel norms, softmax weights at T = 0.07, for every k, with and without the
optional outputs; the same expression in stock PyTorch on the same GPU, chunked over the voxels:
``(bank.float() @ feat[:, chunk].float() / norm).topk(k, 0)``, the weights, the per-class sums and the arg-max; and
vittf_svm_rbf_decide with S support vectors of the same volume -- the same pickup, ring and MFMAs with an exponential and a
second contraction where the k-NN has its selection: the yardstick of what the shared frame costs.  k = 1 is a running maximum
without insertion rounds, so ``knn_ms[k] - knn_ms[1]`` is what the sorted list costs.  Also 64^3 x 32 (a ``_pca32`` file).
Every figure is the median over --steps of one HIP event pair around one call, after --warmup calls; nothing else runs on the
GPU meanwhile.  Algorithmic work of the similarities: 2 nvox F S FLOP, reported against the dense fp16 MFMA peak (2500
TFLOP/s).  Prints one JSON line and writes it to --out.
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


def stock_decide(x, norm, bank, cls_onehot, k, inv_t, chunk=1 << 15):
    """The k-NN decision in stock PyTorch, in voxel chunks (the S x nvox similarity matrix would not fit whole)."""
    import torch
    bf = bank.float()
    labels = torch.empty(x.shape[1], dtype=torch.uint8, device=x.device)
    for v in range(0, x.shape[1], chunk):
        sim = (bf @ x[:, v:v + chunk].float()) / norm[None, v:v + chunk]
        top, idx = sim.topk(k, 0)
        w = torch.exp((top - top[:1]) * inv_t) if inv_t else torch.ones_like(top)
        scores = torch.einsum('kvc,kv->cv', cls_onehot[idx], w)
        labels[v:v + chunk] = scores.argmax(0).to(torch.uint8)
    return labels


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--features', type=int, default=384)
    ap.add_argument('--bank', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--k', type=int, nargs='+', default=[1, 20])
    ap.add_argument('--classes', type=int, default=6)
    ap.add_argument('--temperature', type=float, default=0.07)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'knn_kernels.json'))
    args = ap.parse_args()
    import torch
    import vit_tf_amd as vt
    from vit_tf_amd import _lib
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lib = _lib.require_device()
    c = args.classes
    pairs = vt.svm.pair_list(c)
    inv_t = float(torch.tensor(1.0 / args.temperature, dtype=torch.float32))
    line = {'tool': 'knn_step', 'device': torch.cuda.get_device_name(0), 'classes': c, 'temperature': args.temperature,
            'steps': args.steps, 'warmup': args.warmup, 'peak_fp16_tflops': PEAK_FP16_TFLOPS, 'volumes': {}}
    g = torch.Generator(device=dev).manual_seed(0)
    t = lambda fn: timed(fn, args.steps, args.warmup)          # noqa: E731
    for n, f in [(n, args.features) for n in args.sizes] + [(64, 32)]:
        nvox = n ** 3
        feat = torch.empty((f, n, n, n), dtype=torch.float16, device=dev)
        for c0 in range(0, f, 32):                            # (filled in slabs: no fp32 copy of the whole volume)
            feat[c0:c0 + 32] = (torch.randn((32, n, n, n), generator=g, device=dev) + torch.randn((32, 1, 1, 1), generator=g, device=dev)).half()
        x = feat.reshape(f, nvox)
        norm = vt.similarity.voxel_norms(feat).reshape(-1).contiguous()
        res = {'nvox': nvox, 'features': f, 'volume_mb': round(f * nvox * 2 / 1e6, 1), 'bank': {}}
        labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
        scores = torch.empty((c, nvox), dtype=torch.float32, device=dev)
        for s in args.bank:
            cols = x[:, torch.randperm(nvox, generator=g, device=dev)[:s]].T.contiguous()
            bank = torch.nn.functional.normalize(cols.double(), dim=1).half().contiguous()
            cls = torch.sort(torch.randint(0, c, (s,), generator=g, device=dev)).values.to(torch.uint8)
            onehot = torch.nn.functional.one_hot(cls.long(), c).float()
            ws_bytes = lib.vittf_knn_workspace_bytes(f, s)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            r = {'workspace_mb': round(ws_bytes / 1e6, 2), 'k': {}}
            flop = 2.0 * nvox * f * s
            for k in args.k:
                nn_index = torch.empty((k, nvox), dtype=torch.int32, device=dev)
                nn_sim = torch.empty((k, nvox), dtype=torch.float32, device=dev)
                run = lambda sc, ni, ns: _lib.check(lib.vittf_knn_decide(                                       # noqa: E731
                    _lib.ptr(x), f, nvox, _lib.ptr(bank), _lib.ptr(cls), s, c, k, inv_t, _lib.ptr(norm), _lib.ptr(labels), _lib.ptr(sc),
                    _lib.ptr(ni), _lib.ptr(ns), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
                rk = {}
                rk['knn_ms'], rk['knn_ms_all'] = t(lambda: run(None, None, None))
                rk['knn_with_outputs_ms'], _ = t(lambda: run(scores, nn_index, nn_sim))
                rk['knn_tflops'] = round(flop / (rk['knn_ms'] * 1e-3) / 1e12, 1)
                rk['knn_frac_of_fp16_peak'] = round(rk['knn_tflops'] / PEAK_FP16_TFLOPS, 4)
                run(None, None, None)
                mine = labels.clone()
                stock = stock_decide(x, norm, bank, onehot, k, inv_t)
                rk['labels_differing_from_stock'] = int((stock != mine).sum())
                rk['stock_ms'], _ = t(lambda: stock_decide(x, norm, bank, onehot, k, inv_t))
                r['k'][str(k)] = rk
                del nn_index, nn_sim, stock
            # the RBF decision with S support vectors of the same volume: the shared frame without a selection
            coef = torch.zeros((len(pairs), s), device=dev)
            cl = cls.long()
            for p, (i, j) in enumerate(pairs):
                coef[p] = torch.where(cl == i, 1.0, 0.0) * torch.rand(s, generator=g, device=dev) - torch.where(cl == j, 1.0, 0.0) * torch.rand(s, generator=g, device=dev)
            b = torch.randn(len(pairs), generator=g, device=dev) * 0.1
            gamma = 1.0 / (f * float(x[:, :1 << 16].float().var()))
            rbf_bytes = lib.vittf_svm_rbf_workspace_bytes(f, s, c)
            rbf_ws = torch.empty(rbf_bytes, dtype=torch.uint8, device=dev)
            r['rbf_ms'], _ = t(lambda: _lib.check(lib.vittf_svm_rbf_decide(
                _lib.ptr(x), f, nvox, _lib.ptr(cols), _lib.ptr(coef), _lib.ptr(b), s, c, gamma, None, _lib.ptr(labels), None,
                _lib.ptr(rbf_ws), rbf_bytes, _lib.stream_ptr())))
            res['bank'][str(s)] = r
            print(f'{n}^3 x {f} S={s}: ' + json.dumps({'rbf_ms': r['rbf_ms'], **{f'k{k}': {a: v for a, v in rk.items() if not a.endswith('_all')}
                                                                                 for k, rk in r['k'].items()}}), file=sys.stderr, flush=True)
            del ws, rbf_ws
        line['volumes'][f'{n}^3x{f}'] = res
        del feat, x, scores, labels, norm
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
