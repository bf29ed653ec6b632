#!/usr/bin/env python3
"""Time the two k-means kernels (vittf_kmeans_assign, vittf_kmeans_sums) beside the projection and Gram kernels and beside
stock PyTorch-ROCm doing the same work (one GPU).

    python tools/kmeans_step.py [--sizes 64 128] [--features 384] [--clusters 8 64] [--steps 10] [--warmup 3]
                                [--out profiles/kmeans_kernels.json]

For every size n a synthetic n^3 x F fp16 feature volume (normal values with a per-channel offset, tools/pca_step.py's) and
for every C centroids that are C voxel columns of it: the raw vittf_kmeans_assign and vittf_kmeans_sums calls (both launches
of the latter) on preallocated buffers; in the same process the yardsticks vittf_feature_project at K = 64 (the same loads
as the assignment, a larger store) and vittf_feature_gram (the same reduction as the sums, 78 tiles instead of 12 or 24); and
the stock expressions ``(cent @ feat.float() - h[:, None]).argmax(0)`` and ``torch.zeros(C, F).index_add_(0, labels,
feat.float().T)``, the latter also with the fp32 copy prepared outside the timing.  Every figure is the median over --steps
of one HIP event pair around one call, after --warmup calls; nothing else runs on the GPU meanwhile.  Also recorded: one
whole vt.kmeans.fit (wall clock, iterations) per volume and C.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.pca_step import timed          # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--features', type=int, default=384)
    ap.add_argument('--clusters', type=int, nargs='+', default=[8, 64])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmeans_kernels.json'))
    args = ap.parse_args()
    import torch
    import vit_tf_amd as vt
    from vit_tf_amd import _lib
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lib = _lib.require_device()
    f = args.features
    line = {'tool': 'kmeans_step', 'device': torch.cuda.get_device_name(0), 'features': f, 'steps': args.steps, 'warmup': args.warmup,
            'gram_run': _lib.GRAM_RUN, 'spans': _lib.KMEANS_SPANS, 'volumes': {}}
    g = torch.Generator(device=dev).manual_seed(0)
    t = lambda fn: timed(fn, args.steps, args.warmup)          # noqa: E731
    for n in args.sizes:
        nvox = n ** 3
        feat = torch.empty((f, n, n, n), dtype=torch.float16, device=dev)
        for c0 in range(0, f, 32):                            # (filled in slabs: no fp32 copy of the whole volume)
            feat[c0:c0 + 32] = (torch.randn((32, n, n, n), generator=g, device=dev) + torch.randn((32, 1, 1, 1), generator=g, device=dev)).half()
        x = feat.reshape(f, nvox)
        res = {'nvox': nvox, 'volume_mb': round(f * nvox * 2 / 1e6, 1), 'clusters': {}}
        # yardsticks: the K = 64 projection and the Gram on this volume
        comp = torch.nn.functional.normalize(torch.randn((64, f), generator=g, device=dev), dim=1)
        out = torch.empty((64, nvox), dtype=torch.float16, device=dev)
        res['project64_ms'], res['project64_ms_all'] = t(lambda: _lib.check(lib.vittf_feature_project(
            _lib.ptr(x), f, nvox, _lib.ptr(comp), None, 64, _lib.ptr(out), _lib.stream_ptr())))
        res['gram_ms'], res['gram_ms_all'] = t(lambda: vt.feature_gram(feat))
        del out
        xf = x.float()
        for c in args.clusters:
            cent = x[:, torch.randperm(nvox, generator=g, device=dev)[:c]].T.float().contiguous()
            h = vt.kmeans.half_sq(cent).to(dev)
            labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
            best = torch.empty((nvox,), dtype=torch.float32, device=dev)
            r = {}
            r['assign_ms'], r['assign_ms_all'] = t(lambda: _lib.check(lib.vittf_kmeans_assign(
                _lib.ptr(x), f, nvox, _lib.ptr(cent), _lib.ptr(h), c, _lib.ptr(labels), None, _lib.stream_ptr())))
            r['assign_with_best_ms'], _ = t(lambda: _lib.check(lib.vittf_kmeans_assign(
                _lib.ptr(x), f, nvox, _lib.ptr(cent), _lib.ptr(h), c, _lib.ptr(labels), _lib.ptr(best), _lib.stream_ptr())))
            sums = torch.empty((c, f), dtype=torch.float64, device=dev)
            counts = torch.empty((c,), dtype=torch.int64, device=dev)
            ws_bytes = lib.vittf_kmeans_sums_workspace_bytes(f, nvox, c)
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
            r['sums_workspace_mb'] = round(ws_bytes / 1e6, 1)
            r['sums_ms'], r['sums_ms_all'] = t(lambda: _lib.check(lib.vittf_kmeans_sums(
                _lib.ptr(x), f, nvox, _lib.ptr(labels), c, _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())))
            r['assign_gb_per_s'] = round((2 * f + 1) * nvox / r['assign_ms'] / 1e6, 1)
            r['sums_gb_per_s'] = round((2 * f + 1) * nvox / r['sums_ms'] / 1e6, 1)
            # agreement with the stock expressions on this volume (fp32 scores: labels may differ on near-ties)
            stock_labels = (cent @ xf - h[:, None]).argmax(0)
            r['labels_differing_from_stock'] = int((stock_labels != labels.long()).sum())
            ref = torch.zeros((c, f), dtype=torch.float64, device=dev)
            for v in range(0, nvox, 1 << 16):
                ref.index_add_(0, labels[v:v + (1 << 16)].long(), x[:, v:v + (1 << 16)].double().T)
            r['sums_rel_fro'] = float((sums - ref).norm() / ref.norm())
            r['counts_equal'] = bool(torch.equal(counts, torch.bincount(labels.long(), minlength=c)))
            lab64 = labels.long()
            r['stock_assign_ms'], _ = t(lambda: (cent @ x.float() - h[:, None]).argmax(0))
            r['stock_assign_fp32_input_ms'], _ = t(lambda: (cent @ xf - h[:, None]).argmax(0))
            r['stock_sums_ms'], _ = t(lambda: torch.zeros((c, f), device=dev).index_add_(0, lab64, x.float().T))
            r['stock_sums_fp32_input_ms'], _ = t(lambda: torch.zeros((c, f), device=dev).index_add_(0, lab64, xf.T))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, fit = vt.kmeans.fit(feat, c, seed=0)
            torch.cuda.synchronize()
            r['fit'] = {'seconds': round(time.perf_counter() - t0, 3), 'n_iter': fit.n_iter, 'converged': fit.converged}
            res['clusters'][str(c)] = r
            print(f'{n}^3 C={c}: ' + json.dumps({k: v for k, v in r.items() if not k.endswith('_all')}), file=sys.stderr, flush=True)
            del ws, stock_labels, lab64
        line['volumes'][f'{n}^3'] = res
        del feat, x, xf
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
