#!/usr/bin/env python3
"""Time vittf_forest_decide beside stock PyTorch-ROCm doing the same walk (one GPU), and beside scikit-learn on the host.

    python tools/forest_step.py [--sizes 64 128] [--features 384] [--trees 256 1024] [--depths 0 12] [--classes 6] [--train 3000]
                                [--steps 10] [--warmup 3] [--stock-steps 3] [--cache DIR] [--fit-only] [--out profiles/forest_kernels.json]

For every F (--features, and 32: a ``_pca32`` file) planted 6-class data -- class means 0.3 N(0, 1), unit noise -- gives --train
training rows; vt.forest.fit grows max(--trees) trees on them ('sqrt', bootstrap, seed 0), fully grown (depth 0) and with
max_depth 12, and the smaller forests are the first trees of the larger (a tree does not depend on how many are built).  The
fit is slow host work: with --cache DIR a fitted model is kept there as an .npz and read back by the next run (--fit-only
fills the cache and stops before any GPU work).  For every
size n an n^3 x F fp16 volume of the same distribution, filled on the device.

Per volume and forest: the raw vittf_forest_decide call on uploaded arrays, with and without the votes (median over --steps
of one HIP event pair around one call, after --warmup calls; nothing else runs on the GPU meanwhile); baseline (a), stock
PyTorch on the same GPU: the level-synchronous traversal with tensor gathers, ``node = where(x[feature[node], v] <= thr[node],
left[node], right[node])`` over max_depth rounds, in chunks of 32 trees x 2^18 voxels, then the votes and the arg-max -- its
labels must equal the kernel's (the count of differing labels is reported and must be 0); baseline (b), where scikit-learn
imports: a RandomForestClassifier of the same hyper-parameters fitted on the same rows, clf.predict with n_jobs=16 on 65 536
voxels, EXTRAPOLATED linearly to the volume and marked so.  Node visits (inner nodes tested plus one leaf per tree and voxel)
are counted by the stock traversal.  Prints one JSON line and writes it to --out.
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

SPREAD = 0.3
TREE_CHUNK, VOXEL_CHUNK = 32, 1 << 18


def planted_means(f, classes):
    import numpy as np
    return SPREAD * np.random.default_rng(f).standard_normal((classes, f))


def training_rows(f, classes, n):
    import numpy as np
    rng = np.random.default_rng(f + 1)
    y = rng.integers(0, classes, n)
    return (planted_means(f, classes)[y] + rng.standard_normal((n, f))).astype(np.float16), y


def fitted(f, classes, n, trees, depth, cache):
    """The forest of `trees` trees (depth 0: fully grown) on the planted training rows, from the cache when it is there."""
    import vit_tf_amd as vt
    path = os.path.join(cache, f'forest_f{f}_c{classes}_n{n}_t{trees}_d{depth}.npz') if cache else None
    if path and os.path.exists(path):
        return vt.forest.load_model(path)
    x, y = training_rows(f, classes, n)
    model = vt.forest.fit(x, y, trees=trees, max_depth=depth or None, seed=0)
    if path:
        os.makedirs(cache, exist_ok=True)
        vt.forest.save_model(model, path)
    return model


def first_trees(model, k):
    import vit_tf_amd as vt
    n = int(model.tree_offset[k])
    return vt.forest.ForestModel(model.class_names, model.labels, model.n_features, model.tree_offset[:k + 1], model.feature[:n],
                                 model.threshold[:n], model.left[:n], model.right[:n], model.value[:n], model.fit_time * k / model.trees)


def stock_decide(x, m, count=False):
    """(labels uint8 [nvox], node visits or None): the level-synchronous traversal in stock PyTorch.  m: device tensors
    feature, threshold (fp16), left, right (GLOBAL node indices), value int64 [nodes][C], root int64 [T], max_depth."""
    import torch
    nvox = x.shape[1]
    classes = m['value'].shape[1]
    labels = torch.empty(nvox, dtype=torch.uint8, device=x.device)
    visits = 0
    for v0 in range(0, nvox, VOXEL_CHUNK):
        xs = x[:, v0:v0 + VOXEL_CHUNK]
        cols = torch.arange(xs.shape[1], device=x.device)[None, :]
        votes = torch.zeros((xs.shape[1], classes), dtype=torch.int64, device=x.device)
        for t0 in range(0, m['root'].numel(), TREE_CHUNK):
            node = m['root'][t0:t0 + TREE_CHUNK, None].expand(-1, xs.shape[1]).contiguous()
            for _ in range(m['max_depth']):
                f = m['feature'][node]
                inner = f >= 0
                go = xs[f.clamp(min=0), cols] <= m['threshold'][node]
                node = torch.where(inner, torch.where(go, m['left'][node], m['right'][node]), node)
                if count:
                    visits += int(inner.sum())
            votes += m['value'][node].sum(0)
            if count:
                visits += node.numel()
        labels[v0:v0 + VOXEL_CHUNK] = votes.argmax(1).to(torch.uint8)
    return labels, (visits if count else None)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--features', type=int, default=384)
    ap.add_argument('--trees', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--depths', type=int, nargs='+', default=[0, 12], help='0: fully grown')
    ap.add_argument('--classes', type=int, default=6)
    ap.add_argument('--train', type=int, default=3000)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--stock-steps', type=int, default=3)
    ap.add_argument('--cache', default=None, metavar='DIR')
    ap.add_argument('--fit-only', action='store_true', help='fit (and cache) the forests, no GPU work')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'forest_kernels.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    import vit_tf_amd as vt
    from vit_tf_amd import _lib
    c = args.classes
    shapes = [(n, args.features) for n in args.sizes] + [(64, 32)]
    models = {}
    for f in sorted({f for _, f in shapes}):
        for depth in args.depths:
            t0 = time.time()
            models[f, depth] = fitted(f, c, args.train, max(args.trees), depth, args.cache)
            print(f'F={f} depth={depth or "full"}: {models[f, depth].trees} trees, {models[f, depth].n_nodes} nodes, depth '
                  f'{models[f, depth].max_depth}, fit_time {models[f, depth].fit_time:.1f} s (ready after {time.time() - t0:.1f} s)',
                  file=sys.stderr, flush=True)
    if args.fit_only:
        return
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lib = _lib.require_device()
    try:
        from sklearn.ensemble import RandomForestClassifier
    except ImportError:
        RandomForestClassifier = None
    line = {'tool': 'forest_step', 'device': torch.cuda.get_device_name(0), 'classes': c, 'train_rows': args.train, 'steps': args.steps,
            'warmup': args.warmup, 'stock_steps': args.stock_steps, 'stock_chunk': [TREE_CHUNK, VOXEL_CHUNK], 'volumes': {}}
    g = torch.Generator(device=dev).manual_seed(0)
    for n, f in shapes:
        nvox = n ** 3
        mu = torch.from_numpy(planted_means(f, c)).to(dev, torch.float32)
        cls = torch.randint(0, c, (nvox,), generator=g, device=dev)
        x = torch.empty((f, nvox), dtype=torch.float16, device=dev)
        for c0 in range(0, f, 32):                            # (filled in slabs: no fp32 copy of the whole volume)
            x[c0:c0 + 32] = (mu[:, c0:c0 + 32].T[:, cls] + torch.randn((32, nvox), generator=g, device=dev)).half()
        vt_tile = max(64, min(1024, 1 << ((65536 // f).bit_length() - 1)))       # forest.hip: the widest 128 KiB tile
        res = {'nvox': nvox, 'features': f, 'volume_mb': round(f * nvox * 2 / 1e6, 1), 'tile_voxels': vt_tile,
               'workgroups': -(-nvox // vt_tile), 'tile_lds_bytes': f * vt_tile * 2, 'forests': {}}
        labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
        votes = torch.empty((c, nvox), dtype=torch.uint32, device=dev)
        for depth in args.depths:
            for trees in args.trees:
                model = first_trees(models[f, depth], trees)
                nodes, values, off = (torch.from_numpy(a.view(np.int32 if a.dtype == np.uint32 else np.int16)).to(dev)
                                      for a in vt.forest.pack(model))
                call = lambda v: _lib.check(lib.vittf_forest_decide(                                        # noqa: E731
                    _lib.ptr(x), f, nvox, _lib.ptr(nodes), _lib.ptr(values), _lib.ptr(off), trees, c, model.max_depth, _lib.ptr(labels),
                    _lib.ptr(v), _lib.stream_ptr()))
                r = {'trees': trees, 'nodes': model.n_nodes, 'max_depth': model.max_depth, 'fit_time_s': round(model.fit_time, 1),
                     'forest_bytes': int(nodes.numel() * 4 + values.numel() * 2 + off.numel() * 4)}
                r['kernel_ms'], r['kernel_ms_all'] = timed(lambda: call(None), args.steps, args.warmup)
                r['kernel_with_votes_ms'], _ = timed(lambda: call(votes), args.steps, args.warmup)
                call(votes)
                mine = labels.clone()
                base = torch.from_numpy(np.repeat(model.tree_offset[:-1], np.diff(model.tree_offset))).to(dev)
                sm = {'feature': torch.from_numpy(model.feature).to(dev, torch.int64), 'threshold': torch.from_numpy(model.threshold).to(dev),
                      'left': torch.from_numpy(model.left).to(dev, torch.int64) + base,
                      'right': torch.from_numpy(model.right).to(dev, torch.int64) + base,
                      'value': torch.from_numpy(model.value.astype(np.int64)).to(dev),
                      'root': torch.from_numpy(model.tree_offset[:-1]).to(dev), 'max_depth': model.max_depth}
                stock, visits = stock_decide(x, sm, count=True)
                r['labels_differing_from_stock'] = int((stock != mine).sum())
                r['accuracy_on_planted_classes'] = round(float((mine.long() == cls).float().mean()), 4)
                r['node_visits'] = visits
                r['node_visits_per_s'] = round(visits / (r['kernel_ms'] * 1e-3), 1)
                r['stock_ms'], r['stock_ms_all'] = timed(lambda: stock_decide(x, sm), args.stock_steps, 1)
                r['stock_over_kernel'] = round(r['stock_ms'] / r['kernel_ms'], 2)
                if RandomForestClassifier is not None:
                    xt, yt = training_rows(f, c, args.train)
                    clf = RandomForestClassifier(trees, max_depth=depth or None, random_state=0, n_jobs=16).fit(xt, yt)
                    sub = x[:, :1 << 16].T.float().cpu().numpy()
                    clf.predict(sub[:1024])
                    t0 = time.time()
                    clf.predict(sub)
                    r['sklearn_predict_ms_extrapolated'] = round((time.time() - t0) * 1e3 * nvox / sub.shape[0], 1)
                    r['sklearn_note'] = f'clf.predict, n_jobs=16, measured on {sub.shape[0]} voxels and scaled to {nvox}'
                res['forests'][f"t{trees}_{'full' if not depth else f'd{depth}'}"] = r
                print(f'{n}^3 x {f}: ' + json.dumps({k: v for k, v in r.items() if not k.endswith('_all')}), file=sys.stderr, flush=True)
                del nodes, values, off, sm, stock, mine
        line['volumes'][f'{n}^3x{f}'] = res
        del x, labels, votes, cls
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
