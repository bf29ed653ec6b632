"""k-means clustering of a feature file written by infer.py (or reduce_features.py): an unsupervised label volume.

    python cluster_features.py --features FILE --clusters C [--seed S] [--max-iter N] [--tol T] [--centroids FILE] [--output FILE] [--overwrite]

Reads the feature volume the way reduce_features.py does (so reduced ``_pca32`` / ``_pca64`` files work as they are), runs
Lloyd's k-means on it (vt.kmeans: the assignment and the cluster sums are kernels on the GPU, the c x F arithmetic between
them is host work; k-means++ start from ``--seed``) or takes saved centroids (``--centroids``, so that a time series shares
one labelling: no fit, only the assignment) and writes
  * ``<stem>_clusters<C>.npy``: a bare uint8 (W', H', D') label volume, clusters numbered by descending voxel count;
  * ``<stem>_clusters<C>_centroids.npz``: the centroids and their statistics (only when they were fitted).
The numbering and the saved counts are those of the last Lloyd iteration, the volume is one more assignment to its means: a
fit that stopped on ``--tol`` or ``--max-iter`` rather than on unchanged centroids can move a few voxels in between, so the
sizes printed (those of the volume) may differ slightly from the saved counts and need not descend strictly.
The same seed and the same file give the same bytes.  There is no CPU path.
"""
import sys
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

import vit_tf_amd as vt
from reduce_features import writable_path, load_features


def main(argv=None):
    max_c = vt._lib.KMEANS_MAX_C
    parser = ArgumentParser('Cluster a feature volume with k-means')
    parser.add_argument('--features', type=str, required=True, help='feature file of infer.py / reduce_features.py (.npy / .pt)')
    parser.add_argument('--clusters', type=int, default=None, metavar='C', help=f'clusters, 2..{max_c} (with --centroids: what the file holds)')
    parser.add_argument('--seed', type=int, default=0, help='seed of the k-means++ start')
    parser.add_argument('--max-iter', type=int, default=50, metavar='N', help='most Lloyd iterations')
    parser.add_argument('--tol', type=float, default=1e-4, metavar='T', help='stop when the squared centroid shift is <= T x the mean feature variance')
    parser.add_argument('--centroids', type=str, default=None, metavar='FILE', help='assign to these saved centroids instead of fitting')
    parser.add_argument('--output', type=str, default=None, metavar='FILE', help='label volume (default: <stem>_clusters<C>.npy next to the input)')
    parser.add_argument('--overwrite', action='store_true', help='replace existing output files')
    args = parser.parse_args(argv)

    src = Path(args.features)
    saved = None
    if args.centroids:
        try:
            saved = vt.kmeans.load_clustering(args.centroids)
        except (OSError, ValueError, KeyError) as e:
            print(f'Invalid argument for --centroids: {e}')
            sys.exit(1)
        c = int(saved.centroids.shape[0])
        if args.clusters is not None and args.clusters != c:
            print(f'Invalid argument for --clusters: {args.clusters} asked for, {args.centroids} holds {c}')
            sys.exit(1)
    elif args.clusters is None:
        print('Invalid argument for --clusters: give the number of clusters (or --centroids FILE)')
        sys.exit(1)
    else:
        c = args.clusters
    if not 2 <= c <= max_c:
        print(f'Invalid argument for --clusters: {c} is outside 2..{max_c}')
        sys.exit(1)
    if args.max_iter < 1:
        print(f'Invalid argument for --max-iter: {args.max_iter} is below 1')
        sys.exit(1)
    if not args.tol >= 0:
        print(f'Invalid argument for --tol: {args.tol} is negative')
        sys.exit(1)
    letter, feats = load_features(src)
    f, nvox = int(feats.shape[0]), int(np.prod(feats.shape[1:]))
    if f % 32 or not 32 <= f <= 1024:
        print(f'Invalid argument for --features: F = {f} is not a multiple of 32 in 32..1024')
        sys.exit(1)
    if saved is not None and int(saved.centroids.shape[1]) != f:
        print(f'Invalid argument for --centroids: fitted on F = {int(saved.centroids.shape[1])} features, {src.name} has F = {f}')
        sys.exit(1)
    if c > nvox:
        print(f'Invalid argument for --clusters: {c} clusters of {nvox} voxels')
        sys.exit(1)
    out_path = writable_path(args.output or src.with_name(f'{src.stem}_clusters{c}.npy'), '--output', args.overwrite)
    cent_path = None if saved is not None else writable_path(out_path.with_name(out_path.stem + '_centroids.npz'), '--output', args.overwrite)

    if saved is None:
        labels, result = vt.kmeans.fit(feats, c, seed=args.seed, max_iter=args.max_iter, tol=args.tol)
        how = (f"{result.n_iter} iterations ({'converged' if result.converged else 'not converged'}), "
               f'inertia {float(result.inertia):.6g}')
    else:
        labels = vt.kmeans.assign(feats, saved.centroids)
        how = f'assigned to the centroids of {args.centroids}'
    sizes = torch.bincount(labels.reshape(-1).long(), minlength=c).tolist()          # of the volume that is written
    labels = labels.cpu().numpy()
    print(f'{letter} : {tuple(feats.shape)} -> {labels.shape} uint8, {c} clusters; {how}; sizes {sizes}; saving to: {out_path}')
    np.save(out_path, labels)
    if cent_path is not None:
        vt.kmeans.save_clustering(result, cent_path)
        print(f'Centroids saved to: {cent_path}')
    sys.exit(0)


if __name__ == '__main__':
    main()
