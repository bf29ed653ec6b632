"""PCA reduction of a feature file written by infer.py: the first K principal components of the feature volume.

    python reduce_features.py --features FILE [--components K] [--no-center] [--basis FILE] [--output FILE] [--rgb] [--overwrite]

Reads the feature volume the way predict_ntf.py does (a bare array, the 'k' entry of infer.py's dict, or the only entry of a
one-entry dict), fits a basis on it (vt.pca: Gram kernel on the GPU, the F x F eigenproblem on the host) or takes a saved
one (``--basis``, so that a time series shares one colour space), projects the volume (projection kernel) and writes
  * ``<stem>_pca<K><suffix>``: {letter: fp16 (K, W', H', D')} under the letter of the input, which predict_ntf.py takes as it is;
  * ``<stem>_pca<K>_basis.npz``: the basis (only when one was fitted);
  * with ``--rgb`` ``<stem>_pca_rgb.npy``: uint8 (W', H', D', 3), the first three components, each channel mapped from its
    1st..99th percentile onto 0..255.
``--no-center`` fits on the second moments instead of the covariance: dot products of reduced voxels then approximate those
of the full ones, which is what predict_ntf.py's raw-dot similarity wants.  There is no CPU path.
"""
import os
import sys
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

import vit_tf_amd as vt
from infer import save_features


def load_features(path):
    """(letter, fp16-able (F, W', H', D') tensor) of a feature file: predict_ntf.pick_features' rules."""
    from predict_ntf import pick_features
    path = Path(path)
    if not path.exists():
        print(f'Invalid argument for --features (File does not exist): {path}')
        sys.exit(1)
    if path.suffix in ('.pt', '.pth'):
        data = torch.load(path, weights_only=False)
    elif path.suffix == '.npy':
        data = np.load(path, allow_pickle=True)
        data = data[()] if data.dtype == object else data
    else:
        print(f'Unsupported file extension: {path.suffix}')
        sys.exit(1)
    letter = 'k'
    if isinstance(data, dict) and 'k' not in data and len(data) == 1:
        letter = next(iter(data))
    try:
        feats = pick_features(data)
    except ValueError as e:
        print(f'Invalid argument for --features: {e}')
        sys.exit(1)
    if feats.ndim != 4:
        print(f'Invalid argument for --features: expected a (F, W, H, D) volume, got {tuple(feats.shape)}')
        sys.exit(1)
    return letter, feats


def writable_path(path, flag, overwrite):
    """infer.handle_output_path's refusals for one output file."""
    path = Path(path)
    if path.exists() and not overwrite:
        print(f'Cache file already exists: {path}. Use --overwrite to overwrite.')
        sys.exit(1)
    if not os.access(os.path.dirname(str(path)) or os.getcwd(), os.W_OK):
        print(f'Invalid argument for {flag} (Cannot write to location): {path}')
        sys.exit(1)
    return path


def main(argv=None):
    parser = ArgumentParser('Reduce a feature volume to its first principal components')
    parser.add_argument('--features', type=str, required=True, help='feature file of infer.py (.npy / .pt)')
    parser.add_argument('--components', type=int, default=None, metavar='K', help=f'components to keep, 1..{vt._lib.PCA_MAX_K} (default 32; with --basis: what the basis holds)')
    parser.add_argument('--no-center', action='store_true', help='fit on the second moments (no mean subtraction): keeps dot products')
    parser.add_argument('--basis', type=str, default=None, metavar='FILE', help='apply this saved basis instead of fitting one')
    parser.add_argument('--output', type=str, default=None, metavar='FILE', help='reduced feature file (default: <stem>_pca<K><suffix> next to the input)')
    parser.add_argument('--rgb', action='store_true', help='also write <stem>_pca_rgb.npy: the first three components as a uint8 colour volume')
    parser.add_argument('--overwrite', action='store_true', help='replace existing output files')
    args = parser.parse_args(argv)

    src = Path(args.features)
    basis = None
    if args.basis:
        try:
            basis = vt.pca.load_basis(args.basis)
        except (OSError, ValueError, KeyError) as e:
            print(f'Invalid argument for --basis: {e}')
            sys.exit(1)
        k = int(basis.components.shape[0])
        if args.components is not None and args.components != k:
            print(f'Invalid argument for --components: {args.components} asked for, the basis {args.basis} holds {k}')
            sys.exit(1)
    else:
        k = 32 if args.components is None else args.components
    if not 1 <= k <= vt._lib.PCA_MAX_K:
        print(f'Invalid argument for --components: {k} is outside 1..{vt._lib.PCA_MAX_K}')
        sys.exit(1)
    if args.rgb and k < 3:
        print(f'Invalid argument for --rgb: a colour volume needs at least 3 components, got {k}')
        sys.exit(1)
    letter, feats = load_features(src)
    f = int(feats.shape[0])
    if basis is not None and int(basis.components.shape[1]) != f:
        print(f'Invalid argument for --basis: fitted on F = {int(basis.components.shape[1])} features, {src.name} has F = {f}')
        sys.exit(1)
    if basis is None and k > f:
        print(f'Invalid argument for --components: {k} components of F = {f} features')
        sys.exit(1)
    if f % 32 or not 32 <= f <= 1024:
        print(f'Invalid argument for --features: F = {f} is not a multiple of 32 in 32..1024')
        sys.exit(1)
    out_path = writable_path(args.output or src.with_name(f'{src.stem}_pca{k}{src.suffix}'), '--output', args.overwrite)
    basis_path = None if basis is not None else writable_path(out_path.with_name(out_path.stem + '_basis.npz'), '--output', args.overwrite)
    rgb_path = writable_path(src.with_name(f'{src.stem}_pca_rgb.npy'), '--rgb', args.overwrite) if args.rgb else None

    if basis is None:
        reduced, basis = vt.pca.reduce_features(feats, k, center=not args.no_center)
    else:
        reduced = vt.pca.project(feats, basis)
    reduced = reduced.cpu()
    kept = float(basis.explained_variance.sum() / basis.total_variance) if float(basis.total_variance) > 0 else 0.0
    print(f'{letter} : {tuple(feats.shape)} -> {tuple(reduced.shape)}; the {k} components hold {100 * kept:.1f} % of the '
          f"{'variance' if basis.center else 'second moment'}; saving to: {out_path}")
    save_features({letter: reduced}, out_path)
    if basis_path is not None:
        vt.pca.save_basis(basis, basis_path)
        print(f'PCA basis saved to: {basis_path}')
    if rgb_path is not None:
        np.save(rgb_path, vt.pca.rgb_volume(reduced))
        print(f'Colour volume saved to: {rgb_path}')
    sys.exit(0)


if __name__ == '__main__':
    main()
