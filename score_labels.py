"""Boundary and overlap scores of a predicted uint8 label volume against the ground truth.

    python score_labels.py --target labels.npy --pred PRED.npy [--classes 1 2 3] [--spacing SX SY SZ] [--tolerance T] [--output FILE] [--overwrite]

Both files are bare uint8 (W, H, D) ``.npy`` volumes: a ``labels.npy`` and any ``ntf_pred*.npy`` of predict_ntf.py, ``*_pred*.npy``
of classify_features.py, ``_clusters<C>.npy`` of cluster_features.py or ``_islands.npy`` of label_islands.py.  A target on another
grid is brought to the prediction's grid by nearest-neighbour resampling (vt.scores.resize_nearest_u8); a ``--spacing``, given
for the target's grid, is scaled by the same ratio per axis.  It writes ``<pred stem>_surface.json``:
  * ``classes`` and, per class in that order, the keys of vt.distance.surface_scores: ``hd`` (Hausdorff distance), ``hd95``
    (MedPy's: the 95th percentile of both directed distance sets together), ``assd`` (average symmetric surface distance),
    ``nsd`` (surface Dice at ``--tolerance``), ``n_surface_target``, ``n_surface_pred``.  A class absent from both volumes
    holds NaN and nsd 1, one absent from one of them Infinity and nsd 0 (Python's json spelling of the two);
  * ``overlap``: the confusion-matrix scores of vt.scores.scores for the same pair -- ``labels`` (the values present in either
    volume), ``accuracy``, ``precision``, ``recall``, ``f1``, ``iou``, ``confusion_matrix`` (null when a volume holds a value above 15);
  * ``spacing`` (on the prediction's grid; null for unit voxels), ``tolerance``, ``grid``, ``target_grid`` and ``time`` (seconds).
Distances are in voxels of the prediction's grid, or in the unit of ``--spacing``.  The transforms run on the GPU
(vt.distance); there is no CPU path.
"""
import json
import sys
import time
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

import vit_tf_amd as vt
from reduce_features import writable_path


def load_volume(path, flag):
    """The checks of label_islands.load_label_volume, with the refusal naming `flag`."""
    path = Path(path)
    if not path.exists():
        print(f'Invalid argument for {flag} (File does not exist): {path}')
        sys.exit(1)
    try:
        vol = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        print(f'Invalid argument for {flag}: {path.name} is not a bare .npy array ({e})')
        sys.exit(1)
    if not isinstance(vol, np.ndarray) or vol.dtype != np.uint8 or vol.ndim != 3 or vol.size < 1:
        what = f'{vol.dtype} {vol.shape}' if isinstance(vol, np.ndarray) else type(vol).__name__
        print(f'Invalid argument for {flag}: expected a uint8 (W, H, D) volume, got {what}')
        sys.exit(1)
    return vol


def default_output(pred_path):
    pred_path = Path(pred_path)
    return pred_path.with_name(f'{pred_path.stem}_surface.json')


def grid_spacing(spacing, target_shape, pred_shape):
    """A spacing of the target's grid on the prediction's grid: the same extent per axis over another number of voxels."""
    if spacing is None:
        return None
    return [float(s) * t / p for s, t, p in zip(spacing, target_shape, pred_shape)]


def overlap_scores(target, pred):
    """vt.scores.scores of the pair as plain lists, with the labels its rows stand for; None for values above 15, which
    vittf_confusion_matrix does not count."""
    if max(int(target.max()), int(pred.max())) > 15:
        return None
    cm = vt.scores.confusion_matrix(target, pred)
    present = np.nonzero((cm.sum(0) + cm.sum(1)) > 0)[0]
    acc, prec, rec, f1, iou, cm = vt.scores.scores_from_confusion(cm)
    return {'labels': present.tolist(), 'accuracy': float(acc), 'precision': prec.tolist(), 'recall': rec.tolist(),
            'f1': f1.tolist(), 'iou': iou.tolist(), 'confusion_matrix': cm.tolist()}


def main(argv=None):
    parser = ArgumentParser('Surface-distance and overlap scores of a predicted label volume')
    parser.add_argument('--target', type=str, required=True, help='bare uint8 (W, H, D) .npy: the ground-truth labels')
    parser.add_argument('--pred', type=str, required=True, help='bare uint8 (W, H, D) .npy: a prediction, clusters or islands')
    parser.add_argument('--classes', type=int, nargs='+', default=None, metavar='C', help='label values to score, 0..255 (default: 1 .. the largest value present)')
    parser.add_argument('--spacing', type=float, nargs=3, default=None, metavar=('SX', 'SY', 'SZ'), help="voxel spacing of the target's grid (default: unit voxels)")
    parser.add_argument('--tolerance', type=float, default=1.0, metavar='T', help='tolerance of the surface Dice, in the unit of the distances')
    parser.add_argument('--output', type=str, default=None, metavar='FILE', help='scores file (default: <pred stem>_surface.json next to the prediction)')
    parser.add_argument('--overwrite', action='store_true', help='replace an existing output file')
    args = parser.parse_args(argv)

    for c in args.classes or ():
        if not 0 <= c <= 255:
            print(f'Invalid argument for --classes: {c} is outside 0..255')
            sys.exit(1)
    if args.spacing is not None and not all(np.isfinite(s) and s > 0 for s in args.spacing):
        print(f'Invalid argument for --spacing: {args.spacing} are not three finite positive numbers')
        sys.exit(1)
    if not (np.isfinite(args.tolerance) and args.tolerance >= 0):
        print(f'Invalid argument for --tolerance: {args.tolerance} is not a finite number >= 0')
        sys.exit(1)
    target = load_volume(args.target, '--target')
    pred = load_volume(args.pred, '--pred')
    if max(pred.shape) > vt.distance.MAX_DIM:
        print(f'Invalid argument for --pred: a dimension of {pred.shape} is above {vt.distance.MAX_DIM}')
        sys.exit(1)
    out_path = writable_path(args.output or default_output(args.pred), '--output', args.overwrite)

    t0 = time.time()
    target_grid = list(target.shape)
    spacing = grid_spacing(args.spacing, target.shape, pred.shape)
    if tuple(target.shape) != tuple(pred.shape):
        target = vt.scores.resize_nearest_u8(target, tuple(pred.shape))
    classes = args.classes or list(range(1, int(max(target.max(), pred.max())) + 1))
    result = {'classes': [int(c) for c in classes]}
    if classes:
        surf = vt.distance.surface_scores(target, pred, classes, spacing, args.tolerance)
    else:                                                       # two all-zero volumes: nothing to score
        surf = {k: np.zeros(0) for k in vt.distance.SCORE_KEYS}
    result.update({k: surf[k].tolist() for k in vt.distance.SCORE_KEYS})
    result['overlap'] = overlap_scores(target, pred)
    result.update(spacing=spacing, tolerance=float(args.tolerance), grid=list(pred.shape), target_grid=target_grid,
                  time=time.time() - t0)
    print(f'{Path(args.pred).name} against {Path(args.target).name} : grid {tuple(pred.shape)}, classes {result["classes"]}')
    for k in ('hd', 'hd95', 'assd', 'nsd'):
        print(f'  {k:5s} ' + ' '.join(f'{v:.4g}' for v in result[k]))
    print(f'Surface scores saved to: {out_path}')
    with open(out_path, 'w') as fh:
        json.dump(result, fh)
    sys.exit(0)


if __name__ == '__main__':
    main()
