"""Support-vector classification of a feature volume from annotated voxels: a learned label volume.

    python classify_features.py --data DIR [--num-samples N] [--sampling-mode {uniform,surface,both}] [--kernel {rbf,linear}] [--C 1.0]
                                [--gamma scale|FLOAT] [--normalize] [--background {auto,labels,border,none}] [--tol T] [--model FILE]
                                [--seed S] [--overwrite]

DIR follows predict_ntf.py's directory contract: ``volume.npy`` and ``labels.npy`` (flipped on axis -3), the largest file
whose name contains ``features`` and not ``pred``, and ``annotations.npy`` when ``--num-samples 0`` (otherwise the annotations
are drawn per class from the labels, as predict_ntf.py draws them).  The features at the annotated voxels (sampled as the
similarity query samples them) train a one-vs-one C-SVC on the host (vt.svm.fit, fp64); the pass over the volume -- every
voxel against every support vector -- runs in libvittf (svm.hip).  A background class is added the way the reference's SVM
baseline adds it: as many samples as the largest class from ``labels == 0`` (``labels``) or from the 4-voxel border shell of the
volume (``border``); ``auto`` means ``labels`` when labels.npy exists, else ``border``; ``none`` adds no background class, and
every voxel then gets one of the annotated classes.

Outputs in DIR, with the tag ``<num><mode>_<kernel>[_norm][_nobg]``:
  * ``svm_pred<tag>.npy``: a bare uint8 volume at the feature grid, 0 = background, i + 1 for the i-th annotation class in
    dictionary order (the numbering of predict_ntf.py's label volume; label_islands.py and the scores take it as it is);
  * ``svm_model<tag>.npz``: the model (vt.svm.save_model), for ``--model FILE`` runs that apply it to another volume without
    fitting (a time series shares one classifier);
  * ``svm_metrics<tag>.json`` when labels.npy exists: the keys of ntf_metrics*.json plus fit_time, predict_time and n_sv, the
    prediction nearest-resized to the label volume.
The same directory and flags give the same bytes.  There is no CPU path.
"""
import json
import sys
import time
from argparse import ArgumentParser
from pathlib import Path
from pprint import pprint

import numpy as np
import torch

import vit_tf_amd as vt
from predict_ntf import pick_features, sampling_modes, _metrics

BORDER = 4


def svm_tag(num_samples, sampling_mode, kernel, normalize=False, background=True):
    """The tag of a run's output files: svm_pred<tag>.npy, svm_model<tag>.npz, svm_metrics<tag>.json."""
    return f"{num_samples}{sampling_mode}_{kernel}{'_norm' if normalize else ''}{'' if background else '_nobg'}"


def output_paths(d, tag):
    d = Path(d)
    return d / f'svm_pred{tag}.npy', d / f'svm_model{tag}.npz', d / f'svm_metrics{tag}.json'


def find_feature_file(d):
    """predict_ntf.py's rule: the largest file whose name contains 'features' and not 'pred'; None when there is none."""
    fns = [p for p in Path(d).iterdir() if 'features' in p.name and 'pred' not in p.name]
    return max(fns, key=lambda p: p.stat().st_size) if fns else None


def _fail(flag, why):
    print(f'Invalid argument for --{flag}: {why}')
    sys.exit(1)


def _draw(mode, lab, n, class_id=None):
    if mode == 'surface':
        return sampling_modes[mode](lab, n, class_id=class_id)
    return sampling_modes[mode](lab, n, thin_to_reasonable=True, class_id=class_id)


def main(argv=None):
    parser = ArgumentParser('Classify a feature volume with a support-vector machine trained on annotated voxels')
    parser.add_argument('--data', type=str, required=True, help='directory holding volume, features and annotations / labels')
    parser.add_argument('--num-samples', type=float, default=0.0, help='annotations sampled per class from the labels (0: use the annotation file)')
    parser.add_argument('--sampling-mode', type=str, choices=['uniform', 'surface', 'both'], default='both', help='where samples are drawn from')
    parser.add_argument('--kernel', type=str, choices=list(vt.svm.KERNELS), default='rbf')
    parser.add_argument('--C', type=float, default=1.0, help='box constraint of the C-SVC')
    parser.add_argument('--gamma', type=str, default='scale', help="RBF width: 'scale' (1 / (F var(samples))) or a number")
    parser.add_argument('--normalize', action='store_true', help='L2-normalise every voxel first (cosine geometry)')
    parser.add_argument('--background', type=str, choices=['auto', 'labels', 'border', 'none'], default='auto', help='where the background class is drawn from')
    parser.add_argument('--tol', type=float, default=1e-3, metavar='T', help='largest KKT violation the solver stops at')
    parser.add_argument('--model', type=str, default=None, metavar='FILE', help='apply this saved model instead of fitting')
    parser.add_argument('--seed', type=int, default=0, help='seed of the sample draws')
    parser.add_argument('--overwrite', action='store_true', help='replace existing output files')
    args = parser.parse_args(argv)

    d = Path(args.data)
    if not d.is_dir():
        _fail('data', f'{d} is not a directory')
    if not args.num_samples >= 0:
        _fail('num-samples', f'{args.num_samples} is negative')
    if not (args.C > 0 and np.isfinite(args.C)):
        _fail('C', f'{args.C} is not a positive number')
    if not (args.tol > 0 and np.isfinite(args.tol)):
        _fail('tol', f'{args.tol} is not a positive number')
    gamma = args.gamma
    if gamma != 'scale':
        try:
            gamma = float(gamma)
        except ValueError:
            _fail('gamma', f"{args.gamma!r} is neither 'scale' nor a number")
        if not (np.isfinite(gamma) and gamma >= 0):
            _fail('gamma', f'{args.gamma} is negative or not finite')
    model = None
    if args.model:
        try:
            model = vt.svm.load_model(args.model)
        except (OSError, ValueError, KeyError) as e:
            _fail('model', e)
    has_labels = (d / 'labels.npy').exists()
    background = args.background
    if background == 'auto':
        background = 'labels' if has_labels else 'border'
    if model is None:
        if background == 'labels' and not has_labels:
            _fail('background', f'labels asked for, {d} has no labels.npy')
        if args.num_samples > 0 and not has_labels:
            _fail('num-samples', f'Cannot sample labels if they are not provided ({d} has no labels.npy)')
        if args.num_samples == 0 and not (d / 'annotations.npy').exists():
            _fail('num-samples', f'0 asks for the annotation file, {d} has no annotations.npy')
        kernel, normalize, with_bg = args.kernel, args.normalize, background != 'none'
    else:
        kernel, normalize, with_bg = model.kernel, model.normalize, bool(model.labels[0] == 0)
    mode = 'annotated' if args.num_samples == 0.0 else args.sampling_mode
    tag = svm_tag(args.num_samples, mode, kernel, normalize, with_bg)
    pred_path, model_path, metrics_path = output_paths(d, tag)
    if pred_path.exists() and not args.overwrite:
        print(f'Already inferred SVM preds for {d} using sampling mode {mode} and {args.num_samples} samples')
        sys.exit(0)
    if not (d / 'volume.npy').exists():
        _fail('data', f'{d} has no volume.npy')
    feat_fn = find_feature_file(d)
    if feat_fn is None:
        _fail('data', f'No features found in {d}')
    print(f'Inferring for {d} using sampling mode {mode} and {args.num_samples} samples')

    volume = np.flip(np.load(d / 'volume.npy', allow_pickle=True), axis=-3)
    vol_shape = tuple(int(s) for s in np.squeeze(volume).shape[-3:])
    labels = np.flip(np.load(d / 'labels.npy', allow_pickle=True)[()], axis=-3).copy() if has_labels else None
    features = pick_features(np.load(feat_fn, allow_pickle=True)[()])
    f = int(features.shape[0])
    if features.ndim != 4 or f % 32 or not 32 <= f <= 1024:
        _fail('data', f'{feat_fn.name} holds {tuple(features.shape)}: F = {f} is not a multiple of 32 in 32..1024')
    if kernel == 'rbf' and f > 768:
        _fail('kernel', f'the RBF kernel takes F <= 768, {feat_fn.name} has F = {f}: reduce it first (reduce_features.py)')
    if model is not None and model.sv.shape[1] != f:
        _fail('model', f'fitted on F = {model.sv.shape[1]} features, {feat_fn.name} has F = {f}')

    torch.manual_seed(args.seed)
    t0 = time.time()
    if model is None:
        if args.num_samples == 0.0:
            annotations = {k: torch.as_tensor(v).reshape(-1, 3) for k, v in np.load(d / 'annotations.npy', allow_pickle=True)[()].items()}
        else:
            annotations = {}
            labels_dev = vt.samplers.device_labels(labels)
            for i in range(1, int(labels.max()) + 1):
                total = int((labels_dev == i).sum().item())
                n = min(int(args.num_samples), total) if args.num_samples > 1.0 else int(args.num_samples * total)
                if n > 0:
                    annotations[f'ntf{i}'] = _draw(mode, labels_dev, n, class_id=i)
        annotations = {k: v for k, v in annotations.items() if v.shape[0] > 0}
        names = list(annotations)
        values = list(range(1, len(names) + 1))
        if with_bg:
            n_bg = max(int(v.shape[0]) for v in annotations.values()) if annotations else 0
            if background == 'labels':
                lab0 = vt.samplers.device_labels(labels)
                n_bg = min(n_bg, int((lab0 == 0).sum().item()))
                bg = _draw('uniform' if mode == 'annotated' else mode, lab0, n_bg, class_id=0) if n_bg else torch.zeros((0, 3), dtype=torch.long)
            else:
                shell = torch.ones(vol_shape, dtype=torch.bool)
                shell[BORDER:-BORDER, BORDER:-BORDER, BORDER:-BORDER] = False
                bg = vt.samplers.sample_uniform(shell, min(n_bg, int(shell.sum())), thin_to_reasonable=True)
            if bg.shape[0] > 0:
                annotations['background'] = bg
                values.append(0)
        if len(values) < 2 or len(values) > vt._lib.SVM_MAX_CLASSES:
            _fail('data', f'{len(values)} classes (background included): the classifier takes 2..{vt._lib.SVM_MAX_CLASSES}')
        samples, targets = vt.svm.sample(features, annotations, vol_shape, normalize)
        order = np.argsort(values)                                         # class names in ascending label value
        try:
            model = vt.svm.fit(samples, np.asarray(values)[targets], kernel=kernel, C=args.C, gamma=gamma, tol=args.tol,
                               normalize=normalize, class_names=[list(annotations)[i] for i in order])
        except ValueError as e:
            _fail('num-samples', e)
    t1 = time.time()
    pred_idx = vt.svm.predict(features, model)
    pred = torch.from_numpy(model.labels).to(pred_idx.device)[pred_idx.long()].contiguous()
    torch.cuda.synchronize()
    t2 = time.time()
    pred = pred.cpu().numpy()
    np.save(pred_path, pred)
    if not args.model:
        vt.svm.save_model(model, model_path)
    print(f'Pred: {pred.shape} uint8, classes {model.class_names} as {model.labels.tolist()}, {model.sv.shape[0]} support vectors '
          f'({model.n_support.tolist()} per class); saving to: {pred_path}')
    print('SVM fit time:', t1 - t0)
    print('SVM predict time:', t2 - t1)
    if labels is None:
        sys.exit(0)
    if tuple(pred.shape) != tuple(labels.shape[-3:]):
        pred = vt.scores.resize_nearest_u8(pred, tuple(labels.shape[-3:]))
    n_names = max(int(labels.max()), int(model.labels.max())) + 1
    by_value = {int(v): n for v, n in zip(model.labels, model.class_names)}
    metrics = _metrics(labels, pred, [by_value.get(v, 'background' if v == 0 else f'ntf{v}') for v in range(n_names)])
    metrics['fit_time'] = t1 - t0
    metrics['predict_time'] = t2 - t1
    metrics['n_sv'] = int(model.sv.shape[0])
    print('SVM Metrics:')
    pprint(metrics)
    with open(metrics_path, 'w') as fh:
        json.dump(metrics, fh)
    sys.exit(0)


if __name__ == '__main__':
    main()
