"""Support-vector, random-forest, MLP-head or k-nearest-neighbour classification of a feature volume from annotated voxels: a
learned label volume.

    python classify_features.py --data DIR [--num-samples N] [--sampling-mode {uniform,surface,both}] [--classifier {svm,forest,mlp,knn}]
                                [--kernel {rbf,linear}] [--C 1.0] [--gamma scale|FLOAT] [--normalize] [--tol T]
                                [--trees 256] [--max-depth N] [--max-features sqrt|all|INT|FRACTION] [--min-samples-leaf 1]
                                [--no-bootstrap] [--votes] [--features {dino,handcrafted,intensity}]
                                [--hidden W1[,W2]] [--epochs 100] [--batch 256] [--lr 1e-3] [--weight-decay 1e-2] [--probs]
                                [--k 20] [--temperature 0.07] [--knn-weights {softmax,uniform}]
                                [--background {auto,labels,border,none}] [--model FILE] [--seed S] [--overwrite]

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

``--classifier forest`` trains a random forest instead (vt.forest.fit: CART on the host, slower than scikit-learn's; the pass
over the volume is libvittf's vittf_forest_decide, forest.hip) on the same samples, background class and seed.  It has no
gamma or C, no F <= 768 limit and does not care how the features are scaled.  ``--kernel``, ``--C``, ``--gamma`` and ``--tol``
do not apply (given explicitly they are refused), ``--normalize`` is not built for it.  ``--model FILE`` picks the classifier
by the file.  Outputs, with the tag ``<num><mode>_rf<trees>[_d<depth>][_all|_mf<k>][_nobg]`` (``_all``: --max-features all;
``_mf<k>``: any other value than sqrt):
  * ``rf_pred<tag>.npy``, ``rf_model<tag>.npz`` (vt.forest.save_model), ``rf_metrics<tag>.json`` (n_trees, n_nodes and max_depth
    in the place of n_sv): as the SVM's;
  * with ``--votes``, ``rf_votes<tag>.npy``: uint8 (C, W', H', D'), votes * 255 // (trees * 65535) per class in the order of the
    model's classes (ascending label value) -- a confidence volume for thresholds or the bilateral solver.

``--classifier mlp`` trains an MLP head instead (vt.mlp.fit: numpy fp64 on the host, softmax cross-entropy, AdamW, cosine
schedule; the pass over the volume is libvittf's vittf_mlp_decide, mlp.hip) on the same samples, background class and seed:
the reference's old/compare_feat_sampling_mlp.py.  ``--hidden ""`` (the default) is the linear probe, ``--hidden 32,64`` two
hidden layers (at most two, multiples of 32 in 32..256).  ``--normalize`` gives the reference's cosine geometry (with
``--features dino`` only); ``--kernel``, ``--C``, ``--gamma`` and ``--tol`` given explicitly are refused.  The label is the
plain arg-max of the logits (the reference's ``sigmoid(max logit) > 0.5 else 0`` rule is not reproduced).  Outputs, with the
tag ``<num><mode>[_hand|_intensity]_mlp[<w1>[x<w2>]][_norm][_nobg]``:
  * ``mlp_pred<tag>.npy``, ``mlp_model<tag>.npz`` (vt.mlp.save_model), ``mlp_metrics<tag>.json`` (n_params, hidden, final_loss and
    train_accuracy in the place of n_sv): as the SVM's;
  * with ``--probs``, ``mlp_probs<tag>.npy``: uint8 (C, W', H', D'), floor(255 softmax + 0.5) per class in the order of the
    model's classes (ascending label value) -- calibrated probability volumes for transfer functions, label_islands.py or the
    bilateral solver.

``--classifier knn`` is the weighted k-nearest-neighbour classifier of the DINO evaluation protocol (vt.knn; the pass over the
volume is libvittf's vittf_knn_decide, knn.hip) on the same samples, background class and seed.  It has NO fit: the model is the
bank of annotated samples itself (L2-normalised, rounded once to fp16), so fit_time is the sampling and the rounding only.
Every voxel is compared with every bank sample by cosine similarity; the ``--k`` (1..32, default 20) nearest vote with weights
exp(sim / T) (``--temperature``, default 0.07) or 1 (``--knn-weights uniform``); the label is the arg-max of the per-class sums.
The geometry is always cosine: ``--normalize`` is implied, is accepted and changes nothing, and is not in the tag.  ``--kernel``,
``--C``, ``--gamma``, ``--tol`` given explicitly are refused, and so are ``--votes`` and ``--features handcrafted|intensity``
(cosine distance on standardised channels is not the baseline anyone means; a Euclidean metric is not built).  F <= 768, as for
the RBF machine.  Outputs, with the tag ``<num><mode>_knn<k>[_t<T>][_uni][_nobg]`` (``_t<T>`` only when T is not 0.07, ``_uni``
for uniform weights):
  * ``knn_pred<tag>.npy``, ``knn_model<tag>.npz`` (vt.knn.save_model), ``knn_metrics<tag>.json`` (n_bank, k, temperature and
    weights in the place of n_sv): as the SVM's;
  * with ``--probs``, ``knn_probs<tag>.npy``: uint8 (C, W', H', D'), floor(255 score_c / sum_c score + 0.5) per class in the order
    of the model's classes (ascending label value).

``--features handcrafted`` classifies the VOLUME ITSELF instead of a feature file: the reference baseline's default mode
(predict_svm_rf.py:25-65), an 11-channel vector per voxel at the volume's full resolution -- intensity, gradient magnitude, the
six neighbours and the position, each standardised over the volume (vt.voxel_features; libvittf's voxel_features.hip).
``--features intensity`` is the standardised intensity alone (the reference feeds the raw intensity there: a deliberate
difference -- standardising is an increasing affine map, which leaves a forest's decisions and an RBF machine with
gamma = scale unchanged up to rounding, and it keeps CT-range values representable in fp16).  No feature file is looked for;
the training rows are the features of the annotated voxels themselves, the pass streams the volume slab by slab through the
same decision kernels, and the prediction has the volume's own grid.  ``--normalize`` is refused.  The tag gets ``_hand`` or
``_intensity`` directly behind ``<num><mode>`` (``svm_pred200.0both_hand_rbf.npy``, ``rf_pred200.0both_intensity_rf256.npy``).
``--model FILE`` standardises the new volume with that volume's own statistics, as the reference does for every volume; the
model must have F = 32 (the rows are embedded in a zeroed 32-row matrix).  A model file does not say which features it was
fitted on: a ``_pca32`` model and a hand-crafted one both have F = 32, keeping them apart is the caller's business.
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
FEATURE_TAGS = {'dino': '', 'handcrafted': '_hand', 'intensity': '_intensity'}


def svm_tag(num_samples, sampling_mode, kernel, normalize=False, background=True, features='dino'):
    """The tag of a run's output files: svm_pred<tag>.npy, svm_model<tag>.npz, svm_metrics<tag>.json."""
    return f"{num_samples}{sampling_mode}{FEATURE_TAGS[features]}_{kernel}{'_norm' if normalize else ''}{'' if background else '_nobg'}"


def _paths(d, prefix, tag, extra=None):
    """(prediction, model, metrics[, confidence volume]) files of a run in directory d."""
    d = Path(d)
    paths = d / f'{prefix}_pred{tag}.npy', d / f'{prefix}_model{tag}.npz', d / f'{prefix}_metrics{tag}.json'
    return paths if extra is None else paths + (d / f'{prefix}_{extra}{tag}.npy',)


def output_paths(d, tag):
    return _paths(d, 'svm', tag)


def forest_tag(num_samples, sampling_mode, trees, max_depth=None, max_features='sqrt', background=True, features='dino'):
    """The tag of a forest run's output files: rf_pred<tag>.npy, rf_model<tag>.npz, rf_metrics<tag>.json, rf_votes<tag>.npy."""
    mf = '' if max_features == 'sqrt' else '_all' if max_features == 'all' else f'_mf{max_features}'
    return f"{num_samples}{sampling_mode}{FEATURE_TAGS[features]}_rf{trees}{'' if max_depth is None else f'_d{max_depth}'}{mf}{'' if background else '_nobg'}"


def forest_paths(d, tag):
    return _paths(d, 'rf', tag, 'votes')


def mlp_tag(num_samples, sampling_mode, hidden=(), normalize=False, background=True, features='dino'):
    """The tag of an MLP run's output files: mlp_pred<tag>.npy, mlp_model<tag>.npz, mlp_metrics<tag>.json, mlp_probs<tag>.npy."""
    return (f"{num_samples}{sampling_mode}{FEATURE_TAGS[features]}_mlp{'x'.join(str(w) for w in hidden)}"
            f"{'_norm' if normalize else ''}{'' if background else '_nobg'}")


def mlp_paths(d, tag):
    return _paths(d, 'mlp', tag, 'probs')


def knn_tag(num_samples, sampling_mode, k=20, temperature=0.07, weights='softmax', background=True):
    """The tag of a k-NN run's output files: knn_pred<tag>.npy, knn_model<tag>.npz, knn_metrics<tag>.json, knn_probs<tag>.npy."""
    return (f"{num_samples}{sampling_mode}_knn{k}{'' if temperature == 0.07 else f'_t{temperature:g}'}"
            f"{'_uni' if weights == 'uniform' else ''}{'' if background else '_nobg'}")


def knn_paths(d, tag):
    return _paths(d, 'knn', tag, 'probs')


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


SVM_DEFAULTS = {'kernel': 'rbf', 'C': 1.0, 'gamma': 'scale', 'tol': 1e-3}


class _Classifier:
    """What the four sides of main share.  A side has its argument checks (__init__), file names (paths), fit and report
    (describe, metrics); `kind` is its --classifier value, `extra_flag` the flag that asks for its confidence volume (the fourth
    of its paths), `confidence` what turns the extra output of its predict into that volume's uint8."""
    kind = extra_flag = None

    def __init__(self, args):
        self.args, self.model = args, None

    def refuse_svm_flags(self):
        for k in SVM_DEFAULTS:
            if getattr(self.args, k) is not None:
                _fail(k, f'does not apply to --classifier {self.kind}')

    def configure(self, with_bg):
        """Called once the background decision is known (a loaded model brings its own): fixes the tag's ingredients."""
        self.with_bg = with_bg

    def check_features(self, f, name, holds='fitted on'):
        if self.model is not None and self.model.n_features != f:
            _fail('model', f'{holds} F = {self.model.n_features} features, {name} has F = {f}')

    def wants_extra(self):
        return self.extra_flag is not None and getattr(self.args, self.extra_flag)

    def confidence(self, model, extra):
        return extra

    def predict(self, features, model, paths):
        if not self.wants_extra():
            return self.module.predict(features, model)
        idx, extra = self.module.predict(features, model, True)
        np.save(paths[3], self.confidence(model, extra).cpu().numpy())
        return idx

    def predict_volume(self, volume, stats, channels, model, paths):
        if not self.wants_extra():
            return vt.voxel_features.classify(volume, model, channels, stats)
        idx = torch.empty(volume.numel(), dtype=torch.uint8, device=volume.device)
        # slab by slab: the uint32 votes of a whole volume (C x 537 MB at 512^3) never exist, only their uint8 shares
        conf = np.empty((model.classes, volume.numel()), np.uint8)
        for start, n, labels, extra in vt.voxel_features.slabs(volume, model, channels, stats, want_votes=True):
            idx[start:start + n] = labels
            conf[:, start:start + n] = self.confidence(model, extra).cpu().numpy()
        np.save(paths[3], conf.reshape((model.classes,) + tuple(volume.shape)))
        return idx.reshape(tuple(volume.shape))


class _Svm(_Classifier):
    """The support-vector side of main: its argument checks, file names, fit, pass over the volume and report."""
    name, module, kind = 'SVM', vt.svm, 'svm'

    def __init__(self, args):
        super().__init__(args)
        for k, v in SVM_DEFAULTS.items():
            if getattr(args, k) is None:
                setattr(args, k, v)
        if not (args.C > 0 and np.isfinite(args.C)):
            _fail('C', f'{args.C} is not a positive number')
        if not (args.tol > 0 and np.isfinite(args.tol)):
            _fail('tol', f'{args.tol} is not a positive number')
        self.gamma = args.gamma
        if self.gamma != 'scale':
            try:
                self.gamma = float(self.gamma)
            except ValueError:
                _fail('gamma', f"{args.gamma!r} is neither 'scale' nor a number")
            if not (np.isfinite(self.gamma) and self.gamma >= 0):
                _fail('gamma', f'{args.gamma} is negative or not finite')

    def configure(self, with_bg):
        super().configure(with_bg)
        m = self.model
        self.kernel, self.normalize = (self.args.kernel, self.args.normalize) if m is None else (m.kernel, m.normalize)

    def paths(self, d, num_samples, mode):
        return output_paths(d, svm_tag(num_samples, mode, self.kernel, self.normalize, self.with_bg, self.args.features))

    def check_features(self, f, name):
        if self.kernel == 'rbf' and f > 768:
            _fail('kernel', f'the RBF kernel takes F <= 768, {name} has F = {f}: reduce it first (reduce_features.py)')
        super().check_features(f, name)

    def fit(self, samples, targets, names):
        a = self.args
        return vt.svm.fit(samples, targets, kernel=self.kernel, C=a.C, gamma=self.gamma, tol=a.tol, normalize=self.normalize,
                          class_names=names)

    def describe(self, model):
        return f'{model.sv.shape[0]} support vectors ({model.n_support.tolist()} per class)'

    def metrics(self, model):
        return {'n_sv': int(model.sv.shape[0])}


class _Forest(_Classifier):
    """The random-forest side of main."""
    name, module, kind, extra_flag = 'RF', vt.forest, 'forest', 'votes'

    def __init__(self, args):
        super().__init__(args)
        self.refuse_svm_flags()
        if args.normalize:
            _fail('normalize', 'is not built for --classifier forest')
        if not 1 <= args.trees <= vt._lib.FOREST_MAX_TREES:
            _fail('trees', f'{args.trees} is outside 1..{vt._lib.FOREST_MAX_TREES}')
        if args.max_depth is not None and not 1 <= args.max_depth <= vt._lib.FOREST_MAX_DEPTH:
            _fail('max-depth', f'{args.max_depth} is outside 1..{vt._lib.FOREST_MAX_DEPTH}')
        if args.min_samples_leaf < 1:
            _fail('min-samples-leaf', f'{args.min_samples_leaf} is not positive')
        mf = args.max_features
        if mf not in ('sqrt', 'all'):
            try:
                mf = int(mf)
            except ValueError:
                try:
                    mf = float(mf)
                except ValueError:
                    _fail('max-features', f"{args.max_features!r} is none of 'sqrt', 'all', an integer, a fraction")
            if not (mf >= 1 if isinstance(mf, int) else 0.0 < mf <= 1.0):
                _fail('max-features', f'{args.max_features} is neither an integer of at least 1 nor a fraction in (0, 1]')
        self.max_features = mf
        print('Note: --kernel, --C, --gamma and --tol do not apply to --classifier forest')

    def paths(self, d, num_samples, mode):
        a, m = self.args, self.model
        if m is not None:                                     # a loaded forest: what the file can tell
            tag = forest_tag(num_samples, mode, m.trees, None, 'sqrt', self.with_bg, a.features)
        else:
            tag = forest_tag(num_samples, mode, a.trees, a.max_depth, self.max_features, self.with_bg, a.features)
        return forest_paths(d, tag)

    def check_features(self, f, name):
        super().check_features(f, name)
        if self.model is None and isinstance(self.max_features, int) and self.max_features > f:
            _fail('max-features', f'{self.max_features} is more than the F = {f} of {name}')

    def fit(self, samples, targets, names):
        a = self.args
        return vt.forest.fit(samples, targets, trees=a.trees, max_features=self.max_features, max_depth=a.max_depth,
                             min_samples_leaf=a.min_samples_leaf, bootstrap=not a.no_bootstrap, seed=a.seed, class_names=names)

    def confidence(self, model, votes):
        wide = votes.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        return (wide * 255 // (model.trees * 65535)).to(torch.uint8)

    def describe(self, model):
        return f'{model.trees} trees, {model.n_nodes} nodes, depth {model.max_depth}'

    def metrics(self, model):
        return {'n_trees': model.trees, 'n_nodes': model.n_nodes, 'max_depth': model.max_depth}


class _Mlp(_Classifier):
    """The MLP-head side of main (its uint8 probabilities are the confidence volume as they are)."""
    name, module, kind, extra_flag = 'MLP', vt.mlp, 'mlp', 'probs'

    def __init__(self, args):
        super().__init__(args)
        self.refuse_svm_flags()
        try:
            self.hidden = vt.mlp.parse_hidden(args.hidden)
        except ValueError:
            _fail('hidden', f'{args.hidden!r} is not a comma-separated list of widths')
        L = vt._lib
        if len(self.hidden) > L.MLP_MAX_LAYERS or any(w % 32 or not 32 <= w <= L.MLP_MAX_WIDTH for w in self.hidden):
            _fail('hidden', f'{args.hidden!r}: at most {L.MLP_MAX_LAYERS} widths, multiples of 32 in 32..{L.MLP_MAX_WIDTH}')
        if args.epochs < 1:
            _fail('epochs', f'{args.epochs} is not positive')
        if args.batch < 1:
            _fail('batch', f'{args.batch} is not positive')
        if not (args.lr > 0 and np.isfinite(args.lr)):
            _fail('lr', f'{args.lr} is not a positive number')
        if not (args.weight_decay >= 0 and np.isfinite(args.weight_decay)):
            _fail('weight-decay', f'{args.weight_decay} is negative or not finite')

    def configure(self, with_bg):
        super().configure(with_bg)
        m = self.model
        self.hidden, self.normalize = (self.hidden, self.args.normalize) if m is None else (m.hidden, m.normalize)

    def paths(self, d, num_samples, mode):
        return mlp_paths(d, mlp_tag(num_samples, mode, self.hidden, self.normalize, self.with_bg, self.args.features))

    def fit(self, samples, targets, names):
        a = self.args
        return vt.mlp.fit(samples, targets, hidden=self.hidden, epochs=a.epochs, batch=a.batch, lr=a.lr, weight_decay=a.weight_decay,
                          seed=a.seed, normalize=self.normalize, class_names=names)

    def describe(self, model):
        return f'hidden {list(model.hidden)}, {model.n_params} parameters, training accuracy {model.train_accuracy:.4f}'

    def metrics(self, model):
        return {'n_params': model.n_params, 'hidden': list(model.hidden), 'final_loss': model.final_loss,
                'train_accuracy': model.train_accuracy}


class _Knn(_Classifier):
    """The k-nearest-neighbour side of main."""
    name, module, kind, extra_flag = 'KNN', vt.knn, 'knn', 'probs'

    def __init__(self, args):
        super().__init__(args)
        self.refuse_svm_flags()
        if args.votes:
            _fail('votes', 'does not apply to --classifier knn (--probs writes its per-class shares)')
        if args.features != 'dino':
            _fail('features', f'{args.features} is not built for --classifier knn: its geometry is cosine similarity of the feature file')
        if not 1 <= args.k <= vt._lib.KNN_MAX_K:
            _fail('k', f'{args.k} is outside 1..{vt._lib.KNN_MAX_K}')
        if not (args.temperature > 0 and np.isfinite(args.temperature)):
            _fail('temperature', f'{args.temperature} is not a positive number')
        args.normalize = True                                 # implied: the samples are drawn from the normalised volume

    def configure(self, with_bg):
        super().configure(with_bg)
        a, m = self.args, self.model
        self.k, self.temperature, self.weights = ((a.k, a.temperature, a.knn_weights) if m is None
                                                  else (m.k, m.temperature, m.weights))

    def paths(self, d, num_samples, mode):
        return knn_paths(d, knn_tag(num_samples, mode, self.k, self.temperature, self.weights, self.with_bg))

    def check_features(self, f, name):
        if f > 768:
            _fail('classifier', f'knn takes F <= 768, {name} has F = {f}: reduce it first (reduce_features.py)')
        super().check_features(f, name, 'holds')

    def fit(self, samples, targets, names):
        return vt.knn.fit(samples, targets, k=self.k, temperature=self.temperature, weights=self.weights, class_names=names)

    def confidence(self, model, scores):
        return vt.knn.probabilities(scores)

    def describe(self, model):
        return (f'{model.n_bank} bank samples ({np.bincount(model.bank_class, minlength=model.classes).tolist()} per class), '
                f'k = {model.k}, {model.weights} weights' + (f', T = {model.temperature:g}' if model.weights == 'softmax' else ''))

    def metrics(self, model):
        return {'n_bank': model.n_bank, 'k': model.k, 'temperature': model.temperature, 'weights': model.weights}


def main(argv=None):
    parser = ArgumentParser('Classify a feature volume with a support-vector machine or a random forest trained on annotated voxels')
    parser.add_argument('--data', type=str, required=True, help='directory holding volume, features and annotations / labels')
    parser.add_argument('--num-samples', type=float, default=0.0, help='annotations sampled per class from the labels (0: use the annotation file)')
    parser.add_argument('--sampling-mode', type=str, choices=['uniform', 'surface', 'both'], default='both', help='where samples are drawn from')
    parser.add_argument('--classifier', type=str, choices=['svm', 'forest', 'mlp', 'knn'], default=None, help='svm (the default), forest, mlp or knn; --model FILE implies it')
    parser.add_argument('--kernel', type=str, choices=list(vt.svm.KERNELS), default=None, help='svm: rbf (default) or linear')
    parser.add_argument('--C', type=float, default=None, help='svm: box constraint of the C-SVC (default 1.0)')
    parser.add_argument('--gamma', type=str, default=None, help="svm: RBF width: 'scale' (1 / (F var(samples)), default) or a number")
    parser.add_argument('--normalize', action='store_true', help='L2-normalise every voxel first (cosine geometry)')
    parser.add_argument('--background', type=str, choices=['auto', 'labels', 'border', 'none'], default='auto', help='where the background class is drawn from')
    parser.add_argument('--tol', type=float, default=None, metavar='T', help='svm: largest KKT violation the solver stops at (default 1e-3)')
    parser.add_argument('--trees', type=int, default=256, help='forest: number of trees')
    parser.add_argument('--max-depth', type=int, default=None, metavar='N', help='forest: deepest level of a tree (default: fully grown)')
    parser.add_argument('--max-features', type=str, default='sqrt', help="forest: features tried per node: 'sqrt', 'all', an integer or a fraction")
    parser.add_argument('--min-samples-leaf', type=int, default=1, help='forest: fewest training rows of a leaf')
    parser.add_argument('--no-bootstrap', action='store_true', help='forest: every tree sees every sample once')
    parser.add_argument('--votes', action='store_true', help='forest: also write the per-class vote shares rf_votes<tag>.npy')
    parser.add_argument('--hidden', type=str, default='', metavar='W1[,W2]', help='mlp: hidden widths, comma-separated (default: none, a linear probe)')
    parser.add_argument('--epochs', type=int, default=100, help='mlp: passes over the samples')
    parser.add_argument('--batch', type=int, default=256, help='mlp: samples per step')
    parser.add_argument('--lr', type=float, default=1e-3, help='mlp: initial learning rate of the cosine schedule')
    parser.add_argument('--weight-decay', type=float, default=1e-2, help="mlp: AdamW's decoupled weight decay")
    parser.add_argument('--probs', action='store_true', help='mlp, knn: also write the per-class probabilities mlp_probs<tag>.npy / knn_probs<tag>.npy')
    parser.add_argument('--k', type=int, default=20, help='knn: neighbours that vote (1..32)')
    parser.add_argument('--temperature', type=float, default=0.07, metavar='T', help='knn: temperature of the weights exp(sim / T)')
    parser.add_argument('--knn-weights', type=str, choices=list(vt.knn.WEIGHTS), default='softmax', help='knn: softmax (exp(sim / T), default) or uniform')
    parser.add_argument('--features', type=str, choices=list(FEATURE_TAGS), default='dino',
                        help='dino (default): the feature file; handcrafted: 11 channels computed from the volume itself; intensity: its intensity alone')
    parser.add_argument('--model', type=str, default=None, metavar='FILE', help='apply this saved model instead of fitting')
    parser.add_argument('--seed', type=int, default=0, help='seed of the sample draws')
    parser.add_argument('--overwrite', action='store_true', help='replace existing output files')
    args = parser.parse_args(argv)

    d = Path(args.data)
    if not d.is_dir():
        _fail('data', f'{d} is not a directory')
    if not args.num_samples >= 0:
        _fail('num-samples', f'{args.num_samples} is negative')
    own = args.features != 'dino'                             # the features come from the volume itself
    if own and args.normalize:
        _fail('normalize', f'does not apply to --features {args.features}: the channels are standardised, not directions')
    model = None
    kind = args.classifier
    if args.model:
        of_file = {vt.knn.FORMAT: 'knn', vt.mlp.FORMAT: 'mlp', vt.forest.FORMAT: 'forest'}.get(vt._classify.file_format(args.model), 'svm')
        if kind is not None and kind != of_file:
            _fail('model', f'{args.model} does not hold a {kind} model')
        kind = of_file
    clf = {'forest': _Forest, 'mlp': _Mlp, 'knn': _Knn}.get(kind, _Svm)(args)       # the classifier's own argument checks come first
    if args.model:
        try:
            model = clf.model = clf.module.load_model(args.model)
        except (OSError, ValueError, KeyError) as e:
            _fail('model', e)
    if own and model is not None:
        if model.n_features != 32:
            _fail('model', f'fitted on F = {model.n_features} features, --features {args.features} gives F = 32 (its rows in a zeroed 32-row matrix)')
        if model.normalize:
            _fail('model', f'fitted with --normalize, which --features {args.features} refuses')
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
        with_bg = background != 'none'
    else:
        with_bg = bool(model.labels[0] == 0)
    clf.configure(with_bg)
    mode = 'annotated' if args.num_samples == 0.0 else args.sampling_mode
    paths = clf.paths(d, args.num_samples, mode)
    pred_path, model_path, metrics_path = paths[:3]
    if pred_path.exists() and not args.overwrite:
        print(f'Already inferred {clf.name} preds for {d} using sampling mode {mode} and {args.num_samples} samples')
        sys.exit(0)
    if not (d / 'volume.npy').exists():
        _fail('data', f'{d} has no volume.npy')
    feat_fn = None if own else find_feature_file(d)
    if feat_fn is None and not own:
        _fail('data', f'No features found in {d}')
    print(f'Inferring for {d} using sampling mode {mode} and {args.num_samples} samples')

    volume = np.flip(np.load(d / 'volume.npy', allow_pickle=True), axis=-3)
    vol_shape = tuple(int(s) for s in np.squeeze(volume).shape[-3:])
    labels = np.flip(np.load(d / 'labels.npy', allow_pickle=True)[()], axis=-3).copy() if has_labels else None
    if own:
        try:
            vt.voxel_features.check_shape(np.squeeze(volume).shape)
        except ValueError as e:
            _fail('features', f'volume.npy: {e}')
        channels = vt.voxel_features.CHANNELS if args.features == 'handcrafted' else 1
        clf.check_features(32, f'--features {args.features}')
        try:
            vol_dev = vt.voxel_features._volume(np.ascontiguousarray(np.squeeze(volume), dtype=np.float32))
            vstats = vt.voxel_features.stats(vol_dev)
        except ValueError as e:
            _fail('features', f'volume.npy: {e}')
    else:
        features = pick_features(np.load(feat_fn, allow_pickle=True)[()])
        f = int(features.shape[0])
        if features.ndim != 4 or f % 32 or not 32 <= f <= 1024:
            _fail('data', f'{feat_fn.name} holds {tuple(features.shape)}: F = {f} is not a multiple of 32 in 32..1024')
        clf.check_features(f, feat_fn.name)

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
        if own:
            try:
                samples, targets = vt.voxel_features.sample(vol_dev, annotations, vstats, channels)
            except ValueError as e:
                _fail('data', e)
        else:
            samples, targets = vt.svm.sample(features, annotations, vol_shape, args.normalize)
        order = np.argsort(values)                                         # class names in ascending label value
        try:
            model = clf.fit(samples, np.asarray(values)[targets], [list(annotations)[i] for i in order])
        except ValueError as e:
            _fail('num-samples', e)
    t1 = time.time()
    pred_idx = clf.predict_volume(vol_dev, vstats, channels, model, paths) if own else clf.predict(features, model, paths)
    pred = torch.from_numpy(model.labels).to(pred_idx.device)[pred_idx.long()].contiguous()
    torch.cuda.synchronize()
    t2 = time.time()
    pred = pred.cpu().numpy()
    np.save(pred_path, pred)
    if not args.model:
        clf.module.save_model(model, model_path)
    print(f'Pred: {pred.shape} uint8, classes {model.class_names} as {model.labels.tolist()}, {clf.describe(model)}; '
          f'saving to: {pred_path}')
    print(f'{clf.name} fit time:', t1 - t0)
    print(f'{clf.name} predict time:', t2 - t1)
    if labels is None:
        sys.exit(0)
    if tuple(pred.shape) != tuple(labels.shape[-3:]):
        pred = vt.scores.resize_nearest_u8(pred, tuple(labels.shape[-3:]))
    n_names = max(int(labels.max()), int(model.labels.max())) + 1
    by_value = {int(v): n for v, n in zip(model.labels, model.class_names)}
    metrics = _metrics(labels, pred, [by_value.get(v, 'background' if v == 0 else f'ntf{v}') for v in range(n_names)])
    metrics['fit_time'] = t1 - t0
    metrics['predict_time'] = t2 - t1
    metrics.update(clf.metrics(model))
    print(f'{clf.name} Metrics:')
    pprint(metrics)
    with open(metrics_path, 'w') as fh:
        json.dump(metrics, fh)
    sys.exit(0)


if __name__ == '__main__':
    main()
