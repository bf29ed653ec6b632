"""An MLP head on a feature volume, trained on annotated voxels: the linear probe (no hidden layer) and its one- and
two-hidden-layer relatives, the third learned classifier beside svm.py and forest.py and the only one that gives calibrated
per-class probability volumes.  It follows the reference's old/compare_feat_sampling_mlp.py: Linear (-> ReLU -> Linear)*,
softmax cross-entropy, AdamW, a cosine learning-rate schedule, ``--mlp "32,64"`` hidden widths (none: a linear probe).

``fit`` is host work in numpy fp64 with a hand-written backward pass (no torch autograd, no scikit-learn): the samples are
rounded to fp16 first, nn.Linear's initialisation from np.random.default_rng(seed), one shuffled pass per epoch from the same
generator, AdamW exactly as torch.optim.AdamW defines it, the learning rate of epoch e = lr (1 + cos(pi e / epochs)) / 2
(CosineAnnealingLR(T_max=epochs) stepped per epoch).  ``predict`` is the pass over the volume, libvittf's vittf_mlp_decide
(mlp.hip): the chained small GEMMs on the matrix cores with the hidden activations never leaving the chip.  There is no CPU
path for it.

Differences from the reference, both deliberate: (1) it passes its --wd to nobody and so trains with AdamW's default weight
decay 1e-2 -- our default is that value, said openly; its own settings (10 epochs, lr 1e-4) are reachable through the
arguments, and OUR defaults (100 epochs, lr 1e-3, batch 256) have not been tried on real data.  (2) its label rule
``sigmoid(max logit) > 0.5 else 0`` is NOT reproduced: the label is the plain arg-max of the logits, the lowest index among
equal logits.

Range: the hand-over of the hidden activations between the contractions is range-safe inside the kernel (a power-of-two scale
per voxel, see mlp.hip), so ``decide`` needs no bound on the activations; what it cannot survive is fp32 overflow, and the
model's constructor refuses (ValueError) a head whose Cauchy-Schwarz bound max_j |w_j|_2 max_v |x_v|_2 + |b_j|, propagated
through the layers from the largest norm an fp16 voxel can have, reaches 2^100.
"""
import time

import numpy as np
import torch

from . import _classify, _lib
from ._classify import round_samples, sample                                                    # noqa: F401
from ._featvol import _np

FORMAT = 'vittf-mlp-1'
BETAS = (0.9, 0.999)
EPS = 1e-8
RANGE_LIMIT = 2.0 ** 100


def parse_hidden(text):
    """'32,64' -> (32, 64); '' -> ()."""
    if isinstance(text, (tuple, list)):
        return tuple(int(w) for w in text)
    text = str(text).strip()
    return tuple(int(w) for w in text.split(',')) if text else ()


def activation_bound(weights, biases, x_norm):
    """The Cauchy-Schwarz bound on the magnitude of any pre-activation: layer by layer max_j (|w_j|_2 |a|_2 + |b_j|) with
    |a|_2 <= sqrt(out) max_j |a_j| for the next one.  Returns the list of per-layer bounds (fp64)."""
    out, norm = [], float(x_norm)
    for w, b in zip(weights, biases):
        w = np.asarray(w, np.float64)
        m = float(np.max(np.sqrt((w * w).sum(1)) * norm + np.abs(np.asarray(b, np.float64))))
        out.append(m)
        norm = m * np.sqrt(w.shape[0])
    return out


class MlpModel:
    """A fitted (or imported) head as plain arrays:
      class_names [C] str, labels uint8 [C] (ascending: the value a label volume carries for each class), n_features F,
      normalize (bool: the voxels are divided by their L2 norm first), hidden (tuple of widths),
      weights: list of fp32 [out][in] (in = F, then the widths; the last out = C), biases: list of fp32 [out]
      fit statistics: fit_time (s), loss_history fp64 [epochs] (mean loss of each epoch), train_accuracy."""
    ARRAYS = ('format', 'class_names', 'labels', 'n_features', 'normalize', 'hidden', 'fit_time', 'loss_history', 'train_accuracy')

    def __init__(self, class_names, labels, n_features, normalize, hidden, weights, biases, fit_time=0.0, loss_history=None,
                 train_accuracy=float('nan')):
        self.class_names = [str(n) for n in class_names]
        self.labels = np.ascontiguousarray(labels, dtype=np.uint8).reshape(-1)
        self.n_features, self.normalize = int(n_features), bool(normalize)
        self.hidden = tuple(int(w) for w in hidden)
        self.weights = [np.ascontiguousarray(w, dtype=np.float32) for w in weights]
        self.biases = [np.ascontiguousarray(b, dtype=np.float32).reshape(-1) for b in biases]
        self.fit_time = float(fit_time)
        self.loss_history = np.zeros(0) if loss_history is None else np.ascontiguousarray(loss_history, dtype=np.float64).reshape(-1)
        self.train_accuracy = float(train_accuracy)
        self._check()

    @property
    def classes(self):
        return int(self.labels.size)

    @property
    def n_params(self):
        return int(sum(w.size for w in self.weights) + sum(b.size for b in self.biases))

    @property
    def final_loss(self):
        return float(self.loss_history[-1]) if self.loss_history.size else float('nan')

    def _check(self):
        c, f, L = self.classes, self.n_features, _lib
        _classify.check_classes(self.class_names, self.labels, L.MLP_MAX_CLASSES)
        _classify.check_f(f)
        if len(self.hidden) > L.MLP_MAX_LAYERS:
            raise ValueError(f'at most {L.MLP_MAX_LAYERS} hidden layers, got {len(self.hidden)}')
        for w in self.hidden:
            if w % 32 or not 32 <= w <= L.MLP_MAX_WIDTH:
                raise ValueError(f'a hidden width must be a multiple of 32 in 32..{L.MLP_MAX_WIDTH}, got {w}')
        dims = (f,) + self.hidden + (c,)
        if len(self.weights) != len(dims) - 1 or len(self.biases) != len(dims) - 1:
            raise ValueError(f'{len(self.hidden)} hidden layers take {len(dims) - 1} weight matrices and biases, got '
                             f'{len(self.weights)} and {len(self.biases)}')
        for i, (w, b) in enumerate(zip(self.weights, self.biases)):
            if w.shape != (dims[i + 1], dims[i]) or b.shape != (dims[i + 1],):
                raise ValueError(f'layer {i}: weight {w.shape} / bias {b.shape} are not [{dims[i + 1]}][{dims[i]}] / [{dims[i + 1]}]')
            if not (np.isfinite(w).all() and np.isfinite(b).all()):
                raise ValueError(f'layer {i}: weights and biases must be finite')
        worst = max(activation_bound(self.weights, self.biases, 65504.0 * np.sqrt(f)))
        if not worst < RANGE_LIMIT:
            raise ValueError(f'the head can reach |activation| = {worst:.3g} on fp16 features: beyond 2^100 fp32 arithmetic is not safe')

    def decide_slab(self, x, want_extra):
        """(labels, the uint8 probabilities [C][n] or None) of the (F, n) matrix x, without voxel norms."""
        return decide(x, self, None, False, want_extra)[::2]


# ---------------------------------------------------------------------------------------------- the fit (fp64, host)
def init_params(dims, rng):
    """nn.Linear's initialisation: U(-1/sqrt(in), 1/sqrt(in)) for the weight, then the bias, layer by layer."""
    weights, biases = [], []
    for i in range(len(dims) - 1):
        k = 1.0 / np.sqrt(dims[i])
        weights.append(rng.uniform(-k, k, size=(dims[i + 1], dims[i])))
        biases.append(rng.uniform(-k, k, size=(dims[i + 1],)))
    return weights, biases


def forward(weights, biases, x):
    """fp64 logits [n][C] of rows x [n][F]; also the inputs of every layer (for the backward pass)."""
    acts = [np.asarray(x, np.float64)]
    for i, (w, b) in enumerate(zip(weights, biases)):
        z = acts[-1] @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if i + 1 < len(weights):
            z = np.maximum(z, 0.0)
        acts.append(z)
    return acts[-1], acts[:-1]


def loss_and_grads(weights, biases, x, targets):
    """(mean softmax cross-entropy, [dW], [db]) for class indices `targets` [n]: the backward pass written out."""
    logits, acts = forward(weights, biases, x)
    n = logits.shape[0]
    z = logits - logits.max(1, keepdims=True)
    lse = np.log(np.exp(z).sum(1, keepdims=True))
    logp = z - lse
    loss = float(-logp[np.arange(n), targets].mean())
    dz = np.exp(logp)
    dz[np.arange(n), targets] -= 1.0
    dz /= n
    gw, gb = [None] * len(weights), [None] * len(weights)
    for i in range(len(weights) - 1, -1, -1):
        gw[i] = dz.T @ acts[i]
        gb[i] = dz.sum(0)
        if i:
            dz = (dz @ np.asarray(weights[i], np.float64)) * (acts[i] > 0)        # acts[i] = relu(z_{i-1})
    return loss, gw, gb


def cosine_lr(lr, epoch, epochs):
    """CosineAnnealingLR(T_max=epochs, eta_min=0) stepped once per epoch, in closed form."""
    return lr * (1.0 + np.cos(np.pi * epoch / epochs)) / 2.0


def adamw_step(params, grads, state, lr, weight_decay):
    """One torch.optim.AdamW step in place on the fp64 arrays `params`; state = {'t': int, 'm': [...], 'v': [...]}."""
    state['t'] += 1
    t = state['t']
    bc1, bc2 = 1.0 - BETAS[0] ** t, 1.0 - BETAS[1] ** t
    for p, g, m, v in zip(params, grads, state['m'], state['v']):
        p *= 1.0 - lr * weight_decay
        m *= BETAS[0]
        m += (1.0 - BETAS[0]) * g
        v *= BETAS[1]
        v += (1.0 - BETAS[1]) * g * g
        p -= (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + EPS)


def new_state(params):
    return {'t': 0, 'm': [np.zeros_like(p) for p in params], 'v': [np.zeros_like(p) for p in params]}


def fit(samples, targets, hidden=(), epochs=100, batch=256, lr=1e-3, weight_decay=1e-2, seed=0, normalize=False, class_names=None):
    """MlpModel trained on samples [n][F] with integer targets [n] (label values 0..255; the classes are their distinct
    values, ascending).  See the module docstring for the recipe.  Deterministic: the same seed and samples give the same
    weights, bit for bit."""
    t0 = time.time()
    hidden = parse_hidden(hidden)
    x = round_samples(samples, normalize).astype(np.float64)
    n, f = x.shape
    if n < 1:
        raise ValueError(f'{_np(targets, np.int64).size} targets for {n} samples')
    values, y, names = _classify.class_table(targets, class_names, n, _lib.MLP_MAX_CLASSES, f)
    c = values.size
    if len(hidden) > _lib.MLP_MAX_LAYERS or any(w % 32 or not 32 <= w <= _lib.MLP_MAX_WIDTH for w in hidden):
        raise ValueError(f'hidden must hold at most {_lib.MLP_MAX_LAYERS} widths, multiples of 32 in 32..{_lib.MLP_MAX_WIDTH}, got {hidden}')
    if not (int(epochs) >= 1 and int(batch) >= 1):
        raise ValueError('epochs and batch must be at least 1')
    if not (lr > 0 and np.isfinite(lr) and weight_decay >= 0 and np.isfinite(weight_decay)):
        raise ValueError('lr must be positive and weight_decay not negative')
    _classify.check_names(names, c)
    rng = np.random.default_rng(seed)
    weights, biases = init_params((f,) + hidden + (c,), rng)
    params = [p for pair in zip(weights, biases) for p in pair]
    state = new_state(params)
    history = []
    for e in range(int(epochs)):
        order = rng.permutation(n)
        step_lr = cosine_lr(lr, e, int(epochs))
        total = 0.0
        for s in range(0, n, int(batch)):
            idx = order[s:s + int(batch)]
            loss, gw, gb = loss_and_grads(weights, biases, x[idx], y[idx])
            total += loss * idx.size
            adamw_step(params, [g for pair in zip(gw, gb) for g in pair], state, step_lr, weight_decay)
        history.append(total / n)
    w32 = [w.astype(np.float32) for w in weights]
    b32 = [b.astype(np.float32) for b in biases]
    acc = float((forward(w32, b32, x)[0].argmax(1) == y).mean())
    return MlpModel(names, values, f, normalize, hidden, w32, b32, fit_time=time.time() - t0, loss_history=history, train_accuracy=acc)


def from_torch(head, labels=None, class_names=None, normalize=False):
    """MlpModel of a head trained elsewhere: an nn.Sequential of Linear / ReLU (Linear, then ReLU + Linear pairs) or its
    state dict ('<i>.weight' / '<i>.bias' in layer order).  Anything else is a ValueError."""
    if isinstance(head, torch.nn.Module):
        mods = list(head.children()) if isinstance(head, torch.nn.Sequential) else [head]
        for i, m in enumerate(mods):
            want = torch.nn.Linear if i % 2 == 0 else torch.nn.ReLU
            if not isinstance(m, want):
                raise ValueError(f'module {i} is a {type(m).__name__}: only Linear (-> ReLU -> Linear)* chains are built')
        if len(mods) % 2 == 0:
            raise ValueError('the chain must end in a Linear')
        lin = mods[0::2]
        if any(m.bias is None for m in lin):
            raise ValueError('every Linear must have a bias')
        weights = [m.weight.detach().cpu().numpy() for m in lin]
        biases = [m.bias.detach().cpu().numpy() for m in lin]
    else:
        sd = dict(head)
        wk = [k for k in sd if k.endswith('weight')]
        if not wk or len(sd) != 2 * len(wk):
            raise ValueError('the state dict must hold one weight and one bias per Linear and nothing else')
        try:
            weights = [torch.as_tensor(sd[k]).detach().cpu().numpy() for k in wk]
            biases = [torch.as_tensor(sd[k[:-len('weight')] + 'bias']).detach().cpu().numpy() for k in wk]
        except KeyError as e:
            raise ValueError(f'the state dict lacks {e}') from None
    if any(w.ndim != 2 for w in weights):
        raise ValueError('every weight must be [out][in]')
    c = weights[-1].shape[0]
    values = np.arange(c) if labels is None else labels
    names = [str(v) for v in np.asarray(values).reshape(-1)] if class_names is None else class_names
    return MlpModel(names, values, weights[0].shape[1], normalize, [w.shape[0] for w in weights[:-1]], weights, biases)


# ---------------------------------------------------------------------------------------------- files
def save_model(model, path):
    """An .npz of plain arrays (no pickled objects): MlpModel.ARRAYS plus weight<i> / bias<i>, format = 'vittf-mlp-1'."""
    arrays = {'format': np.asarray(FORMAT), 'class_names': np.asarray(model.class_names, dtype=np.str_), 'labels': model.labels,
              'n_features': np.asarray(model.n_features, np.int64), 'normalize': np.asarray(model.normalize),
              'hidden': np.asarray(model.hidden, np.int64), 'fit_time': np.asarray(model.fit_time, np.float64),
              'loss_history': model.loss_history, 'train_accuracy': np.asarray(model.train_accuracy, np.float64)}
    for i, (w, b) in enumerate(zip(model.weights, model.biases)):
        arrays[f'weight{i}'], arrays[f'bias{i}'] = w, b
    with open(path, 'wb') as fh:
        np.savez(fh, **arrays)


def is_mlp_file(path):
    """True when `path` is an .npz that names itself an MLP model (the command line picks the classifier of --model by it)."""
    return _classify.file_format(path) == FORMAT


def load_model(path):
    """The MlpModel of a file save_model wrote; ValueError for anything else."""
    with _classify.open_model(path, 'an MLP model', MlpModel.ARRAYS, {}, FORMAT) as z:
        hidden = tuple(int(w) for w in z['hidden'].reshape(-1))
        weights, biases = [], []
        for i in range(len(hidden) + 1):
            if f'weight{i}' not in z.files or f'bias{i}' not in z.files:
                raise ValueError(f'it lacks weight{i} / bias{i}')
            if z[f'weight{i}'].dtype != np.float32 or z[f'bias{i}'].dtype != np.float32 or z[f'weight{i}'].ndim != 2:
                raise ValueError(f'weight{i} / bias{i} are not fp32 [out][in] / [out]')
            weights.append(z[f'weight{i}'])
            biases.append(z[f'bias{i}'])
        if z['labels'].dtype != np.uint8:
            raise ValueError(f"labels is {z['labels'].dtype}, not uint8")
        return MlpModel(_classify.names_of(z), z['labels'], int(z['n_features']), bool(z['normalize']), hidden, weights, biases,
                        float(z['fit_time']), z['loss_history'], float(z['train_accuracy']))


# ---------------------------------------------------------------------------------------------- the GPU pass
def decide(x, model, voxel_norm=None, want_logits=False, want_probs=False):
    """(labels uint8 [nvox], logits fp32 [C][nvox] or None, probs uint8 [C][nvox] or None) on the device for the (F, nvox)
    fp16 device matrix `x`: one vittf_mlp_decide call.  probs = floor(255 softmax + 0.5) of the very logits."""
    lib = _lib.require_device()
    f, nvox = x.shape
    _classify.check_model_f(f, model)
    dev = x.device
    c, layers = model.classes, len(model.hidden)
    labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
    logits = torch.empty((c, nvox), dtype=torch.float32, device=dev) if want_logits else None
    probs = torch.empty((c, nvox), dtype=torch.uint8, device=dev) if want_probs else None
    w = torch.from_numpy(np.concatenate([a.reshape(-1) for a in model.weights])).to(dev)
    b = torch.from_numpy(np.concatenate(model.biases)).to(dev)
    widths = (_lib.C.c_int32 * max(layers, 1))(*model.hidden)
    vn = _classify.norm_argument(voxel_norm, nvox, dev)
    with torch.cuda.device(dev):
        ws_bytes = lib.vittf_mlp_workspace_bytes(f, widths, layers, c)
        if ws_bytes == 0:
            raise ValueError(f'vittf_mlp_decide refuses F = {f}, hidden {model.hidden}, {c} classes')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.vittf_mlp_decide(_lib.ptr(x), f, nvox, _lib.ptr(w), _lib.ptr(b), widths, layers, c, _lib.ptr(vn), _lib.ptr(labels),
                                        _lib.ptr(logits), _lib.ptr(probs), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()), 'vittf_mlp_decide')
    return labels, logits, probs


def predict(feat, model, return_probs=False):
    """uint8 device tensor with the voxel shape of `feat` (F, W', H', D'): the class INDEX 0..C-1 of every voxel
    (model.labels[index] is the value a label volume carries); with return_probs also the uint8 [C] + voxel shape softmax
    maps.  A model fitted with `normalize` has the voxels divided by their norms (vt.similarity.voxel_norms)."""
    return _classify.predict_volume(feat, model, lambda x, m, vn: decide(x, m, vn, False, return_probs)[::2], model.normalize)
