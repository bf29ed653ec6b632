"""Writes tests/golden/voxel_features.npz by RUNNING the reference's own ``compose_features`` (predict_svm_rf.py:53-65) on two
small volumes, so that the hand-crafted channels are pinned against the reference where it is absent.

    python tests/golden/make_golden_voxel_features.py [REFERENCE_DIR]       # default /root/reference

The function is imported from the reference as it is, never copied.  Its module imports packages that only its command line
uses (matplotlib, scikit-learn's classifiers and metrics, icecream through infer.py): where one is absent an empty stand-in
module is registered first -- none of them takes part in compose_features.  torch runs on one thread, so that regenerating
gives the same bytes.  The file holds arrays only: the input volumes (tests/voxel_features_data.py's, fp32) and the fp32
outputs [11][n0][n1][n2] for (12, 10, 14) uniform and (9, 17, 5) CT.
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import voxel_features_data as vd   # noqa: E402

CASES = (('uniform', (12, 10, 14)), ('ct', (9, 17, 5)))


class _Anything(types.ModuleType):
    """A stand-in for a package the reference imports at module level and compose_features never touches."""
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return _Anything(f'{self.__name__}.{name}')

    def __call__(self, *a, **k):
        return None


def reference_compose(ref_dir):
    sys.path.insert(0, ref_dir)
    for name in ('matplotlib', 'matplotlib.pyplot', 'sklearn', 'sklearn.svm', 'sklearn.ensemble', 'sklearn.metrics', 'icecream',
                 'torchvision', 'torchvision.transforms', 'torchvision.transforms.functional'):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Anything(name)
    return importlib.import_module('predict_svm_rf').compose_features


def main():
    ref_dir = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    torch.set_num_threads(1)
    compose = reference_compose(ref_dir)
    out = {}
    for content, shape in CASES:
        vol = vd.uniform_volume(shape) if content == 'uniform' else vd.ct_volume(shape)
        with contextlib.redirect_stdout(io.StringIO()):                  # (the function prints its statistics)
            feat = compose(torch.from_numpy(vol.astype(np.float32)))
        assert feat.dtype == torch.float32 and tuple(feat.shape) == (11,) + shape
        out[f'{content}_volume'] = vol
        out[f'{content}_features'] = feat.numpy()
    path = os.path.join(HERE, 'voxel_features.npz')
    with open(path, 'wb') as fh:
        np.savez(fh, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
