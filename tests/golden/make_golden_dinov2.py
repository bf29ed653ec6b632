#!/usr/bin/env python3
"""Generate tests/golden/dinov2_*.npz by RUNNING THE REFERENCE's own ``compute_qkv`` with patch 14 (DINOv2).

    python tests/golden/make_golden_dinov2.py     # needs the reference checkout (see make_golden.py)

The reference's Python API takes any model with the DINO module tree: ``compute_qkv(vol, model, patch_size=14, ...)`` hooks
``blocks[-1].attn.qkv`` and reads ``blocks[-1].attn.num_heads`` (its CLI branch for DINOv2 is dead code, but the harness is
patch-agnostic).  The model is tests/dinov2_ref.py's restatement (explicit LayerScale) with seeded synthetic weights, which
are regenerated from their seed by the tests, not stored.  The reference is imported exactly as make_golden.py imports it
(load_reference / quiet are reused).  Only inputs and expected outputs are stored.

Two archs: (128, 3, 2, 14) and (384, 2, 6, 14) -- the second reaches the ViT-S kernels (block tail, activation-stationary
qkv GEMM, the patch-14 matrix-core embedding).  One volume, (15, 30, 24) at feature_output_size 3, image sizes
(14, 42, 42): dim 0 is resized down (15 -> 14), dims 1 and 2 up (30 -> 42, 24 -> 42); token grids 1 x 3, 1 x 3
and 3 x 3 (f0 != f1); the x axis is one call of 15 slices x 10 tokens = 150 rows (> 128).  Stored: k of every axis, the
pooled 'all' volume of the reference's __main__ loop, and q / k / v of the z axis from one compute_qkv call.
"""
import os
import sys
from collections import defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import REF, check_close, load_reference, quiet   # noqa: E402
from oracle import feature_volume as ofv   # noqa: E402
import dinov2_ref   # noqa: E402
import vit_tf_amd as vt   # noqa: E402  (weights recipe only; no GPU involved)

PATCH = 14
CASES = {
    # name: (arch, weight seed)
    'dinov2_d128': ((128, 3, 2, PATCH), 31),
    'dinov2_d384': ((384, 2, 6, PATCH), 32),
}
VOL_SHAPE, FOS, VOL_SEED = (15, 30, 24), 3, 140


def synthetic_dinov2(arch, seed):
    """The fixtures' weights: the synthetic recipe with the DINOv2 keys (stored grid 37, LayerScale gammas, mask_token)."""
    return vt.synthetic_state_dict(arch, seed, stored_grid=vt.weights.DINOV2_STORED_GRID, layer_scale=True)


def fixture_volume():
    g = torch.Generator().manual_seed(VOL_SEED)
    return (torch.rand(VOL_SHAPE, generator=g) * 3.0 - 1.0).half().float()       # fp16-exact values


def case(ref_infer, arch, seed):
    vol = fixture_volume()
    im_sz, feat_out = ofv.sizing(VOL_SHAPE, FOS, PATCH)
    rec = {'vol': vol.numpy(), 'fos': FOS, 'seed': seed, 'arch': np.array(arch), 'im_sz': np.array(im_sz),
           'feat_out': np.array(feat_out)}

    def fresh():      # a fresh model per call: the reference never removes its hook
        sd = synthetic_dinov2(arch, seed)
        return dinov2_ref.build_dinov2(arch, sd), sd

    for ax in 'zyx':
        model, sd = fresh()
        res = quiet(ref_infer.compute_qkv, vol, model, PATCH, im_sz, batch_size=4, slice_along=ax, return_keys='k')
        rec[f'k_{ax}'] = res['k'].numpy()
        check_close(f'{arch}/k_{ax}', ofv.k_features_axis(vol, model, PATCH, im_sz, ax, batch_size=4), res['k'])
    rec['weights_checksum'] = vt.weights.state_dict_checksum(sd)
    model, _ = fresh()
    qkv = quiet(ref_infer.compute_qkv, vol, model, PATCH, im_sz, batch_size=5, slice_along='z', return_keys=['q', 'k', 'v'])
    for key in 'qv':
        rec[f'{key}_z'] = qkv[key].numpy()
    assert np.array_equal(qkv['k'].numpy(), rec['k_z'])
    # the reference's 'all' mode loop (infer.py __main__)
    acc = defaultdict(float)
    pool = torch.nn.AdaptiveAvgPool3d(output_size=feat_out)
    for ax in ['z', 'y', 'x']:
        model, _ = fresh()
        for k, v in quiet(ref_infer.compute_qkv, vol, model, PATCH, im_sz, pool_fn=pool, batch_size=2, return_keys='k',
                          slice_along=ax).items():
            acc[k] = (torch.as_tensor(acc[k]) + v.squeeze().half())
    rec['k_all'] = acc['k'].numpy()
    model, _ = fresh()
    check_close(f'{arch}/k_all', ofv.feature_volume(vol, model, PATCH, FOS, 'all', batch_size=2), acc['k'])
    return rec


def main():
    if not os.path.isdir(REF):
        raise SystemExit('make_golden_dinov2.py needs the reference checkout (see make_golden.py)')
    torch.manual_seed(0)
    torch.set_num_threads(4)
    ref_infer, _, _ = load_reference()
    for name, (arch, seed) in CASES.items():
        print(f'{name}: reference compute_qkv, patch {PATCH}, arch {arch}')
        path = os.path.join(HERE, f'{name}.npz')
        np.savez_compressed(path, **case(ref_infer, arch, seed))
        print(f'  {name}.npz: {os.path.getsize(path) / 1024:.0f} KiB')


if __name__ == '__main__':
    main()
