#!/usr/bin/env python3
"""Time the Euclidean distance transform (vittf_edt_sq, vittf_edt_sq_weighted) and a whole surface_scores call beside
scipy.ndimage.distance_transform_edt on the host (one GPU).

    python tools/distance_step.py [--sizes 256 512] [--steps 10] [--warmup 3] [--scipy-max 512]
                                  [--out profiles/distance_kernels.json]

For every size n two uint8 n^3 masks: a sparse one (five spheres; the sites are the voxels of the spheres) and a dense random
one (Bernoulli 0.5).  For each, the raw integer and weighted calls (spacing 0.7, 0.7, 2.5) on preallocated buffers, with and
without the feature transform -- the median over --steps of one HIP event pair around one call (its three launches), after
--warmup calls -- the device time per kernel name from torch.profiler (left out with the reason when the profiler is not
available), the bytes each variant moves per voxel and what that is against the achievable HBM rate (6.29 TB/s, the measured
float4 copy), and scipy.ndimage.distance_transform_edt on the same mask on the host (one run, sizes up to --scipy-max); the
integer result is checked against scipy's.  Then one whole vt.distance.surface_scores call for 6 classes on a pair of label
volumes of nested and shifted spheres.  Prints one JSON line and writes it to --out.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.pca_step import timed          # noqa: E402

KERNELS = ('edt_row_kernel', 'edt_line_kernel')
HBM_GB_S = 6290.0
# bytes per voxel: row pass (1 read + value write [+ site write]), axis 1 (value read + write [+ site read + write]), axis 0
BYTES = {('integer', False): (1 + 4) + (4 + 4) + (4 + 4), ('integer', True): (1 + 4 + 4) + (4 + 4 + 8) + (4 + 4 + 8),
         ('weighted', False): (1 + 8) + (8 + 8) + (8 + 4), ('weighted', True): (1 + 8 + 4) + (8 + 8 + 8) + (8 + 4 + 8)}
SPACING = (0.7, 0.7, 2.5)


def kernel_totals(fn):
    """{kernel: [launches, device microseconds in all]} of the transform's kernels inside one fn() call."""
    import torch
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        for k in KERNELS:
            if k in ev.key:
                us = getattr(ev, 'device_time_total', None)
                n, t = out.get(k, (0, 0.0))
                out[k] = (n + ev.count, round(t + float(us if us is not None else ev.cuda_time_total), 2))
    if not out:
        raise RuntimeError('the profiler recorded none of the distance kernels')
    return out


def spheres(n, dev, count=5, seed=0):
    import torch
    g = torch.Generator().manual_seed(seed)
    ax = torch.arange(n, device=dev, dtype=torch.float32)
    vol = torch.zeros((n, n, n), dtype=torch.uint8, device=dev)
    for _ in range(count):
        c = (torch.rand(3, generator=g) * n).tolist()
        r = float(torch.rand(1, generator=g)) * n / 10 + n / 20
        vol |= (((ax[:, None, None] - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[None, None, :] - c[2]) ** 2) <= r * r).to(torch.uint8)
    return vol


def label_pair(n, dev, classes=6):
    """Two uint8 n^3 label volumes with `classes` spherical bodies each, the second set shifted and resized a little."""
    import torch
    ax = torch.arange(n, device=dev, dtype=torch.float32)
    out = []
    for shift, grow in ((0.0, 1.0), (n / 64, 0.93)):
        vol = torch.zeros((n, n, n), dtype=torch.uint8, device=dev)
        for c in range(classes):
            ctr = [n * (0.25 + 0.5 * ((c >> a) & 1)) + shift for a in range(3)]
            r = n * (0.10 + 0.015 * c) * grow
            vol[((ax[:, None, None] - ctr[0]) ** 2 + (ax[None, :, None] - ctr[1]) ** 2 + (ax[None, None, :] - ctr[2]) ** 2) <= r * r] = c + 1
        out.append(vol)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--scipy-max', type=int, default=512, help='largest size at which scipy runs on the host')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'distance_kernels.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from scipy import ndimage
    import vit_tf_amd as vt
    from vit_tf_amd import _lib
    from bench import host_cores
    torch.set_num_threads(host_cores())
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lib = _lib.require_device()
    line = {'tool': 'distance_step', 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
            'spacing': list(SPACING), 'hbm_gb_per_s': HBM_GB_S, 'scipy': 'scipy.ndimage.distance_transform_edt on the host, one thread',
            'volumes': {}}
    t = lambda fn: timed(fn, args.steps, args.warmup)          # noqa: E731
    w2 = (ctypes.c_double * 3)(*(s * s for s in SPACING))
    for n in args.sizes:
        inputs = {'spheres': spheres(n, dev),
                  'random_p0.5': (torch.rand((n, n, n), generator=torch.Generator(device=dev).manual_seed(0), device=dev) < 0.5).to(torch.uint8)}
        res = {}
        for name, src in inputs.items():
            nvox = src.numel()
            r = {'sites': round(float((src != 0).float().mean()), 4)}
            d2i = torch.empty((n, n, n), dtype=torch.int32, device=dev)
            d2f = torch.empty((n, n, n), dtype=torch.float32, device=dev)
            site = torch.empty((n, n, n), dtype=torch.int32, device=dev)
            ws_bytes = lib.vittf_edt_workspace_bytes(n, n, n)
            ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
            calls = {
                ('integer', False): lambda: _lib.check(lib.vittf_edt_sq(_lib.ptr(src), n, n, n, -1, 0, _lib.ptr(d2i), None, _lib.ptr(ws), ws_bytes, _lib.stream_ptr())),
                ('integer', True): lambda: _lib.check(lib.vittf_edt_sq(_lib.ptr(src), n, n, n, -1, 0, _lib.ptr(d2i), _lib.ptr(site), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())),
                ('weighted', False): lambda: _lib.check(lib.vittf_edt_sq_weighted(_lib.ptr(src), n, n, n, -1, 0, w2, _lib.ptr(d2f), None, _lib.ptr(ws), ws_bytes, _lib.stream_ptr())),
                ('weighted', True): lambda: _lib.check(lib.vittf_edt_sq_weighted(_lib.ptr(src), n, n, n, -1, 0, w2, _lib.ptr(d2f), _lib.ptr(site), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())),
            }
            for (path, sites), fn in calls.items():
                key = path + ('_sites' if sites else '')
                ms, every = t(fn)
                q = {'ms': ms, 'ms_all': every, 'bytes_per_voxel': BYTES[path, sites]}
                q['gb_per_s'] = round(BYTES[path, sites] * nvox / ms / 1e6, 1)
                q['share_of_hbm_rate'] = round(q['gb_per_s'] / HBM_GB_S, 4)
                try:
                    q['kernel_launches_us'] = {k: list(v) for k, v in kernel_totals(fn).items()}
                except Exception as e:                          # noqa: BLE001  (the figure is optional, the reason is recorded)
                    q['kernel_launches_us'] = None
                    q['kernel_launches_us_skipped'] = f'{type(e).__name__}: {e}'
                r[key] = q
            r['edt_call_ms'], r['edt_call_ms_all'] = t(lambda: vt.distance.edt(src))      # allocations and the square root included
            calls['integer', False]()
            torch.cuda.synchronize()
            if n <= args.scipy_max:
                host = src.cpu().numpy()
                t0 = time.perf_counter()
                ref = ndimage.distance_transform_edt(host == 0)
                r['scipy_edt_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
                r['speedup_vs_scipy'] = round(r['scipy_edt_ms'] / r['edt_call_ms'], 1)
                r['integer_equals_scipy'] = bool(np.array_equal(d2i.cpu().numpy(), np.rint(ref * ref).astype(np.int64)))
                del host, ref
            res[name] = r
            print(f'{n}^3 {name}: ' + json.dumps({k: v for k, v in r.items() if not k.endswith('_all')}), file=sys.stderr, flush=True)
            del d2i, d2f, site, ws
            torch.cuda.empty_cache()
        target, pred = label_pair(n, dev)
        for spacing, key in ((None, 'surface_scores_6_classes'), (SPACING, 'surface_scores_6_classes_spacing')):
            times = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s = vt.distance.surface_scores(target, pred, range(1, 7), spacing)
                times.append((time.perf_counter() - t0) * 1e3)
            res[key] = {'wall_ms': round(sorted(times)[1], 1), 'wall_ms_all': [round(x, 1) for x in times],
                        'hd': [round(float(x), 3) for x in s['hd']], 'n_surface_target': s['n_surface_target'].tolist()}
        print(f'{n}^3 surface_scores: ' + json.dumps(res['surface_scores_6_classes']), file=sys.stderr, flush=True)
        line['volumes'][f'{n}^3'] = res
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
