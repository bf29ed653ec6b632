#!/usr/bin/env python3
"""Time the connected-component kernels (vittf_label_components, vittf_component_sizes, vittf_filter_components) beside
scipy.ndimage.label on the host (one GPU).

    python tools/components_step.py [--sizes 256 512] [--steps 10] [--warmup 3] [--no-similarity]
                                    [--out profiles/components_kernels.json]

For every size n three uint8 n^3 inputs: the label volume of vt.ct_like_volume(n) (three nested bodies), Bernoulli noise at
p = 0.31 (the 6-neighbour percolation threshold: components snake through many tiles) and one thresholded similarity map of
the benchmark query (bench.py's 512^3 workload and 16 query voxels, `map > 69` as the reference script; 256^3 as it comes, 512^3
through the nearest up-sample the predictions take).  For every input, at connectivity 1: the whole vt.components.label call
(allocations included), the raw vittf_label_components call (its three launches: tile, seam, flatten), vittf_component_sizes
(memset + kernel) and vittf_filter_components on preallocated buffers -- the median over --steps of one HIP event pair around
one call, after --warmup calls -- then the share of every kernel of one label + sizes call from torch.profiler (device time per
kernel name; left out with the reason when the profiler is not available), and scipy.ndimage.label on the same array on the
host (best of two).  The labels are checked against scipy's on every input.  Prints one JSON line and writes it to --out.
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

KERNELS = ('cc_tile_kernel', 'cc_seam_kernel', 'cc_flatten_kernel', 'cc_sizes_kernel')


def kernel_split(fn):
    """{kernel: device microseconds} of the component kernels inside one fn() call, from torch.profiler."""
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
                out[k] = round(float(us if us is not None else ev.cuda_time_total) / max(1, ev.count), 2)
    if not out:
        raise RuntimeError('the profiler recorded none of the component kernels')
    return out


def similarity_set(vt, dev):
    """uint8 256^3 0/1 volume: the first class map of the benchmark's 512^3 query, thresholded like the reference script."""
    import torch
    import bench
    vol, label, _ = bench.make_workload('512', vt)
    model = vt.HipViT(vt.synthetic_state_dict('vits8', 0), 'vits8', 'fp16', device=dev)
    dvol = vt.DeviceVolume(vol, dev)
    feats = vt.feature_volume(None, model, bench.FOS, 'all', dvol=dvol)
    sims = vt.compute_similarities(vol, feats, bench.query_voxels(label), keep_on_device=True)
    out = (next(iter(sims.values())) > 69).to(torch.uint8)
    del model, dvol, feats, sims
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-similarity', action='store_true', help='leave the similarity-map input out (no ViT pass)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'components_kernels.json'))
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
    cc = vt.components
    line = {'tool': 'components_step', 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
            'tile': list(_lib.CC_TILE), 'connectivity': 1, 'scipy': 'scipy.ndimage.label on the host, one thread', 'volumes': {}}
    t = lambda fn: timed(fn, args.steps, args.warmup)          # noqa: E731
    sim256 = None
    if not args.no_similarity:
        try:
            sim256 = similarity_set(vt, dev)
        except Exception as e:                                  # noqa: BLE001  (the figure is optional, the reason is recorded)
            line['similarity_input_skipped'] = f'{type(e).__name__}: {e}'
    for n in args.sizes:
        inputs = {'ct_like_labels': vt.ct_like_volume(n, 0)[1].to(dev),
                  'noise_p0.31': (torch.rand((n, n, n), generator=torch.Generator(device=dev).manual_seed(0), device=dev) < 0.31).to(torch.uint8)}
        if sim256 is not None:
            inputs['similarity_gt69'] = sim256 if n == 256 else vt.scores.resize_nearest_u8(sim256, (n, n, n), keep_on_device=True)
        res = {}
        for name, src in inputs.items():
            src = torch.as_tensor(src).to(dev).contiguous()
            nvox = src.numel()
            r = {'foreground': round(float((src != 0).float().mean()), 4)}
            labels = torch.empty((n, n, n), dtype=torch.int32, device=dev)
            sizes = torch.empty((nvox,), dtype=torch.int32, device=dev)
            dst = torch.empty_like(src)
            ws_bytes = lib.vittf_components_workspace_bytes(n, n, n)
            ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
            raw_label = lambda: _lib.check(lib.vittf_label_components(_lib.ptr(src), n, n, n, -1, 1, _lib.ptr(labels), _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))   # noqa: E731
            raw_sizes = lambda: _lib.check(lib.vittf_component_sizes(_lib.ptr(labels), nvox, _lib.ptr(sizes), _lib.stream_ptr()))   # noqa: E731
            r['label_call_ms'], r['label_call_ms_all'] = t(lambda: cc.label(src, -1, 1))
            r['label_kernels_ms'], r['label_kernels_ms_all'] = t(raw_label)
            r['sizes_ms'], r['sizes_ms_all'] = t(raw_sizes)
            r['filter_ms'], r['filter_ms_all'] = t(lambda: _lib.check(lib.vittf_filter_components(
                _lib.ptr(src), _lib.ptr(labels), _lib.ptr(sizes), nvox, 100, 0, 0, _lib.ptr(dst), _lib.stream_ptr())))
            r['label_bytes_per_voxel_at_hbm_floor'] = 14
            r['label_gb_per_s_at_14_bytes'] = round(14 * nvox / r['label_kernels_ms'] / 1e6, 1)
            try:
                r['kernel_us'] = kernel_split(lambda: (raw_label(), raw_sizes()))
            except Exception as e:                              # noqa: BLE001
                r['kernel_us'] = None
                r['kernel_us_skipped'] = f'{type(e).__name__}: {e}'
            torch.cuda.synchronize()
            host = src.cpu().numpy()
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                ref, ncomp = ndimage.label(host)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            r['scipy_label_ms'] = round(best * 1e3, 1)
            r['components'] = int(ncomp)
            r['speedup_vs_scipy'] = round(r['scipy_label_ms'] / r['label_call_ms'], 1)
            got = labels.cpu().numpy()
            flat = ref.reshape(-1)
            comps, first = np.unique(flat, return_index=True)
            lut = np.zeros(ncomp + 1, np.int64)
            lut[comps] = first + 1
            lut[0] = 0
            r['labels_equal_scipy'] = bool(np.array_equal(got.reshape(-1), lut[flat]))
            r['sizes_equal_bincount'] = bool(np.array_equal(sizes.cpu().numpy(), np.bincount(got.reshape(-1), minlength=nvox + 1)[1:]))
            r['largest'] = int(sizes.max())
            res[name] = r
            print(f'{n}^3 {name}: ' + json.dumps({k: v for k, v in r.items() if not k.endswith('_all')}), file=sys.stderr, flush=True)
            del labels, sizes, dst, ws, got, ref, flat, host
            torch.cuda.empty_cache()
        line['volumes'][f'{n}^3'] = res
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
