#!/usr/bin/env python3
"""Time the volume renderer (vittf_render_prepare, vittf_render_occupancy, vittf_render) beside a stock-PyTorch grid_sample
marcher doing the same frame (one GPU).

    python tools/render_step.py [--sizes 256 512] [--image 1024] [--steps 10] [--warmup 3] [--stock-steps 3]
                                [--out profiles/render_kernels.json] [--pmc-frames VARIANT]

For every size n the synthetic CT-like n^3 volume of vt.synthetic.ct_like_volume with its labels 1..3 as one-hot class maps on
a 64^3 grid, an orthographic camera at azimuth 30 and elevation 20, a square frame, dt = 0.5 voxels, the faint context table
and the default class strengths.  Timed: vittf_render with and without shading, with and without the occupancy grid;
vittf_render_prepare and vittf_render_occupancy on their own -- the median over --steps of one HIP event pair around one call
after --warmup calls, on preallocated buffers.  Then the same frame without shading from ``stock_frame``: torch.nn.functional.
grid_sample over chunks of sample planes, a table gather, and a cumulative product for the transmittance (no early stop and no
skipping: stock PyTorch has neither), --stock-steps event pairs after one warm-up; its image is compared with the kernel's.
Also recorded: the lattice samples inside the grown box (what a marcher without grid and stop visits), the share of empty
bricks, and the bytes a sample asks for (16 for the intensity corners, 8 per class map, 48 more with shading).  Prints one
JSON line and writes it to --out.  With --pmc-frames it renders three frames of one variant per size and stops, without a
file: the workload of ``rocprofv3 --kernel-trace --pmc FETCH_SIZE -- python tools/render_step.py --sizes 512 --pmc-frames
flat_no_grid`` (counters in a run of their own).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.pca_step import timed          # noqa: E402

MAP_GRID = 64
CHUNK = 8                                  # sample planes per grid_sample call of the stock marcher


def ray_setup(cam, size, shape, spacing, dt, dev):
    """Origins and unit directions (h, w, 3) and the first and last lattice index of every ray (first > last: a miss), in torch
    on the device, by the rules of include/vittf.h."""
    import torch
    w, h = size
    v6 = torch.as_tensor(cam.vectors(), device=dev)
    u = (2 * (torch.arange(w, device=dev, dtype=torch.float32) + 0.5) / w - 1).view(1, w, 1)
    v = (1 - 2 * (torch.arange(h, device=dev, dtype=torch.float32) + 0.5) / h).view(h, 1, 1)
    o = v6[0] + u * v6[1] + v * v6[2]
    d = v6[3] + u * v6[4] + v * v6[5]
    d = d / d.norm(dim=-1, keepdim=True)
    sp = torch.tensor(spacing, device=dev, dtype=torch.float32)
    n = torch.tensor(shape, device=dev, dtype=torch.float32)
    lo, hi = -0.5 * sp, (n + 0.5) * sp
    par = d == 0
    safe = torch.where(par, torch.ones_like(d), d)
    t1, t2 = (lo - o) / safe, (hi - o) / safe
    inf = torch.full_like(d, float('inf'))
    tmin = torch.where(par, -inf, torch.minimum(t1, t2)).amax(-1).clamp_min(0)
    tmax = torch.where(par, inf, torch.maximum(t1, t2)).amin(-1)
    hit = (tmin <= tmax) & (~par | ((o >= lo) & (o <= hi))).all(-1)
    first = torch.where(hit, torch.ceil(tmin / dt - 0.5).clamp_min(0), torch.ones_like(tmin)).long()
    last = torch.where(hit, torch.floor(tmax / dt - 0.5), torch.zeros_like(tmax)).long()
    return o, d, first, last


def stock_frame(vol, maps, table, o, d, first, last, spacing, dt, lo, hi, rgbs):
    """Premultiplied (h, w, 4) of the model without shading in stock PyTorch.  vol (1, 1, n0, n1, n2) fp32 holding q, maps
    (1, C, m0, m1, m2) fp32 levels, table (256, 4); o, d, first, last of ray_setup."""
    import torch
    import torch.nn.functional as F
    dev = vol.device
    h, w = o.shape[:2]
    n = torch.tensor(vol.shape[2:], device=dev, dtype=torch.float32)
    sp = torch.tensor(spacing, device=dev, dtype=torch.float32)
    alive = first <= last
    i_lo, i_hi = int(first[alive].min()), int(last[alive].max())
    rgb = torch.zeros((h, w, 3), device=dev)
    alpha = torch.zeros((h, w), device=dev)
    trans = torch.ones((h, w), device=dev)
    lo_t = torch.tensor(lo, device=dev, dtype=torch.float32).view(-1, 1, 1, 1)
    range_t = torch.tensor([b - a for a, b in zip(lo, hi)], device=dev, dtype=torch.float32).view(-1, 1, 1, 1)
    col = torch.as_tensor(rgbs, device=dev)[:, :3]
    strength = torch.as_tensor(rgbs, device=dev)[:, 3].view(-1, 1, 1, 1)
    for start in range(i_lo, i_hi + 1, CHUNK):
        idx = torch.arange(start, min(start + CHUNK, i_hi + 1), device=dev)
        t = ((idx.float() + 0.5) * dt).view(-1, 1, 1, 1)
        p = o[None] + t * d[None]                                                   # (S, h, w, 3)
        on = ((idx.view(-1, 1, 1) >= first[None]) & (idx.view(-1, 1, 1) <= last[None])).float()
        x = p / sp - 0.5
        cov = torch.minimum(x + 1, n - x).clamp(0, 1).prod(-1) * on
        grid = (2 * p / (n * sp) - 1).flip(-1)[None]                                # grid_sample wants (x, y, z) = axes (2, 1, 0)
        inten = F.grid_sample(vol, grid, mode='bilinear', padding_mode='border', align_corners=False)[0, 0]
        tc = inten / 257.0
        ti = tc.floor().clamp(0, 254).long()
        entry = torch.lerp(table[ti], table[ti + 1], (tc - ti)[..., None])          # (S, h, w, 4)
        sigma = entry[..., 3] * cov
        colour = sigma[..., None] * entry[..., :3]
        if maps is not None:
            val = F.grid_sample(maps, grid, mode='bilinear', padding_mode='border', align_corners=False)[0]       # (C, S, h, w)
            sk = strength * ((val - lo_t) / range_t).clamp(0, 1) * cov[None]
            sigma = sigma + sk.sum(0)
            colour = colour + torch.einsum('cshw,ck->shwk', sk, col)
        a = 1 - torch.exp(-sigma * dt)
        through = torch.cumprod(1 - a, 0)
        before = trans[None] * torch.cat([torch.ones_like(through[:1]), through[:-1]])
        wgt = before * a / sigma.clamp_min(1e-30)
        rgb += (wgt[..., None] * colour).sum(0)
        alpha += (before * a).sum(0)
        trans = trans * through[-1]
    return torch.cat([rgb, alpha[..., None]], -1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--image', type=int, default=1024)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--stock-steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render_kernels.json'))
    ap.add_argument('--pmc-frames', default=None, choices=['flat_grid', 'flat_no_grid', 'shaded_grid', 'shaded_no_grid'],
                    help='render three frames of this variant per size and stop: the workload of a rocprofv3 --pmc pass')
    args = ap.parse_args()
    import torch
    import vit_tf_amd as vt
    from vit_tf_amd import _lib
    from bench import host_cores
    torch.set_num_threads(host_cores())
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lib = _lib.require_device()
    render = vt.render
    size, dt, spacing, lo, hi = (args.image, args.image), 0.5, (1.0, 1.0, 1.0), [64] * 3, [192] * 3
    line = {'tool': 'render_step', 'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
            'stock_steps': args.stock_steps, 'image': list(size), 'dt': dt, 'classes': 3, 'map_grid': [MAP_GRID] * 3,
            'camera': 'orthographic, azimuth 30, elevation 20', 'bytes_asked_per_sample': {'intensity': 16, 'per_class_map': 8, 'shading': 48},
            'stock': f'torch.nn.functional.grid_sample marcher, {CHUNK} sample planes a call, no shading, no early stop', 'volumes': {}}
    t = lambda fn: timed(fn, args.steps, args.warmup)          # noqa: E731
    table = torch.as_tensor(render.context_table(), device=dev)
    strengths = [float(render.sigma_from_opacity(0.9, 4.0))] * 3
    rgbs = [list(c) + [s] for c, s in zip(render.PALETTE[:3], strengths)]
    for n in args.sizes:
        vol16, labels = vt.synthetic.ct_like_volume(n)
        vol = vol16.float().to(dev)
        small = vt.scores.resize_nearest_u8(labels, (MAP_GRID,) * 3)
        maps = render.maps_from_labels(torch.as_tensor(small).to(dev), [1, 2, 3]).contiguous()
        cam = render.Camera.orbit(30, 20, shape=(n, n, n), spacing=spacing)
        r = {}
        vmin, vmax = float(vol.min()), float(vol.max())
        q = torch.empty((n, n, n), dtype=torch.uint16, device=dev)
        r['prepare_ms'], r['prepare_ms_all'] = t(lambda: _lib.check(lib.vittf_render_prepare(_lib.ptr(vol), vol.numel(), vmin, vmax, _lib.ptr(q), _lib.stream_ptr())))
        r['prepare_gb_per_s'] = round(6 * vol.numel() / r['prepare_ms'] / 1e6, 1)
        r['occupancy_ms'], r['occupancy_ms_all'] = t(lambda: render.occupancy(q, table, maps, lo))
        occ = render.occupancy(q, table, maps, lo)
        r['bricks'], r['empty_bricks_share'] = occ.numel(), round(float((occ == 0).float().mean()), 4)
        o, d, first, last = ray_setup(cam, size, (n, n, n), spacing, dt, dev)
        r['lattice_samples_in_box'] = int((last - first + 1).clamp_min(0).sum())
        out = torch.empty((size[1], size[0], 4), device=dev)
        if args.pmc_frames:                                  # three frames of one variant and nothing else: a counter pass
            skey, gkey = args.pmc_frames.split('_', 1)
            for _ in range(3):
                render.render(q, cam, size, spacing=spacing, table=table, maps=maps, lo=lo, hi=hi, step=dt,
                              shading=render.SHADING if skey == 'shaded' else None, occupancy=occ if gkey == 'grid' else None, out=out)
            torch.cuda.synchronize()
            print(f'{n}^3 {args.pmc_frames}: 3 frames, {r["lattice_samples_in_box"]} lattice samples in the box each')
            continue
        images = {}
        for shading, skey in ((render.SHADING, 'shaded'), (None, 'flat')):
            for grid, gkey in ((occ, 'grid'), (None, 'no_grid')):
                fn = lambda: render.render(q, cam, size, spacing=spacing, table=table, maps=maps, lo=lo, hi=hi, step=dt,      # noqa: E731
                                           shading=shading, occupancy=grid, out=out)
                ms, every = t(fn)
                r[f'render_{skey}_{gkey}_ms'], r[f'render_{skey}_{gkey}_ms_all'] = ms, every
                r[f'render_{skey}_{gkey}_ns_per_lattice_sample'] = round(ms * 1e6 / r['lattice_samples_in_box'], 4)
                images[skey, gkey] = out.clone()
            r[f'render_{skey}_same_bytes_with_and_without_grid'] = bool(torch.equal(images[skey, 'grid'], images[skey, 'no_grid']))
        volf = q.float()[None, None]
        mapsf = maps.float()[None]
        stock = lambda: stock_frame(volf, mapsf, table, o, d, first, last, spacing, dt, lo, hi, rgbs)          # noqa: E731
        r['stock_flat_ms'], r['stock_flat_ms_all'] = timed(stock, args.stock_steps, 1)
        diff = (stock() - images['flat', 'grid']).abs().max()
        r['stock_vs_kernel_max_abs'] = float(diff)
        r['kernel_over_stock_speedup_flat_grid'] = round(r['stock_flat_ms'] / r['render_flat_grid_ms'], 1)
        r['kernel_over_stock_speedup_flat_no_grid'] = round(r['stock_flat_ms'] / r['render_flat_no_grid_ms'], 1)
        print(f'{n}^3: ' + json.dumps({k: v for k, v in r.items() if not k.endswith('_all')}), file=sys.stderr, flush=True)
        line['volumes'][f'{n}^3'] = r
        del vol, q, volf, mapsf, out, images, occ
        torch.cuda.empty_cache()
    if args.pmc_frames:
        return
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
