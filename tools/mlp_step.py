#!/usr/bin/env python3
"""Time the MLP-head decision entry (vittf_mlp_decide) beside stock PyTorch-ROCm doing the same work (one GPU).

    python tools/mlp_step.py [--sizes 64 128] [--features 384] [--classes 6] [--steps 10] [--warmup 3]
                             [--out profiles/mlp_kernels.json]

For every size n a synthetic n^3 x F fp16 feature volume (tools/pca_step.py's), and for the heads (), (64,), (256,) and
(256, 256) with nn.Linear's initialisation: the raw vittf_mlp_decide call (all three launches: scales, weight images,
decision) on preallocated buffers -- labels only, with the uint8 probabilities, with the fp32 logits -- and the same head in
stock PyTorch on the same GPU, chunked over the voxels: ``head(feat[:, chunk].T.float())``, softmax, arg-max (the chunk keeps
the fp32 copy of the voxels at 256 Ki rows instead of the whole volume).  Also 64^3 x 32 (a ``_pca32`` file).  Every figure
is the median over --steps of one HIP event pair around one call, after --warmup calls; nothing else runs on the GPU
meanwhile.  ``labels_differing_from_stock`` counts the voxels whose label differs from the stock head's (fp32 GEMMs in
another order: near-ties may fall the other way).  Useful work: 2 nvox sum(in x out) FLOP; the matrix cores do two (first
layer) or three (later layers) times that for the operand halves.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.pca_step import timed          # noqa: E402

PEAK_FP16_TFLOPS = 2500.0                 # dense MFMA peak, as bench.py has it
HEADS = ((), (64,), (256,), (256, 256))


def stock_decide(head, x, chunk=1 << 18):
    """(labels uint8 [nvox], probs fp32 of the last chunk) of the torch head over the (F, nvox) fp16 matrix, in voxel chunks."""
    import torch
    labels = torch.empty(x.shape[1], dtype=torch.uint8, device=x.device)
    probs = None
    with torch.no_grad():
        for v in range(0, x.shape[1], chunk):
            probs = torch.softmax(head(x[:, v:v + chunk].T.float()), dim=1)
            labels[v:v + chunk] = probs.argmax(1).to(torch.uint8)
    return labels, probs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--features', type=int, default=384)
    ap.add_argument('--classes', type=int, default=6)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mlp_kernels.json'))
    args = ap.parse_args()
    import ctypes as C
    import torch
    from vit_tf_amd import _lib
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    lib = _lib.require_device()
    c = args.classes
    line = {'tool': 'mlp_step', 'device': torch.cuda.get_device_name(0), 'classes': c, 'steps': args.steps, 'warmup': args.warmup,
            'peak_fp16_tflops': PEAK_FP16_TFLOPS, 'volumes': {}}
    g = torch.Generator(device=dev).manual_seed(0)
    t = lambda fn: timed(fn, args.steps, args.warmup)          # noqa: E731
    for n, f in [(n, args.features) for n in args.sizes] + [(64, 32)]:
        nvox = n ** 3
        feat = torch.empty((f, n, n, n), dtype=torch.float16, device=dev)
        for c0 in range(0, f, 32):                            # (filled in slabs: no fp32 copy of the whole volume)
            feat[c0:c0 + 32] = (torch.randn((32, n, n, n), generator=g, device=dev) + torch.randn((32, 1, 1, 1), generator=g, device=dev)).half()
        x = feat.reshape(f, nvox)
        res = {'nvox': nvox, 'features': f, 'volume_mb': round(f * nvox * 2 / 1e6, 1), 'heads': {}}
        labels = torch.empty((nvox,), dtype=torch.uint8, device=dev)
        logits = torch.empty((c, nvox), dtype=torch.float32, device=dev)
        probs = torch.empty((c, nvox), dtype=torch.uint8, device=dev)
        for hidden in HEADS:
            torch.manual_seed(len(hidden) * 1000 + sum(hidden))
            dims = (f,) + hidden + (c,)
            mods = []
            for i in range(len(dims) - 1):
                mods += [torch.nn.Linear(dims[i], dims[i + 1])] + ([torch.nn.ReLU()] if i + 2 < len(dims) else [])
            head = torch.nn.Sequential(*mods).to(dev)
            lin = [m for m in head if isinstance(m, torch.nn.Linear)]
            w = torch.cat([m.weight.detach().reshape(-1) for m in lin]).contiguous()
            b = torch.cat([m.bias.detach() for m in lin]).contiguous()
            widths = (C.c_int32 * max(len(hidden), 1))(*hidden)
            ws_bytes = lib.vittf_mlp_workspace_bytes(f, widths, len(hidden), c)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            call = lambda z, p: _lib.check(lib.vittf_mlp_decide(                                              # noqa: E731
                _lib.ptr(x), f, nvox, _lib.ptr(w), _lib.ptr(b), widths, len(hidden), c, None, _lib.ptr(labels), _lib.ptr(z), _lib.ptr(p),
                _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
            r = {'workspace_mb': round(ws_bytes / 1e6, 3), 'n_params': int(w.numel() + b.numel())}
            r['decide_ms'], r['decide_ms_all'] = t(lambda: call(None, None))
            r['decide_with_probs_ms'], _ = t(lambda: call(None, probs))
            r['decide_with_logits_ms'], _ = t(lambda: call(logits, None))
            flop = 2.0 * nvox * sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))
            r['useful_tflops'] = round(flop / (r['decide_ms'] * 1e-3) / 1e12, 2)
            r['useful_frac_of_fp16_peak'] = round(r['useful_tflops'] / PEAK_FP16_TFLOPS, 4)
            r['volume_gb_per_s'] = round(2.0 * f * nvox / r['decide_ms'] / 1e6, 1)
            call(None, probs)
            mine = labels.clone()
            stock, stock_probs = stock_decide(head, x)
            r['labels_differing_from_stock'] = int((stock != mine).sum())
            tail = stock_probs.shape[0]
            r['max_prob_difference_last_chunk'] = float((probs[:, nvox - tail:].float() / 255.0 - stock_probs.T).abs().max())
            r['stock_ms'], r['stock_ms_all'] = t(lambda: stock_decide(head, x))
            r['speedup_vs_stock'] = round(r['stock_ms'] / r['decide_with_probs_ms'], 2)
            res['heads'][str(hidden)] = r
            print(f'{n}^3 x {f} head {hidden}: ' + json.dumps({k: v for k, v in r.items() if not k.endswith('_all')}), file=sys.stderr, flush=True)
            del ws, stock, stock_probs, head
        line['volumes'][f'{n}^3x{f}'] = res
        del feat, x, labels, logits, probs
        torch.cuda.empty_cache()
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(text + '\n')


if __name__ == '__main__':
    main()
