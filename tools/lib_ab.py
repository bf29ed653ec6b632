#!/usr/bin/env python3
"""A/B of TWO builds of libvittf.so in one process (the tree's against a copy built from another commit).
  python tools/lib_ab.py tools/micro/build/libvittf_prev.so [batch] [rounds]
      the qkv / fc1 GEMM shapes of ViT-S (K = 384), outputs compared bit for bit
  python tools/lib_ab.py tools/micro/build/libvittf_prev.so attention [result.json] [slices]
      the attention family and the producers of its operands: outputs AND workspaces compared byte for byte over the token
      counts where the kernels change path, then each library timed twice in turn (other, tree, other, tree) on the ViT-S /
      ViT-B shapes; exit status 1 when any comparison differs"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vit_tf_amd import _lib   # noqa: E402


def load_both(other, names):
    libs = {'other': C.CDLL(other), 'tree': _lib.load()}
    for name in names:
        fn = getattr(libs['other'], name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return libs


def same_bytes(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def attention_bits(libs, dev):
    """-> {case: identical} -- every case runs both libraries on the same inputs, outputs and workspaces pre-filled alike."""
    from vit_tf_amd import weights
    res = {}
    st = _lib.stream_ptr
    token_list = (1, 64, 65, 97, 129, 257, 320, 577)
    qscale = 0.125 * 1.4426950408889634

    def qkv_input(batch, tokens, heads, dt, seed, pre):
        x = torch.randn(batch * tokens, 3 * heads * 64, generator=torch.Generator().manual_seed(seed))
        if pre:
            x[:, :heads * 64] *= qscale
        return x.to(dt).to(dev)

    def both(run):
        outs = []
        for k in ('other', 'tree'):
            outs.append(run(libs[k]))
            torch.cuda.synchronize()
        return all(same_bytes(a, b) for a, b in zip(*outs))

    def attention(qkv, batch, tokens, heads, dtn, pre):
        def run(lib):
            out = torch.full((batch * tokens + 2, heads * 64), 7.0, dtype=qkv.dtype, device=dev)
            _lib.check(lib.vittf_attention(_lib.ptr(qkv), _lib.ptr(out), batch, tokens, heads, _lib.DTYPES[dtn], pre, st()))
            return [out]
        return both(run)

    for dtn, dt in (('bf16', torch.bfloat16), ('fp16', torch.float16)):
        for tokens in token_list:
            for pre in (0, 1):
                qkv = qkv_input(2, tokens, 2, dt, tokens + pre, pre)
                res[f'attention {dtn} q_prescaled={pre} 2x{tokens}x2'] = attention(qkv, 2, tokens, 2, dtn, pre)
            # fp8 attention with (slice, head) scales: output and the whole workspace
            qkv = qkv_input(2, tokens, 2, dt, 100 + tokens, 1)
            nws = libs['tree'].vittf_attention_fp8_workspace_bytes(2, tokens, 2)
            assert nws == libs['other'].vittf_attention_fp8_workspace_bytes(2, tokens, 2)

            def run_fp8(lib):
                ws = torch.full((nws,), 0xff, dtype=torch.uint8, device=dev)
                out = torch.full((2 * tokens + 2, 128), 7.0, dtype=dt, device=dev)
                _lib.check(lib.vittf_attention_fp8(_lib.ptr(qkv), _lib.ptr(out), 2, tokens, 2, _lib.DTYPES[dtn], _lib.ptr(ws), nws, st()))
                return [out, ws]
            res[f'attention_fp8 {dtn} 2x{tokens}x2 (output, workspace)'] = both(run_fp8)
        # the rescale paths: the input of tests/test_gpu_kernels.py::test_attention_rescale_branch at gain 60
        tokens, gain = 333, 60.0
        x = torch.randn(tokens, 384, generator=torch.Generator().manual_seed(4)) * 0.5
        q, k = x[:, :128].view(tokens, 2, 64), x[:, 128:256].view(tokens, 2, 64)
        for key_row in (5, 100, 200, 332):
            k[key_row, 0] = q[7 + key_row % 50, 0] * gain
        k[40, 1] = q[3, 1] * -gain
        for pre in (0, 1):
            y = x.clone()
            if pre:
                y[:, :128] *= qscale
            res[f'attention {dtn} q_prescaled={pre} rescale branch 1x333x2'] = attention(y.to(dt).to(dev), 1, tokens, 2, dtn, pre)
        # the qkv projection that writes fp8 q / k rows, then the attention on row scales: output, v third, whole workspace
        heads, kk = 12, 768
        n = 3 * heads * 64
        for tokens in (65, 257):
            rows = 2 * tokens
            g = torch.Generator().manual_seed(tokens)
            a = torch.randn(rows, kk, generator=g).to(dt).to(dev)
            w = (1.3 * torch.randn(n, kk, generator=g) / kk ** 0.5).to(dt).to(dev)
            bias = (0.2 * torch.randn(n, generator=g)).to(dev)
            nws = libs['tree'].vittf_attention_fp8_workspace_bytes(2, tokens, heads)

            def run_rows(lib):
                ws = torch.full((nws,), 0xff, dtype=torch.uint8, device=dev)
                qkv = torch.full((rows + 2, n), 7.0, dtype=dt, device=dev)
                out = torch.full((rows + 2, heads * 64), 7.0, dtype=dt, device=dev)
                _lib.check(lib.vittf_gemm_qkv_fp8(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(qkv), rows, n, kk, tokens, heads,
                                                  _lib.DTYPES[dtn], _lib.ptr(ws), nws, st()))
                _lib.check(lib.vittf_attention_fp8_rows(_lib.ptr(qkv), _lib.ptr(out), 2, tokens, heads, _lib.DTYPES[dtn], _lib.ptr(ws),
                                                        nws, st()))
                return [out, qkv, ws]
            res[f'gemm_qkv_fp8 + attention_fp8_rows {dtn} 2x{tokens}x12 (output, qkv, workspace)'] = both(run_rows)
        # the q pre-scale in each GEMM that owns it: tiles (K = 384), persistent (K = 768), activation-stationary (K = 384)
        for name, rows, n, kk in (('gemm tiles', 2 * 257, 1152, 384), ('gemm persistent', 2 * 257, 2304, 768), ('gemm_as', 2 * 257, 1152, 384)):
            g = torch.Generator().manual_seed(n + kk)
            a = torch.randn(rows, kk, generator=g).to(dt).to(dev)
            w = (1.3 * torch.randn(n, kk, generator=g) / kk ** 0.5).to(dt).to(dev)
            bias = (0.3 * torch.randn(n, generator=g)).to(dev)
            wpk = weights.pack_row_images(w[None])[0] if name == 'gemm_as' else None

            def run_gemm(lib):
                out = torch.full((rows + 2, n), 5.0, dtype=dt, device=dev)
                if wpk is None:
                    _lib.check(lib.vittf_gemm(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), rows, n, kk, _lib.EPI_BIAS_QKV, 257,
                                              _lib.DTYPES[dtn], st()))
                else:
                    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
                    _lib.check(lib.vittf_gemm_as(_lib.ptr(a), _lib.ptr(wpk), _lib.ptr(bias), _lib.ptr(out), rows, n, kk, _lib.EPI_BIAS_QKV,
                                                 _lib.DTYPES[dtn], _lib.ptr(ctr), st()))
                return [out]
            res[f'{name} EPI_BIAS_QKV {dtn} {rows}x{n}x{kk}'] = both(run_gemm)
    return res


def attention_times(libs, dev, slices, rounds=7, reps=10):
    """-> {shape: {'other': [median, median], 'tree': [median, median]}} in ms per call: other, tree, other, tree."""
    tokens = 4097
    st = _lib.stream_ptr
    qscale = 0.125 * 1.4426950408889634
    times = {}

    def timed(call):
        med = {'other': [], 'tree': []}
        for _ in range(3):
            call(libs['tree'])
        torch.cuda.synchronize()
        for _ in range(2):
            for k in ('other', 'tree'):
                call(libs[k])
                ts = []
                for _ in range(rounds):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(reps):
                        call(libs[k])
                    b.record()
                    torch.cuda.synchronize()
                    ts.append(a.elapsed_time(b) / reps)
                med[k].append(round(statistics.median(ts), 4))
        return med

    for name, heads, pre in (('attention q_prescaled=1 ViT-S (6 heads)', 6, 1), ('attention q_prescaled=1 ViT-B (12 heads)', 12, 1),
                             ('attention q_prescaled=0 ViT-S (6 heads)', 6, 0)):
        g = torch.Generator(device=dev).manual_seed(heads + pre)
        qkv = torch.randn(slices * tokens, 3 * heads * 64, generator=g, dtype=torch.half, device=dev)
        if pre:
            qkv[:, :heads * 64] *= qscale
        out = torch.empty(slices * tokens, heads * 64, dtype=torch.half, device=dev)
        times[f'{name} {slices}x{tokens} fp16'] = timed(lambda lib: _lib.check(lib.vittf_attention(
            _lib.ptr(qkv), _lib.ptr(out), slices, tokens, heads, _lib.FP16, pre, st())))
        del qkv, out
    # attention on fp8 rows at ViT-B: the projection (the tree's) fills q8 / k8 and their scales once
    heads, kk = 12, 768
    n, rows = 3 * heads * 64, slices * tokens
    g = torch.Generator(device=dev).manual_seed(1)
    a = torch.randn(rows, kk, generator=g, dtype=torch.half, device=dev)
    w = (1.3 * torch.randn(n, kk, generator=g, device=dev) / kk ** 0.5).half()
    bias = 0.2 * torch.randn(n, generator=g, device=dev)
    nws = libs['tree'].vittf_attention_fp8_workspace_bytes(slices, tokens, heads)
    ws = torch.zeros(nws, dtype=torch.uint8, device=dev)
    qkv = torch.empty(rows, n, dtype=torch.half, device=dev)
    out = torch.empty(rows, heads * 64, dtype=torch.half, device=dev)
    _lib.check(libs['tree'].vittf_gemm_qkv_fp8(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(qkv), rows, n, kk, tokens, heads, _lib.FP16,
                                               _lib.ptr(ws), nws, st()))
    del a
    times[f'attention_fp8_rows ViT-B (12 heads) {slices}x{tokens} fp16'] = timed(lambda lib: _lib.check(lib.vittf_attention_fp8_rows(
        _lib.ptr(qkv), _lib.ptr(out), slices, tokens, heads, _lib.FP16, _lib.ptr(ws), nws, st())))
    return times


def attention_mode(other, out_json, slices):
    libs = load_both(other, ('vittf_attention', 'vittf_attention_fp8', 'vittf_attention_fp8_rows', 'vittf_attention_fp8_workspace_bytes',
                             'vittf_gemm_qkv_fp8', 'vittf_gemm', 'vittf_gemm_as'))
    dev = torch.device('cuda', 0)
    bits = attention_bits(libs, dev)
    for k, same in bits.items():
        print(f'{"identical" if same else "DIFFERENT":9s}  {k}', flush=True)
    different = [k for k, same in bits.items() if not same]
    print(f'byte comparisons: {len(bits) - len(different)} identical, {len(different)} different', flush=True)
    result = {'byte_comparisons': {'identical': len(bits) - len(different), 'different': different, 'cases': sorted(bits)}}
    result['ms_per_call'] = attention_times(libs, dev, slices)
    for k, v in result['ms_per_call'].items():
        print(f'{k}: other {v["other"]}  tree {v["tree"]} ms', flush=True)
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, 'w') as f:
            json.dump(result, f, indent=1)
    return 1 if different else 0


def main():
    other = sys.argv[1]
    if len(sys.argv) > 2 and sys.argv[2] == 'attention':
        sys.exit(attention_mode(other, sys.argv[3] if len(sys.argv) > 3 else None, int(sys.argv[4]) if len(sys.argv) > 4 else 256))
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    libs = load_both(other, ('vittf_gemm',))
    libs = {'tree': libs['tree'], 'other': libs['other']}
    d, tokens = 384, 4097
    rows = batch * tokens
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(0)
    for name, n, epi in (('qkv', 3 * d, _lib.EPI_BIAS_QKV), ('fc1 + GELU', 4 * d, _lib.EPI_BIAS_GELU), ('plain', 3 * d, _lib.EPI_BIAS)):
        acts = [torch.randn(rows, d, generator=g).half().to(dev) for _ in range(3)]
        w = (torch.randn(n, d, generator=g) / d ** 0.5).half().to(dev)
        bias = torch.randn(n, generator=g).to(dev)
        out = torch.empty(rows, n, dtype=torch.half, device=dev)
        turn = [0]

        def call(lib):
            a = acts[turn[0] % 3]
            turn[0] += 1
            _lib.check(lib.vittf_gemm(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(out), rows, n, d, epi, tokens,
                                      _lib.DTYPES['fp16'], _lib.stream_ptr()))
        ref = None
        for k, lib in libs.items():
            turn[0] = 0
            call(lib)
            torch.cuda.synchronize()
            if ref is None:
                ref = out.clone()
            else:
                print(f'{name}: {k} bit-equal to tree: {torch.equal(out, ref)}')
        del ref
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.7:
            for _ in range(5):
                call(libs['tree'])
            torch.cuda.synchronize()
        res = {k: [] for k in libs}
        reps = max(3, 1536 // batch)
        for _ in range(rounds):
            for k, lib in libs.items():
                call(lib)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    call(lib)
                b.record()
                torch.cuda.synchronize()
                res[k].append(a.elapsed_time(b) / reps)
        fl = 2.0 * rows * n * d
        for k in libs:
            med = statistics.median(res[k])
            print(f'{name} [{rows} x {n}] {k:5s}: median {med:.4f} ms  min {min(res[k]):.4f}  {fl / med / 1e9:7.1f} TFLOP/s')
        del acts, out


if __name__ == '__main__':
    main()
