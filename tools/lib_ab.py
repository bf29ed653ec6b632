#!/usr/bin/env python3
"""A/B of TWO builds of libvittf.so in one process (the tree's against a copy built from another commit).
  python tools/lib_ab.py tools/micro/build/libvittf_prev.so [batch] [rounds]
      the qkv / fc1 GEMM shapes of ViT-S (K = 384), outputs compared bit for bit
  python tools/lib_ab.py tools/micro/build/libvittf_prev.so attention [result.json] [slices]
      the attention family and the producers of its operands: outputs AND workspaces compared byte for byte over the token
      counts where the kernels change path, then each library timed twice in turn (other, tree, other, tree) on the ViT-S /
      ViT-B shapes; exit status 1 when any comparison differs
  python tools/lib_ab.py tools/micro/build/libvittf_prev.so classifiers [result.json]
      the decision entries of the classifiers (RBF and linear SVM, k-NN, MLP head) and the two other users of feat_rows.h's
      score loop (PCA projection, k-means assignment): outputs AND workspaces compared byte for byte over the smallest shapes
      that reach every template and edge of the bank frame (csrc/bank_frame.h), then each library timed twice in turn on the
      shapes of tools/svm_step.py, knn_step.py and mlp_step.py (64^3 x 384, 1024 rows); exit status 1 when any comparison
      differs
  python tools/lib_ab.py tools/micro/build/libvittf_prev.so similarity [result.json]
      vittf_similarity, vittf_similarity_query, vittf_similarity_maps_f32 (modes 0, 1, 2) and vittf_sample_features: outputs
      AND workspaces (0xff before the call) compared byte for byte on the shapes and switch settings of
      tests/sim_data.GPU_CASES and on the four quantise shapes, the *_workspace_bytes functions over a grid of arguments, then
      each library timed twice in turn on the bench's 16-query call, the 5 x 1024 call and a 3 + 2-annotation VALU call
      (64^3 x 384 -> 256^3); exit status 1 when any comparison differs"""
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


def both_same(libs, run):
    """run(lib) -> [tensors]: True when both libraries leave the same bytes in every one of them."""
    outs = []
    for k in ('other', 'tree'):
        outs.append(run(libs[k]))
        torch.cuda.synchronize()
    return all(same_bytes(a, b) for a, b in zip(*outs))


def timed(libs, call, rounds=7, reps=10):
    """{'other': [median, median], 'tree': [median, median]} in ms per call(lib): other, tree, other, tree, each figure the
    median of `rounds` event pairs around `reps` calls -- more of them where a call is short, so that a pair spans 5 ms."""
    med = {'other': [], 'tree': []}
    for k in ('other', 'tree'):                               # warm both up: clocks, code objects, caches
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call(libs[k])
        b.record()
        torch.cuda.synchronize()
    reps = max(reps, min(500, int(5.0 * reps / max(a.elapsed_time(b), 1e-3))))
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


def report(bits, times, out_json, count_by=None):
    """Prints both tables, writes them to out_json and returns the exit status: 1 when a byte comparison differs.  The json
    lists the cases by name, or, with count_by(case) -> group, how many ran in each group (the loops define them)."""
    for k, same in bits.items():
        print(f'{"identical" if same else "DIFFERENT":9s}  {k}', flush=True)
    different = [k for k, same in bits.items() if not same]
    print(f'byte comparisons: {len(bits) - len(different)} identical, {len(different)} different', flush=True)
    cases = sorted(bits) if count_by is None else {g: sum(count_by(k) == g for k in bits) for g in sorted(set(map(count_by, bits)))}
    result = {'byte_comparisons': {'identical': len(bits) - len(different), 'different': different, 'cases': cases},
              'ms_per_call': times}
    for k, v in times.items():
        # the tree's slower median against the other's slower median plus the spread of the other's own two rounds
        v['other_spread'] = round(abs(v['other'][0] - v['other'][1]), 4)
        v['within_spread'] = round(max(v['tree']) - max(v['other']), 4) <= v['other_spread']       # (figures of 4 decimals)
        print(f'{k}: other {v["other"]}  tree {v["tree"]} ms, spread of other {v["other_spread"]}: '
              f'{"within" if v["within_spread"] else "BEYOND"}', flush=True)
    if out_json:
        os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
        with open(out_json, 'w') as f:
            json.dump(result, f, indent=1)
    return 1 if different else 0


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

    both = lambda run: both_same(libs, run)                   # noqa: E731

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


def attention_times(libs, dev, slices):
    """-> {shape: timed(..)}."""
    tokens = 4097
    st = _lib.stream_ptr
    qscale = 0.125 * 1.4426950408889634
    times = {}

    for name, heads, pre in (('attention q_prescaled=1 ViT-S (6 heads)', 6, 1), ('attention q_prescaled=1 ViT-B (12 heads)', 12, 1),
                             ('attention q_prescaled=0 ViT-S (6 heads)', 6, 0)):
        g = torch.Generator(device=dev).manual_seed(heads + pre)
        qkv = torch.randn(slices * tokens, 3 * heads * 64, generator=g, dtype=torch.half, device=dev)
        if pre:
            qkv[:, :heads * 64] *= qscale
        out = torch.empty(slices * tokens, heads * 64, dtype=torch.half, device=dev)
        times[f'{name} {slices}x{tokens} fp16'] = timed(libs, lambda lib: _lib.check(lib.vittf_attention(
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
    times[f'attention_fp8_rows ViT-B (12 heads) {slices}x{tokens} fp16'] = timed(libs, lambda lib: _lib.check(lib.vittf_attention_fp8_rows(
        _lib.ptr(qkv), _lib.ptr(out), slices, tokens, heads, _lib.FP16, _lib.ptr(ws), nws, st())))
    return times


def attention_mode(other, out_json, slices):
    libs = load_both(other, ('vittf_attention', 'vittf_attention_fp8', 'vittf_attention_fp8_rows', 'vittf_attention_fp8_workspace_bytes',
                             'vittf_gemm_qkv_fp8', 'vittf_gemm', 'vittf_gemm_as'))
    dev = torch.device('cuda', 0)
    return report(attention_bits(libs, dev), attention_times(libs, dev, slices), out_json)


# ------------------------------------------------------------------------------------------------ classifiers
CLASSIFIER_ENTRIES = ('vittf_svm_rbf_decide', 'vittf_svm_rbf_workspace_bytes', 'vittf_svm_linear_decide', 'vittf_knn_decide',
                      'vittf_knn_workspace_bytes', 'vittf_mlp_decide', 'vittf_mlp_workspace_bytes', 'vittf_feature_project',
                      'vittf_kmeans_assign')


class Calls:
    """The raw decision calls on one device; each method returns run(lib) -> [what the call wrote].  Every output and
    workspace is a new tensor pre-filled the same way before the call (fresh), or, for the timings, one tensor reused."""

    def __init__(self, libs, dev, fresh=True):
        self.libs, self.dev, self.fresh, self.kept = libs, dev, fresh, {}

    def volume(self, f, nvox, seed):
        g = torch.Generator().manual_seed(seed)
        x = (torch.randn(f, nvox, generator=g) + torch.randn(f, 1, generator=g)).half().to(self.dev)
        return x, x.float().norm(dim=0).clamp_min(1e-6).contiguous()

    def rows(self, s, f, seed, unit=False):
        r = torch.randn(s, f, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
        return (torch.nn.functional.normalize(r, dim=1) if unit else r).half().to(self.dev)

    def out(self, shape, dtype, fill=7):
        if not self.fresh and (shape, dtype) in self.kept:
            return self.kept[shape, dtype]
        t = self.kept[shape, dtype] = torch.full(shape, fill, dtype=dtype, device=self.dev)
        return t

    def workspace(self, name, *args):
        n = getattr(self.libs['tree'], name)(*args)
        assert n and n == getattr(self.libs['other'], name)(*args), (name, args, n)
        return n

    def rbf(self, x, norm, sv, classes, seed):
        f, nvox = x.shape
        s, pairs = sv.shape[0], classes * (classes - 1) // 2
        g = torch.Generator().manual_seed(seed)
        coef = torch.randn(pairs, s, generator=g).to(self.dev)
        b = (0.1 * torch.randn(pairs, generator=g)).to(self.dev)
        nws = self.workspace('vittf_svm_rbf_workspace_bytes', f, s, classes)

        def run(lib):
            ws, labels, dec = self.out((nws,), torch.uint8, 0xff), self.out((nvox,), torch.uint8), self.out((pairs, nvox), torch.float32)
            _lib.check(lib.vittf_svm_rbf_decide(_lib.ptr(x), f, nvox, _lib.ptr(sv), _lib.ptr(coef), _lib.ptr(b), s, classes, 1.0 / f,
                                                _lib.ptr(norm), _lib.ptr(labels), _lib.ptr(dec), _lib.ptr(ws), nws, _lib.stream_ptr()))
            return [labels, dec, ws]
        return run

    def linear(self, x, norm, classes, seed):
        f, nvox = x.shape
        pairs = classes * (classes - 1) // 2
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(pairs, f, generator=g) / f ** 0.5).to(self.dev)
        b = (0.1 * torch.randn(pairs, generator=g)).to(self.dev)

        def run(lib):
            labels, dec = self.out((nvox,), torch.uint8), self.out((pairs, nvox), torch.float32)
            _lib.check(lib.vittf_svm_linear_decide(_lib.ptr(x), f, nvox, _lib.ptr(w), _lib.ptr(b), classes, _lib.ptr(norm), _lib.ptr(labels),
                                                   _lib.ptr(dec), _lib.stream_ptr()))
            return [labels, dec]
        return run

    def knn(self, x, norm, bank, classes, k, inv_t, seed, outputs=True):
        f, nvox = x.shape
        s = bank.shape[0]
        cls = torch.sort(torch.randint(0, classes, (s,), generator=torch.Generator().manual_seed(seed))).values.to(torch.uint8).to(self.dev)
        nws = self.workspace('vittf_knn_workspace_bytes', f, s)

        def run(lib):
            ws, labels = self.out((nws,), torch.uint8, 0xff), self.out((nvox,), torch.uint8)
            extra = [self.out((classes, nvox), torch.float32), self.out((k, nvox), torch.int32), self.out((k, nvox), torch.float32)] if outputs else [None] * 3
            _lib.check(lib.vittf_knn_decide(_lib.ptr(x), f, nvox, _lib.ptr(bank), _lib.ptr(cls), s, classes, k, inv_t, _lib.ptr(norm),
                                            _lib.ptr(labels), *[_lib.ptr(e) for e in extra], _lib.ptr(ws), nws, _lib.stream_ptr()))
            return [labels, ws] + [e for e in extra if e is not None]
        return run

    def mlp(self, x, hidden, classes, seed):
        f, nvox = x.shape
        dims = (f,) + tuple(hidden) + (classes,)
        g = torch.Generator().manual_seed(seed)
        w = torch.cat([(torch.randn(dims[i + 1], dims[i], generator=g) / dims[i] ** 0.5).reshape(-1) for i in range(len(dims) - 1)]).to(self.dev)
        b = torch.cat([0.1 * torch.randn(dims[i + 1], generator=g) for i in range(len(dims) - 1)]).to(self.dev)
        widths = (C.c_int32 * max(len(hidden), 1))(*hidden)
        nws = self.workspace('vittf_mlp_workspace_bytes', f, widths, len(hidden), classes)

        def run(lib):
            ws, labels = self.out((nws,), torch.uint8, 0xff), self.out((nvox,), torch.uint8)
            logits, probs = self.out((classes, nvox), torch.float32), self.out((classes, nvox), torch.uint8)
            _lib.check(lib.vittf_mlp_decide(_lib.ptr(x), f, nvox, _lib.ptr(w), _lib.ptr(b), widths, len(hidden), classes, None, _lib.ptr(labels),
                                            _lib.ptr(logits), _lib.ptr(probs), _lib.ptr(ws), nws, _lib.stream_ptr()))
            return [labels, logits, probs]
        return run

    def project(self, x, k, seed):
        f, nvox = x.shape
        g = torch.Generator().manual_seed(seed)
        comp, off = (torch.randn(k, f, generator=g) / f ** 0.5).to(self.dev), torch.randn(f, generator=g).to(self.dev)

        def run(lib):
            out = self.out((k, nvox), torch.float16)
            _lib.check(lib.vittf_feature_project(_lib.ptr(x), f, nvox, _lib.ptr(comp), _lib.ptr(off), k, _lib.ptr(out), _lib.stream_ptr()))
            return [out]
        return run

    def assign(self, x, c, seed):
        f, nvox = x.shape
        cent = torch.randn(c, f, generator=torch.Generator().manual_seed(seed))
        half = (0.5 * cent.double().pow(2).sum(1)).float().to(self.dev)
        cent = cent.to(self.dev)

        def run(lib):
            labels, best = self.out((nvox,), torch.uint8), self.out((nvox,), torch.float32)
            _lib.check(lib.vittf_kmeans_assign(_lib.ptr(x), f, nvox, _lib.ptr(cent), _lib.ptr(half), c, _lib.ptr(labels), _lib.ptr(best),
                                               _lib.stream_ptr()))
            return [labels, best]
        return run


def classifier_bits(libs, dev):
    """-> {case: identical}: the smallest shapes that reach every template and edge of the frame."""
    calls, res = Calls(libs, dev), {}
    same = lambda run: both_same(libs, run)                   # noqa: E731
    inv_t = float(torch.tensor(1.0 / 0.07, dtype=torch.float32))
    for f in (32, 64, 384, 768):                               # F = 64 pads to FP = 128
        for nvox in (1, 127, 128, 129, 1024):                  # 129: unaligned rows and a second workgroup
            x, norm = calls.volume(f, nvox, f + nvox)
            for s in (1, 31, 32, 33, 65):                      # rows of the bank: chunk edges; 65 at F = 384: the two-chunk batch and its odd last chunk
                sv, bank = calls.rows(s, f, s), calls.rows(s, f, 100 + s, unit=True)
                for classes in (2, 8):
                    for vn in (None, norm):
                        res[f'svm_rbf F={f} nvox={nvox} sv={s} classes={classes} voxel_norm={vn is not None} (labels, decisions, workspace)'] = \
                            same(calls.rbf(x, vn, sv, classes, s + classes))
                for k in sorted({min(k, s) for k in (1, 4, 5, 20, 32)}):
                    for weights, it in (('softmax', inv_t), ('uniform', 0.0)):
                        res[f'knn F={f} nvox={nvox} bank={s} k={k} {weights} (labels, scores, neighbours, similarities, workspace)'] = \
                            same(calls.knn(x, norm, bank, 8, k, it, s + k))
    for f in (32, 384):
        for nvox in (129, 1024):
            x, _ = calls.volume(f, nvox, 7 + f + nvox)
            for hidden in ((), (32,), (96, 32)):
                res[f'mlp F={f} nvox={nvox} hidden={hidden} (labels, logits, probabilities)'] = same(calls.mlp(x, hidden, 6, f + len(hidden)))
        x, norm = calls.volume(f, 257, 11 + f)
        res[f'feature_project F={f} nvox=257 k=3 and k=40'] = same(calls.project(x, 3, f)) and same(calls.project(x, 40, f + 1))
        res[f'kmeans_assign F={f} nvox=257 c=5 and c=40'] = same(calls.assign(x, 5, f)) and same(calls.assign(x, 40, f + 1))
    for f in (32, 384, 1024):
        x, norm = calls.volume(f, 129, 13 + f)
        for vn in (None, norm):
            res[f'svm_linear F={f} nvox=129 classes=8 voxel_norm={vn is not None} (labels, decisions)'] = same(calls.linear(x, vn, 8, f))
    return res


def classifier_times(libs, dev):
    """-> {shape: timed(..)} on the shapes of tools/svm_step.py, knn_step.py and mlp_step.py: 64^3 x 384, 1024 rows, 6 classes."""
    calls, times = Calls(libs, dev, fresh=False), {}
    f, nvox, s, classes = 384, 64 ** 3, 1024, 6
    x, norm = calls.volume(f, nvox, 0)
    quiet = lambda run: (lambda lib: run(lib) and None)       # noqa: E731
    times[f'svm_rbf 64^3x{f} sv={s}'] = timed(libs, quiet(calls.rbf(x, None, calls.rows(s, f, 1), classes, 2)))
    times[f'svm_linear 64^3x{f}'] = timed(libs, quiet(calls.linear(x, None, classes, 3)))
    bank = calls.rows(s, f, 4, unit=True)
    inv_t = float(torch.tensor(1.0 / 0.07, dtype=torch.float32))
    for k in (1, 20):
        times[f'knn 64^3x{f} bank={s} k={k}'] = timed(libs, quiet(calls.knn(x, norm, bank, classes, k, inv_t, 5, outputs=False)))
    for hidden in ((), (64,), (256,), (256, 256)):
        times[f'mlp 64^3x{f} hidden={hidden}'] = timed(libs, quiet(calls.mlp(x, hidden, classes, 6)))
    for f in (32, 128):                                        # knn_step.py's 64^3 x 32 (a _pca32 file), and FP = 128
        x, norm = calls.volume(f, nvox, f)
        times[f'svm_rbf 64^3x{f} sv={s}'] = timed(libs, quiet(calls.rbf(x, None, calls.rows(s, f, 1), classes, 2)))
        bank = calls.rows(s, f, 4, unit=True)
        for k in (1, 20) if f == 32 else (20,):
            times[f'knn 64^3x{f} bank={s} k={k}'] = timed(libs, quiet(calls.knn(x, norm, bank, classes, k, inv_t, 5, outputs=False)))
    return times


def classifiers_mode(other, out_json):
    libs = load_both(other, CLASSIFIER_ENTRIES)
    dev = torch.device('cuda', 0)
    return report(classifier_bits(libs, dev), classifier_times(libs, dev), out_json, count_by=lambda case: case.split(' ')[0])


# ------------------------------------------------------------------------------------------------ similarity
SIMILARITY_ENTRIES = ('vittf_similarity', 'vittf_similarity_query', 'vittf_similarity_maps_f32', 'vittf_sample_features',
                      'vittf_similarity_workspace_bytes', 'vittf_similarity_query_workspace_bytes', 'vittf_surface_shell_workspace_bytes')
SIM_SWITCHES = ('VITTF_SIM_MFMA', 'VITTF_SIM_MFMA_MIN', 'VITTF_SIM_MFMA_VB', 'VITTF_SIM_SPLIT', 'VITTF_SIM_QUANT16')
# (feature grid, output shape) of the quantise kernels: x 4, x 16 along the last dim, non-integer ratios, an output row of 15
QUANT_PAIRS = (((8, 8, 8), (32, 32, 32)), ((8, 8, 8), (8, 8, 128)), ((6, 7, 5), (30, 35, 32)), ((8, 8, 8), (8, 8, 15)))


def set_switches(env):
    for k in SIM_SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


class SimCalls:
    """The raw similarity calls on one device; each method returns run(lib) -> [what the call wrote], outputs and workspaces
    new tensors filled with 0xff before every call."""

    def __init__(self, libs, dev):
        self.libs, self.dev = libs, dev

    def fresh(self, n, dtype=torch.uint8):
        return torch.full((n,), 0xff, dtype=torch.uint8, device=self.dev).view(dtype)

    def workspace(self, name, *args):
        n = getattr(self.libs['tree'], name)(*args)
        assert n and n == getattr(self.libs['other'], name)(*args), (name, args, n)
        return n

    @staticmethod
    def starts(counts):
        s = [0]
        for n in counts:
            s.append(s[-1] + n)
        return (C.c_int32 * len(s))(*s)

    def maps_f32(self, x, half, grid, q, counts, mode, vnorm):
        f, nvox, a = x.shape[0], x.shape[1], q.shape[0]
        nws = self.workspace('vittf_similarity_workspace_bytes', len(counts), 0, a)

        def run(lib):
            ws, out = self.fresh(nws), self.fresh(4 * (len(counts) * nvox + 1), torch.float32)
            _lib.check(lib.vittf_similarity_maps_f32(_lib.ptr(x), int(half), f, *grid, _lib.ptr(q), self.starts(counts), len(counts), mode, 2.0,
                                                     _lib.ptr(vnorm), _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream_ptr()))
            return [out, ws]
        return run

    def similarity(self, x, grid, q, counts, o, vnorm, big=0):
        f, nvox, a = x.shape[0], x.shape[1], q.shape[0]
        nws = self.workspace('vittf_similarity_workspace_bytes', len(counts), nvox, a)

        def run(lib):
            ws, out = self.fresh(nws), self.fresh(len(counts) * o[0] * o[1] * o[2] + 16)
            _lib.check(lib.vittf_similarity(_lib.ptr(x), f, *grid, _lib.ptr(q), self.starts(counts), len(counts), big, _lib.ptr(vnorm), *o,
                                            _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream_ptr()))
            return [out, ws]
        return run

    def query(self, x, grid, rel, counts, o, vnorm, keep=None):
        """keep: a dict that holds the workspace and output across calls (the timings), else fresh ones per call"""
        f, nvox, a = x.shape[0], x.shape[1], rel.shape[0]
        nws = self.workspace('vittf_similarity_query_workspace_bytes', len(counts), nvox, a, f)
        rel_h = (C.c_float * (3 * a))(*rel.flatten().tolist())
        starts = self.starts(counts)

        def run(lib):
            if keep is None or 'ws' not in keep:
                ws, out = self.fresh(nws), self.fresh(len(counts) * o[0] * o[1] * o[2] + 16)
                if keep is not None:
                    keep['ws'], keep['out'] = ws, out
            else:
                ws, out = keep['ws'], keep['out']
            _lib.check(lib.vittf_similarity_query(_lib.ptr(x), f, *grid, rel_h, starts, len(counts), 0, _lib.ptr(vnorm), *o, _lib.ptr(out),
                                                  _lib.ptr(ws), nws, _lib.stream_ptr()))
            return [out, ws]
        return run

    def sample(self, x, half, grid, rel, mode, vnorm):
        f, a = x.shape[0], rel.shape[0]
        rel_d = rel.to(self.dev).contiguous()

        def run(lib):
            out = self.fresh(4 * (a * f + 1), torch.float32)
            _lib.check(lib.vittf_sample_features(_lib.ptr(x), int(half), f, *grid, _lib.ptr(rel_d), a, mode, _lib.ptr(vnorm), _lib.ptr(out),
                                                 _lib.stream_ptr()))
            return [out]
        return run


def similarity_workspace_bits(libs):
    """The three public *_workspace_bytes functions of the files this mode covers over a grid of arguments: no GPU needed."""
    n, same = 0, True
    for classes in (0, 1, 2, 3, 8, 32, 33, 40, 256):
        for nvox in (0, 1, 8, 60, 693, 8640, 64 ** 3, 2 ** 31 + 5):
            for a in (0, 1, 7, 8, 31, 32, 33, 64, 65, 1224, 5120):
                same &= libs['tree'].vittf_similarity_workspace_bytes(classes, nvox, a) == libs['other'].vittf_similarity_workspace_bytes(classes, nvox, a)
                for f in (0, 12, 384, 768, 4096):
                    same &= (libs['tree'].vittf_similarity_query_workspace_bytes(classes, nvox, a, f) ==
                             libs['other'].vittf_similarity_query_workspace_bytes(classes, nvox, a, f))
                    n += 1
                n += 1
    for shape in ((0, 1, 1), (1, 1, 1), (3, 5, 16), (17, 70, 9), (512, 512, 512), (2048, 2048, 2048)):
        same &= libs['tree'].vittf_surface_shell_workspace_bytes(*shape) == libs['other'].vittf_surface_shell_workspace_bytes(*shape)
        n += 1
    return {f'workspace_bytes similarity, similarity_query, surface_shell over {n} argument tuples': bool(same)}


def similarity_bits(libs, dev):
    """-> {case: identical}: the shapes and switch settings of tests/sim_data.GPU_CASES through every entry, then the quantise
    pairs under the three settings of VITTF_SIM_QUANT16."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import sim_data as sd
    calls, res = SimCalls(libs, dev), {}
    same = lambda run: both_same(libs, run)                   # noqa: E731
    for case in sd.GPU_CASES:
        name = sd.case_id(case)
        grid, counts, a = tuple(case.grid), tuple(case.counts), int(sum(case.counts))
        d = sd.correlated(grid, counts, case.f, sd.seed_of(case), normalized=False)
        x, q, vnorm = d.X.to(dev), d.q.to(dev), d.vnorm.to(dev)
        rel = torch.rand(a, 3, generator=torch.Generator().manual_seed(a)) * 2.4 - 1.2
        set_switches(case.env)
        for vn in (None, vnorm):
            res[f'maps_f32 mode 0 {name} voxel_norm={vn is not None} (maps, workspace)'] = same(calls.maps_f32(x, True, grid, q, counts, 0, vn))
        res[f'maps_f32 mode 1 {name} (maps, workspace)'] = same(calls.maps_f32(x, True, grid, q, counts, 1, None))
        res[f'maps_f32 mode 2 fp16 {name} (maps, workspace)'] = same(calls.maps_f32(x, True, grid, q, counts, 2, vnorm))
        res[f'maps_f32 mode 2 fp32 {name} (maps, workspace)'] = same(calls.maps_f32(x.float(), False, grid, q, counts, 2, None))
        for o in (grid, tuple(2 * s for s in grid)):
            res[f'similarity {name} -> {o} (maps, workspace)'] = same(calls.similarity(x, grid, q, counts, o, None))
        res[f'similarity big_a_mean {name} (maps, workspace)'] = same(calls.similarity(x, grid, q[:counts[0]], counts[:1], grid, vnorm, big=1))
        if a <= _lib.QUERY_MAX_A:
            for vn in (None, vnorm):
                res[f'similarity_query {name} voxel_norm={vn is not None} (maps, workspace)'] = same(calls.query(x, grid, rel, counts, grid, vn))
        for mode in (0, 1):
            res[f'sample_features mode {mode} {name}'] = same(calls.sample(x, True, grid, rel, mode, vnorm)) and \
                same(calls.sample(x.float(), False, grid, rel, mode, None))
    for grid, o in QUANT_PAIRS:
        counts = (3, 2)
        d = sd.correlated(grid, counts, 64, sum(grid) + sum(o))
        x, q = d.X.to(dev), d.q.to(dev)
        rel = torch.rand(5, 3, generator=torch.Generator().manual_seed(sum(o))) * 2 - 1
        for q16 in ('1', '2', '0'):
            set_switches({'VITTF_SIM_QUANT16': q16})
            res[f'quantize {grid} -> {o} VITTF_SIM_QUANT16={q16}: similarity, similarity_query (maps, workspace)'] = \
                same(calls.similarity(x, grid, q, counts, o, None)) and same(calls.query(x, grid, rel, counts, o, None))
    set_switches({})
    return res


def similarity_times(libs, dev):
    """-> {shape: timed(..)}: the bench's 16-query call, BASELINE configs[4] (5 x 1024 annotations) and a VALU call, all on a
    64^3 x 384 volume with 256^3 maps."""
    calls, times = SimCalls(libs, dev), {}
    f, grid, o = 384, (64, 64, 64), (256, 256, 256)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.nn.functional.normalize(torch.randn(f, 64 ** 3, generator=g, device=dev), dim=0).half()
    quiet = lambda run: (lambda lib: run(lib) and None)       # noqa: E731
    for name, counts in (('similarity_query 16 annotations (matrix cores)', (16,)), ('similarity_query 3 + 2 annotations (VALU)', (3, 2))):
        rel = torch.rand(sum(counts), 3, generator=torch.Generator().manual_seed(1)) * 2 - 1
        times[f'{name} 64^3x{f} -> 256^3'] = timed(libs, quiet(calls.query(x, grid, rel, counts, o, None, keep={})))
    counts = (1024,) * 5
    q = x[:, torch.randint(0, 64 ** 3, (sum(counts),), generator=g, device=dev)].T.float().contiguous()
    nws = calls.workspace('vittf_similarity_workspace_bytes', 5, 64 ** 3, sum(counts))
    ws, out, starts = calls.fresh(nws), calls.fresh(5 * 256 ** 3), calls.starts(counts)
    times[f'similarity 5 x 1024 annotations 64^3x{f} -> 256^3'] = timed(libs, lambda lib: _lib.check(lib.vittf_similarity(
        _lib.ptr(x), f, *grid, _lib.ptr(q), starts, 5, 0, None, *o, _lib.ptr(out), _lib.ptr(ws), nws, _lib.stream_ptr())))
    return times


def similarity_mode(other, out_json):
    libs = load_both(other, SIMILARITY_ENTRIES)
    bits = similarity_workspace_bits(libs)
    dev = torch.device('cuda', 0)
    bits.update(similarity_bits(libs, dev))
    return report(bits, similarity_times(libs, dev), out_json, count_by=lambda case: case.split(' ')[0])


def main():
    other = sys.argv[1]
    if len(sys.argv) > 2 and sys.argv[2] == 'similarity':
        sys.exit(similarity_mode(other, sys.argv[3] if len(sys.argv) > 3 else None))
    if len(sys.argv) > 2 and sys.argv[2] == 'attention':
        sys.exit(attention_mode(other, sys.argv[3] if len(sys.argv) > 3 else None, int(sys.argv[4]) if len(sys.argv) > 4 else 256))
    if len(sys.argv) > 2 and sys.argv[2] == 'classifiers':
        sys.exit(classifiers_mode(other, sys.argv[3] if len(sys.argv) > 3 else None))
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
