"""CPU: the routing of the similarity calls (csrc/sim_route.h) through its host driver tools/micro/sim_route_host.cpp, built
with the system C++ compiler -- the kernel name of every row of sim_data.GPU_CASES (what tests/test_gpu_similarity_maps.py
asserts on the GPU), the quantise kernel of the shapes the byte-equality tests of tests/test_gpu_kernels.py run, and the
properties of the chunk plans the VALU kernels are launched with."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sim_data as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACH, MAXC = 16, 8


@pytest.fixture(scope='module')
def route(tmp_path_factory):
    """route(lines, env) -> one dict per case line; the switches travel as the driver's environment, as in the library."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no C++ compiler')
    exe = str(tmp_path_factory.mktemp('sim_route') / 'sim_route_host')
    subprocess.run([cxx, '-std=c++17', '-O1', os.path.join(ROOT, 'tools', 'micro', 'sim_route_host.cpp'), '-o', exe], check=True, timeout=300)

    def run(lines, env=None):
        clean = {k: v for k, v in os.environ.items() if not k.startswith('VITTF_SIM_')}
        r = subprocess.run([exe], input='\n'.join(lines) + '\n', env={**clean, **(env or {})}, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = [json.loads(line) for line in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def _counts(counts):
    return 'counts=' + ','.join(map(str, counts))


@pytest.mark.parametrize('case', sd.GPU_CASES, ids=[sd.case_id(c) for c in sd.GPU_CASES])
def test_route_names_of_the_gpu_cases(route, case):
    nvox = int(np.prod(case.grid))
    got, = route([f'f={case.f} nvox={nvox} half=1 mode=0 feat=256 ws=1 cus=256 {_counts(case.counts)}'], case.env)
    assert got['accumulate']['name'] == case.kernel


def test_route_leaves_the_matrix_cores(route):
    """What takes a call off the matrix cores, one condition at a time, on a shape they take by default (and VITTF_SIM_MFMA is
    read like the other switches: per process start of the driver, per call in the library)."""
    base = {'f': 384, 'nvox': 8640, 'half': 1, 'mode': 0, 'feat': 256, 'ws': 1, 'cus': 256}
    line = lambda **kw: ' '.join(f'{k}={v}' for k, v in {**base, **kw}.items()) + ' ' + _counts((70, 3, 33))   # noqa: E731
    names = [r['accumulate']['name'] for r in route([line(), line(ws=0), line(mode=1), line(mode=2), line(f=380), line(feat=8), line(cus=8),
                                                      line(nvox=8642), line(feat=264, f=768)])]
    assert names == ['sim_mfma_kernel', 'sim_accumulate_split', 'sim_accumulate_split', 'sim_accumulate_split', 'sim_accumulate_split',
                     'sim_mfma_kernel', 'sim_mfma_kernel<2 voxel blocks>', 'sim_mfma_kernel', 'sim_accumulate']
    forms = [r['accumulate']['form'] for r in route([line(), line(feat=8), line(nvox=8642)])]
    assert forms == ['dma', 'strided', 'strided']
    assert route([line()], {'VITTF_SIM_MFMA': '0'})[0]['accumulate']['name'] == 'sim_accumulate_split'
    assert route([line()], {'VITTF_SIM_MFMA': '0', 'VITTF_SIM_SPLIT': '0'})[0]['accumulate']['name'] == 'sim_accumulate'


# (grid, output shape = vol_shape // 2) of test_quantize_16_per_thread_matches_bytewise_kernel and
# test_similarity_query_one_call_same_bytes, and the form VITTF_SIM_QUANT16=1 (the default) gives each
QUANT_CASES = [((8, 8, 8), (32, 32, 32), ('pow2', 2)),           # x 4
               ((6, 7, 5), (30, 35, 32), ('16', 0)),             # ratios 5, 5, 6.4
               ((16, 16, 16), (17, 10, 48), ('16', 0)),          # x 3 along the last dim
               ((8, 8, 8), (8, 8, 15), ('bytes', 0)),            # an output row of 15
               ((64, 64, 64), (256, 256, 256), ('pow2', 2)),     # the bench's query
               ((16, 16, 16), (32, 32, 32), ('pow2', 1)),
               ((16, 16, 16), (16, 16, 16), ('pow2', 0)),
               ((8, 8, 8), (8, 8, 128), ('pow2', 4))]            # x 16


@pytest.mark.parametrize('quant16', ['1', '2', '0', None])
def test_quantize_form(route, quant16):
    line = lambda g, o, out: f'classes=2 n2={g[2]} o0={o[0]} o1={o[1]} o2={o[2]} sim=256 out={out} counts=3,2'   # noqa: E731
    env = {} if quant16 is None else {'VITTF_SIM_QUANT16': quant16}
    aligned = route([line(g, o, 256) for g, o, _ in QUANT_CASES], env)
    off_by_one = route([line(g, o, 257) for g, o, _ in QUANT_CASES], env)
    for (g, o, (form, shift)), a, b in zip(QUANT_CASES, aligned, off_by_one):
        if quant16 == '2' and form == 'pow2':
            form, shift = '16', 0
        if quant16 == '0':
            form, shift = 'bytes', 0
        assert a['quantize'] == {'form': form, 'shift': shift}, (g, o)
        assert b['quantize'] == {'form': 'bytes', 'shift': 0}, (g, o)


PLAN_COUNTS = [(70, 3, 33), (17, 16, 1, 40), (1,) * 20, (2,) * 40, (16,), (1,), (1024, 200), (15,) + (1,) * 9]


@pytest.mark.parametrize('counts', PLAN_COUNTS, ids=['-'.join(map(str, c)) if len(c) <= 4 else f'{c[0]}-then-{c[-1]}x{len(c) - 1}' for c in PLAN_COUNTS])
def test_chunk_plan_properties(route, counts):
    chunks = route([_counts(counts)])[0]['chunks']
    start = sd.starts_of(counts)
    total, classes = int(start[-1]), len(counts)
    cls_of = np.repeat(np.arange(classes), counts)                   # class of every annotation
    a0 = 0
    touching = {c: [] for c in range(classes)}
    for i, ch in enumerate(chunks):
        n = ch['n']
        assert ch['a0'] == a0 and ch['n_ann'] == n and 1 <= n <= ACH            # the chunks partition [0, A) in order
        mine = cls_of[a0:a0 + n]
        assert ch['c0'] == mine[0] and ch['nc'] == mine[-1] - mine[0] + 1 and ch['nc'] <= MAXC
        assert ch['cls'] == [int(c) - ch['c0'] for c in mine] + [-1] * (ACH - n)
        # a chunk ends only at 16 annotations, at the end of the list, or in front of a ninth class
        assert n == ACH or a0 + n == total or cls_of[a0 + n] - ch['c0'] == MAXC
        for j in range(ch['nc']):
            touching[ch['c0'] + j].append((i, ch['first'][j], ch['last'][j], ch['count'][j]))
        assert all(ch['first'][j] == 0 and ch['last'][j] == 0 for j in range(ch['nc'], MAXC))
        a0 += n
    assert a0 == total
    for c in range(classes):
        seen = touching[c]
        assert [i for i, *_ in seen] == list(range(seen[0][0], seen[-1][0] + 1))      # consecutive chunks
        assert [f for _, f, _, _ in seen] == [1] + [0] * (len(seen) - 1)               # first: the earliest chunk, only
        assert [l for _, _, l, _ in seen] == [0] * (len(seen) - 1) + [1]               # last: the latest chunk, only
        assert all(k == counts[c] for *_, k in seen)


def test_chunk_plans_checked_by_hand(route):
    ones, mixed = route([_counts((1,) * 20), _counts((17, 16, 1, 40))])
    assert [ch['n'] for ch in ones['chunks']] == [8, 8, 4]
    assert (mixed['chunks'][2]['a0'], mixed['chunks'][2]['nc']) == (32, 3)
