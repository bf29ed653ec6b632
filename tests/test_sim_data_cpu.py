"""CPU: the host side of the similarity class-map tests (tests/sim_data.py) -- the fp64 reference against the oracle that
the reference's goldens pin, the derived bound against float32 emulations of the right arithmetic and of three subtly wrong
kernels (the GPU tests can fail), the share of entries on the 0.25 threshold in every GPU case, and the properties the
exact lattice rests on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import similarity as osim
import sim_data as sd

IDS = [sd.case_id(c) for c in sd.GPU_CASES]


def _ratio(got, d):
    err = (got.double() - d.ref).abs()
    return torch.where(d.bound > 0, err / d.bound.clamp_min(1e-300), torch.where(err > 0, float('inf'), 0.0).double())


# ---------------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize('normalized', [True, False])
def test_reference_matches_oracle(normalized):
    """oracle.similarity.class_similarity (fp32, pinned by the reference's goldens) lies within the bound of the fp64
    reference, entry by entry, incl. a one-annotation class and the cosine path (the oracle normalises the volume, the
    reference divides the dot product)."""
    grid, counts = (6, 7, 8), (5, 1, 12)
    d = sd.correlated(grid, counts, 64, 3, normalized)
    ref, bound, edge = sd.class_maps_ref(d.X, d.q, counts, d.vnorm)
    assert ref.shape == bound.shape == edge.shape == (3, 336) and ref.dtype == bound.dtype == torch.float64
    vol = d.X.float() if normalized else F.normalize(d.X.float(), dim=0)
    st = sd.starts_of(counts)
    for c in range(3):
        want = osim.class_similarity(vol.reshape(64, *grid), d.q[st[c]:st[c + 1]]).reshape(-1)
        assert float(want.max()) > 0.01
        assert bool(((want.double() - ref[c]).abs() <= bound[c]).all()), c
        assert torch.allclose(want.double()[~edge[c]], ref[c][~edge[c]], rtol=1e-5, atol=1e-8)
    # an fp32 rounding bound, not a tolerance: 2.5 (F + 8) 2^-24 at s = 1 is 1.1e-5 for F = 64
    assert float(bound[~edge].max()) < 2e-5


def test_reference_by_hand():
    """Two voxels, three queries, worked out by hand: 0.25 is kept (>=), a negative dot product is dropped."""
    X = torch.tensor([[1.0, 0.5], [0.0, 0.5]]).half()
    q = torch.tensor([[1.0, 0.0], [0.25, 0.0], [-1.0, 0.5]])
    ref, bound, edge = sd.class_maps_ref(X, q, (2, 1))
    assert ref[0].tolist() == pytest.approx([(1 + 2.0 ** -5) / 2, (0.5 ** 2.5 + 0) / 2], rel=1e-15) and ref[1].tolist() == [0.0, 0.0]
    assert edge.tolist() == [[True, False], [False, False]]
    assert float(bound[0, 0]) >= 0.25 ** 2.5 / 2 and float(bound[1].max()) == 0.0
    ref_n, _, _ = sd.class_maps_ref(X, q, (2, 1), vnorm=torch.tensor([2.0, 1.0]))
    assert ref_n[0].tolist() == pytest.approx([0.5 ** 2.5 / 2, 0.5 ** 2.5 / 2], rel=1e-15)


def test_generators():
    d = sd.correlated((6, 7, 8), (5, 1, 12), 384, 11)
    again = sd.correlated((6, 7, 8), (5, 1, 12), 384, 11)
    assert torch.equal(d.X, again.X) and torch.equal(d.q, again.q)
    assert d.X.dtype == torch.float16 and d.q.dtype == torch.float32 and d.X.shape == (384, 336) and d.q.shape == (18, 384)
    assert float((d.q.half().float() != d.q).float().mean()) > 0.9           # the queries need their lo halves
    assert torch.allclose(d.X.float().norm(dim=0), torch.ones(336), atol=2e-3)
    c = sd.correlated((6, 7, 8), (5, 1, 12), 384, 11, normalized=False)
    assert c.vnorm.dtype == torch.float32 and float(c.vnorm.min()) > 1.05
    assert torch.allclose(c.vnorm.double(), c.X.double().norm(dim=0), rtol=1e-7)
    t = sd.coherent_tails((6, 7, 8), (5, 1, 12), 384, 11)
    assert len(set(t.targets.tolist())) == 18
    h = t.X[:, t.targets].T
    assert torch.equal(t.q.half(), h) and bool(((t.q - h.float()) * h.float() >= 0).all())
    assert torch.equal((t.q - h.float()).double(), h.double() * 2.0 ** -12)


# ---------------------------------------------------------------------------------------------- the tests can fail
@pytest.mark.parametrize('counts', [(3,), (8,), (16,), (32,), (2,) * 40, (1024, 3)], ids=str)
def test_lost_lo_half_breaks_the_bound(counts):
    """Queries rounded once to fp16: at the targeted voxels of every class of at most 32 annotations the error is at least
    3 times the bound, while the hi + lo arithmetic stays inside it everywhere."""
    d = sd.case_data(sd.Case(grid=sd.G, counts=counts), 'tails')
    right = _ratio(sd.emulate(d), d)
    assert float(right.max()) <= 1.0
    wrong = _ratio(sd.emulate(d, 'no_lo'), d)
    st = sd.starts_of(counts)
    hit = [wrong[c, d.targets[st[c]:st[c + 1]]] for c, n in enumerate(counts) if n <= 32]
    lowest = min(float(h.min()) for h in hit)
    print(f'lo half lost, counts {counts}: error / bound at the targets >= {lowest:.2f}; right arithmetic <= {float(right.max()):.3f}')
    assert len(hit) >= 1 and lowest >= 3.0


@pytest.mark.parametrize('mutant', ['drop_last', 'pad_row'])
@pytest.mark.parametrize('counts', [(70, 3, 33), (1024, 200)], ids=str)
def test_miscounted_class_breaks_the_bound(counts, mutant):
    """One annotation dropped from, or one foreign query counted into, a class: at least 90 % of that class's voxels break
    the bound, also for 1 of 1024."""
    d = sd.case_data(sd.Case(grid=sd.G, counts=counts), 'correlated')
    assert float(_ratio(sd.emulate(d), d).max()) <= 1.0
    wrong = _ratio(sd.emulate(d, mutant), d)
    hit = [c for c, n in enumerate(counts) if mutant == 'drop_last' or n % 32]
    assert len(hit) >= 1
    for c in hit:
        share = float((wrong[c] > 1.0).float().mean())
        print(f'{mutant}, counts {counts}, class {c}: {100 * share:.1f} % of the voxels break the bound')
        assert share >= 0.9, (c, share)
    for c in set(range(len(counts))) - set(hit):
        assert float(wrong[c].max()) <= 1.0


@pytest.mark.parametrize('normalized', [True, False], ids=['unit', 'cosine'])
@pytest.mark.parametrize('case', sd.GPU_CASES, ids=IDS)
def test_edge_share_of_gpu_cases(case, normalized):
    """Reference-only condition of every GPU case: the threshold term widens the bound on at most 10 % of the entries, 1 %
    for classes of at most 100 annotations; and the maps are not trivially zero."""
    d = sd.case_data(case, 'correlated', normalized)
    sd.check_edge_share(d)
    assert float(d.ref.max()) > 0.01 and float(d.bound[~d.edge].max()) < 1e-4
    if normalized and sd.has_tails(case):
        sd.check_edge_share(sd.case_data(case, 'tails'))


# ---------------------------------------------------------------------------------------------- lattice
def _lattice_sums(d, act, cls):
    lit = d.X[d.feat].double()
    return torch.stack([(act[cls == c, None] * lit[cls == c]).sum(0) for c in range(len(d.counts))])


@pytest.mark.parametrize('grid,counts,f', [(sd.G, (70, 3, 33), 384), (sd.G, (1024, 200), 384), (sd.G, tuple(range(1, 34)), 384),
                                           (sd.CUBE, (2,) * 40, 768), (sd.ODD, (17, 16, 1, 40), 384), (sd.TINY, (9, 2), 384)],
                         ids=lambda p: str(p).replace(' ', ''))
def test_lattice_is_exact_and_sensitive(grid, counts, f):
    d = sd.lattice(grid, counts, f, 5)
    nvox = int(np.prod(grid))
    cls = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    assert set(d.X.unique().tolist()) <= {0.0, 1.0} and torch.equal(d.q.half().float(), d.q)
    assert int((d.q != 0).sum()) == len(cls) and set(d.q[d.q != 0].tolist()) <= set(sd.LATTICE_W)
    # exact in float32: multiples of 2^-5 below 2^24 * 2^-5, equal to what the definition gives
    assert torch.equal(d.sums, _lattice_sums(d, d.act, cls))
    assert torch.equal(d.sums * 32, (d.sums * 32).round()) and float(d.sums.max()) * 32 < 2 ** 24
    assert torch.equal(d.sums.float().double(), d.sums)
    ref, bound, _ = sd.class_maps_ref(d.X, d.q, counts)
    n = torch.tensor(counts, dtype=torch.float64)[:, None]
    assert torch.equal(ref, d.sums / n)
    got = sd.emulate(d)
    ulp = torch.from_numpy(np.spacing((d.sums / n).float().numpy())).double()
    assert bool(((got.double() - d.sums / n).abs() <= ulp).all())              # the division is the only inexact step
    pow2 = torch.tensor([c & (c - 1) == 0 for c in counts])
    assert torch.equal(got[pow2].double(), (d.sums / n)[pow2])
    # every annotation matches voxels in every full 256-voxel tile; neighbouring voxels differ; 0.25 sits on the threshold
    lit = d.X[d.feat] > 0
    full = nvox // sd.TILE * sd.TILE
    if full:
        assert bool(lit[:, :full].reshape(len(cls), -1, sd.TILE).any(2).all())
    else:
        assert bool(lit.any(1)[d.act > 0].all())
    assert bool((d.X[:, 1:] != d.X[:, :-1]).any(0).all())
    on_edge = (d.act == 2.0 ** -5)
    assert bool(on_edge.any()) and bool(lit[on_edge].any())
    strict = torch.where(d.act == 2.0 ** -5, torch.zeros_like(d.act), d.act)          # > instead of >=
    assert not torch.equal(_lattice_sums(d, strict, cls), d.sums)
    # any single annotation with a non-zero activation dropped, duplicated or counted into the neighbouring class moves the
    # sums of its class by its activation wherever its feature is lit -- and it is lit somewhere
    live = d.act > 0
    assert bool(lit[live].any(1).all()) and int(live.sum()) >= len(cls) // 2
    st = sd.starts_of(counts)
    for c in range(len(counts)):
        first, last = int(st[c]), int(st[c + 1]) - 1
        assert bool(live[first]) and bool(live[last])
        act = d.act.clone(); act[last] = 0                                            # dropped
        assert not torch.equal(_lattice_sums(d, act, cls)[c], d.sums[c])
        act = d.act.clone(); act[last] *= 2                                           # duplicated
        assert not torch.equal(_lattice_sums(d, act, cls)[c], d.sums[c])
        if c + 1 < len(counts):
            moved = cls.clone(); moved[last] = c + 1                                  # counted into the next class
            s = _lattice_sums(d, d.act, moved)
            assert not torch.equal(s[c], d.sums[c]) and not torch.equal(s[c + 1], d.sums[c + 1])
    for mutant in ('drop_last', 'pad_row'):
        assert not torch.equal(sd.emulate(d, mutant), got), mutant
    # a voxel read from the neighbouring column
    shifted = _lattice_sums(sd.SimpleNamespace(X=torch.roll(d.X, 1, 1), feat=d.feat, counts=counts), d.act, cls)
    assert float((shifted != d.sums).float().mean()) > 0.5
