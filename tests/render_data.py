"""The rendering model of include/vittf.h restated in numpy, and the scenes the render tests share.

``reference(scene, dtype)`` is vectorised over the pixels and loops over the lattice samples; it never skips anything, has
the kernel's T < 2^-10 stop, and runs in float64 (the truth) or float32 (its own rounding error, from which the tests take
their tolerance).  ``prepare`` and ``occupancy`` restate the two integer results, ``sample_sigma_by_brick`` the property the
occupancy grid must have.  Nothing here imports the code under test.
"""
import functools
import struct
import zlib

import numpy as np

STOP = 2.0 ** -10
TINY = 1e-30
BRICK = 8


# ---------------------------------------------------------------------------- volumes, maps, tables, cameras
def volume(shape, seed=0, touch_border=False):
    """fp32 volume: air (-1000) with a one-voxel air border, two planted blobs and mild noise; touch_border runs a slab of
    matter through the border on two sides."""
    rng = np.random.default_rng(seed)
    idx = np.indices(shape).astype(np.float64)
    n = np.asarray(shape, np.float64)[:, None, None, None]
    vol = np.full(shape, -1000.0)
    for centre, radius, value in (((0.35, 0.4, 0.45), 0.28, 400.0), ((0.7, 0.6, 0.55), 0.2, 1500.0)):
        c = np.asarray(centre)[:, None, None, None] * n
        r2 = (((idx + 0.5 - c) / (radius * n)) ** 2).sum(0)
        vol = np.where(r2 <= 1.0, value * (1.0 - 0.5 * r2), vol)
    vol += rng.normal(0.0, 5.0, shape)
    air = np.ones(shape, bool)
    air[1:-1, 1:-1, 1:-1] = False
    vol[air] = -1000.0
    if touch_border:
        vol[:, shape[1] // 2 - 1:shape[1] // 2 + 1, :shape[2] // 2] = 900.0
    return vol.astype(np.float32)


def prepare(vol, vmin=None, vmax=None):
    v = vol.astype(np.float64)
    vmin = float(vol.min()) if vmin is None else vmin
    vmax = float(vol.max()) if vmax is None else vmax
    return np.rint(65535.0 * np.clip((v - vmin) / (vmax - vmin), 0.0, 1.0)).astype(np.uint16)


def class_maps(classes, grid, seed=0, radius=0.3):
    """uint8 (C, m0, m1, m2): smooth bumps of `radius` (a share of the grid) at seeded centres, zero elsewhere."""
    rng = np.random.default_rng(100 + seed)
    idx = np.indices(grid).astype(np.float64)
    n = np.asarray(grid, np.float64)[:, None, None, None]
    out = np.zeros((classes,) + tuple(grid), np.uint8)
    for c in range(classes):
        centre = rng.uniform(0.25, 0.75, 3)[:, None, None, None] * n
        r2 = (((idx + 0.5 - centre) / (radius * n)) ** 2).sum(0)
        out[c] = np.rint(255.0 * np.clip(1.3 - 1.3 * r2, 0.0, 1.0)).astype(np.uint8)
    return out


def table(kind='ramp'):
    """fp32 (256, 4): 'ramp' is zero up to entry 40 and rises after it (so air is clear), 'zero' has no extinction at all,
    'dense' is strong enough for rays to reach the T stop."""
    x = np.arange(256, dtype=np.float64) / 255.0
    t = np.zeros((256, 4), np.float64)
    t[:, 0], t[:, 1], t[:, 2] = 0.3 + 0.7 * x, 0.2 + 0.5 * x, 1.0 - 0.8 * x
    if kind == 'ramp':
        t[:, 3] = 0.08 * np.clip((x - 40 / 255.0) / (1 - 40 / 255.0), 0.0, 1.0)
    elif kind == 'dense':
        t[:, 3] = 1.5 * np.clip((x - 40 / 255.0) / (1 - 40 / 255.0), 0.0, 1.0)
    elif kind != 'zero':
        raise ValueError(kind)
    return t.astype(np.float32)


def _basis(fwd, up=(0.0, 0.0, 1.0)):
    fwd = np.asarray(fwd, np.float64) / np.linalg.norm(fwd)
    right = np.cross(fwd, up)
    if np.linalg.norm(right) < 1e-6:
        right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    return fwd, right, np.cross(right, fwd)


def camera(kind, shape, spacing):
    """fp32 (6, 3): eye, ox, oy, fwd, dx, dy.  'axis0' .. 'axis2': orthographic with rays exactly along an axis (zero direction
    components); 'oblique': orthographic; 'outside' / 'inside': perspective with the eye outside / inside the box; 'miss':
    every ray passes beside the box."""
    ext = np.asarray(shape, np.float64) * np.asarray(spacing, np.float64)
    centre, radius = ext / 2, np.linalg.norm(ext) / 2
    zero = np.zeros(3)
    if kind in ('axis0', 'axis1', 'axis2'):
        a = int(kind[-1])
        fwd = np.eye(3)[a]
        right, upv = np.eye(3)[(a + 1) % 3], np.eye(3)[(a + 2) % 3]
        cam = (centre - fwd * 2 * radius, right * 0.55 * ext[(a + 1) % 3], upv * 0.55 * ext[(a + 2) % 3], fwd, zero, zero)
    elif kind == 'oblique':
        fwd, right, upv = _basis((-0.6, -0.5, -0.45))
        cam = (centre - fwd * 2 * radius, right * radius * 0.9, upv * radius * 0.7, fwd, zero, zero)
    elif kind == 'outside':
        fwd, right, upv = _basis((0.7, -0.55, -0.35))
        cam = (centre - fwd * 2.2 * radius, zero, zero, fwd, right * 0.55, upv * 0.42)
    elif kind == 'inside':
        fwd, right, upv = _basis((-0.3, 0.8, 0.25))
        cam = (centre - fwd * 0.15 * radius, zero, zero, fwd, right * 0.8, upv * 0.6)
    elif kind == 'miss':
        fwd, right, upv = _basis((0.0, 1.0, 0.0))
        cam = (centre - fwd * 2 * radius + np.array([3.0 * ext[0], 0.0, 0.0]), right * 0.5 * ext[0], upv * 0.5 * ext[2], fwd, zero, zero)
    else:
        raise ValueError(kind)
    return np.asarray(cam, np.float32)


# ---------------------------------------------------------------------------- the scenes
# name: (volume shape, touch border, map grid, classes, (width, height), camera, spacing, dt, shading, table)
SHADE = (0.3, 0.7, 600.0)
FLAT = (1.0, 0.0, 1.0)
SCENES = {
    'axis0_c0':        ((9, 11, 13), False, None, 0, (33, 17), 'axis0', (1, 1, 1), 0.5, FLAT, 'ramp'),
    'axis1_c1':        ((9, 11, 13), False, (5, 6, 7), 1, (33, 17), 'axis1', (1, 1, 1), 1.0, SHADE, 'ramp'),
    'axis2_c3':        ((32, 32, 32), False, (8, 8, 8), 3, (64, 48), 'axis2', (1, 1, 2.5), 0.5, SHADE, 'ramp'),
    'oblique_c3':      ((32, 32, 32), False, (5, 6, 7), 3, (64, 48), 'oblique', (1, 1, 1), 0.5, SHADE, 'ramp'),
    'oblique_c8_flat': ((40, 24, 17), True, (8, 8, 8), 8, (33, 17), 'oblique', (1, 1, 2.5), 1.0, FLAT, 'ramp'),
    'outside_c8':      ((40, 24, 17), True, (5, 6, 7), 8, (64, 48), 'outside', (1, 1, 1), 0.5, SHADE, 'ramp'),
    'outside_dense':   ((32, 32, 32), False, (8, 8, 8), 1, (64, 48), 'outside', (1, 1, 1), 0.5, SHADE, 'dense'),
    'inside_c3':       ((40, 24, 17), True, (8, 8, 8), 3, (64, 48), 'inside', (1, 1, 2.5), 0.5, SHADE, 'ramp'),
    'inside_c0_dense': ((32, 32, 32), False, None, 0, (33, 17), 'inside', (1, 1, 1), 1.0, FLAT, 'dense'),
    'miss_c1':         ((9, 11, 13), False, (5, 6, 7), 1, (33, 17), 'miss', (1, 1, 1), 0.5, SHADE, 'ramp'),
    'zero_sigma_c3':   ((32, 32, 32), False, (8, 8, 8), 3, (33, 17), 'oblique', (1, 1, 1), 0.5, SHADE, 'zero'),
    'zero_table_c0':   ((9, 11, 13), False, None, 0, (64, 48), 'outside', (1, 1, 2.5), 1.0, SHADE, 'zero'),
    'sparse_c3':       ((40, 24, 17), False, (8, 8, 8), 3, (64, 48), 'oblique', (1, 1, 1), 0.5, SHADE, 'ramp'),
}
MAP_RADIUS = {'sparse_c3': 0.15}                   # small class bodies: runs of empty bricks along the long axis
ZERO_SCENES = ('miss_c1', 'zero_sigma_c3', 'zero_table_c0')
OCCUPANCY_SCENES = ('sparse_c3', 'inside_c3', 'outside_dense')


@functools.lru_cache(maxsize=None)
def scene(name):
    """The inputs of one scene as a dict of numpy arrays and numbers (built once; treat as read-only)."""
    shape, touch, grid, classes, size, cam, spacing, dt, shade, tab = SCENES[name]
    vol = volume(shape, seed=sum(shape), touch_border=touch)
    s = {'name': name, 'volume': vol, 'q': prepare(vol), 'spacing': np.asarray(spacing, np.float32), 'table': table(tab),
         'size': size, 'camera': camera(cam, shape, spacing), 'dt': float(dt), 'shade': np.asarray(shade, np.float32),
         'maps': None, 'lo': [], 'hi': [], 'colors': np.zeros((0, 3), np.float32), 'strengths': np.zeros((0,), np.float32)}
    if classes:
        rng = np.random.default_rng(classes)
        s['maps'] = class_maps(classes, grid, seed=classes, radius=MAP_RADIUS.get(name, 0.3))
        s['lo'] = [int(v) for v in rng.integers(20, 100, classes)]
        s['hi'] = [int(v) for v in rng.integers(140, 256, classes)]
        s['colors'] = rng.uniform(0.1, 1.0, (classes, 3)).astype(np.float32)
        strength = 0.0 if name == 'zero_sigma_c3' else (2.0 if tab == 'dense' else 0.25)
        s['strengths'] = (strength * rng.uniform(0.5, 1.0, classes)).astype(np.float32)
    return s


# ---------------------------------------------------------------------------- the model
def _trilinear(grid, x, dtype):
    """Border-clamped trilinear value of grid (3-D array) at index coordinates x (3, N), clamped to the corners' range; also
    floor(x) as integers and the fractions."""
    fl = np.floor(x)
    f = (x - fl).astype(dtype)
    i0 = fl.astype(np.int64)
    val, flat = _corner_lerp(grid, i0, f, dtype)
    return np.clip(val, flat.min(0), flat.max(0)), i0, f


def _corner_lerp(grid, i0, f, dtype):
    """(the trilinear value of the cell at i0 (3, N) with fractions f, its eight border-clamped corner values (8, N))."""
    hi = np.asarray(grid.shape, np.int64)[:, None] - 1
    a, b = np.clip(i0, 0, hi), np.clip(i0 + 1, 0, hi)
    g = grid.astype(dtype)
    c = [[[g[(a, b)[j0][0], (a, b)[j1][1], (a, b)[j2][2]] for j2 in (0, 1)] for j1 in (0, 1)] for j0 in (0, 1)]
    lerp = lambda p, q, w: p + w * (q - p)                     # noqa: E731
    plane = [lerp(lerp(c[j0][0][0], c[j0][0][1], f[2]), lerp(c[j0][1][0], c[j0][1][1], f[2]), f[1]) for j0 in (0, 1)]
    return lerp(plane[0], plane[1], f[0]), np.stack([c[j0][j1][j2] for j0 in (0, 1) for j1 in (0, 1) for j2 in (0, 1)])


def _shifted(grid, i0, f, axis, shift, dtype):
    """The trilinear value one voxel along `axis` (shift +1 or -1) with the centre's fractions, border-clamped."""
    j = i0.copy()
    j[axis] += shift
    return _corner_lerp(grid, j, f, dtype)[0]


def rays(s, dtype):
    """Origins (3, N), unit directions (3, N), first and last lattice index (N,; first > last for a miss), row-major pixels."""
    w, h = s['size']
    cam = s['camera'].astype(dtype)
    sp = s['spacing'].astype(dtype)
    n = np.asarray(s['q'].shape, dtype)
    dt = dtype(s['dt'])
    px, py = np.meshgrid(np.arange(w, dtype=dtype), np.arange(h, dtype=dtype))
    u = (dtype(2) * (px.ravel() + dtype(0.5)) / dtype(w) - dtype(1)).astype(dtype)
    v = (dtype(1) - dtype(2) * (py.ravel() + dtype(0.5)) / dtype(h)).astype(dtype)
    o = cam[0][:, None] + u[None] * cam[1][:, None] + v[None] * cam[2][:, None]
    d = cam[3][:, None] + u[None] * cam[4][:, None] + v[None] * cam[5][:, None]
    d = d / np.sqrt((d * d).sum(0))[None]
    tmin, tmax = np.zeros(o.shape[1], dtype), np.full(o.shape[1], np.inf, dtype)
    hit = np.ones(o.shape[1], bool)
    for a in range(3):
        lo, hi = dtype(-0.5) * sp[a], (n[a] + dtype(0.5)) * sp[a]
        par = d[a] == 0
        hit &= ~par | ((o[a] >= lo) & (o[a] <= hi))
        da = np.where(par, dtype(1), d[a])
        t1, t2 = (lo - o[a]) / da, (hi - o[a]) / da
        tmin = np.where(par, tmin, np.maximum(tmin, np.minimum(t1, t2)))
        tmax = np.where(par, tmax, np.minimum(tmax, np.maximum(t1, t2)))
    hit &= tmin <= tmax
    first = np.where(hit, np.maximum(np.ceil(np.where(hit, tmin, 0) / dt - dtype(0.5)), 0), 1).astype(np.int64)
    last = np.where(hit, np.floor(np.where(hit, tmax, 0) / dt - dtype(0.5)), 0).astype(np.int64)
    return o.astype(dtype), d.astype(dtype), first, last


def sample(s, o, d, i, dtype):
    """Everything the model says about lattice sample i of the rays (o, d): total sigma (N,), sum_k sigma_k rgb_k (3, N), the
    shade (N,) and floor(x) of the intensity grid (3, N)."""
    sp = s['spacing'].astype(dtype)[:, None]
    n = np.asarray(s['q'].shape, dtype)[:, None]
    t = (dtype(i) + dtype(0.5)) * dtype(s['dt'])
    p = (o + t * d).astype(dtype)
    x = (p / sp - dtype(0.5)).astype(dtype)
    inten, i0, f = _trilinear(s['q'], x, dtype)
    ni = np.asarray(s['q'].shape, np.int64)[:, None]
    cov_axis = np.where((i0 >= 0) & (i0 < ni), dtype(1) - f, dtype(0)) + np.where((i0 >= -1) & (i0 < ni - 1), f, dtype(0))
    cov = cov_axis[0] * cov_axis[1] * cov_axis[2]
    tab = s['table'].astype(dtype)
    tc = inten / dtype(257)
    ti = np.minimum(tc.astype(np.int64), 254)
    tf = (tc - ti.astype(dtype))[:, None]
    entry = tab[ti] + tf * (tab[ti + 1] - tab[ti])
    sigma = (entry[:, 3] * cov).astype(dtype)
    colour = sigma[None] * entry[:, :3].T
    if s['maps'] is not None:
        m = np.asarray(s['maps'].shape[1:], dtype)[:, None]
        xm = (p / (n * sp) * m - dtype(0.5)).astype(dtype)
        for k in range(s['maps'].shape[0]):
            val = _trilinear(s['maps'][k], xm, dtype)[0]
            omega = np.clip((val - dtype(s['lo'][k])) / dtype(s['hi'][k] - s['lo'][k]), dtype(0), dtype(1))
            sk = (s['strengths'].astype(dtype)[k] * omega * cov).astype(dtype)
            sigma = sigma + sk
            colour = colour + sk[None] * s['colors'].astype(dtype)[k][:, None]
    ka, kd, eps = (dtype(v) for v in s['shade'])
    shade = np.full(sigma.shape, ka, dtype)
    if kd != 0:
        g = np.stack([(_shifted(s['q'], i0, f, a, 1, dtype) - _shifted(s['q'], i0, f, a, -1, dtype)) / (dtype(2) * sp[a, 0])
                      for a in range(3)])
        shade = ka + kd * np.abs((g * d).sum(0)) / (np.sqrt((g * g).sum(0)) + eps)
    return sigma.astype(dtype), colour.astype(dtype), shade.astype(dtype), i0


def reference(s, dtype=np.float64):
    """(image (h, w, 4) in dtype, the smallest transmittance any ray had when it was last tested against the stop)."""
    w, h = s['size']
    o, d, first, last = rays(s, dtype)
    npx = o.shape[1]
    rgb, alpha, trans = np.zeros((3, npx), dtype), np.zeros(npx, dtype), np.ones(npx, dtype)
    alive = first <= last
    dt = dtype(s['dt'])
    if alive.any():
        for i in range(int(first[alive].min()), int(last[alive].max()) + 1):
            on = alive & (first <= i) & (i <= last)
            if not on.any():
                continue
            idx = np.nonzero(on)[0]
            sigma, colour, shade, _ = sample(s, o[:, idx], d[:, idx], i, dtype)
            a = (dtype(1) - np.exp(-sigma * dt)).astype(dtype)
            wgt = trans[idx] * a * shade / np.maximum(sigma, dtype(TINY))
            wgt = np.where(sigma > 0, wgt, dtype(0))
            rgb[:, idx] += (wgt[None] * colour).astype(dtype)
            alpha[idx] += (trans[idx] * a).astype(dtype)
            trans[idx] = (trans[idx] * (dtype(1) - a)).astype(dtype)
            alive[idx[trans[idx] < dtype(STOP)]] = False
    img = np.concatenate([rgb, alpha[None]]).T.reshape(h, w, 4)
    assert img.dtype == dtype
    return img, float(trans.min())


@functools.lru_cache(maxsize=None)
def references(name):
    """(fp64 image, fp32 image, smallest transmittance of the fp64 run) of a scene, computed once."""
    s = scene(name)
    img64, tmin = reference(s, np.float64)
    img32, _ = reference(s, np.float32)
    return img64, img32, tmin


def tolerance(name):
    """8 max|ref32 - ref64| -- the factor for another operation order and the hardware exp -- plus 2^-10 where some ray of the
    fp64 run gets below T = 2^-9: the most one disagreeing stop decision can cost."""
    img64, img32, tmin = references(name)
    own = float(np.abs(img32.astype(np.float64) - img64).max())
    return 8.0 * own + (STOP if tmin < 2.0 ** -9 else 0.0), own, tmin


# ---------------------------------------------------------------------------- occupancy
def occupancy(s):
    """uint8 brick grid by the integer rule of include/vittf.h (0 = empty)."""
    q = s['q']
    n = q.shape
    nb = tuple((x + BRICK - 1) // BRICK for x in n)
    occ = np.zeros(nb, np.uint8)
    sig = s['table'][:, 3]
    for b in np.ndindex(*nb):
        sl = tuple(slice(8 * b[a], min(8 * b[a] + 8, n[a] - 1) + 1) for a in range(3))
        qmin, qmax = int(q[sl].min()), int(q[sl].max())
        full = bool((sig[qmin // 257:min(255, qmax // 257 + 1) + 1] != 0).any())
        if not full and s['maps'] is not None:
            m = s['maps'].shape[1:]
            ml = tuple(slice(max(0, (8 * b[a] - 1) * m[a] // n[a] - 1), min(m[a] - 1, (8 * b[a] + 10) * m[a] // n[a] + 1) + 1)
                       for a in range(3))
            full = any(int(s['maps'][k][ml].max()) > s['lo'][k] for k in range(s['maps'].shape[0]))
        occ[b] = 1 if full else 0
    return occ


def sample_sigma_by_brick(s):
    """The largest fp64 sigma of any lattice sample of the scene's rays per brick (a grid of the occupancy's shape)."""
    dtype = np.float64
    o, d, first, last = rays(s, dtype)
    n = np.asarray(s['q'].shape, np.int64)
    nb = tuple((x + BRICK - 1) // BRICK for x in s['q'].shape)
    top = np.zeros(nb, np.float64)
    alive = first <= last
    if not alive.any():
        return top
    for i in range(int(first[alive].min()), int(last[alive].max()) + 1):
        idx = np.nonzero(alive & (first <= i) & (i <= last))[0]
        if idx.size == 0:
            continue
        sigma, _, _, i0 = sample(s, o[:, idx], d[:, idx], i, dtype)
        b = np.clip(i0, 0, n[:, None] - 1) // BRICK
        np.maximum.at(top, (b[0], b[1], b[2]), sigma)
    return top


# ---------------------------------------------------------------------------- reading a PNG back
def decode_png(path):
    """(h, w, channels) uint8 of a non-interlaced 8-bit PNG whose rows all use filter 0, with every chunk's CRC checked."""
    raw = open(path, 'rb').read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n'
    at, chunks = 8, []
    while at < len(raw):
        n, = struct.unpack('>I', raw[at:at + 4])
        kind, body = raw[at + 4:at + 8], raw[at + 8:at + 8 + n]
        assert struct.unpack('>I', raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks][0] == b'IHDR' and chunks[-1] == (b'IEND', b'')
    w, h, depth, color, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    ch = {0: 1, 2: 3, 6: 4}[color]
    rows = np.frombuffer(zlib.decompress(b''.join(b for k, b in chunks if k == b'IDAT')), np.uint8).reshape(h, 1 + w * ch)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, ch)
