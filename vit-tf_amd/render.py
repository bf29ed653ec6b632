"""Direct volume rendering of an intensity volume with class maps or a label volume as per-class opacity.

``prepare`` turns the fp32 volume into the uint16 copy every gather reads, ``occupancy`` marks the 8^3 bricks that no sample
can see, ``render`` marches one ray per pixel (libvittf's render.hip: manual trilinear gathers, one lane per ray in 8 x 8
screen tiles, jumps over empty bricks) and returns premultiplied fp32 RGBA on the device.  ``Camera.orbit`` places an
orthographic or a perspective camera around the volume, ``maps_from_labels`` makes one-hot 0/255 maps of a label volume
(their trilinear interpolation gives smooth surfaces), ``composite`` puts an image over a background and ``write_png``
writes it with the standard library alone.  The rendering model is stated in include/vittf.h.  Torch only allocates and
does the arithmetic of the final composite; the three passes over the volume are HIP kernels and there is no CPU path.
"""
import ctypes as C
import math
import struct
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

MAX_DIM = _lib.RENDER_MAX_DIM
MAX_IMAGE = _lib.RENDER_MAX_IMAGE
MAX_CLASSES = _lib.RENDER_MAX_CLASSES
BRICK = 8
# a fixed palette for the classes 1..8 (Okabe and Ito's colour-blind-safe eight, black replaced by white)
PALETTE = ((0.90, 0.62, 0.00), (0.34, 0.71, 0.91), (0.00, 0.62, 0.45), (0.94, 0.89, 0.26),
           (0.00, 0.45, 0.70), (0.84, 0.37, 0.00), (0.80, 0.47, 0.65), (1.00, 1.00, 1.00))
SHADING = (0.35, 0.65, 655.35)            # ka, kd, eps: eps is 1 % of the intensity range per world unit
NO_SHADING = (1.0, 0.0, 1.0)


def _vec3(v, what, positive=False):
    try:
        a = np.asarray([float(x) for x in v], np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'{what} must be three numbers, got {v!r}') from None
    if a.shape != (3,) or not np.isfinite(a).all() or (positive and not (a > 0).all()):
        raise ValueError(f'{what} must be three finite{" positive" if positive else ""} numbers, got {v!r}')
    return a


def _check_shape(shape, what='the volume'):
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or min(shape) < 2 or max(shape) > MAX_DIM or shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError(f'{what} of shape {shape} cannot be rendered (three dimensions in 2..{MAX_DIM}, fewer than 2^31 voxels)')
    return shape


@dataclass(frozen=True)
class Camera:
    """Pixel (u, v) in [-1, 1]^2 (u right, v up) starts at eye + u ox + v oy and looks along fwd + u dx + v dy, in world units
    (volume axis a runs from 0 to n_a s_a).  Orthographic: dx = dy = 0; perspective: ox = oy = 0."""
    eye: tuple
    ox: tuple
    oy: tuple
    fwd: tuple
    dx: tuple
    dy: tuple

    def vectors(self):
        """The 18 floats of vittf_render's camera_host: eye, ox, oy, fwd, dx, dy."""
        v = np.asarray([self.eye, self.ox, self.oy, self.fwd, self.dx, self.dy], np.float32)
        if v.shape != (6, 3) or not np.isfinite(v).all() or not np.any(v[3]):
            raise ValueError('a camera is six finite 3-vectors with fwd != 0')
        return v

    @staticmethod
    def orbit(azimuth, elevation, distance=None, fov=None, *, shape, spacing=(1.0, 1.0, 1.0), aspect=1.0):
        """A camera on a sphere around the centre of the box, looking at it.  azimuth turns about volume axis 2 from axis 0
        towards axis 1, elevation rises towards +axis 2 (degrees); axis 2 points up in the image (axis 1 at the poles).
        distance: eye to centre (default: outside the box's circumscribed sphere).  fov None: orthographic, the image spans
        the circumscribed sphere along its shorter side; else the vertical field of view of a perspective camera in degrees.
        aspect = width / height of the image."""
        shape = _check_shape(shape)
        s = _vec3(spacing, 'spacing', positive=True)
        az, el = math.radians(float(azimuth)), math.radians(float(elevation))
        if not (math.isfinite(az) and math.isfinite(el) and float(aspect) > 0 and math.isfinite(float(aspect))):
            raise ValueError('azimuth, elevation and aspect must be finite, aspect > 0')
        if fov is not None and not 0 < float(fov) < 180:
            raise ValueError(f'fov must lie in (0, 180) degrees, got {fov!r}')
        ext = np.asarray(shape, np.float64) * s
        centre, radius = ext / 2, float(np.linalg.norm(ext)) / 2
        out = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        fwd = -out
        up = np.array([0.0, 0.0, 1.0])
        right = np.cross(fwd, up)
        if np.linalg.norm(right) < 1e-6:
            right = np.cross(fwd, np.array([0.0, 1.0, 0.0]))
        right /= np.linalg.norm(right)
        upv = np.cross(right, fwd)
        wide, tall = max(float(aspect), 1.0), max(1.0 / float(aspect), 1.0)
        zero = (0.0, 0.0, 0.0)
        if fov is None:
            dist = 2.0 * radius if distance is None else float(distance)
            half = radius
            cam = (centre + dist * out, right * half * wide, upv * half * tall, fwd, zero, zero)
        else:
            tan = math.tan(math.radians(float(fov)) / 2)
            dist = 1.1 * radius / math.sin(math.radians(float(fov)) / 2) if distance is None else float(distance)
            cam = (centre + dist * out, zero, zero, fwd, right * tan * float(aspect), upv * tan)
        if not (math.isfinite(dist) and dist >= 0):
            raise ValueError(f'distance must be a finite number >= 0, got {distance!r}')
        return Camera(*(tuple(float(x) for x in v) for v in cam))


def sigma_from_opacity(opacity, length):
    """The extinction per world unit under which a homogeneous slab `length` thick has the given opacity (0 <= opacity < 1)."""
    opacity = np.asarray(opacity, np.float64)
    if not (np.isfinite(opacity).all() and (opacity >= 0).all() and (opacity < 1).all() and length > 0):
        raise ValueError('opacity must lie in [0, 1) and length must be > 0')
    return -np.log1p(-opacity) / float(length)


def ramp_table(opacity=0.9, length=32.0, start=0.15, color=(1.0, 1.0, 1.0)):
    """The default transfer function without maps: a grey ramp.  Nothing below `start` of the intensity range, then the opacity
    per `length` world units rises linearly to `opacity` at the top; the colour rises with the intensity."""
    x = np.linspace(0.0, 1.0, 256)
    table = np.zeros((256, 4), np.float32)
    table[:, :3] = (np.asarray(color, np.float64)[None] * (0.25 + 0.75 * x[:, None])).astype(np.float32)
    table[:, 3] = sigma_from_opacity(np.clip((x - start) / (1.0 - start), 0.0, 1.0) * opacity, length)
    return table


def context_table(opacity=0.08, length=32.0, start=0.15):
    """The default transfer function beside class maps: a faint grey context, so that the classes carry the image."""
    return ramp_table(opacity, length, start, (0.8, 0.8, 0.8))


def _check_table(table):
    t = torch.as_tensor(table)
    if t.dtype != torch.float32 or tuple(t.shape) != (256, 4):
        raise ValueError(f'a transfer function is a float32 (256, 4) table of (r, g, b, sigma), got {t.dtype} {tuple(t.shape)}')
    if not bool(torch.isfinite(t).all()) or bool((t[:, 3] < 0).any()):
        raise ValueError('a transfer function must be finite with sigma >= 0')
    return t


def _check_q(q):
    if not isinstance(q, torch.Tensor) or q.dtype != torch.uint16 or q.ndim != 3:
        raise ValueError('q must be the uint16 device volume that prepare() returns')
    _check_shape(q.shape)
    return q


def _check_maps(maps, lo, hi=None):
    """(maps or None, lo list, hi list): uint8 (C, m0, m1, m2) with C <= 8 and integer thresholds 0 <= lo < hi <= 255."""
    if maps is None:
        return None, [], []
    t = maps if isinstance(maps, torch.Tensor) else torch.as_tensor(np.asarray(maps))
    if t.dtype != torch.uint8 or t.ndim != 4:
        raise ValueError(f'maps must be uint8 (C, m0, m1, m2), got {t.dtype} {tuple(t.shape)}')
    c = int(t.shape[0])
    if c > MAX_CLASSES:
        raise ValueError(f'{c} class maps: at most {MAX_CLASSES} can be rendered')
    if c == 0:
        return None, [], []
    _check_shape(t.shape[1:], 'a class map')

    def levels(v, default, what):
        v = [default] * c if v is None else ([v] * c if np.ndim(v) == 0 else list(v))
        if len(v) != c or not all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) and 0 <= int(x) <= 255 for x in v):
            raise ValueError(f'{what} must be {c} integers in 0..255, got {v!r}')
        return [int(x) for x in v]

    lo, hi = levels(lo, 64, 'lo'), levels(hi, 192, 'hi')
    if not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f'every lo must be below its hi, got lo {lo} and hi {hi}')
    return t, lo, hi


def _on_device(t, device=None):
    if device is None:
        device = t.device if t.is_cuda else torch.device('cuda', torch.cuda.current_device())
    return t.to(device=device).contiguous()


def prepare(volume, vmin=None, vmax=None):
    """The uint16 device copy of an fp32 (n0, n1, n2) volume that occupancy() and render() read:
    rint(65535 clamp((V - vmin) / (vmax - vmin), 0, 1)), computed in fp64 (vittf_render_prepare).  vmin, vmax default to the
    volume's own extremes; a constant volume has no range and is refused."""
    t = volume if isinstance(volume, torch.Tensor) else torch.as_tensor(np.asarray(volume))
    if t.dtype != torch.float32 or t.ndim != 3:
        raise ValueError(f'the volume must be float32 with 3 dimensions, got {t.dtype} {tuple(t.shape)}')
    shape = _check_shape(t.shape)
    for v in (vmin, vmax):
        if v is not None and not math.isfinite(float(v)):
            raise ValueError('vmin and vmax must be finite')
    lib = _lib.require_device()
    src = _on_device(t)
    vmin = float(src.min()) if vmin is None else float(vmin)
    vmax = float(src.max()) if vmax is None else float(vmax)
    if not (math.isfinite(vmin) and math.isfinite(vmax) and vmin < vmax):
        raise ValueError(f'the intensity window [{vmin}, {vmax}] is empty or not finite')
    q = torch.empty(shape, dtype=torch.uint16, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.vittf_render_prepare(_lib.ptr(src), src.numel(), vmin, vmax, _lib.ptr(q), _lib.stream_ptr()),
                   'vittf_render_prepare')
    return q


def maps_from_labels(labels, values=None):
    """One-hot uint8 maps (C, n0, n1, n2) of 0 / 255 on the labels' own grid, map c for values[c] (default: 1 .. the largest
    label).  A tensor on the labels' device (numpy labels: on the CPU)."""
    t = labels if isinstance(labels, torch.Tensor) else torch.as_tensor(np.asarray(labels))
    if t.dtype != torch.uint8 or t.ndim != 3:
        raise ValueError(f'labels must be a uint8 volume with 3 dimensions, got {t.dtype} {tuple(t.shape)}')
    values = list(range(1, int(t.max()) + 1)) if values is None else [int(v) for v in values]
    if not values or len(values) > MAX_CLASSES or not all(0 <= v <= 255 for v in values):
        raise ValueError(f'{len(values)} label values: 1..{MAX_CLASSES} values in 0..255 can be rendered')
    sel = torch.tensor(values, dtype=torch.uint8, device=t.device).view(-1, 1, 1, 1)
    return (t[None] == sel).to(torch.uint8) * 255


def occupancy(q, table, maps=None, lo=None):
    """uint8 device tensor (ceil(n0 / 8), ceil(n1 / 8), ceil(n2 / 8)): 0 for every 8^3 brick of q in which no sample can have
    sigma > 0 under this table, these maps and these lower thresholds (vittf_render_occupancy)."""
    q = _check_q(q)
    table = _check_table(table)
    maps, lo, _ = _check_maps(maps, lo)
    lib = _lib.require_device()
    return _occupancy(lib, q, _on_device(table, q.device), None if maps is None else _on_device(maps, q.device), lo)


def _occupancy(lib, q, table, maps, lo):
    n = tuple(int(x) for x in q.shape)
    occ = torch.empty(tuple((x + BRICK - 1) // BRICK for x in n), dtype=torch.uint8, device=q.device)
    assert occ.numel() == lib.vittf_render_occupancy_bytes(*n)
    c = 0 if maps is None else int(maps.shape[0])
    m = (0, 0, 0) if maps is None else tuple(int(x) for x in maps.shape[1:])
    with torch.cuda.device(q.device):
        _lib.check(lib.vittf_render_occupancy(_lib.ptr(q), *n, _lib.ptr(table), _lib.ptr(maps), c, *m, (C.c_int32 * 8)(*lo),
                                              _lib.ptr(occ), _lib.stream_ptr()), 'vittf_render_occupancy')
    return occ


def render(q, camera, size, spacing=(1.0, 1.0, 1.0), table=None, maps=None, lo=None, hi=None, colors=None, strengths=None,
           step=0.5, shading=SHADING, occupancy='auto', out=None):
    """Premultiplied fp32 RGBA (height, width, 4) on q's device (vittf_render).
      q          the uint16 volume of prepare();          camera   a Camera;          size   (width, height)
      spacing    world units per voxel along (n0, n1, n2);  step    the sample distance dt in world units
      table      float32 (256, 4) of (r, g, b, sigma per world unit); default ramp_table(), with maps context_table()
      maps       uint8 (C, m0, m1, m2), C <= 8, on any grid over the same box; lo, hi: integer levels (one or C of them,
                 default 64 and 192) between which a class turns from clear to its full strength
      colors     C (r, g, b) (default PALETTE);   strengths   C extinctions per world unit at omega = 1 (default: opacity
                 0.9 per 4 world units)
      shading    (ka, kd, eps) of the headlight, or None for none
      occupancy  'auto': build the brick grid first; None: march without it; or the tensor of occupancy() for these arguments
      out        a float32 (height, width, 4) device tensor to fill."""
    q = _check_q(q)
    if not isinstance(camera, Camera):
        raise ValueError('camera must be a render.Camera')
    cam = camera.vectors()
    try:
        width, height = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f'size must be (width, height), got {size!r}') from None
    if not (1 <= width <= MAX_IMAGE and 1 <= height <= MAX_IMAGE):
        raise ValueError(f'an image of {width} x {height} cannot be rendered (1..{MAX_IMAGE} each way)')
    sp = _vec3(spacing, 'spacing', positive=True)
    if not (isinstance(step, (int, float, np.floating, np.integer)) and math.isfinite(float(step)) and float(step) > 0):
        raise ValueError(f'step must be a finite number > 0, got {step!r}')
    maps, lo, hi = _check_maps(maps, lo, hi)
    c = 0 if maps is None else int(maps.shape[0])
    table = _check_table((context_table() if c else ramp_table()) if table is None else table)
    colors = np.asarray(PALETTE[:c] if colors is None else colors, np.float32).reshape(-1, 3)
    strengths = np.full((c,), sigma_from_opacity(0.9, 4.0), np.float32) if strengths is None else np.asarray(strengths, np.float32).reshape(-1)
    if colors.shape[0] != c or strengths.shape[0] != c or not (np.isfinite(colors).all() and np.isfinite(strengths).all() and (strengths >= 0).all()):
        raise ValueError(f'colors and strengths must hold {c} finite entries each, strengths >= 0')
    shade = np.asarray(NO_SHADING if shading is None else shading, np.float32).reshape(-1)
    if shade.shape != (3,) or not (np.isfinite(shade).all() and shade[0] >= 0 and shade[1] >= 0 and shade[2] > 0):
        raise ValueError(f'shading must be (ka >= 0, kd >= 0, eps > 0), got {shading!r}')
    if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == (height, width, 4)
                                and out.is_contiguous() and out.device == q.device):
        raise ValueError(f'out must be a contiguous float32 ({height}, {width}, 4) tensor on the device of q')
    if not (occupancy is None or isinstance(occupancy, torch.Tensor) or occupancy == 'auto'):
        raise ValueError("occupancy must be 'auto', None or the tensor of occupancy()")
    lib = _lib.require_device()
    q = q.contiguous()
    n = tuple(int(x) for x in q.shape)
    table = _on_device(table, q.device)
    maps = None if maps is None else _on_device(maps, q.device)
    m = (0, 0, 0) if maps is None else tuple(int(x) for x in maps.shape[1:])
    if isinstance(occupancy, torch.Tensor):
        occ = occupancy
        if occ.dtype != torch.uint8 or tuple(occ.shape) != tuple((x + BRICK - 1) // BRICK for x in n) or occ.device != q.device:
            raise ValueError('occupancy must be the uint8 brick grid of occupancy() for this volume, on its device')
        occ = occ.contiguous()
    else:
        occ = _occupancy(lib, q, table, maps, lo) if occupancy == 'auto' else None
    rgba = torch.empty((height, width, 4), dtype=torch.float32, device=q.device) if out is None else out
    rgbs = np.concatenate([colors, strengths[:, None]], axis=1).astype(np.float32).reshape(-1)
    f32 = lambda a, k: (C.c_float * k)(*(float(x) for x in a))          # noqa: E731
    with torch.cuda.device(q.device):
        _lib.check(lib.vittf_render(_lib.ptr(q), *n, f32(sp, 3), _lib.ptr(table), _lib.ptr(maps), c, *m, (C.c_int32 * 8)(*lo),
                                    (C.c_int32 * 8)(*hi), f32(rgbs, 32) if c else None, _lib.ptr(occ), f32(cam.reshape(-1), 18),
                                    width, height, float(step), f32(shade, 3), _lib.ptr(rgba), _lib.stream_ptr()), 'vittf_render')
    return rgba


def composite(rgba, background=(0.0, 0.0, 0.0)):
    """uint8 (h, w, 3) of a premultiplied (h, w, 4) image over a background colour: rint(255 clamp(rgb + (1 - A) bg, 0, 1)).
    A tensor on the image's device (numpy in: numpy out)."""
    bg = _vec3(background, 'background')
    as_numpy = not isinstance(rgba, torch.Tensor)
    t = torch.as_tensor(np.asarray(rgba)) if as_numpy else rgba
    if t.ndim != 3 or t.shape[2] != 4 or not t.is_floating_point():
        raise ValueError(f'rgba must be a floating-point (h, w, 4) image, got {t.dtype} {tuple(t.shape)}')
    t = t.to(torch.float32)
    b = torch.tensor(bg, dtype=torch.float32, device=t.device)
    u8 = torch.round((t[..., :3] + (1.0 - t[..., 3:]) * b).clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    return u8.numpy() if as_numpy else u8


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def write_png(path, u8):
    """An 8-bit PNG of a uint8 (h, w), (h, w, 3) or (h, w, 4) image (grey, RGB, RGBA with straight alpha), written with zlib."""
    a = u8.cpu().numpy() if isinstance(u8, torch.Tensor) else np.asarray(u8)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or a.size == 0 or (a.ndim == 3 and a.shape[2] not in (3, 4)):
        raise ValueError(f'an image is uint8 (h, w), (h, w, 3) or (h, w, 4), got {a.dtype} {a.shape}')
    h, w = a.shape[:2]
    color_type = 0 if a.ndim == 2 else (2 if a.shape[2] == 3 else 6)
    rows = np.ascontiguousarray(a).reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rows], axis=1).tobytes()          # filter 0 in front of every row
    png = (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, color_type, 0, 0, 0)) +
           _chunk(b'IDAT', zlib.compress(raw, 6)) + _chunk(b'IEND', b''))
    with open(path, 'wb') as fh:
        fh.write(png)
