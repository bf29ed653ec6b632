"""Render a volume, with class maps or a label volume as per-class opacity, to an 8-bit PNG.

    python render_volume.py --data DIR [--maps FILE | --labels FILE] [--spacing SX SY SZ] [--size W H] [--azimuth A] [--elevation E]
                            [--fov F] [--step DT] [--lo L] [--hi H] [--tf FILE] [--no-shading] [--background R G B]
                            [--turntable N] [--output FILE] [--overwrite]

``DIR/volume.npy`` is loaded with the flip of predict_ntf.py, so every result computed from it lines up.  ``--maps`` takes a
uint8 (C, W', H', D') array (``mlp_probs*``, ``knn_probs*``, ``rf_votes*``) or the dict of a ``similarities.npy``; ``--labels``
a bare uint8 label volume (``ntf_pred*``, ``*_pred*``, ``_clusters<C>``, ``_islands``; the data directory's own ``labels.npy``
is flipped like the volume), whose values 1..C become one-hot maps.  Either may sit on a coarser grid than the volume and may
be named relative to DIR.  At most 8 classes.  Without either the volume alone is rendered with a grey ramp; with one the
volume is a faint grey context and class c takes colour c of vt.render.PALETTE, clear below level ``--lo`` and at full
strength from ``--hi`` on.  ``--tf`` replaces the intensity transfer function by a float32 (256, 4) ``.npy`` of (r, g, b,
extinction per world unit).  ``--fov`` (degrees) makes the camera a perspective one, without it it is orthographic;
``--turntable N`` writes N frames a full turn apart as ``<output stem>_000.png`` ...  The marcher runs on the GPU (vt.render);
there is no CPU path.
"""
import sys
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

import vit_tf_amd as vt
from reduce_features import writable_path


def fail(message):
    print(message)
    sys.exit(1)


def find(path, data, flag):
    """The file as named, else under the data directory."""
    for p in (Path(path), data / path):
        if p.is_file():
            return p
    fail(f'Invalid argument for {flag} (File does not exist): {path}')


def load_npy(path, flag, allow_pickle=False):
    try:
        return np.load(path, allow_pickle=allow_pickle)
    except (OSError, ValueError) as e:
        fail(f'Invalid argument for {flag}: {Path(path).name} is not a readable .npy file ({e})')


def load_maps(path, flag='--maps'):
    """uint8 (C, m0, m1, m2) from a bare array or a similarities dict (classes in the dict's order)."""
    raw = load_npy(path, flag, allow_pickle=True)
    if raw.dtype == object and raw.shape == ():
        raw = raw[()]
    if isinstance(raw, dict):
        if not raw:
            fail(f'Invalid argument for {flag}: {Path(path).name} holds no class map')
        try:
            raw = np.stack([np.asarray(v) for v in raw.values()])
        except ValueError:
            fail(f'Invalid argument for {flag}: the class maps of {Path(path).name} differ in shape')
    if not isinstance(raw, np.ndarray) or raw.dtype != np.uint8 or raw.ndim != 4 or raw.shape[0] < 1 or min(raw.shape[1:]) < 2:
        what = f'{raw.dtype} {raw.shape}' if isinstance(raw, np.ndarray) else type(raw).__name__
        fail(f"Invalid argument for {flag}: expected uint8 (C, W', H', D') maps or a similarities dict, got {what}")
    if raw.shape[0] > vt.render.MAX_CLASSES:
        fail(f'Invalid argument for {flag}: {raw.shape[0]} classes, at most {vt.render.MAX_CLASSES} can be rendered')
    return raw


def load_labels(path, flag='--labels'):
    """(uint8 label volume, its values 1..C)."""
    vol = load_npy(path, flag)
    if not isinstance(vol, np.ndarray) or vol.dtype != np.uint8 or vol.ndim != 3 or min(vol.shape) < 2:
        what = f'{vol.dtype} {vol.shape}' if isinstance(vol, np.ndarray) else type(vol).__name__
        fail(f'Invalid argument for {flag}: expected a uint8 (W, H, D) label volume, got {what}')
    if Path(path).name == 'labels.npy':
        vol = np.flip(vol, axis=-3).copy()
    top = int(vol.max())
    if top > vt.render.MAX_CLASSES:
        fail(f'Invalid argument for {flag}: labels up to {top}, at most {vt.render.MAX_CLASSES} classes can be rendered')
    if top < 1:
        fail(f'Invalid argument for {flag}: {Path(path).name} holds no label above 0')
    return vol, list(range(1, top + 1))


def frame_paths(output, count):
    output = Path(output)
    if count is None:
        return [output]
    return [output.with_name(f'{output.stem}_{k:03d}{output.suffix or ".png"}') for k in range(count)]


def main(argv=None):
    parser = ArgumentParser('Direct volume rendering of a volume and its class maps or labels')
    parser.add_argument('--data', type=str, required=True, help='directory holding volume.npy')
    which = parser.add_mutually_exclusive_group()
    which.add_argument('--maps', type=str, default=None, metavar='FILE', help="uint8 (C, W', H', D') class maps or a similarities.npy dict")
    which.add_argument('--labels', type=str, default=None, metavar='FILE', help='bare uint8 label volume; values 1..C become the classes')
    parser.add_argument('--spacing', type=float, nargs=3, default=[1.0, 1.0, 1.0], metavar=('SX', 'SY', 'SZ'), help='voxel spacing of the volume (default: unit voxels)')
    parser.add_argument('--size', type=int, nargs=2, default=[512, 512], metavar=('W', 'H'), help='image size in pixels')
    parser.add_argument('--azimuth', type=float, default=30.0, help='degrees about volume axis 2')
    parser.add_argument('--elevation', type=float, default=20.0, help='degrees towards +axis 2')
    parser.add_argument('--fov', type=float, default=None, help='vertical field of view in degrees (default: orthographic)')
    parser.add_argument('--step', type=float, default=0.5, metavar='DT', help='sample distance in world units')
    parser.add_argument('--lo', type=int, default=64, help='map level up to which a class is clear')
    parser.add_argument('--hi', type=int, default=192, help='map level from which a class has its full strength')
    parser.add_argument('--tf', type=str, default=None, metavar='FILE', help='float32 (256, 4) .npy: (r, g, b, extinction per world unit)')
    parser.add_argument('--no-shading', action='store_true', help='no headlight shading')
    parser.add_argument('--background', type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=('R', 'G', 'B'), help='background colour, 0..1')
    parser.add_argument('--turntable', type=int, default=None, metavar='N', help='write N frames a full turn apart')
    parser.add_argument('--output', type=str, default=None, metavar='FILE', help='PNG file (default: DIR/render.png)')
    parser.add_argument('--overwrite', action='store_true', help='replace existing output files')
    args = parser.parse_args(argv)

    data = Path(args.data)
    if not (data / 'volume.npy').is_file():
        fail(f'Invalid argument for --data (File does not exist): {data / "volume.npy"}')
    if not all(np.isfinite(s) and s > 0 for s in args.spacing):
        fail(f'Invalid argument for --spacing: {args.spacing} are not three finite positive numbers')
    if not all(1 <= v <= vt.render.MAX_IMAGE for v in args.size):
        fail(f'Invalid argument for --size: {args.size} is outside 1..{vt.render.MAX_IMAGE}')
    if not (np.isfinite(args.azimuth) and np.isfinite(args.elevation)):
        fail('Invalid argument for --azimuth / --elevation: not finite')
    if args.fov is not None and not 0 < args.fov < 180:
        fail(f'Invalid argument for --fov: {args.fov} is outside (0, 180)')
    if not (np.isfinite(args.step) and args.step > 0):
        fail(f'Invalid argument for --step: {args.step} is not a finite number > 0')
    if not 0 <= args.lo < args.hi <= 255:
        fail(f'Invalid argument for --lo / --hi: need 0 <= lo < hi <= 255, got {args.lo} and {args.hi}')
    if not all(np.isfinite(b) and 0 <= b <= 1 for b in args.background):
        fail(f'Invalid argument for --background: {args.background} is outside 0..1')
    if args.turntable is not None and not 1 <= args.turntable <= 999:
        fail(f'Invalid argument for --turntable: {args.turntable} is outside 1..999')
    maps = labels = values = table = None
    if args.maps:
        maps = load_maps(find(args.maps, data, '--maps'))
    if args.labels:
        labels, values = load_labels(find(args.labels, data, '--labels'))
    if args.tf:
        table = load_npy(find(args.tf, data, '--tf'), '--tf')
        if not isinstance(table, np.ndarray) or table.dtype != np.float32 or table.shape != (256, 4) or not np.isfinite(table).all() \
                or (table[:, 3] < 0).any():
            fail('Invalid argument for --tf: expected a finite float32 (256, 4) table with extinction >= 0')
    outputs = [writable_path(p, '--output', args.overwrite) for p in frame_paths(args.output or data / 'render.png', args.turntable)]

    volume = np.flip(np.load(data / 'volume.npy', allow_pickle=True).astype(np.float32), axis=-3).copy()
    if volume.ndim != 3 or min(volume.shape) < 2 or max(volume.shape) > vt.render.MAX_DIM:
        fail(f'Invalid argument for --data: a volume of shape {volume.shape} cannot be rendered')
    render = vt.render
    q = render.prepare(volume)
    if labels is not None:
        maps = render.maps_from_labels(labels, values)
    size = tuple(args.size)
    if table is None:
        table = render.ramp_table() if maps is None else render.context_table()
    occ = render.occupancy(q, table, maps, args.lo)              # one brick grid for every frame
    for k, path in enumerate(outputs):
        azimuth = args.azimuth + (360.0 * k / len(outputs) if args.turntable else 0.0)
        cam = render.Camera.orbit(azimuth, args.elevation, fov=args.fov, shape=volume.shape, spacing=args.spacing, aspect=size[0] / size[1])
        rgba = render.render(q, cam, size, spacing=args.spacing, table=table, maps=maps, lo=args.lo, hi=args.hi, step=args.step,
                             shading=None if args.no_shading else render.SHADING, occupancy=occ)
        render.write_png(path, render.composite(rgba, args.background))
        print(f'Rendering saved to: {path}')
    sys.exit(0)


if __name__ == '__main__':
    main()
