"""Connected components of a uint8 label volume: the separate bodies ("islands") of a class, a cluster or a prediction.

    python label_islands.py --labels FILE [--value V | --each-value] [--connectivity {1,2,3}] [--min-size N] [--max-islands K] [--output FILE] [--overwrite]

Reads a bare uint8 (W, H, D) ``.npy`` -- a ``_clusters<C>.npy`` of cluster_features.py, an ``ntf_pred*.npy`` of predict_ntf.py
or a ``labels.npy`` -- and labels the bodies of a set of its voxels on the GPU (vt.components): the voxels that are not 0 by
default, those holding ``--value V``, or with ``--each-value`` every value but 255 with neighbours linked only within one
value, which splits every cluster of a k-means volume into its bodies in one pass.  ``--connectivity`` 1, 2, 3 = 6, 18, 26
neighbours.  Bodies below ``--min-size`` voxels are dropped, the ``--max-islands`` (at most 255) largest are kept.  It writes
  * ``<stem>_islands.npy``: a bare uint8 (W, H, D) volume, islands numbered 1..K by descending size (the lower first voxel
    first among equal sizes), 0 elsewhere;
  * ``<stem>_islands.npz``: plain arrays ``sizes`` (int64 [K]), ``lowest_index`` (int64 [K], the smallest linear voxel index
    of each island) and ``values`` (uint8 [K], the value the island holds in the input).
The same file and flags give the same bytes.  There is no CPU path.
"""
import io
import sys
import zipfile
from argparse import ArgumentParser
from pathlib import Path

import numpy as np

import vit_tf_amd as vt
from reduce_features import writable_path


def load_label_volume(path):
    """The uint8 (W, H, D) array of a bare .npy; prints the refusal and exits 1 for anything else."""
    path = Path(path)
    if not path.exists():
        print(f'Invalid argument for --labels (File does not exist): {path}')
        sys.exit(1)
    try:
        vol = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as e:
        print(f'Invalid argument for --labels: {path.name} is not a bare .npy array ({e})')
        sys.exit(1)
    if not isinstance(vol, np.ndarray) or vol.dtype != np.uint8 or vol.ndim != 3 or vol.size < 1:
        what = f'{vol.dtype} {vol.shape}' if isinstance(vol, np.ndarray) else type(vol).__name__
        print(f'Invalid argument for --labels: expected a uint8 (W, H, D) volume, got {what}')
        sys.exit(1)
    return vol


def save_table(path, **arrays):
    """An .npz of plain arrays whose bytes depend on the arrays alone (np.savez stamps every member with the time of day)."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main(argv=None):
    parser = ArgumentParser('Label the connected components of a uint8 label volume')
    parser.add_argument('--labels', type=str, required=True, help='bare uint8 (W, H, D) .npy: clusters, a prediction or labels')
    parser.add_argument('--value', type=int, default=None, metavar='V', help='label the voxels holding V, 0..255 (default: the voxels that are not 0)')
    parser.add_argument('--each-value', action='store_true', help='label the bodies of every value but 255 in one pass')
    parser.add_argument('--connectivity', type=int, choices=[1, 2, 3], default=1, help='1, 2, 3 = 6, 18, 26 neighbours')
    parser.add_argument('--min-size', type=int, default=1, metavar='N', help='drop islands of fewer than N voxels')
    parser.add_argument('--max-islands', type=int, default=255, metavar='K', help='keep the K largest islands, 1..255')
    parser.add_argument('--output', type=str, default=None, metavar='FILE', help='island volume (default: <stem>_islands.npy next to the input)')
    parser.add_argument('--overwrite', action='store_true', help='replace existing output files')
    args = parser.parse_args(argv)

    if args.value is not None and args.each_value:
        print('Invalid argument for --each-value: it cannot be combined with --value')
        sys.exit(1)
    if args.value is not None and not 0 <= args.value <= 255:
        print(f'Invalid argument for --value: {args.value} is outside 0..255')
        sys.exit(1)
    if args.min_size < 1:
        print(f'Invalid argument for --min-size: {args.min_size} is below 1')
        sys.exit(1)
    if not 1 <= args.max_islands <= 255:
        print(f'Invalid argument for --max-islands: {args.max_islands} is outside 1..255')
        sys.exit(1)
    src = Path(args.labels)
    vol = load_label_volume(src)
    out_path = writable_path(args.output or src.with_name(f'{src.stem}_islands.npy'), '--output', args.overwrite)
    table_path = writable_path(out_path.with_suffix('.npz'), '--output', args.overwrite)

    select = vt.components.EACH_VALUE if args.each_value else (-1 if args.value is None else args.value)
    labels = vt.components.label(vol, select, args.connectivity)
    ids, counts = vt.components.table(labels)
    found = int(ids.numel())
    big = counts >= args.min_size                              # counts descend: a prefix
    ids, counts = ids[big][:args.max_islands], counts[big][:args.max_islands]
    islands = vt.components.relabel(labels, ids, args.max_islands).cpu().numpy()
    lowest = (ids - 1).cpu().numpy().astype(np.int64)
    sizes = counts.cpu().numpy().astype(np.int64)
    values = vol.reshape(-1)[lowest].astype(np.uint8)
    rule = 'each value' if args.each_value else ('!= 0' if args.value is None else f'== {args.value}')
    print(f'{src.name} : {vol.shape} uint8, set {rule}, connectivity {args.connectivity}: {found} islands, {len(sizes)} kept '
          f'(min size {args.min_size}, at most {args.max_islands}); sizes {sizes[:8].tolist()}{" ..." if len(sizes) > 8 else ""}; '
          f'saving to: {out_path}')
    np.save(out_path, islands)
    save_table(table_path, sizes=sizes, lowest_index=lowest, values=values)
    print(f'Island table saved to: {table_path}')
    sys.exit(0)


if __name__ == '__main__':
    main()
