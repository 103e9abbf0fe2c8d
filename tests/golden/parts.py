"""Golden fixtures in parts.  No committed file may exceed 1 MiB, so a fixture whose compressed arrays do not fit is
stored as NAME.npz, NAME.part2.npz, NAME.part3.npz, ... with disjoint keys; load_npz() returns them as one dict (keys
in the order they were saved) and save_npz() writes them."""
import io
import os

import numpy as np

PART_BYTES = 960 * 1024   # per file, under the 1 MiB limit with room for the zip directory


def _part_path(path, i):
    return path if i == 1 else "%s.part%d.npz" % (path[:-len(".npz")], i)


def load_npz(path):
    out, i = {}, 1
    while os.path.exists(_part_path(path, i)):
        out.update(np.load(_part_path(path, i), allow_pickle=False))
        i += 1
    if not out:
        raise FileNotFoundError(path)
    return out


def save_npz(path, arrays):
    """np.savez_compressed(path, **arrays), split into parts of at most PART_BYTES; stale parts are removed."""
    parts, cur, size = [], {}, 0
    for k, v in arrays.items():
        b = io.BytesIO()
        np.savez_compressed(b, **{k: v})
        n = len(b.getvalue())
        if cur and size + n > PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += n
    parts.append(cur)
    for i, p in enumerate(parts, 1):
        np.savez_compressed(_part_path(path, i), **p)
    i = len(parts) + 1
    while os.path.exists(_part_path(path, i)):
        os.remove(_part_path(path, i))
        i += 1
    return len(parts)
