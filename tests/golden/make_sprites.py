"""Packs the sprites the PNG decoder test reads into tests/golden/reference_sprites.npz.

  python tests/golden/make_sprites.py <folder holding datasets/rpg-maker-xp>

Every third file, in sorted path order, of the reference's rpg-maker-xp sprite set (1176 RGBA PNGs) is stored byte for
byte: `names` (path below the dataset folder), `offsets` (n + 1 byte offsets) and `data` (the concatenated files)."""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(root):
    base = os.path.join(root, "datasets", "rpg-maker-xp")
    files = sorted(glob.glob(os.path.join(base, "*", "*", "*.png")))
    assert len(files) == 1176, len(files)
    files = files[::3]
    blobs = [open(f, "rb").read() for f in files]
    offsets = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
    names = np.array([os.path.relpath(f, base).replace(os.sep, "/") for f in files])
    data = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    np.savez(os.path.join(HERE, "reference_sprites.npz"), names=names, offsets=offsets, data=data)
    print(len(files), "sprites,", data.size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
