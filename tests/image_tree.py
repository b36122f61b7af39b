"""A generated image-dataset tree in the reference's file-list format, for the loader tests: per split a JSON with label_names, image_names (absolute
paths) and image_labels; images are PNG and JPEG of mixed sizes, with grayscale (L) and RGBA files among them."""
import json
import os

import numpy as np
from PIL import Image


def write_image(path, h, w, mode, rng):
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    # a smooth component, so that resizes and the contrast mean are not all noise
    yy, xx = np.mgrid[0:h, 0:w]
    a = ((a.astype(np.int32) // 2 + (yy * 97 // max(h, 1))[..., None] + (xx * 53 // max(w, 1))[..., None]) % 256).astype(np.uint8)
    im = Image.fromarray(a)
    if mode == 'L':
        im = im.convert('L')
    elif mode == 'RGBA':
        im = im.convert('RGBA')
    im.save(path, quality=90) if path.endswith('.jpg') else im.save(path)


def make_split(root, name, n_classes, per_class, sizes, seed=0, label_base=0):
    """root/<name>.json over n_classes x per_class images; sizes: list of (h, w) cycled through."""
    rng = np.random.default_rng(seed)
    img_dir = os.path.join(root, 'images_' + name)
    os.makedirs(img_dir, exist_ok=True)
    names, labels = [], []
    k = 0
    for c in range(n_classes):
        for i in range(per_class):
            h, w = sizes[k % len(sizes)]
            mode = ('RGB', 'L', 'RGBA', 'RGB')[k % 4]
            ext = '.png' if (k % 3 == 1 or mode == 'RGBA') else '.jpg'
            p = os.path.join(img_dir, 'c%03d_%03d%s' % (c, i, ext))
            write_image(p, h, w, mode, rng)
            names.append(os.path.abspath(p))
            labels.append(label_base + c)
            k += 1
    with open(os.path.join(root, name + '.json'), 'w') as fh:
        json.dump({'label_names': ['class%d' % (label_base + c) for c in range(n_classes)], 'image_names': names, 'image_labels': labels}, fh)
    return os.path.join(root, name + '.json')


def make_dataset(root, splits=('base', 'val', 'novel'), n_classes=6, per_class=8, sizes=((60, 80), (37, 45), (105, 105), (90, 70)), seed=0):
    os.makedirs(root, exist_ok=True)
    return [make_split(root, s, n_classes, per_class, sizes, seed + i, label_base=100 * i) for i, s in enumerate(splits)]
