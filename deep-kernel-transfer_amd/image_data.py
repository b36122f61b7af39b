"""Episodic loader of the reference's image datasets (CUB, miniImagenet, omniglot, emnist, cross, cross_char), with the per-episode transform on the GPU.

The reference (data/dataset.py SetDataset + data/datamgr.py TransformLoader) decodes and augments every image on the CPU for every episode.  Here every
image is decoded once (PIL, a thread pool) and the episode's images are transformed by one call of libdkt_data.so (csrc/dkt_augment.hip) that
reproduces Pillow + torchvision bit for bit:
  training (aug=True):  RandomResizedCrop(S) -> ImageJitter(Brightness, Contrast, Color; 0.4) -> RandomHorizontalFlip -> ToTensor -> Normalize
  evaluation:           Resize((a, a)), a = int(1.15 S) -> CenterCrop(S) -> ToTensor -> Normalize
Two modes: resident (the whole split decoded into one GPU uint8 pool at construction, when it fits DKT_IMAGE_CACHE_GB, default 16) and streaming
(the next episode's images decoded ahead on the pool, one pinned host-to-device copy per episode).  docs/DATA_PIPELINE.md has the details.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, configs

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
JITTER = 0.4                                   # Brightness, Contrast, Color
DATASETS = ('CUB', 'miniImagenet', 'omniglot', 'emnist', 'cross', 'cross_char')

# the reference's scripts that write each file list (its filelists/ tree)
_WRITERS = {
    ('CUB', None): 'filelists/CUB/write_CUB_filelist.py',
    ('miniImagenet', None): 'filelists/miniImagenet/write_miniImagenet_filelist.py',
    ('miniImagenet', 'all'): 'filelists/miniImagenet/write_cross_filelist.py',
    ('omniglot', None): 'filelists/omniglot/write_omniglot_filelist.py',
    ('omniglot', 'noLatin'): 'filelists/omniglot/write_cross_char_base_filelist.py',
    ('emnist', None): 'filelists/emnist/write_cross_char_valnovel_filelist.py',
}


def filelist_for(dataset, split):
    """(directory key of configs.data_dir, file name) of a split, as the reference's train.py / test.py choose them."""
    if dataset not in DATASETS:
        raise ValueError("unknown dataset '%s' (one of %s, or synthetic)" % (dataset, ', '.join(DATASETS)))
    if split not in ('base', 'val', 'novel'):
        raise ValueError("unknown split '%s'" % split)
    if dataset == 'cross':
        return ('miniImagenet', 'all.json') if split == 'base' else ('CUB', split + '.json')
    if dataset == 'cross_char':
        return ('omniglot', 'noLatin.json') if split == 'base' else ('emnist', split + '.json')
    return dataset, split + '.json'


def filelist_path(dataset, split):
    key, name = filelist_for(dataset, split)
    return os.path.join(configs.data_dir[key], name)


def read_filelist(path, dataset_key=None):
    """{'label_names', 'image_names', 'image_labels'} of a reference file list; a missing file names the script that writes it."""
    if not os.path.isfile(path):
        key = dataset_key or os.path.basename(os.path.dirname(os.path.normpath(path)))
        stem = os.path.splitext(os.path.basename(path))[0]
        writer = _WRITERS.get((key, stem)) or _WRITERS.get((key, None)) or 'filelists/<dataset>/write_*_filelist.py'
        raise FileNotFoundError("file list %s not found: write it with the reference's %s and point configs.data_dir['%s'] at its directory"
                                % (path, writer, key))
    with open(path) as fh:
        meta = json.load(fh)
    for k in ('image_names', 'image_labels'):
        if k not in meta:
            raise ValueError("file list %s has no '%s'" % (path, k))
    if len(meta['image_names']) != len(meta['image_labels']):
        raise ValueError("file list %s: %d image_names, %d image_labels" % (path, len(meta['image_names']), len(meta['image_labels'])))
    return meta


def _threads():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def image_size_of(path):
    """(H, W) from the file header (no decode)."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
    return h, w


def decode(path):
    """uint8 [H, W, 3]: PIL Image.open(p).convert('RGB'), the reference's SubDataset.__getitem__."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'))


def eval_geometry(S):
    """(a, offset): Resize((a, a)) with a = int(1.15 S), CenterCrop(S) at round((a - S) / 2) (Python rounding, torchvision's)."""
    a = int(S * 1.15)
    return a, int(round((a - S) / 2.0))


def draw_crop_params(rng, H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), attempts=10):
    """torchvision RandomResizedCrop.get_params, vectorised over images: H, W int arrays [B] -> (y0, x0, h, w) int64 arrays [B].
    Per image: up to `attempts` draws of area * U(scale) and exp(U(log ratio)), w = round(sqrt(A r)), h = round(sqrt(A / r)), the first with
    0 < w <= W and 0 < h <= H wins and the offsets are uniform integers; otherwise the central crop clamped to the ratio range."""
    H = np.asarray(H, dtype=np.int64)
    W = np.asarray(W, dtype=np.int64)
    B = H.shape[0]
    area = (H * W).astype(np.float64)[:, None]
    target = area * rng.uniform(scale[0], scale[1], size=(B, attempts))
    ar = np.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1]), size=(B, attempts)))
    w = np.round(np.sqrt(target * ar)).astype(np.int64)
    h = np.round(np.sqrt(target / ar)).astype(np.int64)
    ok = (w > 0) & (w <= W[:, None]) & (h > 0) & (h <= H[:, None])
    first = np.argmax(ok, axis=1)
    hit = ok[np.arange(B), first]
    cw = w[np.arange(B), first]
    ch = h[np.arange(B), first]
    # fallback: central crop
    in_ratio = W / H
    fw = np.where(in_ratio < ratio[0], W, np.where(in_ratio > ratio[1], np.round(H * ratio[1]).astype(np.int64), W))
    fh = np.where(in_ratio < ratio[0], np.round(W / ratio[0]).astype(np.int64), H)
    cw = np.where(hit, cw, fw)
    ch = np.where(hit, ch, fh)
    uy, ux = rng.random(B), rng.random(B)
    y0 = np.where(hit, np.minimum((uy * (H - ch + 1)).astype(np.int64), H - ch), (H - ch) // 2)
    x0 = np.where(hit, np.minimum((ux * (W - cw + 1)).astype(np.int64), W - cw), (W - cw) // 2)
    return y0, x0, ch, cw, hit


def draw_jitter(rng, B):
    """ImageJitter's factors 1 + 0.4 (2u - 1), fp32 like the reference's torch arithmetic: [B, 3] (Brightness, Contrast, Color)."""
    u = rng.random((B, 3), dtype=np.float32)
    return (np.float32(JITTER) * (u * np.float32(2.0) - np.float32(1.0)) + np.float32(1.0)).astype(np.float32)


def build_table(offsets, H, W, S, aug, rng=None):
    """int64 [B, 12] table of include/dkt_abi_data.h (ws_off left 0) + the jitter [B, 3] / flip [B] draws (None in evaluation)."""
    B = len(offsets)
    t = np.zeros((B, _lib.AUG_COLS), dtype=np.int64)
    t[:, 0], t[:, 1], t[:, 2] = offsets, H, W
    if aug:
        y0, x0, h, w, _ = draw_crop_params(rng, H, W)
        t[:, 3], t[:, 4], t[:, 5], t[:, 6] = y0, x0, h, w
        t[:, 7], t[:, 8] = S, S
        jit = draw_jitter(rng, B)
        flip = (rng.random(B) < 0.5).astype(np.uint8)
        return t, jit, flip
    a, o = eval_geometry(S)
    t[:, 5], t[:, 6] = H, W
    t[:, 7], t[:, 8], t[:, 9], t[:, 10] = a, a, o, o
    return t, None, None


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def augment(pool, table, S, jitter=None, flip=None, mean=MEAN, std=STD, out=None):
    """One libdkt_data.so call: pool = CUDA uint8 tensor of HWC RGB images, table = int64 numpy [B, 12] (see include/dkt_abi_data.h), jitter = fp32 [B, 3]
    and flip = uint8 [B] (numpy or CUDA tensors, or None) -> CUDA fp32 [B, 3, S, S] on pool's device and current stream."""
    lib = _lib.load_data()
    dev = pool.device
    table = np.ascontiguousarray(table, dtype=np.int64)
    B = table.shape[0]
    ws = ctypes.c_size_t(0)
    _lib.check(lib.dkt_augment_plan(table.ctypes.data_as(ctypes.c_void_p), B, S, ctypes.byref(ws)), "dkt_augment_plan")

    def dev_copy(a, dtype):
        if a is None:
            return None
        if isinstance(a, torch.Tensor):
            return a.to(dev, dtype, non_blocking=True).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).pin_memory().to(dev, non_blocking=True)

    table_dev = dev_copy(table, torch.int64)
    jit_dev = dev_copy(jitter, torch.float32)
    flip_dev = dev_copy(flip, torch.uint8)
    if out is None:
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    wsb = torch.empty(max(16, ws.value), dtype=torch.uint8, device=dev)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    st = lib.dkt_augment_u8(_ptr(pool), pool.numel(), table.ctypes.data_as(ctypes.c_void_p), _ptr(table_dev), B, _ptr(jit_dev), _ptr(flip_dev),
                            S, m, s, _ptr(out), _ptr(wsb), wsb.numel(), stream)
    _lib.check(st, "dkt_augment_u8")
    return out


def pil_reference(img, row, S, jitter=None, flip=False, mean=MEAN, std=STD):
    """The CPU pipeline the kernel reproduces, for one image: PIL RGB image + its table row (+ jitter factors, flip) -> fp32 [3, S, S] through Pillow's
    crop / resize / ImageEnhance / transpose and torchvision's ToTensor + Normalize arithmetic.  Tests and tools compare against it; the loader never
    calls it."""
    from PIL import Image, ImageEnhance
    H, W, y0, x0, h, w, rh, rw, oy, ox = (int(v) for v in row[1:11])
    im = img.crop((x0, y0, x0 + w, y0 + h)).resize((rw, rh), Image.BILINEAR)
    im = im.crop((ox, oy, ox + S, oy + S))
    if jitter is not None:
        for f, enh in zip(jitter, (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)):
            im = enh(im).enhance(float(f)).convert('RGB')
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    x = torch.from_numpy(np.array(im, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    return x.sub_(torch.tensor(mean, dtype=torch.float32)[:, None, None]).div_(torch.tensor(std, dtype=torch.float32)[:, None, None])


class FilelistEpisodeLoader:
    """Episodes of a reference file list with the iteration contract of data.SyntheticEpisodeLoader: len() = n_episode, iteration yields
    (x [n_way, per, 3, S, S] fp32, y [n_way, per] int64), both CUDA tensors on the device current at construction.  Per episode (the reference's
    EpisodicBatchSampler + SetDataset): torch.randperm(n_classes)[:n_way] over the sorted unique labels, then the first n_support + n_query images of a
    fresh shuffle of each chosen class; y holds the file list's labels.  `last_params` keeps what the last episode drew (paths, table, jitter, flip),
    so that it can be replayed on the CPU with pil_reference()."""

    def __init__(self, filelist, n_way, n_support, n_query, n_episode=100, image_size=84, aug=False, seed=0, mode=None, dataset_key=None):
        meta = read_filelist(filelist, dataset_key)
        self.n_way, self.per, self.n_episode, self.S, self.aug = n_way, n_support + n_query, n_episode, image_size, bool(aug)
        self.paths = list(meta['image_names'])
        labels = np.asarray(meta['image_labels'], dtype=np.int64)
        self.classes = np.unique(labels)
        self.members = [np.nonzero(labels == c)[0] for c in self.classes]
        for c, m in zip(self.classes.tolist(), self.members):
            if len(m) < self.per:
                raise ValueError("%s: class %d has %d images, an episode takes n_support + n_query = %d of each class"
                                 % (filelist, c, len(m), self.per))
        if len(self.classes) < n_way:
            raise ValueError("%s has %d classes, an episode needs n_way = %d" % (filelist, len(self.classes), n_way))
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.gen = torch.Generator().manual_seed(1000 + seed)
        self.rng = np.random.default_rng(2000 + seed)
        self.pool_threads = ThreadPoolExecutor(max_workers=_threads())
        hw = np.array(list(self.pool_threads.map(image_size_of, self.paths)), dtype=np.int64).reshape(-1, 2)
        self.H, self.W = hw[:, 0], hw[:, 1]
        nbytes = self.H * self.W * 3
        budget = float(os.environ.get('DKT_IMAGE_CACHE_GB', '16')) * 2 ** 30
        self.mode = mode or ('resident' if nbytes.sum() <= budget else 'streaming')
        if self.mode not in ('resident', 'streaming'):
            raise ValueError("mode must be 'resident' or 'streaming'")
        self.last_params = None
        if self.mode == 'resident':
            self.offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
            self.pool = torch.empty(int(nbytes.sum()), dtype=torch.uint8, device=self.device)
            for i, arr in enumerate(self.pool_threads.map(decode, self.paths)):
                self._check_decoded(i, arr)
                o = int(self.offsets[i])
                self.pool[o:o + arr.size].copy_(torch.from_numpy(arr.reshape(-1)))
            self.pool_threads.shutdown()
            self.pool_threads = None

    def _check_decoded(self, i, arr):
        if arr.shape != (self.H[i], self.W[i], 3):
            raise ValueError("%s decodes to %s, its header says %dx%d" % (self.paths[i], arr.shape, self.H[i], self.W[i]))

    def __len__(self):
        return self.n_episode

    def _draw(self):
        """(image indices [n_way * per], labels [n_way, per], table, jitter, flip) of one episode; table offsets are filled by the caller."""
        pick = torch.randperm(len(self.classes), generator=self.gen)[:self.n_way].tolist()
        idx = np.concatenate([m[self.rng.permutation(len(m))[:self.per]] for m in (self.members[c] for c in pick)])
        y = np.repeat(self.classes[pick], self.per).reshape(self.n_way, self.per)
        table, jit, flip = build_table(np.zeros(len(idx), np.int64), self.H[idx], self.W[idx], self.S, self.aug, self.rng)
        return idx, y, table, jit, flip

    def _stage(self, idx):
        """streaming: decode the episode's images on the thread pool (futures)."""
        return [self.pool_threads.submit(decode, self.paths[i]) for i in idx]

    def _emit(self, idx, y, table, jit, flip, pool):
        self.last_params = {'paths': [self.paths[i] for i in idx], 'table': table.copy(), 'jitter': jit, 'flip': flip, 'S': self.S}
        x = augment(pool, table, self.S, jit, flip)
        return (x.view(self.n_way, self.per, 3, self.S, self.S),
                torch.from_numpy(y).pin_memory().to(self.device, non_blocking=True))

    def __iter__(self):
        if self.mode == 'resident':
            for _ in range(self.n_episode):
                idx, y, table, jit, flip = self._draw()
                table[:, 0] = self.offsets[idx]
                yield self._emit(idx, y, table, jit, flip, self.pool)
            return
        nxt = None
        for e in range(self.n_episode):
            cur = nxt if nxt is not None else (lambda d: (d, self._stage(d[0])))(self._draw())
            nxt = None
            if e + 1 < self.n_episode:                       # decode the next episode ahead while this one is transformed and consumed
                d = self._draw()
                nxt = (d, self._stage(d[0]))
            (idx, y, table, jit, flip), futs = cur
            arrs = [f.result() for f in futs]
            nb = np.array([a.size for a in arrs], dtype=np.int64)
            table[:, 0] = np.concatenate([[0], np.cumsum(nb)[:-1]])
            host = torch.empty(int(nb.sum()), dtype=torch.uint8, pin_memory=True)
            hv = host.numpy()
            for i, a in enumerate(arrs):
                self._check_decoded(idx[i], a)
                o = int(table[i, 0])
                hv[o:o + a.size] = a.reshape(-1)
            pool = host.to(self.device, non_blocking=True)
            yield self._emit(idx, y, table, jit, flip, pool)

    def __del__(self):
        ex = getattr(self, 'pool_threads', None)
        if ex is not None:
            ex.shutdown(wait=False, cancel_futures=True)
