"""Image-dataset path timings (docs/DATA_PIPELINE.md): generates its own JPEG trees in a temp dir (CUB-like 500x375, Omniglot-like 105x105), then
  (a) libdkt_data.so time per 105-image episode at S = 84 and 224 (device events around back-to-back calls; host time of a call alone),
  (b) loader episodes/s: FilelistEpisodeLoader resident and streaming, and a 16-thread CPU PIL pipeline of the same transforms,
  (c) DKT.train_loop ms per episode, Conv4 84x84 5-way 5-shot, on the CUB-like tree against the synthetic loader.
Measurement tooling; prints only (--json PATH also writes the numbers)."""
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dkt_amd  # noqa: E402
from dkt_amd import image_data  # noqa: E402
from dkt_amd.data import SyntheticEpisodeLoader  # noqa: E402


def make_tree(root, n_classes, per_class, size, seed):
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    names, labels = [], []
    for c in range(n_classes):
        base = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
        for i in range(per_class):
            a = np.asarray(Image.fromarray(base).resize(size[::-1], Image.BILINEAR)).astype(np.int16)
            a = np.clip(a + rng.integers(-40, 40, a.shape), 0, 255).astype(np.uint8)
            p = os.path.join(root, "c%03d_%03d.jpg" % (c, i))
            Image.fromarray(a).save(p, quality=90)
            names.append(p)
            labels.append(c)
    path = os.path.join(root, "base.json")
    with open(path, "w") as fh:
        json.dump({"label_names": [str(c) for c in range(n_classes)], "image_names": names, "image_labels": labels}, fh)
    return path


def kernel_time(dev, S, B=105, reps=50):
    rng = np.random.default_rng(S)
    imgs = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8) for _ in range(B)]
    pool = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    offs = np.arange(B, dtype=np.int64) * imgs[0].size
    H, W = np.full(B, 375), np.full(B, 500)
    tables = [image_data.build_table(offs, H, W, S, True, rng) for _ in range(reps)]
    out = torch.empty((B, 3, S, S), device=dev)
    for t in tables[:5]:
        image_data.augment(pool, *t[:1], S, t[1], t[2], out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    h0 = time.perf_counter()
    for t in tables:
        image_data.augment(pool, t[0], S, t[1], t[2], out=out)
    host = (time.perf_counter() - h0) / reps
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, host * 1e3


def loader_rate(path, mode, n_ep=30):
    ld = image_data.FilelistEpisodeLoader(path, 5, 5, 16, n_episode=n_ep, image_size=84, aug=True, seed=1, mode=mode)
    for _ in zip(range(2), ld):
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for x, y in ld:
        pass
    torch.cuda.synchronize()
    return n_ep / (time.perf_counter() - t0)


def cpu_pil_rate(path, n_ep=4):
    meta = image_data.read_filelist(path)
    rng = np.random.default_rng(0)
    names = meta["image_names"]

    def one(p):
        im = Image.open(p).convert("RGB")
        h, w = im.size[1], im.size[0]
        t, jit, flip = image_data.build_table([0], [h], [w], 84, True, rng)
        return image_data.pil_reference(im, t[0], 84, jit[0], bool(flip[0]))

    with ThreadPoolExecutor(16) as ex:
        t0 = time.perf_counter()
        for e in range(n_ep):
            batch = [names[(e * 105 + i) % len(names)] for i in range(105)]
            torch.stack(list(ex.map(one, batch)))
        return n_ep / (time.perf_counter() - t0)


def train_ms(dev, loader, n_ep):
    m = dkt_amd.DKT(dkt_amd.backbone.Conv4, n_way=5, n_support=5).to(dev)
    m.train()
    so = sys.stdout
    sys.stdout = open(os.devnull, "w")
    try:
        it = iter(loader)
        warm = [next(it) for _ in range(3)]
        m.train_loop(0, warm, None, print_freq=1000)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.train_loop(1, loader, None, print_freq=1000)
        torch.cuda.synchronize()
    finally:
        sys.stdout = so
    return 1e3 * (time.perf_counter() - t0) / n_ep


def main():
    dev = torch.device("cuda", 0)
    res = {}
    for S in (84, 224):
        k, h = kernel_time(dev, S)
        res["call_ms_S%d" % S], res["host_ms_S%d" % S] = k, h
        print("(a) S=%3d: augment call %.3f ms per 105-image episode (device events), host %.3f ms per call" % (S, k, h), flush=True)
    with tempfile.TemporaryDirectory() as d:
        cub = make_tree(os.path.join(d, "CUB"), 20, 25, (375, 500), 0)
        omni = make_tree(os.path.join(d, "omniglot"), 20, 25, (105, 105), 1)
        for name, path in (("CUB-like 500x375", cub), ("Omniglot-like 105x105", omni)):
            r, s = loader_rate(path, "resident"), loader_rate(path, "streaming")
            c = cpu_pil_rate(path)
            res[name] = {"resident_eps": r, "streaming_eps": s, "cpu_pil16_eps": c}
            print("(b) %s: resident %.1f episodes/s, streaming %.1f episodes/s, 16-thread CPU PIL %.1f episodes/s" % (name, r, s, c), flush=True)
        n = 40
        ms_img = train_ms(dev, image_data.FilelistEpisodeLoader(cub, 5, 5, 16, n_episode=n, image_size=84, aug=True, seed=2), n)
        ms_syn = train_ms(dev, SyntheticEpisodeLoader(5, 5, 16, n, 84), n)
        res["train_ms_image"], res["train_ms_synthetic"] = ms_img, ms_syn
        print("(c) Conv4 84x84 train_loop: image tree %.2f ms / episode, synthetic %.2f ms / episode (ratio %.2f); CPU PIL pipeline alone %.1f ms / episode"
              % (ms_img, ms_syn, ms_img / ms_syn, 1e3 / res["CUB-like 500x375"]["cpu_pil16_eps"]), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
