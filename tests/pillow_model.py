"""numpy models of the Pillow arithmetic that csrc/dkt_augment.hip reproduces (docs/DATA_PIPELINE.md), for the tests: bilinear resize of a crop, the
three ImageEnhance blends, ToTensor + Normalize.  Python floats are IEEE doubles without contraction, like Pillow's C."""
import math

import numpy as np

PREC = 22


def coeffs(in_size, out_size):
    """Per output index: (xmin, quantised int weights) of Pillow's bilinear filter (precompute_coeffs + normalize_coeffs_8bpc)."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    out = []
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        ss = 1.0 / fs
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ws = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax)]
        ww = 0.0
        for w in ws:
            ww += w
        ws = [w / ww if ww != 0.0 else w for w in ws]
        out.append((xmin, np.array([int(0.5 + w * (1 << PREC)) for w in ws], dtype=np.int64)))
    return out


def _pass(a, cf, axis):
    """One separable pass over `axis` of the uint8 array a (H, W, 3)."""
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    res = np.empty((len(cf),) + a.shape[1:], dtype=np.int64)
    for o, (xmin, k) in enumerate(cf):
        acc = (1 << (PREC - 1)) + np.tensordot(k, a[xmin:xmin + len(k)], axes=(0, 0))
        res[o] = np.clip(acc >> PREC, 0, 255)
    return np.moveaxis(res, 0, axis).astype(np.uint8)


def resize_crop(img, y0, x0, h, w, rh, rw):
    """img.crop((x0, y0, x0 + w, y0 + h)).resize((rw, rh), BILINEAR) for an RGB uint8 array [H, W, 3]."""
    win = img[y0:y0 + h, x0:x0 + w]
    tmp = _pass(win, coeffs(w, rw), 1)
    return _pass(tmp, coeffs(h, rh), 0)


def gray(a):
    a = a.astype(np.int64)
    return ((19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16)


def blend(d, p, alpha):
    """ImagingBlend: float32 arithmetic, clamped, truncated."""
    d = np.asarray(d, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    t = d + np.float32(alpha) * (p - d)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def jitter(a, fb, fc, fs):
    """Brightness, Contrast, Color with factors (fb, fc, fs), the reference's ImageJitter order."""
    a = blend(0, a, fb)
    mean = int(float(gray(a).sum()) / a[..., 0].size + 0.5)
    a = blend(mean, a, fc)
    return blend(gray(a)[..., None], a, fs)


def to_tensor_normalize(a, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    x = np.transpose(a, (2, 0, 1)).astype(np.float32) / np.float32(255)
    return (x - np.asarray(mean, np.float32)[:, None, None]) / np.asarray(std, np.float32)[:, None, None]
