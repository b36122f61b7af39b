"""CPU-side checks of the image-dataset path: the numpy models of Pillow's resize and ImageEnhance arithmetic (the contract csrc/dkt_augment.hip
implements) are bit-exact against Pillow; libdkt_data.so exports exactly include/dkt_abi_data.h, does not spill and rejects bad arguments before any
launch; FilelistEpisodeLoader's file choice, class pools, crop parameters and error messages."""
import ctypes
import json
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image, ImageEnhance

import dkt_amd
from dkt_amd import configs, image_data
from dkt_amd.data import get_episode_loader

import image_tree
import pillow_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
FAKE = 0x10000          # a well-aligned non-NULL address: every call below must return before it is dereferenced or a kernel is launched


# ---- numpy models vs Pillow -------------------------------------------------------------------------------------------------------------------

def _pil_resize(img, y0, x0, h, w, rh, rw):
    return np.asarray(Image.fromarray(img).crop((x0, y0, x0 + w, y0 + h)).resize((int(rw), int(rh)), Image.BILINEAR))


def test_resize_model_bitexact_random():
    rng = np.random.default_rng(0)
    for _ in range(24):
        H, W = (int(v) for v in rng.integers(1, 601, 2))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w = int(rng.integers(1, H - y0 + 1)), int(rng.integers(1, W - x0 + 1))
        rh, rw = (int(v) for v in rng.integers(1, 300, 2))
        assert np.array_equal(M.resize_crop(img, y0, x0, h, w, rh, rw), _pil_resize(img, y0, x0, h, w, rh, rw)), (H, W, y0, x0, h, w, rh, rw)


@pytest.mark.parametrize("S", [28, 84, 224])
def test_resize_model_bitexact_pipeline_sizes(S):
    rng = np.random.default_rng(S)
    a, o = image_data.eval_geometry(S)
    for H, W in [(1, 1), (17, 300), (32, 32), (105, 105), (375, 500), (600, 600)]:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert np.array_equal(M.resize_crop(img, 0, 0, H, W, a, a), _pil_resize(img, 0, 0, H, W, a, a))     # eval (up- and downscaling)
        y0, x0, h, w, _ = image_data.draw_crop_params(rng, [H], [W])
        args = (int(y0[0]), int(x0[0]), int(h[0]), int(w[0]), S, S)
        assert np.array_equal(M.resize_crop(img, *args), _pil_resize(img, *args))                               # aug: the crop is a new image


def test_crop_is_not_resize_box():
    """crop(box).resize() clamps the filter to the window; resize(box=) reads pixels outside it: the two differ, the model follows the former."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (120, 160, 3), dtype=np.uint8)
    boxed = np.asarray(Image.fromarray(img).resize((28, 28), Image.BILINEAR, box=(30, 20, 130, 100)))
    model = M.resize_crop(img, 20, 30, 80, 100, 28, 28)
    assert np.array_equal(model, _pil_resize(img, 20, 30, 80, 100, 28, 28))
    assert not np.array_equal(model, boxed)


def test_jitter_model_bitexact():
    rng = np.random.default_rng(1)
    factors = [np.float32(0.6), np.float32(1.4)] + list(image_data.draw_jitter(rng, 60).reshape(-1))
    for i in range(60):
        S = (28, 84, 224)[i % 3]
        img = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
        f = [factors[(3 * i + k) % len(factors)] for k in range(3)]
        im = Image.fromarray(img)
        for fa, e in zip(f, (ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color)):
            im = e(im).enhance(float(fa)).convert('RGB')
        assert np.array_equal(np.asarray(im), M.jitter(img, *f)), f


def test_to_tensor_normalize_model_matches_reference_helper():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)
    row = np.array([0, 40, 50, 0, 0, 40, 50, 40, 50, 0, 0, 0])
    ref = image_data.pil_reference(Image.fromarray(img), row, 28).numpy()
    assert np.array_equal(ref.view(np.int32), M.to_tensor_normalize(img[:28, :28]).view(np.int32))


# ---- libdkt_data.so -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data_lib():
    dkt_amd._lib.build()
    return dkt_amd._lib.load_data()


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(dkt_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run([OBJDUMP, "-T", path], capture_output=True, text=True, check=True).stdout
    return sorted({line.split()[-1] for line in out.splitlines() if " .text" in line and line.split()[-1].startswith("dkt_")})


def test_data_library_exports_exactly_its_header(data_lib):
    declared = _declared("dkt_abi_data.h")
    assert declared == ["dkt_augment_plan", "dkt_augment_u8", "dkt_data_abi_version"]
    assert sorted(dkt_amd._lib.DATA_SIGNATURES) == declared
    assert _exports(dkt_amd._lib.DATA_LIB_PATH) == declared
    assert data_lib.dkt_data_abi_version() == dkt_amd._lib.data_abi_version_of_header() == 1
    # the product library does not carry them
    assert not any(n.startswith("dkt_augment") for n in _exports(dkt_amd._lib.LIB_PATH))


def test_data_library_does_not_spill(data_lib):
    path = os.path.join(os.path.dirname(dkt_amd._lib.LIB_PATH), "build", "libdkt_data.so.resource_usage.json")
    usage = json.load(open(path))
    assert len(usage) == 3 and any("aug_coeff_kernel" in k for k in usage)
    assert all(u.get("vgpr_spill", 0) == 0 and u.get("scratch", 0) == 0 for u in usage.values())
    assert dkt_amd._lib.check_resources(usage) == []


def _row(H=40, W=50, y0=0, x0=0, h=None, w=None, rh=28, rw=28, oy=0, ox=0, off=0):
    return [off, H, W, y0, x0, h or H, w or W, rh, rw, oy, ox, 0]


def _plan(lib, rows, S=28):
    t = np.ascontiguousarray(np.array(rows, dtype=np.int64))
    ws = ctypes.c_size_t(0)
    st = lib.dkt_augment_plan(t.ctypes.data_as(ctypes.c_void_p), len(rows), S, ctypes.byref(ws))
    return st, t, ws.value


def test_plan_layout_and_rejections(data_lib):
    st, t, ws = _plan(data_lib, [_row(), _row(H=500, W=375, rh=32, rw=32, oy=2, ox=2)])
    # per image: xmin, n, ymin, n [S] + S x (Kx + Ky) 22-bit weights, Pillow's ksize = 2 ceil(max(in / out, 1)) + 1 taps per output index
    assert st == 0 and t[0, 11] == 0 and t[1, 11] == 4 * 28 + 28 * (5 + 5)
    assert ws == 4 * (t[1, 11] + 4 * 28 + 28 * (25 + 33))
    bad = [
        _row(H=0), _row(W=16385), _row(y0=1),                        # window outside the image (y0 + h > H)
        _row(x0=-1, w=10), _row(rh=27),                              # resize target smaller than S
        _row(oy=1), _row(ox=-1), _row(off=-3), _row(rw=16385),
    ]
    for r in bad:
        assert _plan(data_lib, [r])[0] == -1, r
    assert _plan(data_lib, [_row()], S=0)[0] == -1
    assert _plan(data_lib, [_row(rh=300, rw=300)], S=257)[0] == -1
    assert _plan(data_lib, [_row(H=16384, W=16384, rh=28, rw=28)], S=28)[0] == 0     # no source-size limit below 16384 per side


def test_augment_argument_errors_do_not_launch(data_lib):
    L, p = data_lib, FAKE
    st, t, ws = _plan(L, [_row(), _row(H=17, W=300)])
    th = t.ctypes.data_as(ctypes.c_void_p)
    m = (ctypes.c_float * 3)(0.485, 0.456, 0.406)
    s = (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    pool = 40 * 50 * 3 + 17 * 300 * 3
    t[1, 0] = 40 * 50 * 3
    st, t, ws = _plan(L, t.tolist())
    th = t.ctypes.data_as(ctypes.c_void_p)

    def call(pool_p=p, pool_bytes=pool, table=th, tdev=p, B=2, jit=None, flip=None, S=28, mean=m, std=s, out=p, wsp=p, wsb=ws):
        return L.dkt_augment_u8(pool_p, pool_bytes, table, tdev, B, jit, flip, S, mean, std, out, wsp, wsb, None)

    assert call(pool_p=None) == -1 and call(table=None) == -1 and call(tdev=None) == -1 and call(out=None) == -1 and call(wsp=None) == -1
    assert call(mean=None) == -1 and call(std=None) == -1
    assert call(B=0) == -1 and call(S=0) == -1 and call(S=257) == -1
    assert call(pool_bytes=pool - 1) == -1                        # the second image would end past the pool
    assert call(wsb=ws - 4) == -3                                 # workspace too small
    assert call(out=p + 2) == -1 and call(wsp=p + 4) == -1 and call(jit=p + 1) == -1
    z = (ctypes.c_float * 3)(0.229, 0.0, 0.225)
    assert call(std=z) == -1
    t2 = t.copy()
    t2[1, 11] += 4                                                # a table that was not planned
    assert call(table=t2.ctypes.data_as(ctypes.c_void_p)) == -1
    t3 = t.copy()
    t3[0, 7] = 27                                                 # resize target below S
    assert call(table=t3.ctypes.data_as(ctypes.c_void_p)) == -1


# ---- loader logic --------------------------------------------------------------------------------------------------------------------------------

def test_split_to_file_mapping(monkeypatch):
    dd = {k: '/d/%s/' % k for k in ('CUB', 'miniImagenet', 'omniglot', 'emnist')}
    monkeypatch.setattr(configs, 'data_dir', dd)
    for ds in ('CUB', 'miniImagenet', 'omniglot', 'emnist'):
        for sp in ('base', 'val', 'novel'):
            assert image_data.filelist_path(ds, sp) == '/d/%s/%s.json' % (ds, sp)
    assert image_data.filelist_path('cross', 'base') == '/d/miniImagenet/all.json'
    assert image_data.filelist_path('cross', 'val') == '/d/CUB/val.json'
    assert image_data.filelist_path('cross', 'novel') == '/d/CUB/novel.json'
    assert image_data.filelist_path('cross_char', 'base') == '/d/omniglot/noLatin.json'
    assert image_data.filelist_path('cross_char', 'val') == '/d/emnist/val.json'
    assert image_data.filelist_path('cross_char', 'novel') == '/d/emnist/novel.json'
    with pytest.raises(ValueError):
        image_data.filelist_for('QMUL', 'base')


def test_missing_filelist_names_path_and_writer(tmp_path, monkeypatch):
    monkeypatch.setitem(configs.data_dir, 'CUB', str(tmp_path / 'nowhere') + '/')
    p = SimpleNamespace(dataset='CUB')
    with pytest.raises(FileNotFoundError) as ei:
        get_episode_loader(p, 'base', 5, 5, 16, 1, 84, aug=True)
    msg = str(ei.value)
    assert str(tmp_path / 'nowhere' / 'base.json') in msg and 'filelists/CUB/write_CUB_filelist.py' in msg
    monkeypatch.setitem(configs.data_dir, 'omniglot', str(tmp_path / 'o') + '/')
    with pytest.raises(FileNotFoundError, match='write_cross_char_base_filelist.py'):
        get_episode_loader(SimpleNamespace(dataset='cross_char'), 'base', 5, 1, 1, 1, 28)
    monkeypatch.setitem(configs.data_dir, 'miniImagenet', str(tmp_path / 'm') + '/')
    with pytest.raises(FileNotFoundError, match='write_cross_filelist.py'):
        get_episode_loader(SimpleNamespace(dataset='cross'), 'base', 5, 1, 1, 1, 84)


def test_too_small_class_is_rejected(tmp_path):
    base = image_tree.make_split(str(tmp_path), 'base', 5, 4, [(20, 30)])
    with pytest.raises(ValueError, match=r'class \d+ has 4 images.*n_support \+ n_query = 6'):
        image_data.FilelistEpisodeLoader(base, 5, 1, 5, n_episode=1, image_size=28)


def test_tree_decodes_to_rgb_and_headers_match(tmp_path):
    base = image_tree.make_split(str(tmp_path), 'base', 2, 4, [(20, 30), (7, 9)])
    meta = image_data.read_filelist(base)
    modes = set()
    for p in meta['image_names']:
        with Image.open(p) as im:
            modes.add(im.mode)
        a = image_data.decode(p)
        assert a.dtype == np.uint8 and a.shape[2] == 3 and a.shape[:2] == image_data.image_size_of(p)
    assert {'L', 'RGBA', 'RGB'} <= modes
    assert any(p.endswith('.png') for p in meta['image_names']) and any(p.endswith('.jpg') for p in meta['image_names'])


def test_crop_params_inside_image_and_fallback():
    rng = np.random.default_rng(0)
    H = np.array([1, 2, 17, 375, 500, 105, 1, 3000, 16384] * 50)
    W = np.array([1, 300, 300, 500, 375, 105, 5000, 2, 16384] * 50)
    y0, x0, h, w, hit = image_data.draw_crop_params(rng, H, W)
    assert ((h >= 1) & (w >= 1) & (y0 >= 0) & (x0 >= 0) & (y0 + h <= H) & (x0 + w <= W)).all()
    # extreme aspect ratios never draw an accepted crop: the central fallback clamped to the ratio range
    ext = (W / H > 100) | (H / W > 100)
    assert ext.any() and not hit[ext].any()
    i = np.nonzero((H == 1) & (W == 5000))[0][0]
    assert (h[i], w[i], y0[i], x0[i]) == (1, round(1 * 4 / 3), 0, (5000 - 1) // 2)
    i = np.nonzero((H == 3000) & (W == 2))[0][0]
    assert (h[i], w[i], y0[i], x0[i]) == (round(2 / 0.75), 2, (3000 - 3) // 2, 0)
    assert hit[(H == 375) & (W == 500)].mean() > 0.9


def test_eval_geometry():
    assert image_data.eval_geometry(84) == (96, 6)
    assert image_data.eval_geometry(28) == (32, 2)
    assert image_data.eval_geometry(224) == (257, 16)        # round(16.5) == 16, Python's rounding like torchvision's


def test_episode_draw_class_pools_and_labels(tmp_path, monkeypatch):
    base = image_tree.make_split(str(tmp_path), 'base', 7, 6, [(20, 30), (11, 13)], label_base=40)
    monkeypatch.setattr(image_data.torch.cuda, 'current_device', lambda: 0)
    ld = image_data.FilelistEpisodeLoader(base, 5, 2, 3, n_episode=2, image_size=28, aug=True, mode='streaming')
    labels = np.asarray(image_data.read_filelist(base)['image_labels'])
    assert ld.classes.tolist() == list(range(40, 47))
    for _ in range(4):
        idx, y, table, jit, flip = ld._draw()
        assert y.shape == (5, 5) and len(set(y[:, 0].tolist())) == 5 and (y == y[:, :1]).all()
        assert (labels[idx].reshape(5, 5) == y).all()
        assert all(len(set(r)) == 5 for r in idx.reshape(5, 5).tolist())                  # distinct images within a class
        assert table.shape == (25, 12) and jit.shape == (25, 3) and flip.shape == (25,)
        assert ((jit >= 0.6) & (jit <= 1.4)).all() and jit.dtype == np.float32
        assert (table[:, 7] == 28).all() and (table[:, 8] == 28).all()
    ld.pool_threads.shutdown()
