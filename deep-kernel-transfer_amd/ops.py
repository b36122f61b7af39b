"""Torch-facing wrappers over the C ABI (include/dkt_abi.h): raw device pointers + the current HIP
stream go down, nothing else.  PyTorch only owns the memory and the stream.

Every function REQUIRES float32 CUDA (ROCm) tensors and raises otherwise -- there is no CPU path.  The one exception is the trunk output X of
the front-end calls (bn_stats, gram_bn, gram_bn_train, gram_bn_bwd, affine_normalize, normalize_bn_bwd, episode_loss_bn): bfloat16 / float16 X
(a backbone under torch.autocast) goes to the 16-bit kernels of libdkt_x16.so (include/dkt_abi_x16.h), with dX in X's dtype; never an fp32 copy.

Autograd surface
  episode_loss_linear(z, y, sv, mean, noise, cls_weight) -> obj[B]   (fused: gram -> mll -> gram_bwd)
  base_matrix(z, kind, lengthscale) -> E[B,N,N]                       (differentiable Gram / RBF)
  mll_objective(e, y, sv, mean, noise, cls_weight) -> obj[B], aux     (differentiable in e, sv, mean, noise)
  laplace_objective / dirichlet_objective and their episode_loss_* forms: the same episode under a Bernoulli (Laplace approximation) or a
  Dirichlet classification likelihood (docs/LAPLACE.md, docs/DIRICHLET.md)
  loo_objective and its episode_loss_loo* forms: the Gaussian model fitted by its leave-one-out predictive likelihood (libdkt_loo.so; docs/LOO.md)
which replace `-self.mll(self.model(*inputs), targets)` + `.backward()` of the reference
(methods/DKT.py:161-163, methods/DKT_regression.py:53-56).
At test time (no autograd): predict / predict_var (mean, diagonal variance) and posterior (libdkt_post.so; docs/POSTERIOR.md): the joint posterior of the
query rows -- full covariance, its factor, joint and marginal predictive log likelihood, function draws.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Callable, NamedTuple, Optional

import torch

from . import _lib

KERNEL_LINEAR = 0
KERNEL_RBF = 1
KERNEL_SQDIST = 2
KERNEL_LINEAR_UNIT = 3      # linear + the promise |a| <= 1 element-wise (rows went through F.normalize)
GRAM_UNIT_ROWS = 1          # the same promise for the rows of Z in gram_bwd
GRAM_W_SYMMETRIC = 2        # gram_bwd: every W[b] is symmetric (as dkt_mll_f32 writes it)
MLL_WANT_GRAD = 1
MLL_WANT_CHOL = 2
MLL_FORCE_GENERIC = 4
MLL_FORCE_REG = 8
MLL_FORCE_BLOCKED = 16
MLL_FORCE_F32MFMA = 32
MLL_E_PER_CLASS = 64
MLL_FORCE_TILED = 128
MLL_FORCE_BAND = 256
MLL_NO_KAPPA_GUARD = 512

LINEAR_KINDS = ("linear", "cossim", "bncossim")
RBF_KINDS = ("rbf", "RBF")
MATERN_KINDS = ("matern",)
POLY_KINDS = {"poli1": 1, "poli2": 2}


def kind_id(kernel: str) -> int:
    if kernel in LINEAR_KINDS:
        return KERNEL_LINEAR
    if kernel in RBF_KINDS:
        return KERNEL_RBF
    raise ValueError("[ERROR] the kernel '" + str(kernel) + "' is not supported!")


def _req(t: torch.Tensor, name: str, ndim: Optional[int] = None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("dkt_amd.ops: `%s` must be a CUDA/ROCm tensor -- the DKT hot path is HIP-only "
                           "(no CPU fallback)" % name)
    if t.dtype != torch.float32:
        raise RuntimeError("dkt_amd.ops: `%s` must be float32, got %s" % (name, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise RuntimeError("dkt_amd.ops: `%s` must have %d dims, got %s" % (name, ndim, tuple(t.shape)))
    return t.contiguous()


_X16_DTYPES = {torch.bfloat16: _lib.X_BF16, torch.float16: _lib.X_F16}


def _req_x(t: torch.Tensor, name: str, ndim: Optional[int] = None) -> torch.Tensor:
    """The trunk output of the front-end calls: float32 (the product library), bfloat16 or float16 (libdkt_x16.so)."""
    if isinstance(t, torch.Tensor) and t.dtype in _X16_DTYPES:
        if not t.is_cuda:
            raise RuntimeError("dkt_amd.ops: `%s` must be a CUDA/ROCm tensor -- the DKT hot path is HIP-only (no CPU fallback)" % name)
        if ndim is not None and t.dim() != ndim:
            raise RuntimeError("dkt_amd.ops: `%s` must have %d dims, got %s" % (name, ndim, tuple(t.shape)))
        return t.contiguous()
    return _req(t, name, ndim)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------
# The front door of the per-class GP calls: ONE place that says what such a problem looks like (`_problem`), what element strides the C ABI gets for an operand
# that is shared by the class models or has a class axis (`_class_strides`), and how outputs and workspaces are made (`_f32`, `_i32`, `_workspace`).  All of it
# allocates through this module's `torch`: the guard arena (tests/guard_arena.py) swaps that attribute, an allocation made anywhere else escapes it.
# ------------------------------------------------------------------------------------------------
_OPTIONAL_HYPERS = ("cls_weight", "scale")     # may be None (the kernels take NULL: weight / scale 1); every other per-class vector is required


class _Problem(NamedTuple):
    """B episodes of C class models on N rows, validated and contiguous.  base: [B,N,N] (shared by the class models) or [B,C,N,N] (per_class), or None and
    rows: [B,N,D]; y (and noise_rows, or None): [C,N] (every episode) or [B,C,N]; hypers: the per-class vectors, [C] each, in the order they were named."""
    base: Optional[torch.Tensor]
    rows: Optional[torch.Tensor]
    y: torch.Tensor
    noise_rows: Optional[torch.Tensor]
    hypers: tuple
    b: int
    c: int
    n: int
    d: Optional[int]                  # columns of rows
    per_class: bool
    base_strides: Optional[tuple]     # (batch_stride, class_stride) of base, in elements
    y_bstride: int                    # 0: y is shared by the episodes
    nr_bstride: int
    dev: torch.device


def _class_strides(t: torch.Tensor, c: int, item_ndim: int = 2) -> tuple:
    """(batch_stride, class_stride) in elements of a contiguous [B, ...item] (shared by the C class models: class stride 0) or [B, C, ...item]."""
    size = 1
    for s in t.shape[-item_ndim:]:
        size *= s
    return (c * size, size) if t.dim() == item_ndim + 2 else (size, 0)


def _hypers(fn: str, c: int, hypers: dict) -> tuple:
    """The per-class vectors of `fn`, each flattened to a contiguous [C]; None stays None where the ABI allows it."""
    out = []
    for name, h in hypers.items():
        if h is None and name not in _OPTIONAL_HYPERS:
            raise RuntimeError("%s: `%s` is required (only %s may be None)" % (fn, name, " / ".join(_OPTIONAL_HYPERS)))
        if h is not None:
            if isinstance(h, torch.Tensor) and h.dim() != 1:         # ([C,1], [1,C], a scalar: flattened; a [C] as it is, no view made on the launch-bound paths)
                h = h.reshape(-1)
            h = _req(h, name, 1)
            if h.numel() != c:
                raise RuntimeError("%s: `%s` must have C=%d elements, got %d" % (fn, name, c, h.numel()))
        out.append(h)
    return tuple(out)


def _problem(fn: str, y, base=None, rows=None, noise_rows=None, base_name: str = "e", y_name: str = "y", **hypers) -> _Problem:
    """Validate the operands of the per-class GP call `fn` (its public name, for the messages): a base matrix or rows, y, optionally noise_rows, and the
    per-class vectors by name.  A vector may be None only under a name listed in _OPTIONAL_HYPERS (the ABI takes NULL for those): a call with another
    optional vector adds its name there; any other None is refused by name.  Every rejection is a RuntimeError that starts with `fn` (or with dkt_amd.ops: where `_req` refuses a tensor)."""
    d = strides = None
    if rows is not None:
        rows = _req(rows, "z", 3)
        b, n, d = rows.shape
        per_class, dev = False, rows.device
    else:
        base = _req(base, base_name)
        if base.dim() not in (3, 4) or base.shape[-1] != base.shape[-2]:
            raise RuntimeError("%s: %s must be [B,N,N] or [B,C,N,N], got %s" % (fn, base_name, tuple(base.shape)))
        b, n = base.shape[0], base.shape[-1]
        per_class, dev = base.dim() == 4, base.device
    y = _req(y, y_name)
    if y.dim() not in (2, 3) or y.shape[-1] != n or (y.dim() == 3 and y.shape[0] != b):
        raise RuntimeError("%s: %s must be [C,N] or [B,C,N] with B=%d, N=%d, got %s" % (fn, y_name, b, n, tuple(y.shape)))
    c = y.shape[-2]
    if per_class and base.shape[1] != c:
        raise RuntimeError("%s: a per-class %s must be [B,C=%d,N,N], got %s" % (fn, base_name, c, tuple(base.shape)))
    if base is not None:
        strides = _class_strides(base, c)
    nr_bstride = 0
    if noise_rows is not None:
        noise_rows = _req(noise_rows, "noise_rows")
        if noise_rows.dim() not in (2, 3) or tuple(noise_rows.shape[-2:]) != (c, n) or (noise_rows.dim() == 3 and noise_rows.shape[0] != b):
            raise RuntimeError("%s: noise_rows must be [C,N] or [B,C,N] like %s %s, got %s" % (fn, y_name, tuple(y.shape), tuple(noise_rows.shape)))
        nr_bstride = c * n if noise_rows.dim() == 3 else 0
    return _Problem(base, rows, y, noise_rows, _hypers(fn, c, hypers), b, c, n, d, per_class, strides, c * n if y.dim() == 3 else 0, nr_bstride, dev)


def _f32(dev, *shape) -> torch.Tensor:
    return torch.empty(shape, device=dev, dtype=torch.float32)


def _i32(dev, *shape) -> torch.Tensor:
    return torch.empty(shape, device=dev, dtype=torch.int32)


def _workspace(nbytes: int, dev=None) -> Optional[torch.Tensor]:
    """The scratch of a library call from its *_workspace_bytes* query: None for 0, else float32 of (nbytes + 3) // 4 elements.  Every query -- csrc/:
    dkt_mll_workspace_bytes_for (the plan of dkt_mll.hip over the band, tiled, blocked and generic counts), dkt_laplace_grad_, dkt_mll_rownoise_,
    dkt_bn_param_grads_workspace_bytes; csrc_ext/: dkt_loofs_, dkt_posterior_workspace_bytes; libdkt_smk.so: dkt_smk_task_workspace_bytes -- returns a float
    count times sizeof(float): 0 or a positive multiple of 4.  For those, the sizes this module used to spell out -- (nbytes + 3) // 4, (max(nbytes, 4) + 3) // 4,
    nbytes // 4, max(nbytes, 4) // 4 -- are the same element count, a block of exactly nbytes (what the guard arena's placement verdict looks for).  They differ
    at 0 only: smk_task_bwd took one float there.  Its query is 0 exactly for B, D or Q <= 0, which dkt_smk_task_bwd_f32 refuses (DKT_ERR_BAD_ARG) in the
    same test that refuses a NULL workspace."""
    return torch.empty((nbytes + 3) // 4, device=dev, dtype=torch.float32) if nbytes else None


# Optional per-kernel timing (bench.py): HIP events recorded on the stream the kernel is launched on
# (torch's current stream), read back after the timed region -- no synchronisation while recording.
_kernel_events = None


def kernel_timing(enable: bool) -> None:
    global _kernel_events
    _kernel_events = {} if enable else None


def kernel_timing_results() -> dict:
    """name -> (launches, mean ms).  Call after torch.cuda.synchronize()."""
    out = {}
    for name, pairs in (_kernel_events or {}).items():
        ms = [a.elapsed_time(b) for a, b in pairs]
        out[name] = (len(ms), sum(ms) / max(len(ms), 1))
    return out


class _timed:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _kernel_events is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if _kernel_events is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _kernel_events.setdefault(self.name, []).append((self.a, b))
        return False


# ------------------------------------------------------------------------------------------------
# raw (non-differentiable) entry points
# ------------------------------------------------------------------------------------------------
# Switches the PRODUCT library reads (dispatch thresholds / the process-wide exact-fp32 request of include/dkt_abi.h); everything else is a variant switch that only
# the twins library (libdkt_twins.so, -DDKT_TWINS) knows: with DKT_TWINS=1 in the environment AND one of them set, the calls of this module go to that library
# (tests, A/B tools).  Without DKT_TWINS=1 the variant switches have no effect at all.  The names are the table the libraries themselves read: csrc/dkt_switches.def.
with open(os.path.join(_lib.CSRC, "dkt_switches.def")) as _fh:
    _SWITCH_TABLE = re.findall(r"^X\((\w+), (PRODUCT|VARIANT)\)", _fh.read(), re.M)
_PRODUCT_SWITCHES = tuple("DKT_" + n for n, c in _SWITCH_TABLE if c == "PRODUCT")
_VARIANT_SWITCHES = tuple("DKT_" + n for n, c in _SWITCH_TABLE if c == "VARIANT")
_ENV_SWITCHES = _PRODUCT_SWITCHES + _VARIANT_SWITCHES
_env_seen = {}           # id(lib) -> {switch: value} as of the library's last (re)read of the environment


def _sync_env(lib, names=None) -> None:
    """The library reads its switches once; when a test or an A/B tool changed one inside this process, tell it.  `names`: the switches that can matter for this
    library (the product reads the 4 product switches only: ~ 4 instead of ~ 30 environment look-ups per call on the launch-bound small-batch paths).  The snapshot
    is per library and covers every switch, whichever subset a call compares: a process that alternates the two name sets on the same library (DKT_TWINS toggled)
    reloads only when a switch really changed."""
    seen = _env_seen.get(id(lib))
    if seen is None or any(os.environ.get(k) != seen[k] for k in (names or _ENV_SWITCHES)):
        snap = {k: os.environ.get(k) for k in _ENV_SWITCHES}
        if seen is not None or any(v is not None for v in snap.values()):
            _lib.reload_env(lib)
        _env_seen[id(lib)] = snap


def _lib_now(want_twin: bool = False):
    """The library this call goes to: the product, or -- DKT_TWINS=1 and a variant switch set (or `want_twin`: a call that names a validation twin the
    product library serves with its generic kernel, e.g. force_f32mfma) -- the twins build of the same ABI.  DKT_TWINS=force: the twins build for every call."""
    tw = os.environ.get("DKT_TWINS")
    if tw is None or tw == "0":                               # the product library, no variant switch can apply: one lookup per call, the 4 product switches synced
        lib = _lib.load()
        _sync_env(lib, _PRODUCT_SWITCHES)
        return lib
    if tw == "force":                                         # (tests of the twins library's own instantiations)
        lib = _lib.load_twins()
    elif os.environ.get("DKT_TWINS") == "1" and (want_twin or os.environ.get("DKT_MLL_F32MFMA") == "1" or any(os.environ.get(k) is not None for k in _VARIANT_SWITCHES)):
        lib = _lib.load_twins()
    else:
        lib = _lib.load()
    _sync_env(lib)
    return lib


def _front_end(stem: str, x: torch.Tensor, args: list, xpos: int) -> None:
    """Launch a front-end call on X = args[xpos]: dkt_<stem>_f32 of the product library (or its twins build) for fp32 X, as always; dkt_<stem>_x16 of
    libdkt_x16.so for bfloat16 / float16 X, with its `xdtype` inserted right after X (there is no twin of those: DKT_TWINS does not apply)."""
    xdt = _X16_DTYPES.get(x.dtype)
    if xdt is None:
        name, lib = "dkt_%s_f32" % stem, _lib_now()
    else:
        name, lib = "dkt_%s_x16" % stem, _lib.load_x16()
        _sync_env(lib, _PRODUCT_SWITCHES)
        args = args[:xpos + 1] + [xdt] + args[xpos + 1:]
    with _timed(name):
        st = getattr(lib, name)(*args)
    _lib.check(st, name)


def gram(a: torch.Tensor, bm: Optional[torch.Tensor] = None, kind: int = KERNEL_LINEAR,
         lengthscale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """E[b] = k(a[b], bm[b]); a:[B,M,D], bm:[B,N,D] or None (symmetric)."""
    a = _req(a, "a", 3)
    b_, m, d = a.shape
    if bm is not None:
        bm = _req(bm, "bm", 3)
        if bm.shape[0] != b_ or bm.shape[2] != d:
            raise RuntimeError("gram: shape mismatch %s vs %s" % (tuple(a.shape), tuple(bm.shape)))
        n = bm.shape[1]
    else:
        n = m
    if kind not in (KERNEL_LINEAR, KERNEL_LINEAR_UNIT):
        lengthscale = _req(lengthscale.reshape(-1), "lengthscale", 1)
    e = torch.empty((b_, m, n), device=a.device, dtype=torch.float32)
    lib = _lib_now()
    with _timed("dkt_gram_f32"):
        st = lib.dkt_gram_f32(_p(a), _p(bm), _p(e), b_, m, n, d, kind, _p(lengthscale), _stream())
    _lib.check(st, "dkt_gram_f32")
    return e


def mll(e: torch.Tensor, y: torch.Tensor, sv: torch.Tensor, mean: torch.Tensor, noise: torch.Tensor,
        want_grad: bool = False, want_chol: bool = False, cls_weight: Optional[torch.Tensor] = None,
        jitter0: float = 1e-6, max_tries: int = 3, force_generic: bool = False, force_reg: bool = False,
        force_blocked: bool = False, force_f32mfma: bool = False, force_tiled: bool = False, force_band: bool = False, no_kappa_guard: bool = False) -> dict:
    """Exact-GP marginal log likelihood of C models per episode.  e:[B,N,N] (one base matrix shared by the class models) or
    [B,C,N,N] (one per class model: DKT_MLL_E_PER_CLASS -- then w is [B,C,N,N] too); y:[C,N] (shared) or [B,C,N].
    force_*: the parity-tested twins of the default kernels (DKT_MLL_FORCE_* of include/dkt_abi.h)."""
    pr = _problem("mll", y, base=e, sv=sv, mean=mean, noise=noise, cls_weight=cls_weight)
    e, y, (sv, mean, noise, cls_weight) = pr.base, pr.y, pr.hypers
    b_, c_, n, per_class, y_bstride, dev = pr.b, pr.c, pr.n, pr.per_class, pr.y_bstride, pr.dev
    logp, alpha, jit, info = _f32(dev, b_, c_), _f32(dev, b_, c_, n), _f32(dev, b_, c_), _i32(dev, b_, c_)
    flags = ((MLL_FORCE_GENERIC if force_generic else 0) | (MLL_FORCE_BLOCKED if force_blocked else 0) |
             (MLL_FORCE_F32MFMA if force_f32mfma else 0) | MLL_E_PER_CLASS * per_class | (MLL_FORCE_TILED if force_tiled else 0) | (MLL_FORCE_BAND if force_band else 0) | (MLL_NO_KAPPA_GUARD if no_kappa_guard else 0))
    chol = w = dsv = dmean = dnoise = None
    if want_chol:
        flags |= MLL_WANT_CHOL
        chol = _f32(dev, b_, c_, n, n)
    if want_grad:
        flags |= MLL_WANT_GRAD
        w = _f32(dev, *e.shape)                                # (in the layout of e: [B,N,N] summed over the classes, or [B,C,N,N])
        dsv, dmean, dnoise = _f32(dev, b_, c_), _f32(dev, b_, c_), _f32(dev, b_, c_)
    if force_reg and n + 1 <= 128:                           # (beyond its range the call takes the default kernels, as DKT_MLL_FORCE_REG did)
        # the round-1 register-sweep kernel: a validation twin in the measurement library (libdkt_diag.so) since round 4, not part of the product ABI
        if per_class or force_generic or force_blocked or force_f32mfma:
            raise RuntimeError("mll: force_reg combines with want_grad / want_chol only")
        dlib = _lib.load_diag()
        st = dlib.dkt_diag_mll_reg_f32(_p(e), _p(y), y_bstride, _p(sv), _p(mean), _p(noise), b_, c_, n, float(jitter0), int(max_tries),
                                       flags & (MLL_WANT_GRAD | MLL_WANT_CHOL), _p(cls_weight), _p(logp), _p(alpha), _p(chol), _p(w), _p(dsv), _p(dmean), _p(dnoise),
                                       _p(jit), _p(info), _stream())
        _lib.check(st, "dkt_diag_mll_reg_f32")
        return dict(logp=logp, alpha=alpha, jitter=jit, info=info, chol=chol, w=w, dsv=dsv, dmean=dmean, dnoise=dnoise)
    lib = _lib_now(want_twin=force_f32mfma)
    ws_bytes = int(lib.dkt_mll_workspace_bytes_for(b_, c_, n, flags))           # what THIS call needs (the flag-less query covers every flag combination)
    ws = _workspace(ws_bytes, dev)
    with _timed("dkt_mll_f32"):
        st = lib.dkt_mll_f32(_p(e), _p(y), y_bstride, _p(sv), _p(mean), _p(noise), b_, c_, n,
                             float(jitter0), int(max_tries), flags, _p(cls_weight), _p(logp), _p(alpha),
                             _p(chol), _p(w), _p(dsv), _p(dmean), _p(dnoise), _p(jit), _p(info), _p(ws),
                             ws_bytes, _stream())
    _lib.check(st, "dkt_mll_f32")
    return dict(logp=logp, alpha=alpha, jitter=jit, info=info, chol=chol, w=w, dsv=dsv, dmean=dmean, dnoise=dnoise)


def gram_bwd(w: torch.Tensor, z: torch.Tensor, ep_scale: Optional[torch.Tensor] = None, unit_rows: bool = False,
             w_symmetric: bool = False) -> torch.Tensor:
    """dZ[b] = ep_scale[b] * (W[b] + W[b]^T) Z[b].  unit_rows: the caller guarantees |z| <= 1 element-wise (rows that went
    through F.normalize), which lets the kernel use the scaled 2-way f16 split (DKT_GRAM_UNIT_ROWS).  w_symmetric: the caller
    states W[b] = W[b]^T (what dkt_mll_f32 writes): DKT_GRAM_W_SYMMETRIC, used by the 128 < N <= 448 kernel."""
    w = _req(w, "w", 3)
    z = _req(z, "z", 3)
    b_, n, d = z.shape
    if tuple(w.shape) != (b_, n, n):
        raise RuntimeError("gram_bwd: w must be [B,N,N]")
    if ep_scale is not None:
        ep_scale = _req(ep_scale.reshape(-1), "ep_scale", 1)
        if ep_scale.numel() != b_:
            raise RuntimeError("gram_bwd: ep_scale must have B elements")
    dz = torch.empty_like(z)
    lib = _lib_now()
    with _timed("dkt_gram_bwd_f32"):
        st = lib.dkt_gram_bwd_f32(_p(w), _p(z), _p(dz), b_, n, d, _p(ep_scale),
                                  (GRAM_UNIT_ROWS if unit_rows else 0) | (GRAM_W_SYMMETRIC if w_symmetric else 0), _stream())
    _lib.check(st, "dkt_gram_bwd_f32")
    return dz


def _req_distance_bwd(fn: str, w: torch.Tensor, m: torch.Tensor, mname: str, lengthscale: torch.Tensor):
    """Arguments of rbf_bwd / sqdist_bwd: w and the forward's matrix of the same [B,N,N] shape (a smaller w would be read past its end), ONE lengthscale
    (the kernels read element 0: a [C] tensor would silently mean class 0 -- per-class lengthscales go through class_kernel_bwd)."""
    w = _req(w, "w", 3)
    m = _req(m, mname, 3)
    if not isinstance(lengthscale, torch.Tensor):
        raise RuntimeError("%s: lengthscale must be a tensor" % fn)
    if m.shape[1] != m.shape[2]:
        raise RuntimeError("%s: %s must be [B,N,N], got %s" % (fn, mname, tuple(m.shape)))
    if w.shape != m.shape:
        raise RuntimeError("%s: w %s must have the shape of %s %s" % (fn, tuple(w.shape), mname, tuple(m.shape)))
    if lengthscale.numel() != 1:
        raise RuntimeError("%s: lengthscale must have one element (got %d); per-class lengthscales go through class_kernel_bwd" % (fn, lengthscale.numel()))
    return w, m, _req(lengthscale.reshape(-1), "lengthscale", 1)


def rbf_bwd(w: torch.Tensor, e: torch.Tensor, lengthscale: torch.Tensor):
    w, e, lengthscale = _req_distance_bwd("rbf_bwd", w, e, "e", lengthscale)
    b_, n, _ = e.shape
    wp = torch.empty_like(e)
    dl = torch.empty((b_,), device=e.device, dtype=torch.float32)
    lib = _lib_now()
    with _timed("dkt_rbf_bwd_f32"):
        st = lib.dkt_rbf_bwd_f32(_p(w), _p(e), _p(lengthscale), _p(wp), _p(dl), b_, n, _stream())
    _lib.check(st, "dkt_rbf_bwd_f32")
    return wp, dl


def sqdist_bwd(w: torch.Tensor, u: torch.Tensor, lengthscale: torch.Tensor):
    w, u, lengthscale = _req_distance_bwd("sqdist_bwd", w, u, "u", lengthscale)
    b_, n, _ = u.shape
    wp = torch.empty_like(u)
    dl = torch.empty((b_,), device=u.device, dtype=torch.float32)
    lib = _lib_now()
    _lib.check(lib.dkt_sqdist_bwd_f32(_p(w), _p(u), _p(lengthscale), _p(wp), _p(dl), b_, n, _stream()), "dkt_sqdist_bwd_f32")
    return wp, dl


def _matern25(u: torch.Tensor) -> torch.Tensor:
    """MaternKernel(nu=2.5) from the scaled squared distance (gpytorch clamps d2 >= 1e-30 before the sqrt).  Differentiable torch form, used by
    base_matrix() under autograd; the no-autograd paths take the HIP class map (dkt_class_kernel_f32)."""
    r = torch.sqrt(5.0 * u.clamp_min(1e-30))
    return (1.0 + r + r * r / 3.0) * torch.exp(-r)


def kernel_matrix(a: torch.Tensor, bm: Optional[torch.Tensor], kernel: str, lengthscale: Optional[torch.Tensor] = None,
                  offset: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Base kernel matrix k(a, bm) of ONE model (no autograd): all kernel types of ExactGPLayer (reference DKT.py:352-370).  Matern / polynomial:
    the contraction (dkt_gram_f32) + the element-wise class map of a one-class "episode" (dkt_class_kernel_f32)."""
    if kernel in LINEAR_KINDS:
        return gram(a, bm, KERNEL_LINEAR)
    if kernel in RBF_KINDS:
        return gram(a, bm, KERNEL_RBF, lengthscale)
    if kernel in MATERN_KINDS or kernel in POLY_KINDS:
        for nm, t in (("lengthscale", lengthscale), ("offset", offset)):
            if t is not None and t.numel() != 1:           # ONE model: per-class parameters go to kernel_matrix_per_class (a [C] tensor here would silently mean class 0)
                raise RuntimeError("kernel_matrix: %s must have one element (got %d); use kernel_matrix_per_class for per-class parameters" % (nm, t.numel()))
        return kernel_matrix_per_class(a, bm, kernel, None if lengthscale is None else lengthscale.reshape(-1)[:1],
                                       None if offset is None else offset.reshape(-1)[:1])[:, 0]
    raise ValueError("[ERROR] the kernel '" + str(kernel) + "' is not supported!")


def predict(ex: torch.Tensor, alpha: torch.Tensor, sv: torch.Tensor, mean: torch.Tensor, want_labels: bool = True):
    """mu[b,c,q] = mean[c] + sv[c] sum_n ex[b,(c,)q,n] alpha[b,c,n]; labels[b,q] = argmax_c mu (first maximum wins).
    ex: [B,M,N] (one base cross kernel shared by the class models: dkt_predict_f32) or [B,C,M,N] (one per class model: dkt_predict_per_class_f32)."""
    ex = _req(ex, "ex")
    alpha = _req(alpha, "alpha", 3)
    per_class, c_ = ex.dim() == 4, alpha.shape[1]
    if ex.dim() not in (3, 4) or alpha.shape[0] != ex.shape[0] or alpha.shape[2] != ex.shape[-1] or (per_class and ex.shape[1] != c_):
        raise RuntimeError("predict: ex must be [B,M,N] or [B,C,M,N] and alpha [B,C,N], got %s and %s" % (tuple(ex.shape), tuple(alpha.shape)))
    b_, m, n = ex.shape[0], ex.shape[-2], ex.shape[-1]
    sv = _req(sv.reshape(-1), "sv", 1)
    mean = _req(mean.reshape(-1), "mean", 1)
    mu = _f32(ex.device, b_, c_, m)
    labels = _i32(ex.device, b_, m) if want_labels else None
    lib = _lib_now()
    name = ("dkt_predict_f32", "dkt_predict_per_class_f32")[per_class]
    _lib.check(getattr(lib, name)(_p(ex), _p(alpha), _p(sv), _p(mean), _p(mu), _p(labels), b_, c_, m, n, _stream()), name)
    return mu, labels


def predict_var(ex: torch.Tensor, exx: torch.Tensor, chol: torch.Tensor, sv: torch.Tensor, noise: torch.Tensor):
    """var[b,c,q] = sv[c] exx[b,q] - sv[c]^2 |L[b,c]^-1 ex[b,q]|^2 + noise[c] (dkt_predict_var_f32).
    ex: [B,M,N] base cross kernel, exx: [B,M] its prior diagonal k(x*, x*), chol: [B,C,N,N] lower factors of mll(want_chol=True); sv, noise: C elements."""
    ex = _req(ex, "ex", 3)
    exx = _req(exx, "exx", 2)
    chol = _req(chol, "chol", 4)
    b_, m, n = ex.shape
    c_ = chol.shape[1]
    if tuple(exx.shape) != (b_, m):
        raise RuntimeError("predict_var: exx must be [B,M] = %s for ex %s, got %s" % ((b_, m), tuple(ex.shape), tuple(exx.shape)))
    if chol.shape[0] != b_ or chol.shape[2] != n or chol.shape[3] != n:
        raise RuntimeError("predict_var: chol must be [B,C,N,N] with B=%d, N=%d of ex %s, got %s" % (b_, n, tuple(ex.shape), tuple(chol.shape)))
    sv, noise = _hypers("predict_var", c_, dict(sv=sv, noise=noise))
    var = _f32(ex.device, b_, c_, m)
    lib = _lib_now()
    _lib.check(lib.dkt_predict_var_f32(_p(ex), _p(exx), _p(chol), _p(sv), _p(noise), _p(var), b_, c_, m, n, _stream()),
               "dkt_predict_var_f32")
    return var


def smk(x1: torch.Tensor, x2: Optional[torch.Tensor], weights: torch.Tensor, means: torch.Tensor, scales: torch.Tensor,
        want_terms: bool = False):
    """Spectral-mixture matrix E[b] = k(x1[b], x2[b]) (x2 None: symmetric); weights [Q], means / scales [Q,D]
    (constrained values).  Returns (E, Eq) with Eq [B,Q,M,N] the per-mixture terms (None unless want_terms)."""
    x1 = _req(x1, "x1", 3)
    b_, m, d = x1.shape
    if x2 is not None:
        x2 = _req(x2, "x2", 3)
        if x2.shape[0] != b_ or x2.shape[2] != d:
            raise RuntimeError("smk: shape mismatch %s vs %s" % (tuple(x1.shape), tuple(x2.shape)))
        n = x2.shape[1]
    else:
        n = m
    weights = _req(weights.reshape(-1), "weights", 1)
    q = weights.numel()
    means = _req(means.reshape(q, -1), "means", 2)
    scales = _req(scales.reshape(q, -1), "scales", 2)
    if means.shape[1] != d or scales.shape[1] != d:
        raise RuntimeError("smk: means / scales must be [Q,D] with D = %d" % d)
    e = torch.empty((b_, m, n), device=x1.device, dtype=torch.float32)
    eq = torch.empty((b_, q, m, n), device=x1.device, dtype=torch.float32) if want_terms else None
    lib = _lib_now()
    with _timed("dkt_smk_f32"):
        st = lib.dkt_smk_f32(_p(x1), _p(x2), _p(weights), _p(means), _p(scales), _p(e), _p(eq), b_, m, n, d, q, _stream())
    _lib.check(st, "dkt_smk_f32")
    return e, eq


def smk_bwd(ge: torch.Tensor, eq: torch.Tensor, x: torch.Tensor, weights: torch.Tensor, means: torch.Tensor,
            scales: torch.Tensor):
    """Chain rule of the symmetric spectral-mixture matrix: (dx [B,N,D], dmeans [B,Q,D], dscales [B,Q,D])."""
    ge = _req(ge, "ge", 3)
    eq = _req(eq, "eq", 4)
    x = _req(x, "x", 3)
    b_, n, d = x.shape
    q = eq.shape[1]
    weights = _req(weights.reshape(-1), "weights", 1)
    means = _req(means.reshape(q, -1), "means", 2)
    scales = _req(scales.reshape(q, -1), "scales", 2)
    dx = torch.empty_like(x)
    dmeans = torch.empty((b_, q, d), device=x.device, dtype=torch.float32)
    dscales = torch.empty((b_, q, d), device=x.device, dtype=torch.float32)
    lib = _lib_now()
    with _timed("dkt_smk_bwd_f32"):
        st = lib.dkt_smk_bwd_f32(_p(ge), _p(eq), _p(x), _p(weights), _p(means), _p(scales), _p(dx), _p(dmeans), _p(dscales),
                                 b_, n, d, q, _stream())
    _lib.check(st, "dkt_smk_bwd_f32")
    return dx, dmeans, dscales


# ------------------------------------------------------------------------------------------------
# autograd
# ------------------------------------------------------------------------------------------------
class _BaseMatrixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, lengthscale, kind):
        e = gram(z, None, kind, lengthscale)
        ctx.kind = kind
        ctx.save_for_backward(z, e if kind == KERNEL_RBF else None, lengthscale)
        return e

    @staticmethod
    def backward(ctx, ge):
        z, e, lengthscale = ctx.saved_tensors
        ge = ge.contiguous()
        dl = None
        if ctx.kind == KERNEL_RBF:
            wp, dlb = rbf_bwd(ge, e, lengthscale)
            dz = gram_bwd(wp, z)
            if ctx.needs_input_grad[1]:
                dl = dlb.sum().reshape(lengthscale.shape)
        else:
            dz = gram_bwd(ge, z)
        return (dz if ctx.needs_input_grad[0] else None), dl, None


class _SqDistFn(torch.autograd.Function):
    """U[b] = |z_i - z_j|^2 / l^2 (differentiable in z and l): the building block of the Matern kernel."""

    @staticmethod
    def forward(ctx, z, lengthscale):
        u = gram(z, None, KERNEL_SQDIST, lengthscale)
        ctx.save_for_backward(z, u, lengthscale)
        return u

    @staticmethod
    def backward(ctx, gu):
        z, u, lengthscale = ctx.saved_tensors
        wp, dlb = sqdist_bwd(gu.contiguous(), u, lengthscale)
        dz = gram_bwd(wp, z) if ctx.needs_input_grad[0] else None
        dl = dlb.sum().reshape(lengthscale.shape) if ctx.needs_input_grad[1] else None
        return dz, dl


class _SpectralMixtureFn(torch.autograd.Function):
    """E = SpectralMixtureKernel(z, z) differentiable in z, the mixture weights, means and scales."""

    @staticmethod
    def forward(ctx, z, weights, means, scales):
        e, eq = smk(z, None, weights, means, scales, want_terms=True)
        ctx.save_for_backward(z, eq, weights, means, scales)
        return e

    @staticmethod
    def backward(ctx, ge):
        z, eq, weights, means, scales = ctx.saved_tensors
        ge = ge.contiguous()
        dz, dmb, dsb = smk_bwd(ge, eq, z, weights, means, scales)
        dw = (ge.unsqueeze(1) * eq).sum((0, 2, 3)).reshape(weights.shape) if ctx.needs_input_grad[1] else None
        dm = dmb.sum(0).reshape(means.shape) if ctx.needs_input_grad[2] else None
        ds = dsb.sum(0).reshape(scales.shape) if ctx.needs_input_grad[3] else None
        return (dz if ctx.needs_input_grad[0] else None), dw, dm, ds


def spectral_mixture_matrix(z: torch.Tensor, weights: torch.Tensor, means: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Differentiable symmetric spectral-mixture matrix [B,N,N] of z [B,N,D] (reference DKT_regression.py:121-122)."""
    return _SpectralMixtureFn.apply(z, weights, means, scales)


# task-resident spectral mixture (libdkt_smk.so, include/dkt_abi_smk.h): many small tasks, a lane per entry, no Eq round trip
def smk_task_supported(m: int, n: int, d: int, q: int, symmetric: bool = True) -> bool:
    """Whether dkt_smk_task_f32 (symmetric: N <= 32; cross: M <= 256, N <= 32) and, when symmetric, its backward take this shape."""
    return (1 <= n <= _lib.SMK_MAX_N and 1 <= m <= (_lib.SMK_MAX_N if symmetric else _lib.SMK_MAX_M) and 1 <= d <= _lib.SMK_MAX_D
            and 1 <= q <= _lib.SMK_MAX_Q)


def _smk_hypers(weights, means, scales, d: int):
    weights = _req(weights.reshape(-1), "weights", 1)
    q = weights.numel()
    means = _req(means.reshape(q, -1), "means", 2)
    scales = _req(scales.reshape(q, -1), "scales", 2)
    if means.shape[1] != d or scales.shape[1] != d:
        raise RuntimeError("smk_task: means / scales must be [Q,D] with D = %d" % d)
    return weights, means, scales, q


def smk_task(x1: torch.Tensor, x2: Optional[torch.Tensor], weights: torch.Tensor, means: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Spectral-mixture matrix E[b] = k(x1[b], x2[b]) of libdkt_smk.so (x2 None: symmetric, exactly); the arguments of `smk`.  A shape outside
    the library's limits raises (DKT_ERR_SHAPE): `smk_task_supported` tells beforehand."""
    x1 = _req(x1, "x1", 3)
    b_, m, d = x1.shape
    if x2 is not None:
        x2 = _req(x2, "x2", 3)
        if x2.shape[0] != b_ or x2.shape[2] != d:
            raise RuntimeError("smk_task: shape mismatch %s vs %s" % (tuple(x1.shape), tuple(x2.shape)))
        n = x2.shape[1]
    else:
        n = m
    weights, means, scales, q = _smk_hypers(weights, means, scales, d)
    e = torch.empty((b_, m, n), device=x1.device, dtype=torch.float32)
    with _timed("dkt_smk_task_f32"):
        st = _lib.load_smk().dkt_smk_task_f32(_p(x1), _p(x2), _p(weights), _p(means), _p(scales), _p(e), b_, m, n, d, q, _stream())
    _lib.check(st, "dkt_smk_task_f32")
    return e


def smk_task_bwd(ge: torch.Tensor, x: torch.Tensor, weights: torch.Tensor, means: torch.Tensor, scales: torch.Tensor):
    """Chain rule of the symmetric task-resident matrix: (dx [B,N,D], dweights [Q], dmeans [Q,D], dscales [Q,D]), the hyper-parameter
    gradients summed over the B tasks inside the library (fixed order, bitwise reproducible)."""
    x = _req(x, "x", 3)
    b_, n, d = x.shape
    ge = _req(ge, "ge", 3)
    if tuple(ge.shape) != (b_, n, n):
        raise RuntimeError("smk_task_bwd: ge must be [B,N,N] = %s, got %s" % ((b_, n, n), tuple(ge.shape)))
    weights, means, scales, q = _smk_hypers(weights, means, scales, d)
    lib = _lib.load_smk()
    dx = torch.empty_like(x)
    dw = torch.empty((q,), device=x.device, dtype=torch.float32)
    dm = torch.empty((q, d), device=x.device, dtype=torch.float32)
    ds = torch.empty((q, d), device=x.device, dtype=torch.float32)
    ws = _workspace(int(lib.dkt_smk_task_workspace_bytes(b_, n, d, q)), x.device)
    with _timed("dkt_smk_task_bwd_f32"):
        st = lib.dkt_smk_task_bwd_f32(_p(ge), _p(x), _p(weights), _p(means), _p(scales), _p(dx), _p(dw), _p(dm), _p(ds), _p(ws), b_, n, d, q,
                                      _stream())
    _lib.check(st, "dkt_smk_task_bwd_f32")
    return dx, dw, dm, ds


class _SpectralMixtureTaskFn(torch.autograd.Function):
    """E = SpectralMixtureKernel(z, z) of libdkt_smk.so, differentiable in z, the mixture weights, means and scales."""

    @staticmethod
    def forward(ctx, z, weights, means, scales):
        e = smk_task(z, None, weights, means, scales)
        ctx.save_for_backward(z, weights, means, scales)
        return e

    @staticmethod
    def backward(ctx, ge):
        z, weights, means, scales = ctx.saved_tensors
        dz, dw, dm, ds = smk_task_bwd(ge.contiguous(), z, weights, means, scales)
        need = ctx.needs_input_grad
        return (dz if need[0] else None, dw.reshape(weights.shape) if need[1] else None, dm.reshape(means.shape) if need[2] else None,
                ds.reshape(scales.shape) if need[3] else None)


def spectral_mixture_matrix_task(z: torch.Tensor, weights: torch.Tensor, means: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """`spectral_mixture_matrix` for many small tasks (libdkt_smk.so); a shape outside that library's limits takes `spectral_mixture_matrix`."""
    z = _req(z, "z", 3)
    if not smk_task_supported(z.shape[1], z.shape[1], z.shape[2], weights.numel(), True):
        return spectral_mixture_matrix(z, weights, means, scales)
    return _SpectralMixtureTaskFn.apply(z, weights, means, scales)


def smk_any(x1: torch.Tensor, x2: Optional[torch.Tensor], weights: torch.Tensor, means: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Forward only: `smk_task` where its limits allow, else the product library's `smk`."""
    m, d = x1.shape[1], x1.shape[2]
    n = m if x2 is None else x2.shape[1]
    if smk_task_supported(m, n, d, weights.numel(), x2 is None):
        return smk_task(x1, x2, weights, means, scales)
    return smk(x1, x2, weights, means, scales)[0]


CLASSMAP_RBF, CLASSMAP_MATERN25, CLASSMAP_POLY = 0, 1, 2


# Laplace-approximation GP classification: mode finding and prediction (libdkt_gpc.so, include/dkt_abi_gpc.h) have no autograd; training goes through
# `laplace_objective` below (dkt_laplace_grad_f32 of the product library: the gradient of the approximate log marginal likelihood at the mode)
def laplace_supported(n: int, c: int) -> bool:
    """Whether dkt_gpc_mode_f32 / dkt_gpc_predict_f32 take N support rows and C binary problems per episode."""
    return 1 <= n <= _lib.GPC_MAX_N and 1 <= c <= _lib.GPC_MAX_C


def laplace_mode(K: torch.Tensor, Y: torch.Tensor, max_iter: int = 100) -> dict:
    """Posterior modes of B x C binary Laplace GPC problems in ONE launch (scikit-learn's `_posterior_mode`, the Newton loop inside the kernel).
    K: [B,N,N] (shared by the C problems of an episode) or [B,C,N,N]; Y: targets in {0,1}, [C,N] (every episode) or [B,C,N].
    Returns dict(f [B,C,N], g = y - pi [B,C,N], w_sr = W^1/2 [B,C,N], chol = L [B,C,N,N], lml [B,C], iters [B,C] int32): g, w_sr, chol are those of
    the last executed iteration and S = W^1/2 B^-1 W^1/2 = (L^-1 diag(w_sr))^T (L^-1 diag(w_sr)); `laplace_predict` solves with L instead of forming S."""
    pr = _problem("laplace_mode", Y, base=K, base_name="K", y_name="Y")
    b_, c_, n, dev = pr.b, pr.c, pr.n, pr.dev
    out = dict(f=_f32(dev, b_, c_, n), g=_f32(dev, b_, c_, n), w_sr=_f32(dev, b_, c_, n), chol=_f32(dev, b_, c_, n, n), lml=_f32(dev, b_, c_),
               iters=_i32(dev, b_, c_))
    with _timed("dkt_gpc_mode_f32"):
        st = _lib.load_gpc().dkt_gpc_mode_f32(_p(pr.base), *pr.base_strides, _p(pr.y), pr.y_bstride,
                                              _p(out["f"]), _p(out["g"]), _p(out["w_sr"]), _p(out["chol"]), _p(out["lml"]), _p(out["iters"]),
                                              b_, c_, n, int(max_iter), _stream())
    _lib.check(st, "dkt_gpc_mode_f32")
    return out


def laplace_predict(Ks: torch.Tensor, kss: torch.Tensor, mode: dict):
    """Latent mean and variance, class probability and one-vs-rest label at M query points, ONE launch (scikit-learn's binary `predict_proba` per
    class and `OneVsRestClassifier.predict`).  Ks: cross kernel [B,M,N] or [B,C,M,N]; kss: prior variance of the queries [B,M] or [B,C,M]; mode: of
    `laplace_mode`.  Returns (mu, var, prob [B,C,M], labels [B,M] int32: the LAST of several equal maxima of prob; C == 1: mu > 0)."""
    Ks, kss = _req(Ks, "Ks"), _req(kss, "kss")
    g, w_sr, chol = _req(mode["g"], "mode['g']", 3), _req(mode["w_sr"], "mode['w_sr']", 3), _req(mode["chol"], "mode['chol']", 4)
    b_, c_, n = g.shape
    m = Ks.shape[-2] if Ks.dim() in (3, 4) else -1
    if (tuple(Ks.shape) not in ((b_, m, n), (b_, c_, m, n)) or tuple(kss.shape) not in ((b_, m), (b_, c_, m))
            or tuple(w_sr.shape) != (b_, c_, n) or tuple(chol.shape) != (b_, c_, n, n)):
        raise RuntimeError("laplace_predict: Ks %s / kss %s do not fit a mode of B=%d, C=%d, N=%d" % (tuple(Ks.shape), tuple(kss.shape), b_, c_, n))
    dev = Ks.device
    mu, var, prob, labels = _f32(dev, b_, c_, m), _f32(dev, b_, c_, m), _f32(dev, b_, c_, m), _i32(dev, b_, m)
    with _timed("dkt_gpc_predict_f32"):
        st = _lib.load_gpc().dkt_gpc_predict_f32(_p(Ks), *_class_strides(Ks, c_), _p(kss), *_class_strides(kss, c_, 1), _p(g), _p(w_sr), _p(chol),
                                                 _p(mu), _p(var), _p(prob), _p(labels), b_, c_, m, n, _stream())
    _lib.check(st, "dkt_gpc_predict_f32")
    return mu, var, prob, labels


def laplace_grad(K: torch.Tensor, Y: torch.Tensor, f_hat: torch.Tensor, cls_weight: Optional[torch.Tensor], scale: Optional[torch.Tensor] = None):
    """Laplace log marginal likelihood at the mode f_hat and its gradient (dkt_laplace_grad_f32; docs/LAPLACE.md "Training").  K: [B,N,N] (shared by the
    C problems of an episode) or [B,C,N,N]; the covariance of problem (b, c) is scale[c] * K; Y in {0,1}: [C,N] or [B,C,N]; f_hat [B,C,N] of
    `laplace_mode` on those covariances.  Returns (lml [B,C] unweighted, dK = cls_weight_c scale_c d lml / d K_c -- [B,C,N,N], or [B,N,N] summed over the
    classes for a shared K --, dscale [B,C] = cls_weight_c <d lml / d K_c, K>)."""
    pr = _problem("laplace_grad", Y, base=K, base_name="K", y_name="Y", cls_weight=cls_weight, scale=scale)
    (cw, sc), b_, c_, n, dev = pr.hypers, pr.b, pr.c, pr.n, pr.dev
    f_hat = _req(f_hat, "f_hat", 3)
    if tuple(f_hat.shape) != (b_, c_, n):
        raise RuntimeError("laplace_grad: f_hat must be [B,C,N] = %s of K and Y, got %s" % ((b_, c_, n), tuple(f_hat.shape)))
    lml, dscale, dk = _f32(dev, b_, c_), _f32(dev, b_, c_), _f32(dev, *pr.base.shape)
    lib = _lib_now()
    ws_bytes = 0 if pr.per_class else int(lib.dkt_laplace_grad_workspace_bytes(b_, c_, n))
    ws = _workspace(ws_bytes, dev)
    with _timed("dkt_laplace_grad_f32"):
        st = lib.dkt_laplace_grad_f32(_p(pr.base), *pr.base_strides, _p(sc), _p(pr.y), pr.y_bstride,
                                      _p(f_hat), _p(cw), _p(lml), _p(dk), _p(dscale), b_, c_, n, _p(ws), ws_bytes, _stream())
    _lib.check(st, "dkt_laplace_grad_f32")
    return lml, dk, dscale


def _laplace_forward(K, Y, cls_weight, scale, max_iter):
    """mode (no autograd) -> lml and its gradient at the mode -> obj[b] = sum_c cls_weight[c] lml[b,c].  No read-back."""
    with torch.no_grad():
        if scale is None:
            kc = K
        else:                                 # dkt_gpc_mode_f32 takes the covariances themselves: a transient [B,C,N,N] (dkt_laplace_grad_f32 reads K and scale)
            kc = (K if K.dim() == 4 else K.unsqueeze(1)) * scale.reshape(1, -1, 1, 1)
        md = laplace_mode(kc, Y, max_iter)
        lml, dk, dscale = laplace_grad(K, Y, md["f"], cls_weight, scale)
        return objective(lml, cls_weight), lml, md["iters"], dk, dscale


# Dirichlet classification likelihood (Milios et al. 2018; docs/DIRICHLET.md): class labels as Gaussian targets with a fixed noise per row, exact inference
def dirichlet_targets(y_pm1: torch.Tensor, alpha_eps: float = 0.01):
    """+-1 one-vs-rest labels -> (ytilde, noise_rows) of the same shape: a = alpha_eps + [y > 0], noise_rows = log(1 / a + 1), ytilde = log a - noise_rows / 2
    (the log-normal match of the Gamma marginals of a Dirichlet: 0.688184, -0.334142 on the positive class and 4.615121, -6.912731 elsewhere at 0.01)."""
    a = float(alpha_eps) + (y_pm1 > 0).to(torch.float32)
    noise_rows = torch.log(1.0 / a + 1.0)
    return (torch.log(a) - 0.5 * noise_rows).contiguous(), noise_rows.contiguous()


def mll_rownoise(e: torch.Tensor, y: torch.Tensor, noise_rows: torch.Tensor, sv: torch.Tensor, mean: torch.Tensor, want_grad: bool = False,
                 want_chol: bool = False, cls_weight: Optional[torch.Tensor] = None) -> dict:
    """Exact-GP marginal log likelihood with a noise per ROW, K_c = sv_c E + diag(noise_rows_c) (dkt_mll_rownoise_f32; N <= 127, C <= 32, no jitter ladder).
    e: [B,N,N] (shared by the class models) or [B,C,N,N]; y, noise_rows: [C,N] (every episode) or [B,C,N]; sv, mean: C elements.
    Returns dict(logp [B,C] unweighted, alpha [B,C,N], info [B,C] int32, chol [B,C,N,N] | None, and with want_grad de = cls_weight_c sv_c G_c ([B,C,N,N], or
    [B,N,N] summed over the classes for a shared e), dsv = cls_weight_c <G_c, e>, dmean = cls_weight_c sum alpha [B,C]), G = d logp / d K."""
    pr = _problem("mll_rownoise", y, base=e, noise_rows=noise_rows, sv=sv, mean=mean, cls_weight=cls_weight)
    (sv, mean, cw), b_, c_, n, dev = pr.hypers, pr.b, pr.c, pr.n, pr.dev
    logp, alpha, info = _f32(dev, b_, c_), _f32(dev, b_, c_, n), _i32(dev, b_, c_)
    flags = (MLL_WANT_GRAD if want_grad else 0) | (MLL_WANT_CHOL if want_chol else 0)
    chol = _f32(dev, b_, c_, n, n) if want_chol else None
    de = dsv = dmean = None
    ws_bytes = 0
    lib = _lib_now()
    if want_grad:
        de, dsv, dmean = _f32(dev, *pr.base.shape), _f32(dev, b_, c_), _f32(dev, b_, c_)
        if not pr.per_class:
            ws_bytes = int(lib.dkt_mll_rownoise_workspace_bytes(b_, c_, n))
    ws = _workspace(ws_bytes, dev)
    with _timed("dkt_mll_rownoise_f32"):
        st = lib.dkt_mll_rownoise_f32(_p(pr.base), *pr.base_strides, _p(pr.y), pr.y_bstride, _p(pr.noise_rows), pr.nr_bstride, _p(sv), _p(mean), _p(cw),
                                      _p(logp), _p(alpha), _p(de), _p(dsv), _p(dmean), _p(chol), _p(info), b_, c_, n, flags, _p(ws), ws_bytes, _stream())
    _lib.check(st, "dkt_mll_rownoise_f32")
    return dict(logp=logp, alpha=alpha, info=info, chol=chol, de=de, dsv=dsv, dmean=dmean)


# Leave-one-out predictive log likelihood (GPML 5.4.2; libdkt_loo.so, include/dkt_abi_loo.h; docs/LOO.md): the second objective of a Gaussian likelihood
LOO_WANT_GRAD = 1


def loo_supported(n: int, c: int) -> bool:
    """Whether dkt_loo_f32 takes N rows and C class models per episode."""
    return 1 <= n <= _lib.LOO_MAX_N and 1 <= c <= _lib.LOO_MAX_C


def _loo_outputs(pr: _Problem):
    """loo [B,C], alpha, mu_loo, var_loo [B,C,N], jitter [B,C], info [B,C] int32 of `loo` / `loo_lowrank`."""
    b_, c_, n, dev = pr.b, pr.c, pr.n, pr.dev
    return _f32(dev, b_, c_), _f32(dev, b_, c_, n), _f32(dev, b_, c_, n), _f32(dev, b_, c_, n), _f32(dev, b_, c_), _i32(dev, b_, c_)


def loo(e: torch.Tensor, y: torch.Tensor, sv: torch.Tensor, mean: torch.Tensor, noise: torch.Tensor, want_grad: bool = False,
        cls_weight: Optional[torch.Tensor] = None, jitter0: float = 1e-6, max_tries: int = 3) -> dict:
    """Leave-one-out predictive log likelihood of C exact-GP models per episode, K_c = sv_c E + noise_c I (dkt_loo_f32: ONE launch, the jitter ladder of
    `mll` inside the kernel; N <= 127, C <= 32).  e: [B,N,N] (shared by the class models) or [B,C,N,N]; y: [C,N] (every episode) or [B,C,N]; sv, mean, noise:
    C elements.  Returns dict(loo [B,C] unweighted, alpha, mu_loo, var_loo [B,C,N] -- the leave-one-out predictive mean and variance of every row --,
    jitter [B,C], info [B,C] int32 (0 = ok; otherwise every output of that problem is NaN), and with want_grad w = cls_weight_c sv_c d loo / d K_c
    ([B,C,N,N], or [B,N,N] summed over the classes for a shared e), dsv, dmean, dnoise [B,C] raw, as `mll` reports its own)."""
    pr = _problem("loo", y, base=e, sv=sv, mean=mean, noise=noise, cls_weight=cls_weight)
    (sv, mean, noise, cw), b_, c_, dev = pr.hypers, pr.b, pr.c, pr.dev
    val, alpha, mu, var, jit, info = _loo_outputs(pr)
    w = dsv = dmean = dnoise = None
    if want_grad:
        w, dsv, dmean, dnoise = _f32(dev, *pr.base.shape), _f32(dev, b_, c_), _f32(dev, b_, c_), _f32(dev, b_, c_)
    with _timed("dkt_loo_f32"):
        st = _lib.load_loo().dkt_loo_f32(_p(pr.base), *pr.base_strides, _p(pr.y), pr.y_bstride, _p(sv), _p(mean), _p(noise), _p(cw),
                                         b_, c_, pr.n, float(jitter0), int(max_tries), LOO_WANT_GRAD if want_grad else 0, _p(val), _p(alpha),
                                         _p(mu), _p(var), _p(w), _p(dsv), _p(dmean), _p(dnoise), _p(jit), _p(info), _stream())
    _lib.check(st, "dkt_loo_f32")
    return dict(loo=val, alpha=alpha, mu_loo=mu, var_loo=var, w=w, dsv=dsv, dmean=dmean, dnoise=dnoise, jitter=jit, info=info)


# ---- the leave-one-out likelihood in feature space (libdkt_loofs.so, include/dkt_abi_loofs.h; docs/LOOFS.md) ----
def loo_lowrank_supported(n: int, d: int, c: int) -> bool:
    """Shapes dkt_loofs_f32 takes: K_c = sv_c Z Z^T + noise_c I with D <= 64, D % 4 == 0, C <= 32, any number of rows (the limits of rownoise_lowrank_supported)."""
    return n >= 1 and 1 <= d <= _lib.LOOFS_MAX_D and d % 4 == 0 and 1 <= c <= _lib.LOOFS_MAX_C


def loo_lowrank_applies(n: int, d: int, c: int, on_gpu: bool = True) -> bool:
    """Does a leave-one-out episode of the linear kernels run in feature space?  DKT_LOO_LOWRANK: 1 (default) = episodes of more than FUSED_EP_MAX_N = 128 rows, the
    line `lowrank_applies` draws for the marginal likelihood (an episode of exactly 128 rows has no route: the resident kernel stops at 127; docs/LOOFS.md);
    0 = never; force = wherever the shape is supported (tests: against the resident kernel below 128 rows).  Only for rows on the GPU."""
    mode = os.environ.get("DKT_LOO_LOWRANK", "1")
    if mode == "0" or not on_gpu or not loo_lowrank_supported(n, d, c):
        return False
    return mode == "force" or n > FUSED_EP_MAX_N


def loo_lowrank(z: torch.Tensor, y: torch.Tensor, sv: torch.Tensor, mean: torch.Tensor, noise: torch.Tensor, want_grad: bool = False,
                cls_weight: Optional[torch.Tensor] = None, jitter0: float = 1e-6, max_tries: int = 3) -> dict:
    """`loo` for the linear kernels on the rows themselves, K_c = sv_c Z Z^T + noise_c I (dkt_loofs_f32: ONE launch, the jitter ladder inside the kernel on the
    D x D matrix Z^T Z + (noise_c + jitter) / sv_c I; D <= 64, any N: no N x N matrix exists).  z: [B,N,D]; y: [C,N] (every episode) or [B,C,N]; sv, mean, noise:
    C elements.  Returns the dict of `loo` with dz [B,N,D] = sum_c cls_weight_c d loo_c / d Z in the place of w (None without want_grad, like dsv, dmean, dnoise)."""
    pr = _problem("loo_lowrank", y, rows=z, sv=sv, mean=mean, noise=noise, cls_weight=cls_weight)
    z, (sv, mean, noise, cw), b_, c_, n, d, dev = pr.rows, pr.hypers, pr.b, pr.c, pr.n, pr.d, pr.dev
    val, alpha, mu, var, jit, info = _loo_outputs(pr)
    dz = dsv = dmean = dnoise = None
    if want_grad:
        dz = torch.empty_like(z)
        dsv, dmean, dnoise = _f32(dev, b_, c_), _f32(dev, b_, c_), _f32(dev, b_, c_)
    lib = _lib.load_loofs()
    ws_bytes = int(lib.dkt_loofs_workspace_bytes(b_, c_, n, d))
    ws = _workspace(ws_bytes, dev)
    with _timed("dkt_loofs_f32"):
        st = lib.dkt_loofs_f32(_p(z), _p(pr.y), pr.y_bstride, _p(sv), _p(mean), _p(noise), _p(cw), b_, c_, n, d, float(jitter0), int(max_tries),
                               LOO_WANT_GRAD if want_grad else 0, _p(val), _p(alpha), _p(mu), _p(var), _p(dz), _p(dsv), _p(dmean), _p(dnoise), _p(jit), _p(info),
                               _p(ws), ws_bytes, _stream())
    _lib.check(st, "dkt_loofs_f32")
    return dict(loo=val, alpha=alpha, mu_loo=mu, var_loo=var, dz=dz, dsv=dsv, dmean=dmean, dnoise=dnoise, jitter=jit, info=info)


# The joint posterior at test time (GPML 2.2; libdkt_post.so, include/dkt_abi_post.h; docs/POSTERIOR.md): full covariance, test likelihood, function draws
def posterior_supported(n: int, m: int, c: int) -> bool:
    """Whether dkt_posterior_f32 takes N support rows, M query rows and C models per episode."""
    return 1 <= n <= _lib.POST_MAX_N and 1 <= m <= _lib.POST_MAX_M and 1 <= c <= _lib.POST_MAX_C


def posterior(e_ss: torch.Tensor, e_qs: torch.Tensor, e_qq: torch.Tensor, y: torch.Tensor, sv: torch.Tensor, mean: torch.Tensor, noise: torch.Tensor,
              yq: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None, with_noise: bool = True, want_cov: bool = True, want_chol: bool = False,
              jitter0: float = 1e-6, max_tries: int = 3) -> dict:
    """The joint posterior of C exact-GP models per episode at M query rows, K_c = sv_c E_ss + noise_c I (dkt_posterior_f32: ONE launch, the jitter ladder of
    `mll` inside the kernel for K and for Sigma apart; N, M <= 127, C <= 32).  e_ss: [B,N,N], e_qs: [B,M,N] (query against support), e_qq: [B,M,M] -- each shared
    by the class models, or with a class axis [B,C,...]; y: [C,N] (every episode) or [B,C,N]; sv, mean, noise: C elements; yq: [B,C,M] held-out targets or None;
    eps: [B,C,S,M] standard normals or None; with_noise: the predictive covariance of observations (+ noise I) or of the latent function.
    Returns dict(mu [B,C,M], cov [B,C,M,M] (None unless want_cov; bitwise symmetric), chol [B,C,M,M] lower factor of cov + jitter_q I (None unless want_chol),
    logp, lpd [B,C] the joint and the marginal log predictive density of yq (None without yq), samples [B,C,S,M] = mu + chol eps (None without eps),
    jitter_s, jitter_q [B,C], info_s, info_q [B,C] int32: info_s != 0 -- every output of that problem is NaN; info_q != 0 -- chol, logp and samples are)."""
    shapes = [tuple(t.shape) if isinstance(t, torch.Tensor) else None for t in (e_ss, e_qs, e_qq, y)]
    if None in shapes or len(shapes[0]) not in (3, 4) or len(shapes[1]) not in (3, 4) or len(shapes[2]) not in (3, 4) or len(shapes[3]) not in (2, 3):
        raise RuntimeError("posterior: e_ss, e_qs, e_qq must be [B,(C,)N,N], [B,(C,)M,N], [B,(C,)M,M] and y [C,N] or [B,C,N], got %s" % (shapes,))
    b_, n, m, c_ = shapes[0][0], shapes[0][-1], shapes[1][-2], shapes[3][-2]
    ok = shapes[0][-2] == n and shapes[1][-1] == n and shapes[2][-2:] == (m, m) and shapes[3][-1] == n
    ok = ok and all(s[0] == b_ and (len(s) == 3 or s[1] == c_) for s in shapes[:3]) and (len(shapes[3]) == 2 or shapes[3][0] == b_)
    ok = ok and (yq is None or tuple(yq.shape) == (b_, c_, m)) and (eps is None or (eps.dim() == 4 and tuple(eps.shape[:2]) + (eps.shape[3],) == (b_, c_, m)))
    ok = ok and all(isinstance(t, torch.Tensor) and t.numel() == c_ for t in (sv, mean, noise))
    if not ok:
        raise RuntimeError("posterior: inconsistent shapes: e_ss %s, e_qs %s, e_qq %s, y %s, yq %s, eps %s, sv / mean / noise of %s elements" % (
            shapes[0], shapes[1], shapes[2], shapes[3], None if yq is None else tuple(yq.shape), None if eps is None else tuple(eps.shape),
            [t.numel() if isinstance(t, torch.Tensor) else None for t in (sv, mean, noise)]))
    if not posterior_supported(n, m, c_):
        raise RuntimeError("posterior: N = %d support rows, M = %d query rows, C = %d models: dkt_posterior_f32 serves 1 <= N <= %d, 1 <= M <= %d, 1 <= C <= %d"
                           % (n, m, c_, _lib.POST_MAX_N, _lib.POST_MAX_M, _lib.POST_MAX_C))
    pr = _problem("posterior", y, base=e_ss, base_name="e_ss", sv=sv, mean=mean, noise=noise)       # (the shapes are settled above, before any tensor is refused)
    e_qs, e_qq, (sv, mean, noise), dev = _req(e_qs, "e_qs"), _req(e_qq, "e_qq"), pr.hypers, pr.dev
    yq = None if yq is None else _req(yq, "yq", 3)
    s_ = 0 if eps is None else eps.shape[2]
    eps = None if s_ == 0 else _req(eps, "eps", 4)
    mu = _f32(dev, b_, c_, m)
    cov = _f32(dev, b_, c_, m, m) if want_cov else None
    chol = _f32(dev, b_, c_, m, m) if want_chol else None
    logp, lpd = (_f32(dev, b_, c_), _f32(dev, b_, c_)) if yq is not None else (None, None)
    samples = _f32(dev, b_, c_, s_, m) if s_ else None
    jit_s, jit_q, info_s, info_q = _f32(dev, b_, c_), _f32(dev, b_, c_), _i32(dev, b_, c_), _i32(dev, b_, c_)
    lib = _lib.load_post()
    ws_bytes = int(lib.dkt_posterior_workspace_bytes(b_, c_, m, 1 if want_cov else 0))
    ws = _workspace(ws_bytes, dev)
    with _timed("dkt_posterior_f32"):
        st = lib.dkt_posterior_f32(_p(pr.base), *pr.base_strides, _p(e_qs), *_class_strides(e_qs, c_), _p(e_qq), *_class_strides(e_qq, c_), _p(pr.y),
                                   pr.y_bstride, _p(sv), _p(mean), _p(noise), _p(yq), _p(eps), b_, c_, n, m, s_, 1 if with_noise else 0,
                                   float(jitter0), int(max_tries), _p(mu), _p(cov), _p(chol), _p(logp), _p(lpd), _p(samples), _p(jit_s), _p(jit_q),
                                   _p(info_s), _p(info_q), _p(ws), ws_bytes, _stream())
    _lib.check(st, "dkt_posterior_f32")
    return dict(mu=mu, cov=cov, chol=chol, logp=logp, lpd=lpd, samples=samples, jitter_s=jit_s, jitter_q=jit_q, info_s=info_s, info_q=info_q)


def dirichlet_proba(mu: torch.Tensor, var: torch.Tensor, eps: torch.Tensor):
    """prob[b,q,c] = mean_s softmax_c(mu[b,c,q] + sqrt(max(var[b,c,q], 0)) eps[s,c]) (dkt_dirichlet_proba_f32): mu, var [B,C,M] the latent posterior of
    `predict` / `predict_var` (zero noise), eps [S,C] the caller's standard normals, shared by every query (common random numbers).
    Returns (prob [B,M,C], labels [B,M] int32 = argmax_c mu, the first maximum)."""
    mu = _req(mu, "mu", 3)
    var = _req(var, "var", 3)
    eps = _req(eps, "eps", 2)
    b_, c_, m = mu.shape
    if tuple(var.shape) != (b_, c_, m) or eps.shape[1] != c_ or eps.shape[0] < 1:
        raise RuntimeError("dirichlet_proba: var must be %s like mu and eps [S,C=%d], got %s and %s" % (tuple(mu.shape), c_, tuple(var.shape), tuple(eps.shape)))
    prob = torch.empty((b_, m, c_), device=mu.device, dtype=torch.float32)
    labels = torch.empty((b_, m), device=mu.device, dtype=torch.int32)
    with _timed("dkt_dirichlet_proba_f32"):
        st = _lib_now().dkt_dirichlet_proba_f32(_p(mu), _p(var), _p(eps), _p(prob), _p(labels), b_, c_, m, eps.shape[0], _stream())
    _lib.check(st, "dkt_dirichlet_proba_f32")
    return prob, labels


def _classmap_of(kernel: str, lengthscale, offset):
    """(map id, power, parameter [C], base-matrix kind) of a kernel whose class models own their base-kernel parameter."""
    if kernel in POLY_KINDS:
        return CLASSMAP_POLY, POLY_KINDS[kernel], offset, KERNEL_LINEAR
    if kernel in MATERN_KINDS:
        return CLASSMAP_MATERN25, 0, lengthscale, KERNEL_SQDIST
    if kernel in RBF_KINDS:
        return CLASSMAP_RBF, 0, lengthscale, KERNEL_SQDIST
    raise ValueError("[ERROR] the kernel '" + str(kernel) + "' has no per-class base-kernel parameter")


def class_kernel(base: torch.Tensor, cmap: int, power: int, param: torch.Tensor) -> torch.Tensor:
    """E[B,C,...] = f(base[B,...]; param[c]) -- the C class kernels of an episode from its ONE contraction (dkt_class_kernel_f32)."""
    base = _req(base, "base")
    param = _req(param.reshape(-1), "param", 1)
    b_, c = base.shape[0], param.numel()
    nn = base[0].numel()
    e = torch.empty((b_, c) + tuple(base.shape[1:]), device=base.device, dtype=torch.float32)
    lib = _lib_now()
    with _timed("dkt_class_kernel_f32"):
        st = lib.dkt_class_kernel_f32(_p(base), int(cmap), _p(param), int(power), _p(e), b_, c, nn, _stream())
    _lib.check(st, "dkt_class_kernel_f32")
    return e


def class_kernel_bwd(w: torch.Tensor, base: torch.Tensor, cmap: int, power: int, param: torch.Tensor):
    """Chain rule behind the per-class marginal-likelihood launch: w [B,C,N,N] = d obj / d E (symmetric per matrix) -> (Wp [B,N,N] for
    gram_bwd, dparam [B,C])."""
    w = _req(w, "w", 4)
    base = _req(base, "base", 3)
    param = _req(param.reshape(-1), "param", 1)
    b_, c, n, _ = w.shape
    if tuple(w.shape) != (b_, c, n, n) or tuple(base.shape) != (b_, n, n) or param.numel() != c:          # (a w of fewer columns would be read past its end)
        raise RuntimeError("class_kernel_bwd: w must be [B,C,N,N], base [B,N,N] and param [C]")
    wp = torch.empty_like(base)
    lib = _lib_now()
    nsplit = int(lib.dkt_class_kernel_bwd_nsplit(b_, n))
    dparam = torch.empty((b_, nsplit, c), device=w.device, dtype=torch.float32)
    with _timed("dkt_class_kernel_bwd_f32"):
        st = lib.dkt_class_kernel_bwd_f32(_p(w), _p(base), int(cmap), _p(param), int(power), _p(wp), _p(dparam), b_, c, n, _stream())
    _lib.check(st, "dkt_class_kernel_bwd_f32")
    return wp, (dparam[:, 0] if nsplit == 1 else dparam.sum(1))


def mll_per_class_supported(n: int, c: int) -> bool:
    """Sizes the one-launch per-class path serves: dkt_mll_f32 with DKT_MLL_E_PER_CLASS takes every N in one call (N <= 127 one wave per matrix,
    128 <= N <= 447 the tile-array pipeline; both with the jitter ladder); beyond N = 447 its one-launch kernel is the generic one, and the host
    prefers one single-model call per class there (the blocked path serves those).  dkt_class_kernel_bwd_f32: C <= 32."""
    return c <= 32 and n + 1 <= 448


def base_matrix_per_class(z: torch.Tensor, kernel: str, lengthscale: Optional[torch.Tensor] = None,
                          offset: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable E[B,C,N,N] for the kernels whose class models own their base-kernel parameter (one ExactGPLayer per class,
    reference DKT.py:63-66, 352-365): rbf / matern (lengthscale [C]), poli1 / poli2 (offset [C]).  The O(N^2 D) contraction -- the
    squared distances or the Gram -- is built ONCE per episode (dkt_gram_f32); the per-class map is element-wise."""
    one = torch.ones(1, device=z.device, dtype=torch.float32)
    if kernel in POLY_KINDS:
        g = _BaseMatrixFn.apply(z, torch.zeros(1, device=z.device, dtype=torch.float32), KERNEL_LINEAR)
        return (g.unsqueeze(1) + offset.reshape(1, -1, 1, 1)) ** POLY_KINDS[kernel]
    u = _SqDistFn.apply(z, one).unsqueeze(1) / (lengthscale.reshape(1, -1, 1, 1) ** 2)         # |z_i - z_j|^2 / l_c^2
    if kernel in MATERN_KINDS:
        return _matern25(u)
    if kernel in RBF_KINDS:
        return torch.exp(-0.5 * u)
    raise ValueError("[ERROR] the kernel '" + str(kernel) + "' has no per-class base-kernel parameter")


def kernel_matrix_per_class(a: torch.Tensor, bm: Optional[torch.Tensor], kernel: str, lengthscale: Optional[torch.Tensor] = None,
                            offset: Optional[torch.Tensor] = None) -> torch.Tensor:
    """k_c(a, bm) for every class model, [B,C,M,N] (no autograd): one contraction (dkt_gram_f32), the C class maps in one launch
    (dkt_class_kernel_f32)."""
    cmap, power, param, base_kind = _classmap_of(kernel, lengthscale, offset)
    one = torch.ones(1, device=a.device, dtype=torch.float32)
    return class_kernel(gram(a, bm, base_kind, one if base_kind == KERNEL_SQDIST else None), cmap, power, param.detach())


def base_matrix(z: torch.Tensor, kernel: str = "bncossim", lengthscale: Optional[torch.Tensor] = None,
                offset: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable symmetric base kernel matrix E[B,N,N] of z[B,N,D] for every kernel type of the reference's
    ExactGPLayer (DKT.py:352-370): linear / cossim / bncossim, rbf, matern (nu = 2.5), poli1, poli2."""
    if kernel in MATERN_KINDS:
        return _matern25(_SqDistFn.apply(z, lengthscale))
    if kernel in POLY_KINDS:
        g = _BaseMatrixFn.apply(z, torch.zeros(1, device=z.device, dtype=torch.float32), KERNEL_LINEAR)
        return (g + offset.reshape(())) ** POLY_KINDS[kernel]
    kind = kind_id(kernel)
    if kind == KERNEL_RBF and lengthscale is None:
        raise RuntimeError("rbf needs a lengthscale tensor")
    if lengthscale is None:
        lengthscale = torch.zeros(1, device=z.device, dtype=torch.float32)
    return _BaseMatrixFn.apply(z, lengthscale, kind)


def objective(logp: torch.Tensor, cls_weight: Optional[torch.Tensor]) -> torch.Tensor:
    """obj[b] = sum_c cls_weight[c] logp[b,c] (dkt_objective_f32: one launch, fixed order) -- the sum over the class models of SumMarginalLogLikelihood (DKT.py:70-71, 161)."""
    if os.environ.get("DKT_FUSED_REDUCTIONS", "1") == "0":                 # the tensor expressions (their twin; three launches)
        return logp.sum(1) if cls_weight is None else (logp * cls_weight.reshape(1, -1)).sum(1)
    logp = _req(logp, "logp", 2)
    b_, c_ = logp.shape
    cw = None if cls_weight is None else _req(cls_weight.reshape(-1), "cls_weight", 1)
    obj = torch.empty((b_,), device=logp.device, dtype=torch.float32)
    with _timed("dkt_objective_f32"):
        _lib.check(_lib_now().dkt_objective_f32(_p(logp), _p(cw), _p(obj), b_, c_, _stream()), "dkt_objective_f32")
    return obj


def hyper_grads(gobj: torch.Tensor, cls_weight: Optional[torch.Tensor], dsv, dmean, dnoise, shapes):
    """(g_sv, g_mean, g_noise)[c] = cls_weight[c] sum_b gobj[b] d_x[b,c] for the d_x that are not None (dkt_hyper_grads_f32: ONE launch, fixed summation order),
    reshaped to `shapes`; None where d_x is None."""
    if os.environ.get("DKT_FUSED_REDUCTIONS", "1") == "0":                 # the tensor expressions (their twin; a multiply + two launches per parameter)
        gw = gobj.reshape(-1, 1) * (1.0 if cls_weight is None else cls_weight.reshape(1, -1))
        return tuple(None if d is None else (gw * d).sum(0).reshape(sh) for d, sh in zip((dsv, dmean, dnoise), shapes))
    gobj = _req(gobj.reshape(-1), "gobj", 1)
    ds = [None if d is None else _req(d, "d", 2) for d in (dsv, dmean, dnoise)]
    if all(d is None for d in ds):
        return None, None, None
    b_, c_ = next(d for d in ds if d is not None).shape
    cw = None if cls_weight is None else _req(cls_weight.reshape(-1), "cls_weight", 1)
    gs = [None if d is None else torch.empty((c_,), device=gobj.device, dtype=torch.float32) for d in ds]
    with _timed("dkt_hyper_grads_f32"):
        _lib.check(_lib_now().dkt_hyper_grads_f32(_p(gobj), _p(cw), _p(ds[0]), _p(ds[1]), _p(ds[2]), _p(gs[0]), _p(gs[1]), _p(gs[2]), b_, c_, _stream()), "dkt_hyper_grads_f32")
    return tuple(None if g is None else g.reshape(sh) for g, sh in zip(gs, shapes))


# ------------------------------------------------------------------------------------------------------
# Linear kernels in FEATURE space: D <= 64 < N (Conv4S / Omniglot; include/dkt_abi.h "dkt_lowrank_*", csrc/dkt_lowrank.hip)
# ------------------------------------------------------------------------------------------------------
FUSED_EP_MAX_N = 128          # the episode-resident fused kernels of dkt_frontend.hip (Zn never written); above it: dkt_frontend_big.hip
LOWRANK_DP = 64               # DKT_LOWRANK_DP
LOWRANK_MIN_N = 80            # below it the D x D problem (5 x 5 tiles) is no smaller than the N x N one
LOWRANK_MIN_B = 3072          # episodes of N <= 128 rows: batches from which the feature-space step wins (below, both steps are bound by their launches, and it has 5 to the N x N step's 3:
                              # tools/lowrank_small_batch_probe.py -- 0.35 vs 0.31 ms up to 1024 episodes of 105 rows; 0.69 vs 1.03 ms at 8192)


def lowrank_supported(n: int, d: int, c: int) -> bool:
    """Shapes the feature-space calls (dkt_lowrank_*) serve and are meant for: K_c = sv_c Z Z^T + noise_c I with D <= 64, D % 4 == 0, C <= 32 and an episode of at
    least 80 rows (the Omniglot / Conv4S episodes: D = 64, N = 105 or 420)."""
    return d <= LOWRANK_DP and d % 4 == 0 and c <= 32 and n >= LOWRANK_MIN_N


def lowrank_applies(n: int, d: int, c: int, b: int = LOWRANK_MIN_B, front_end: bool = False) -> bool:
    """Does this call take the feature-space episode?  DKT_LOWRANK: 1 (default) = where it wins -- every batch of episodes with more than 128 rows (one 420-row episode:
    0.35 instead of 1.2 ms, 1024 of them: 0.49 instead of 16.9 ms), and for N <= 128 from LOWRANK_MIN_B episodes per call (never behind the fused bn_out front end, whose
    episode-resident kernels for N <= 128 are as fast at 8192 episodes and faster below); 0 = never (the N x N kernels: the twin the tests compare); force = wherever the
    shape is supported (tests)."""
    mode = os.environ.get("DKT_LOWRANK", "1")
    if mode == "0" or not lowrank_supported(n, d, c):
        return False
    if mode == "force" or n > FUSED_EP_MAX_N:
        return True
    return (not front_end) and b >= LOWRANK_MIN_B


_lowrank_zeros = {}


def _zeros_cached(c: int, dev) -> torch.Tensor:
    """[C] zeros (the mean of the D x D models), one tensor per (device, C): never written."""
    if torch.cuda.is_current_stream_capturing():          # (a tensor born inside a graph capture lives in the graph's private pool: not cached)
        return torch.zeros(c, device=dev, dtype=torch.float32)
    key = (dev, int(c))
    t = _lowrank_zeros.get(key)
    if t is None:
        t = _lowrank_zeros[key] = torch.zeros(c, device=dev, dtype=torch.float32)
    return t


def _lowrank_forward(z, y, sv, mean, noise, cls_weight, jitter0, max_tries, unit_rows) -> dict:
    """The forward calls of the feature-space episode (no autograd): noise floor -> A, P -> the D x D models -> alpha, logp, gradients.
    Returns obj, logp, alpha, info, jitter (total), v / t / wd (for the backward), dsv, dmean, dnoise."""
    pr = _problem("episode_loss_linear", y, rows=z, sv=sv, mean=mean, noise=noise, cls_weight=cls_weight)
    z, y, (sv_, mean_, noise_in, cw_) = pr.rows, pr.y, pr.hypers
    b_, c_, n, d, y_bstride, dev = pr.b, pr.c, pr.n, pr.d, pr.y_bstride, pr.dev
    lib = _lib_now()
    # the rung of the jitter ladder that lifts the noise floor of the (rank-deficient) N x N matrix above fp32 rounding -- 0 for any sane noise; rows that
    # went through F.normalize have |z_i|^2 = 1, otherwise one reduction over Z finds the largest diagonal element of Z Z^T.  NOTE: that
    # maximum is taken over the WHOLE call, so for un-normalised `linear` features with a noise below 2^-22 max K_ii one large-norm row raises the rung of every
    # episode of the batch (the N x N path and psd_safe_cholesky decide per matrix).  cossim / bncossim (unit rows) and any noise >= 1e-5 are unaffected; the rung is
    # reported per (episode, class) in `jitter` either way.
    zmax2 = None if unit_rows else z.square().sum(2).amax().reshape(1).contiguous()
    noise_ = torch.empty_like(noise_in)
    pre = torch.empty_like(noise_in)
    _lib.check(lib.dkt_lowrank_noise_floor_f32(_p(sv_), _p(noise_in), _p(zmax2), float(jitter0), int(max_tries), _p(noise_), _p(pre), c_, _stream()),
               "dkt_lowrank_noise_floor_f32")
    a, p = _f32(dev, b_, LOWRANK_DP, LOWRANK_DP), _f32(dev, b_, c_, LOWRANK_DP)
    with _timed("dkt_lowrank_gram_f32"):
        st = lib.dkt_lowrank_gram_f32(_p(z), _p(y), y_bstride, _p(mean_), _p(a), _p(p), b_, c_, n, d, _stream())
    _lib.check(st, "dkt_lowrank_gram_f32")
    # the D x D models.  Unit rows (cossim / bncossim): cond(K') <= 1 + sv lambda_max / noise, and the kappa guard of dkt_mll_f32 prices the trace N instead of
    # lambda_max (N = 420 rows would trip it at sv > 1.2 for a true condition of a few hundred on batch-normalised rows).  Measured without the guard on aligned
    # (non-negative) unit rows, where lambda_max is 0.35 .. 0.83 N: at cond(K_c) = 1.5e3 .. 1.04e4 (N = 420) and 4e2 .. 2.6e3 (N = 105) the worst errors against
    # float64 are logp 2.7e-5 (limit 1e-4), alpha 3.3e-5 (5e-4), dZ 4.1e-5 (1e-3) -- tests/test_lowrank_gpu.py, the table of DESIGN.md 4.6; rows without the
    # promise keep the guard
    out = mll(a, p, sv_, _zeros_cached(c_, dev), noise_, want_grad=True, cls_weight=cw_, jitter0=jitter0, max_tries=max_tries, no_kappa_guard=bool(unit_rows))
    logp, alpha, v = _f32(dev, b_, c_), _f32(dev, b_, c_, n), _f32(dev, b_, c_, n)
    dsv, dmean, dnoise, jit, obj = _f32(dev, b_, c_), _f32(dev, b_, c_), _f32(dev, b_, c_), _f32(dev, b_, c_), _f32(dev, b_)
    with _timed("dkt_lowrank_finish_f32"):
        st = lib.dkt_lowrank_finish_f32(_p(z), _p(y), y_bstride, _p(sv_), _p(mean_), _p(noise_), _p(cw_), _p(out["alpha"]), _p(out["logp"]), _p(out["dnoise"]),
                                        _p(out["jitter"]), _p(pre), _p(jit), _p(obj), _p(logp), _p(alpha), _p(v), _p(dsv), _p(dmean), _p(dnoise), b_, c_, n, d, _stream())
    _lib.check(st, "dkt_lowrank_finish_f32")
    return dict(obj=obj, logp=logp, alpha=alpha, info=out["info"], jitter=jit, v=v, t=out["alpha"], wd=out["w"], dsv=dsv, dmean=dmean, dnoise=dnoise)


def _lowrank_backward(z, v, t, wd, gobj) -> torch.Tensor:
    """dZ[b] = gobj[b] (V^T T + 2 Z W')  (dkt_lowrank_bwd_f32)."""
    b_, n, d = z.shape
    dz = torch.empty_like(z)
    lib = _lib_now()
    with _timed("dkt_lowrank_bwd_f32"):
        st = lib.dkt_lowrank_bwd_f32(_p(z), _p(v), _p(t), _p(wd), _p(_req(gobj.reshape(-1), "gobj", 1)), _p(dz), b_, v.shape[1], n, d, _stream())
    _lib.check(st, "dkt_lowrank_bwd_f32")
    return dz


# ---- the Dirichlet likelihood in feature space (include/dkt_abi.h "dkt_rownoise_lowrank_*", csrc/dkt_mll_rownoise.hip; docs/DIRICHLET.md) ----
ROWNOISE_LOWRANK_STATE = LOWRANK_DP * (LOWRANK_DP + 1)      # floats per (episode, class) of the opaque state: t [DP], B^-1 [DP,DP]


def rownoise_lowrank_supported(n: int, d: int, c: int) -> bool:
    """Shapes the feature-space row-noise calls take: K_c = sv_c Z Z^T + diag(noise_rows_c) with D <= 64, D % 4 == 0, C <= 32, any number of rows."""
    return n >= 1 and 1 <= d <= LOWRANK_DP and d % 4 == 0 and 1 <= c <= _lib.LAPLACE_MAX_C


def rownoise_lowrank_applies(n: int, d: int, c: int, on_gpu: bool = True) -> bool:
    """Does a Dirichlet episode of the linear kernels run in feature space?  DKT_DIRICHLET_LOWRANK: 1 (default) = above the 127 rows of the resident kernel;
    0 = never; force = wherever the shape is supported (tests: against the resident kernel below 128 rows).  Only for rows on the GPU."""
    mode = os.environ.get("DKT_DIRICHLET_LOWRANK", "1")
    if mode == "0" or not on_gpu or not rownoise_lowrank_supported(n, d, c):
        return False
    return mode == "force" or n > _lib.LAPLACE_MAX_N


def rownoise_lowrank(z: torch.Tensor, y: torch.Tensor, noise_rows: torch.Tensor, sv: torch.Tensor, mean: torch.Tensor,
                     cls_weight: Optional[torch.Tensor] = None, want_grad: bool = False) -> dict:
    """`mll_rownoise` for the linear kernels on the rows themselves, K_c = sv_c Z Z^T + diag(noise_rows_c) (dkt_rownoise_lowrank_f32; D <= 64, any N: no
    N x N matrix exists).  z: [B,N,D]; y, noise_rows: [C,N] or [B,C,N]; sv, mean: C elements.
    Returns dict(logp [B,C] unweighted, alpha [B,C,N], info [B,C] int32, state (opaque: what `rownoise_lowrank_bwd` / `rownoise_lowrank_predict` read), and
    with want_grad dsv = cls_weight_c d logp / d sv_c, dmean = cls_weight_c sum alpha [B,C])."""
    pr = _problem("rownoise_lowrank", y, rows=z, noise_rows=noise_rows, sv=sv, mean=mean, cls_weight=cls_weight)
    (sv, mean, cw), b_, c_, n, dev = pr.hypers, pr.b, pr.c, pr.n, pr.dev
    logp, alpha, info, state = _f32(dev, b_, c_), _f32(dev, b_, c_, n), _i32(dev, b_, c_), _f32(dev, b_, c_, ROWNOISE_LOWRANK_STATE)
    dsv = _f32(dev, b_, c_) if want_grad else None
    dmean = _f32(dev, b_, c_) if want_grad else None
    with _timed("dkt_rownoise_lowrank_f32"):
        st = _lib_now().dkt_rownoise_lowrank_f32(_p(pr.rows), _p(pr.y), pr.y_bstride, _p(pr.noise_rows), pr.nr_bstride, _p(sv),
                                                 _p(mean), _p(cw), _p(logp), _p(alpha), _p(info), _p(dsv), _p(dmean), _p(state), state.numel() * 4,
                                                 b_, c_, n, pr.d, _stream())
    _lib.check(st, "dkt_rownoise_lowrank_f32")
    return dict(logp=logp, alpha=alpha, info=info, state=state, dsv=dsv, dmean=dmean)


def rownoise_lowrank_bwd(z, y, noise_rows, sv, mean, cls_weight, state: torch.Tensor, gobj: torch.Tensor) -> torch.Tensor:
    """dZ [B,N,D] of sum_b gobj[b] sum_c cls_weight[c] logp[b,c] from the state `rownoise_lowrank` left (dkt_rownoise_lowrank_bwd_f32: the classes in
    index order, no atomics)."""
    pr = _problem("rownoise_lowrank_bwd", y, rows=z, noise_rows=noise_rows, sv=sv, mean=mean, cls_weight=cls_weight)
    (sv, mean, cw), b_, c_ = pr.hypers, pr.b, pr.c
    state = _req(state, "state", 3)
    gobj = _req(gobj.reshape(-1), "gobj", 1)
    if tuple(state.shape) != (b_, c_, ROWNOISE_LOWRANK_STATE) or gobj.numel() != b_:
        raise RuntimeError("rownoise_lowrank_bwd: state must be the [%d,%d,%d] of rownoise_lowrank and gobj [%d]" % (b_, c_, ROWNOISE_LOWRANK_STATE, b_))
    dz = torch.empty_like(pr.rows)
    with _timed("dkt_rownoise_lowrank_bwd_f32"):
        st = _lib_now().dkt_rownoise_lowrank_bwd_f32(_p(pr.rows), _p(pr.y), pr.y_bstride, _p(pr.noise_rows), pr.nr_bstride,
                                                     _p(sv), _p(mean), _p(cw), _p(state), state.numel() * 4, _p(gobj), _p(dz), b_, c_, pr.n, pr.d, _stream())
    _lib.check(st, "dkt_rownoise_lowrank_bwd_f32")
    return dz


def rownoise_lowrank_predict(zq: torch.Tensor, state: torch.Tensor, sv: torch.Tensor, mean: torch.Tensor):
    """The latent posterior of the class models at the queries zq [B,M,D] from the state of `rownoise_lowrank` on the conditioning rows
    (dkt_rownoise_lowrank_predict_f32): (mu [B,C,M], var [B,C,M] without observation noise, labels [B,M] int32 = argmax_c mu, the first maximum)."""
    zq = _req(zq, "zq", 3)
    state = _req(state, "state", 3)
    b_, m, d = zq.shape
    c_ = state.shape[1]
    if state.shape[0] != b_ or state.shape[2] != ROWNOISE_LOWRANK_STATE:
        raise RuntimeError("rownoise_lowrank_predict: state must be the [B=%d,C,%d] of rownoise_lowrank, got %s" % (b_, ROWNOISE_LOWRANK_STATE, tuple(state.shape)))
    sv, mean = _hypers("rownoise_lowrank_predict", c_, dict(sv=sv, mean=mean))
    mu, var, labels = _f32(zq.device, b_, c_, m), _f32(zq.device, b_, c_, m), _i32(zq.device, b_, m)
    with _timed("dkt_rownoise_lowrank_predict_f32"):
        st = _lib_now().dkt_rownoise_lowrank_predict_f32(_p(zq), _p(state), state.numel() * 4, _p(sv), _p(mean), _p(mu), _p(var), _p(labels), b_, c_, m, d,
                                                         _stream())
    _lib.check(st, "dkt_rownoise_lowrank_predict_f32")
    return mu, var, labels


# ------------------------------------------------------------------------------------------------------
# BNCosSim front half fused into the Gram build (reference methods/DKT.py:48,141-142,375-378)
# ------------------------------------------------------------------------------------------------------
def bn_stats(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float = 1e-5) -> dict:
    """Train-mode BatchNorm1d statistics per episode: x:[B,N,D] -> mean, rstd, a, s, var_unbiased (each [B,D]);
    y = a x + s is bn_out(x).  x: float32, bfloat16 or float16 (the statistics are fp32 either way)."""
    x = _req_x(x, "x", 3)
    b_, n, d = x.shape
    if d % 4:
        raise RuntimeError("bn_stats: D must be a multiple of 4")
    gamma = None if gamma is None else _req(gamma.reshape(-1), "gamma", 1)
    beta = None if beta is None else _req(beta.reshape(-1), "beta", 1)
    out = {k: torch.empty((b_, d), device=x.device, dtype=torch.float32) for k in ("mean", "rstd", "a", "s", "var_unbiased")}
    _front_end("bn_stats", x, [_p(x), _p(gamma), _p(beta), float(eps), _p(out["mean"]), _p(out["rstd"]), _p(out["a"]),
                               _p(out["s"]), _p(out["var_unbiased"]), b_, n, d, _stream()], 0)
    return out


def _ab_stride(a: torch.Tensor, s: torch.Tensor, b_: int, d: int) -> int:
    if a.shape != s.shape:
        raise RuntimeError("gram_bn: a and s must have the same shape")
    if a.dim() == 1 and a.shape[0] == d:
        return 0
    if a.dim() == 2 and tuple(a.shape) == (b_, d):
        return d
    raise RuntimeError("gram_bn: a / s must be [D] or [B,D]")


def gram_bn(x: torch.Tensor, a: torch.Tensor, s: torch.Tensor):
    """E[b] = Zn Zn^T with Zn = normalize(a x + s) (never materialised); returns (E [B,N,N], rnorm [B,N]).  x: float32, bfloat16 or float16."""
    x = _req_x(x, "x", 3)
    b_, n, d = x.shape
    if n > 128 or d % 4:
        raise RuntimeError("gram_bn: needs N <= 128 and D %% 4 == 0 (got N=%d, D=%d)" % (n, d))
    a = _req(a, "a")
    s = _req(s, "s")
    stride = _ab_stride(a, s, b_, d)
    e = torch.empty((b_, n, n), device=x.device, dtype=torch.float32)
    rnorm = torch.empty((b_, n), device=x.device, dtype=torch.float32)
    _front_end("gram_bn", x, [_p(x), _p(a), _p(s), stride, _p(e), _p(rnorm), b_, n, d, _stream()], 0)
    return e, rnorm


def gram_bn_train(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float = 1e-5):
    """bn_stats + gram_bn in one pass over x (train-mode BatchNorm1d statistics taken inside the Gram kernel's staging path).
    Returns (E [B,N,N], rnorm [B,N], stats dict as bn_stats).  x: float32, bfloat16 or float16."""
    x = _req_x(x, "x", 3)
    b_, n, d = x.shape
    if n > 128 or d % 4:
        raise RuntimeError("gram_bn_train: needs N <= 128 and D %% 4 == 0 (got N=%d, D=%d)" % (n, d))
    gamma = None if gamma is None else _req(gamma.reshape(-1), "gamma", 1)
    beta = None if beta is None else _req(beta.reshape(-1), "beta", 1)
    out = {k: torch.empty((b_, d), device=x.device, dtype=torch.float32) for k in ("mean", "rstd", "a", "s", "var_unbiased")}
    e = torch.empty((b_, n, n), device=x.device, dtype=torch.float32)
    rnorm = torch.empty((b_, n), device=x.device, dtype=torch.float32)
    _front_end("gram_bn_train", x, [_p(x), _p(gamma), _p(beta), float(eps), _p(out["mean"]), _p(out["rstd"]), _p(out["a"]),
                                    _p(out["s"]), _p(out["var_unbiased"]), _p(e), _p(rnorm), b_, n, d, _stream()], 0)
    return e, rnorm, out


def gram_bn_bwd(w, e, x, a, s, rnorm, mean=None, rstd=None, ep_scale=None):
    """Backward of gram_bn (+ train-mode batch statistics when mean/rstd are given): returns (dX, dgamma_part, dbeta_part);
    the last two are [B,D] per-episode parts (None in eval mode).  x: float32, bfloat16 or float16; dX comes back in x's dtype."""
    x = _req_x(x, "x", 3)
    b_, n, d = x.shape
    w = _req(w, "w", 3)
    e = _req(e, "e", 3)
    a = _req(a, "a")
    s = _req(s, "s")
    rnorm = _req(rnorm, "rnorm", 2)
    stride = _ab_stride(a, s, b_, d)
    train = mean is not None
    if train:
        mean = _req(mean, "mean", 2)
        rstd = _req(rstd, "rstd", 2)
    if ep_scale is not None:
        ep_scale = _req(ep_scale.reshape(-1), "ep_scale", 1)
    dx = torch.empty_like(x)
    dg = torch.empty((b_, d), device=x.device, dtype=torch.float32) if train else None
    db = torch.empty((b_, d), device=x.device, dtype=torch.float32) if train else None
    _front_end("gram_bn_bwd", x, [_p(w), _p(e), _p(x), _p(a), _p(s), stride, _p(mean), _p(rstd), _p(rnorm), _p(ep_scale),
                                  _p(dx), _p(dg), _p(db), b_, n, d, _stream()], 2)
    return dx, dg, db


def bn_param_grads(dg: torch.Tensor, db: torch.Tensor):
    """(dgamma [D], dbeta [D]) = the sums over the episodes of the per-episode parts [B,D] gram_bn_bwd / normalize_bn_bwd return (dkt_bn_param_grads_f32: fixed
    order; one launch up to 256 episodes, two beyond -- as two tensor reductions: two launches + four buffer fills).  One episode: the parts ARE the sums."""
    dg = _req(dg, "dgamma_part", 2)
    db = _req(db, "dbeta_part", 2)
    b_, d = dg.shape
    if db.shape != dg.shape:
        raise RuntimeError("bn_param_grads: the two parts must have the same shape")
    if b_ == 1:
        return dg.reshape(d), db.reshape(d)
    if os.environ.get("DKT_FUSED_REDUCTIONS", "1") == "0":                 # the tensor expressions (their twin)
        return dg.sum(0), db.sum(0)
    lib = _lib_now()
    og = torch.empty((d,), device=dg.device, dtype=torch.float32)
    ob = torch.empty((d,), device=dg.device, dtype=torch.float32)
    ws_bytes = int(lib.dkt_bn_param_grads_workspace_bytes(b_, d))
    ws = _workspace(ws_bytes, dg.device)
    with _timed("dkt_bn_param_grads_f32"):
        st = lib.dkt_bn_param_grads_f32(_p(dg), _p(db), _p(og), _p(ob), b_, d, _p(ws), ws_bytes, _stream())
    _lib.check(st, "dkt_bn_param_grads_f32")
    return og, ob


def affine_normalize(x: torch.Tensor, a: torch.Tensor, s: torch.Tensor):
    """Zn = y / max(|y|_2, 1e-12), y = a x + s, row by row; a, s: [D] or [B,D].  Returns (Zn [B,N,D], rnorm [B,N]) (dkt_affine_normalize_f32: the front end of
    episodes with more than 128 rows, whose Gram kernels take unit rows as input).  x: float32, bfloat16 or float16; Zn is float32."""
    x = _req_x(x, "x", 3)
    b_, n, d = x.shape
    a = _req(a, "a")
    s = _req(s, "s")
    stride = _ab_stride(a, s, b_, d)
    zn = torch.empty_like(x) if x.dtype == torch.float32 else torch.empty((b_, n, d), device=x.device, dtype=torch.float32)
    rnorm = torch.empty((b_, n), device=x.device, dtype=torch.float32)
    _front_end("affine_normalize", x, [_p(x), _p(a), _p(s), stride, _p(zn), _p(rnorm), b_, n, d, _stream()], 0)
    return zn, rnorm


def normalize_bn_bwd(dzn, zn, x, a, rnorm, mean=None, rstd=None):
    """Backward of affine_normalize (+ the train-mode batch statistics behind a, s when mean / rstd are given): (dX, dgamma_part [B,D], dbeta_part [B,D]) --
    the parts are None without statistics (dkt_normalize_bn_bwd_f32).  x: float32, bfloat16 or float16; dX comes back in x's dtype."""
    dzn = _req(dzn, "dzn", 3)
    zn = _req(zn, "zn", 3)
    x = _req_x(x, "x", 3)
    b_, n, d = x.shape
    a = _req(a, "a")
    rnorm = _req(rnorm, "rnorm", 2)
    stride = _ab_stride(a, a, b_, d)
    train = mean is not None
    if train:
        mean = _req(mean, "mean", 2)
        rstd = _req(rstd, "rstd", 2)
    dx = torch.empty_like(x)
    dg = torch.empty((b_, d), device=x.device, dtype=torch.float32) if train else None
    db = torch.empty((b_, d), device=x.device, dtype=torch.float32) if train else None
    ws = torch.empty((b_, n), device=x.device, dtype=torch.float32)
    _front_end("normalize_bn_bwd", x, [_p(dzn), _p(zn), _p(x), _p(a), stride, _p(mean), _p(rstd), _p(rnorm), _p(dx), _p(dg), _p(db), _p(ws), b_, n, d,
                                       _stream()], 2)
    return dx, dg, db


# ------------------------------------------------------------------------------------------------------
# Training episodes: a front end (how E is made) x an objective (what is solved on it), behind ONE autograd Function.
# Both are pairs of plain functions (no autograd) under a class used as a namespace; everything is positional, so a call costs no more host time than a
# hand-written Function, and a helper names what it reads by unpacking against its own `forward`:
#   front.forward(objv, *front arguments)  -> (m, outs, saved, static)
#       m: E -- or, for an objective with `on_features`, the pair (rows Z [B,N,D], unit_rows); outs: its non-differentiable outputs (E first, None where no E
#       exists); saved: the tensors its backward needs; static: shapes and flags for it
#   objv.forward(m, *objective arguments)  -> (obj [B], aux, saved, static)
#       aux: its non-differentiable outputs in the order the public functions return them; saved / static as above
#   objv.de(saved) -> d obj / d E as the forward left it (W of dkt_mll_f32, dK of dkt_laplace_grad_f32, dE of dkt_mll_rownoise_f32); an `on_features` objective has
#       objv.drows(z, saved, gobj) -> dZ instead
#   front.backward(saved, static, objv, osaved, gobj, *needs_input_grad of the front arguments) -> their gradients, a tuple
#   objv.backward(saved, static, gobj, *needs_input_grad of the objective arguments)            -> their gradients, a tuple
# `front.nargs` is the number of front arguments.  No route reads anything back to the host: every one is graph-capturable.
# ------------------------------------------------------------------------------------------------------
def _sum_episodes(gobj: torch.Tensor, part: torch.Tensor, shape) -> torch.Tensor:
    """sum_b gobj[b] part[b, :] -- the gradient of a [C] parameter from its per-episode parts [B,C]."""
    return (gobj.reshape(-1, 1) * part).sum(0).reshape(shape)


class _Gaussian:
    """Exact-GP marginal likelihood on E [B,N,N] or [B,C,N,N]: logp, W = d obj / d E and the hyper-parameter parts in ONE launch (dkt_mll_f32) ->
    obj[b] = sum_c cls_weight[c] logp[b,c].  Outputs (logp, alpha, info, jitter)."""
    on_features = resident_only = False

    @staticmethod
    def forward(e, y, sv, mean, noise, cls_weight, jitter0, max_tries):
        out = mll(e, y, sv, mean, noise, want_grad=True, cls_weight=cls_weight, jitter0=jitter0, max_tries=max_tries)
        obj = objective(out["logp"], cls_weight)
        return (obj, (out["logp"], out["alpha"], out["info"], out["jitter"]), (out["w"], out["dsv"], out["dmean"], out["dnoise"], cls_weight),
                (sv.shape, mean.shape, noise.shape))

    @staticmethod
    def de(saved):
        w, *_ = saved
        return w

    @staticmethod
    def backward(saved, shapes, gobj, need_y, need_sv, need_mean, need_noise, *_):
        *_, dsv, dmean, dnoise, cw = saved
        return (None,) + hyper_grads(gobj, cw, dsv if need_sv else None, dmean if need_mean else None, dnoise if need_noise else None, shapes) + (None, None, None)


class _LooCV(_Gaussian):
    """Leave-one-out predictive log likelihood of the same Gaussian model on E [B,N,N] or [B,C,N,N]: loo, W = d obj / d E and the hyper-parameter parts in ONE
    launch (dkt_loo_f32) -> obj[b] = sum_c cls_weight[c] loo[b,c].  Outputs (loo, alpha, info, jitter, mu_loo, var_loo).  Episodes of up to 127 rows (larger ones
    of the linear kernels: _FeatureSpaceLooCV): behind the BN trunk front end it takes the resident form only.  `de` and `backward` are the Gaussian objective's: W and the raw
    parts follow the conventions of dkt_mll_f32."""
    on_features, resident_only = False, True

    @staticmethod
    def forward(e, y, sv, mean, noise, cls_weight, jitter0, max_tries):
        with torch.no_grad():
            out = loo(e, y, sv, mean, noise, want_grad=True, cls_weight=cls_weight, jitter0=jitter0, max_tries=max_tries)
            obj = objective(out["loo"], cls_weight)
        return (obj, (out["loo"], out["alpha"], out["info"], out["jitter"], out["mu_loo"], out["var_loo"]),
                (out["w"], out["dsv"], out["dmean"], out["dnoise"], cls_weight), (sv.shape, mean.shape, noise.shape))


class _FeatureSpaceLooCV(_LooCV):
    """The same objective for the linear kernels in feature space (D <= 64, any N), on the rows Z and not on E: the D x D matrices Z^T Z + (noise_c + jitter) / sv_c I,
    loo, the hyper-parameter parts and dZ = sum_c cls_weight_c d loo_c / d Z in ONE launch (dkt_loofs_f32).  Neither E nor W is ever formed: the 20-way episodes
    of 400 / 420 rows.  `backward` is the Gaussian objective's."""
    on_features, resident_only = True, False
    de = None

    @staticmethod
    def forward(rows, y, sv, mean, noise, cls_weight, jitter0, max_tries):
        z, _ = rows
        with torch.no_grad():
            out = loo_lowrank(z, y, sv, mean, noise, want_grad=True, cls_weight=cls_weight, jitter0=jitter0, max_tries=max_tries)
            obj = objective(out["loo"], cls_weight)
        return (obj, (out["loo"], out["alpha"], out["info"], out["jitter"], out["mu_loo"], out["var_loo"]),
                (out["dz"], out["dsv"], out["dmean"], out["dnoise"], cls_weight), (sv.shape, mean.shape, noise.shape))

    @staticmethod
    def drows(z, saved, gobj):
        dz, *_ = saved
        return dz * gobj.reshape(-1, 1, 1)


class _FeatureSpaceGaussian(_Gaussian):
    """The same objective for the linear kernels in feature space (D <= 64 < N), on the rows Z and not on E:
       A = Z^T Z, P = Z^T (Y - m) (dkt_lowrank_gram_f32) -> the D x D model K'_c = sv_c A + noise_c I through dkt_mll_f32 (jitter ladder and all)
       -> alpha, logp, hyper-parameter gradients, V (dkt_lowrank_finish_f32); dZ = g_b (V^T T + 2 Z W') (dkt_lowrank_bwd_f32) from (v, t, wd) in the place of W.
    Neither E[B,N,N] nor W[B,N,N] is ever formed (reference lines replaced: methods/DKT.py:375-378, 161-163)."""
    on_features = True
    de = None

    @staticmethod
    def forward(rows, y, sv, mean, noise, cls_weight, jitter0, max_tries):
        z, unit_rows = rows
        o = _lowrank_forward(z, y, sv, mean, noise, cls_weight, jitter0, max_tries, unit_rows)           # (normalises them: `_problem`)
        return (o["obj"], (o["logp"], o["alpha"], o["info"], o["jitter"]), (o["v"], o["t"], o["wd"], o["dsv"], o["dmean"], o["dnoise"], cls_weight),
                (sv.shape, mean.shape, noise.shape))

    @staticmethod
    def drows(z, saved, gobj):
        v, t, wd, *_ = saved
        return _lowrank_backward(z, v, t, wd, gobj)


class _Laplace:
    """Bernoulli likelihood, K_c = sv_c E: the mode without autograd, then lml, dE and the parts of d sv at the mode (`_laplace_forward`).  Outputs (lml, iters).
    Episodes of up to 127 rows: behind the BN trunk front end it takes the resident form only."""
    on_features, resident_only = False, True

    @staticmethod
    def forward(e, y, sv, cls_weight, max_iter):
        obj, lml, iters, dk, dscale = _laplace_forward(e, y, cls_weight, sv, max_iter)
        return obj, (lml, iters), (dk, dscale), None if sv is None else sv.shape

    @staticmethod
    def de(saved):
        dk, _ = saved
        return dk

    @staticmethod
    def backward(saved, sv_shape, gobj, need_y, need_sv, *_):
        _, dscale = saved
        return None, (_sum_episodes(gobj, dscale, sv_shape) if need_sv else None), None, None


class _Dirichlet:
    """Dirichlet classification likelihood, K_c = sv_c E + diag(noise_rows_c) on the transformed labels: logp, dE and the parts of d sv, d mean in ONE call
    (dkt_mll_rownoise_f32; exact, no Newton loop, no jitter ladder).  Outputs (logp, alpha, info).  Episodes of up to 127 rows: behind the BN trunk front
    end it takes the resident form only."""
    on_features, resident_only = False, True

    @staticmethod
    def forward(e, ytilde, noise_rows, sv, mean, cls_weight):
        with torch.no_grad():
            out = mll_rownoise(e, ytilde, noise_rows, sv, mean, want_grad=True, cls_weight=cls_weight)
            obj = objective(out["logp"], cls_weight)
        return obj, (out["logp"], out["alpha"], out["info"]), (out["de"], out["dsv"], out["dmean"]), (sv.shape, mean.shape)

    @staticmethod
    def de(saved):
        de, *_ = saved
        return de

    @staticmethod
    def backward(saved, shapes, gobj, need_y, need_noise_rows, need_sv, need_mean, *_):
        _, dsv, dmean, *_ = saved                                                 # (both carry cls_weight already)
        return (None, None, _sum_episodes(gobj, dsv, shapes[0]) if need_sv else None, _sum_episodes(gobj, dmean, shapes[1]) if need_mean else None, None)


class _FeatureSpaceDirichlet(_Dirichlet):
    """The same objective for the linear kernels in feature space (D <= 64, any N), on the rows Z and not on E: the D x D models B_c = I + sv_c Z^T
    diag(noise_rows_c)^-1 Z in ONE call (dkt_rownoise_lowrank_f32), dZ from the state it leaves (dkt_rownoise_lowrank_bwd_f32).  Neither E nor dE is ever
    formed: the 20-way episodes of 400 / 420 rows."""
    on_features, resident_only = True, False
    de = None

    @staticmethod
    def forward(rows, ytilde, noise_rows, sv, mean, cls_weight):
        z, _ = rows
        with torch.no_grad():
            out = rownoise_lowrank(z, ytilde, noise_rows, sv, mean, cls_weight, want_grad=True)
            obj = objective(out["logp"], cls_weight)
        kept = (ytilde, noise_rows, sv, mean, cls_weight)                         # (as given: `rownoise_lowrank_bwd` normalises them as `rownoise_lowrank` did)
        return obj, (out["logp"], out["alpha"], out["info"]), (out["state"], out["dsv"], out["dmean"]) + kept, (sv.shape, mean.shape)

    @staticmethod
    def drows(z, saved, gobj):
        state, _, _, ytilde, noise_rows, sv, mean, cw = saved
        return rownoise_lowrank_bwd(z, ytilde, noise_rows, sv, mean, cw, state, gobj)


def _rows_grad(objv, osaved, z, gobj, unit_rows):
    """dZ of E = Z Z^T with the upstream gradient folded in as ep_scale: g_b (dE + dE^T) Z (dkt_gram_bwd_f32; dE is symmetric as dkt_mll_f32 and
    dkt_laplace_grad_f32 write it), or what the feature-space objective makes of the rows itself."""
    if objv.on_features:
        return objv.drows(z, osaved, gobj)
    return gram_bwd(objv.de(osaved), z, gobj, unit_rows=unit_rows, w_symmetric=True)


class _GivenE:
    """E is an argument; its gradient is grad_out * dE.  No output of its own."""
    nargs = 1

    @staticmethod
    def forward(objv, e):
        return e, (), (), None

    @staticmethod
    def backward(saved, static, objv, osaved, gobj, need_e):
        de = objv.de(osaved)                                                      # [B,N,N] or [B,C,N,N] (per-class E)
        return (de * gobj.reshape([-1] + [1] * (de.dim() - 1)) if need_e else None,)


class _LinearGram:
    """linear / cossim / bncossim: E = Z Z^T (dkt_gram_f32); the feature-space objective takes Z itself and E is None.  Output E."""
    nargs = 2

    @staticmethod
    def forward(objv, z, unit_rows):
        unit_rows = bool(unit_rows)
        if objv.on_features:
            z = _req(z, "z", 3)
            return (z, unit_rows), (None,), (z,), unit_rows
        e = gram(z, None, KERNEL_LINEAR_UNIT if unit_rows else KERNEL_LINEAR)
        return e, (e,), (z,), unit_rows

    @staticmethod
    def backward(saved, unit_rows, objv, osaved, gobj, need_z, *_):
        z, = saved
        return (_rows_grad(objv, osaved, z, gobj, unit_rows) if need_z else None), None


class _ClassKernel:
    """The kernels whose class models own a base-kernel parameter (rbf / matern: lengthscale [C]; poli1 / poli2: offset [C]; reference DKT.py:63-66, 352-365):
    ONE contraction per episode (dkt_gram_f32: squared distances or Gram) -> the C class kernels E [B,C,N,N] (dkt_class_kernel_f32); backward
    dkt_class_kernel_bwd_f32 (sum over the classes, parameter gradients) -> dkt_gram_bwd_f32 (upstream grad as ep_scale).  Output E."""
    nargs = 5

    @staticmethod
    def forward(objv, z, param, cmap, power, base_kind):
        one = torch.ones(1, device=z.device, dtype=torch.float32)
        base = gram(z, None, base_kind, one if base_kind == KERNEL_SQDIST else None)
        e = class_kernel(base, cmap, power, param)
        return e, (e,), (z, base, param), (int(cmap), int(power))

    @staticmethod
    def backward(saved, maps, objv, osaved, gobj, need_z, need_param, *_):
        z, base, param = saved
        dz = gparam = None
        if need_z or need_param:
            wp, dpar = class_kernel_bwd(objv.de(osaved), base, maps[0], maps[1], param)
            if need_z:
                dz = gram_bwd(wp, z, gobj)
            if need_param:
                gparam = _sum_episodes(gobj, dpar, param.shape)
        return dz, gparam, None, None, None


class _BnTrunk:
    """Straight from the trunk output X: [BatchNorm1d(train) +] F.normalize + linear Gram.  use_bn=False is the plain cossim kernel (no bn_out: affine map = identity).
    Up to 128 rows, resident: dkt_gram_bn_train_f32 (statistics + Gram in one pass over x; DKT_FUSED_STATS=0: dkt_bn_stats_f32 + dkt_gram_bn_f32), backward
    dkt_gram_bn_bwd_f32, which takes the Laplace dE exactly as it takes the Gaussian W; the normalised features are never written to memory.
    More than 128 rows (the 20-way shapes) or the feature-space objective, big: dkt_bn_stats_f32 -> dkt_affine_normalize_f32 (Zn written once: the large-N Gram
    kernels take unit rows as input) -> dkt_gram_f32, or no E at all in feature space (D <= 64 < N, Conv4S / Omniglot: csrc/dkt_lowrank.hip); backward
    dkt_gram_bwd_f32 / dkt_lowrank_bwd_f32 -> dkt_normalize_bn_bwd_f32.
    X in bfloat16 / float16 (a mixed-precision backbone): the same route through the *_x16 twins of the front-end calls; the gradient of X comes back
    in X's dtype, everything behind the front end (Zn, E, the objective, the hyper-parameter and BatchNorm gradients) is fp32.
    Outputs E (None in feature space), batch_mean, batch_var_unbiased, a, s, rnorm."""
    nargs = 5

    @staticmethod
    def forward(objv, x, gamma, beta, eps, use_bn):
        use_bn = bool(use_bn)
        n, d = x.shape[1], x.shape[2]
        big = objv.on_features or (n > FUSED_EP_MAX_N and not objv.resident_only)
        e = zn = None
        if use_bn and not big and os.environ.get("DKT_FUSED_STATS", "1") != "0":
            e, rnorm, st = gram_bn_train(x, gamma, beta, eps)               # statistics + Gram in one pass over x
        elif use_bn:
            st = bn_stats(x, gamma, beta, eps)
        if use_bn:
            a, s, bmean, rstd, bvar = st["a"], st["s"], st["mean"], st["rstd"], st["var_unbiased"]
        else:
            a = torch.ones(d, device=x.device, dtype=torch.float32)
            s = torch.zeros(d, device=x.device, dtype=torch.float32)
            bmean = rstd = bvar = torch.zeros(0, device=x.device, dtype=torch.float32)
        static = (use_bn, None if gamma is None else gamma.shape, None if beta is None else beta.shape)
        if big:
            zn, rnorm = affine_normalize(x, a, s)
            if objv.on_features:
                return (zn, True), (None, bmean, bvar, a, s, rnorm), (x, a, s, bmean, rstd, rnorm, None, zn), static
            e = gram(zn, None, KERNEL_LINEAR_UNIT)
            return e, (e, bmean, bvar, a, s, rnorm), (x, a, s, bmean, rstd, rnorm, None, zn), static
        if e is None:
            e, rnorm = gram_bn(x, a, s)
        return e, (e, bmean, bvar, a, s, rnorm), (x, a, s, bmean, rstd, rnorm, e, None), static

    @staticmethod
    def backward(saved, static, objv, osaved, gobj, need_x, need_gamma, need_beta, *_):
        x, a, s, bmean, rstd, rnorm, e, zn = saved                                 # resident: E, no Zn; big: Zn, and E is not kept
        use_bn, gamma_shape, beta_shape = static
        if not use_bn:
            bmean = rstd = None
        if zn is not None:
            dx, dg, db = normalize_bn_bwd(_rows_grad(objv, osaved, zn, gobj, True), zn, x, a, rnorm, bmean, rstd)
        else:
            dx, dg, db = gram_bn_bwd(objv.de(osaved), e, x, a, s, rnorm, bmean, rstd, gobj)
        ggamma = gbeta = None
        if dg is not None and (need_gamma or need_beta):
            sg, sb = bn_param_grads(dg, db)
            ggamma = sg.reshape(gamma_shape) if need_gamma else None
            gbeta = sb.reshape(beta_shape) if need_beta else None
        return (dx if need_x else None), ggamma, gbeta, None, None


class _EpisodeFn(torch.autograd.Function):
    """obj [B] of a (front end, objective) pair and, behind it, the objective's outputs and the front end's, all non-differentiable.  The arguments are the
    front end's, then the objective's (the signatures of their `forward`s)."""

    @staticmethod
    def forward(ctx, front, objv, *args):
        n = front.nargs
        m, outs, saved, static = front.forward(objv, *args[:n])
        obj, aux, osaved, ostatic = objv.forward(m, *args[n:])
        ctx.save_for_backward(*saved, *osaved)
        ctx.episode = (front, objv, len(saved), static, ostatic)
        outs = aux + outs
        ctx.mark_non_differentiable(*[o for o in outs if o is not None])
        ctx.set_materialize_grads(False)       # (otherwise autograd zero-fills a gradient tensor for every non-differentiable output: E alone is 361 MB at cfg2)
        return (obj,) + outs

    @staticmethod
    def backward(ctx, gobj, *_unused):
        need = ctx.needs_input_grad
        if gobj is None:
            return (None,) * len(need)
        front, objv, nsaved, static, ostatic = ctx.episode
        saved = ctx.saved_tensors
        osaved = saved[nsaved:]
        gobj = gobj.contiguous()
        n = 2 + front.nargs                                                        # (front, objv) come first
        return ((None, None) + front.backward(saved[:nsaved], static, objv, osaved, gobj, *need[2:n])
                + objv.backward(osaved, ostatic, gobj, *need[n:]))


class _Objective(NamedTuple):
    on_e: type                            # the class that works on E
    on_rows: Optional[type]               # its feature-space form (`on_features`: works on the rows, no E), or None
    applies: Optional[Callable]           # applies(n, d, c, ...): does an episode of the linear kernels take the feature-space form?
    outputs: tuple                        # its non-differentiable outputs, in the order `forward` returns them


# What is solved on an episode, by name.  The first output is the log probability per (episode, class) whatever the objective calls it (the marginal
# likelihood, the leave-one-out likelihood `loo`, the Laplace approximation `lml`).
OBJECTIVES = {
    "gaussian": _Objective(_Gaussian, _FeatureSpaceGaussian, lowrank_applies, ("logp", "alpha", "info", "jitter")),
    "loo": _Objective(_LooCV, _FeatureSpaceLooCV, loo_lowrank_applies, ("logp", "alpha", "info", "jitter", "mu_loo", "var_loo")),
    "laplace": _Objective(_Laplace, None, None, ("logp", "iters")),
    "dirichlet": _Objective(_Dirichlet, _FeatureSpaceDirichlet, rownoise_lowrank_applies, ("logp", "alpha", "info")),
}
OBJECTIVE_OUTPUTS = {name: row.outputs for name, row in OBJECTIVES.items()}
LAPLACE_MAX_ITER = 100                    # the Newton iterations the Laplace objective allows its mode search (`max_iter` of the public calls)
# the outputs of the front ends (E is None where the episode ran in feature space): an `_EpisodeFn` result is ("obj",) + OBJECTIVE_OUTPUTS[...] + one of these
GIVEN_E_OUTPUTS = ()
ROWS_OUTPUTS = ("e",)                                                                   # _LinearGram, _ClassKernel
BN_TRUNK_OUTPUTS = ("e", "batch_mean", "batch_var_unbiased", "a", "s", "rnorm")


_ROWS_FRONTS = (_LinearGram, _BnTrunk)                # their first argument is the [B,N,D] operand a feature-space objective can take in the place of E


def _episode(front, fargs: tuple, name: str, oargs: tuple):
    """obj [B] and the outputs of one (front end, objective) pair: `front` with its arguments, the objective `name` of OBJECTIVES with its arguments (the
    targets first).  The ONE place that asks the objective's `applies` whether the episode runs in feature space: the marginal likelihood draws its line by the
    batch size and by the fused front end, the others by where the rows live."""
    row, rows = OBJECTIVES[name], fargs[0]
    on_rows = (row.applies is not None and front in _ROWS_FRONTS and rows.dim() == 3
               and row.applies(rows.shape[1], rows.shape[2], oargs[0].shape[-2], *((rows.shape[0], front is _BnTrunk) if name == "gaussian" else (rows.is_cuda,))))
    return _EpisodeFn.apply(front, row.on_rows if on_rows else row.on_e, *fargs, *oargs)


def _rows_front(z, kernel: str, lengthscale, offset, unit_rows):
    """(front end, its arguments) of the episodes z [B,N,D] under `kernel`: the linear Gram, or the contraction + class maps of the kernels with per-class
    parameters."""
    z = _req(z, "z", 3)
    if kernel in LINEAR_KINDS:
        return _LinearGram, (z, unit_rows)
    cmap, power, param, base_kind = _classmap_of(kernel, lengthscale, offset)
    return _ClassKernel, (z, param, cmap, power, base_kind)


def mll_objective(e, y, sv, mean, noise, cls_weight, jitter0: float = 1e-6, max_tries: int = 3):
    """Returns (obj, logp, alpha, info, jitter): obj [B], logp [B,C], alpha [B,C,N], info [B,C], jitter [B,C]."""
    return _episode(_GivenE, (e,), "gaussian", (y, sv, mean, noise, cls_weight, jitter0, max_tries))


def laplace_objective(K, Y, cls_weight, scale=None, max_iter: int = 100):
    """Differentiable (in K and scale) Laplace training objective of B episodes; arguments as `laplace_grad`.  Returns (obj, logp, iters): obj [B], logp [B,C]
    the approximate log marginal likelihood lml, iters [B,C].  Forward: `laplace_mode` without autograd, then `laplace_grad`; no host read-back
    (graph-capturable like the other episode calls)."""
    return _episode(_GivenE, (K,), "laplace", (Y, scale, cls_weight, max_iter))


def episode_loss_laplace(z, y, sv, cls_weight, kernel: str, lengthscale=None, offset=None, unit_rows: bool = False, max_iter: int = 100):
    """Bernoulli-likelihood training episode(s) z [B,N,D] (N <= 127, C <= 32), y in {0,1}: K_c = sv_c * k_c(z, z).  Returns (obj, logp, iters, e): obj [B],
    logp [B,C] (lml), iters [B,C], E."""
    return _episode(*_rows_front(z, kernel, lengthscale, offset, unit_rows), "laplace", (y, sv, cls_weight, max_iter))


def episode_loss_laplace_bn(x, gamma, beta, y, sv, cls_weight, eps: float = 1e-5, use_bn: bool = True, max_iter: int = 100):
    """x [B,N,D] trunk output BEFORE bn_out, N <= 127.  Returns (obj, logp, iters, e, batch_mean, batch_var_unbiased, a, s, rnorm)."""
    return _episode(_BnTrunk, (x, gamma, beta, eps, use_bn), "laplace", (y, sv, cls_weight, max_iter))


def dirichlet_objective(e, ytilde, noise_rows, sv, mean, cls_weight):
    """Differentiable (in e, sv, mean) Dirichlet-likelihood objective of B episodes; arguments as `mll_rownoise`, ytilde / noise_rows of `dirichlet_targets`.
    Returns (obj, logp, alpha, info): obj [B], logp [B,C], alpha [B,C,N], info [B,C].  One launch (two for a shared e), no host read-back."""
    return _episode(_GivenE, (e,), "dirichlet", (ytilde, noise_rows, sv, mean, cls_weight))


def episode_loss_dirichlet(z, ytilde, noise_rows, sv, mean, cls_weight, kernel: str, lengthscale=None, offset=None, unit_rows: bool = False):
    """Dirichlet-likelihood training episode(s) z [B,N,D] (N <= 127, C <= 32): K_c = sv_c * k_c(z, z) + diag(noise_rows_c).  The linear kernels with
    D <= 64 take any N: above 127 rows (rownoise_lowrank_applies) the episode runs in feature space and E is None.
    Returns (obj, logp, alpha, info, e): obj [B], logp [B,C], alpha [B,C,N], info [B,C], E."""
    return _episode(*_rows_front(z, kernel, lengthscale, offset, unit_rows), "dirichlet", (ytilde, noise_rows, sv, mean, cls_weight))


def episode_loss_dirichlet_bn(x, gamma, beta, ytilde, noise_rows, sv, mean, cls_weight, eps: float = 1e-5, use_bn: bool = True):
    """x [B,N,D] trunk output BEFORE bn_out (float32, bfloat16 or float16), N <= 127 -- or, with D <= 64, any N: above 127 rows the episode runs in
    feature space (rownoise_lowrank_applies) and E is None.
    Returns (obj, logp, alpha, info, e, batch_mean, batch_var_unbiased, a, s, rnorm)."""
    return _episode(_BnTrunk, (x, gamma, beta, eps, use_bn), "dirichlet", (ytilde, noise_rows, sv, mean, cls_weight))


def loo_objective(e, y, sv, mean, noise, cls_weight, jitter0: float = 1e-6, max_tries: int = 3):
    """Differentiable (in e, sv, mean, noise) leave-one-out objective of B episodes, obj[b] = sum_c cls_weight[c] loo[b,c]; arguments as `loo`.
    Returns (obj, logp, alpha, info, jitter, mu_loo, var_loo): obj [B], logp [B,C] (loo), alpha [B,C,N], info [B,C], jitter [B,C], mu_loo [B,C,N],
    var_loo [B,C,N].  One launch, no host read-back."""
    return _episode(_GivenE, (e,), "loo", (y, sv, mean, noise, cls_weight, jitter0, max_tries))


def episode_loss_loo(z, y, sv, mean, noise, cls_weight, kernel: str, lengthscale=None, offset=None, unit_rows: bool = False,
                     jitter0: float = 1e-6, max_tries: int = 3):
    """Leave-one-out training episode(s) z [B,N,D] (N <= 127, C <= 32): K_c = sv_c * k_c(z, z) + noise_c I, every kernel of the marginal-likelihood path.
    The linear kernels with D <= 64 take any N above 128 rows (loo_lowrank_applies): the episode runs in feature space and E is None.
    Returns (obj, logp, alpha, info, jitter, mu_loo, var_loo, e): obj [B], logp [B,C] (loo), alpha [B,C,N], info, jitter [B,C], mu_loo, var_loo [B,C,N], E."""
    return _episode(*_rows_front(z, kernel, lengthscale, offset, unit_rows), "loo", (y, sv, mean, noise, cls_weight, jitter0, max_tries))


def episode_loss_loo_bn(x, gamma, beta, y, sv, mean, noise, cls_weight, eps: float = 1e-5, jitter0: float = 1e-6, max_tries: int = 3, use_bn: bool = True):
    """x [B,N,D] trunk output BEFORE bn_out (float32, bfloat16 or float16), N <= 127 -- or, with D <= 64, any N above 128 rows: the episode runs in
    feature space (loo_lowrank_applies) and E is None.
    Returns (obj, logp, alpha, info, jitter, mu_loo, var_loo, e, batch_mean, batch_var_unbiased, a, s, rnorm)."""
    return _episode(_BnTrunk, (x, gamma, beta, eps, use_bn), "loo", (y, sv, mean, noise, cls_weight, jitter0, max_tries))


def episode_loss_class_kernel(z, y, sv, mean, noise, cls_weight, kernel: str, lengthscale=None, offset=None,
                              jitter0: float = 1e-6, max_tries: int = 3):
    """Training episode(s) z:[B,N,D] for rbf / matern / poli1 / poli2 with per-class lengthscale / offset [C], sizes of
    mll_per_class_supported().
    Returns (obj, logp, alpha, info, jitter, e): obj [B], logp [B,C], alpha [B,C,N], info [B,C], jitter [B,C], E [B,C,N,N]."""
    cmap, power, param, base_kind = _classmap_of(kernel, lengthscale, offset)
    return _episode(_ClassKernel, (_req(z, "z", 3), param, cmap, power, base_kind), "gaussian", (y, sv, mean, noise, cls_weight, jitter0, max_tries))


def episode_loss_bn(x, gamma, beta, y, sv, mean, noise, cls_weight, eps: float = 1e-5, jitter0: float = 1e-6, max_tries: int = 3,
                    use_bn: bool = True, full: bool = False):
    """x:[B,N,D] trunk output BEFORE bn_out (float32, bfloat16 or float16).
    Returns (obj, logp, alpha, info, jitter, e, batch_mean, batch_var_unbiased): obj [B], E (None when the episode ran in feature space: lowrank_applies),
    batch_mean [B,D], batch_var_unbiased [B,D] -- the last two feed the caller's running-statistics update -- plus, with full=True, the folded
    affine map a, s and the row scales rnorm (zn = (a x + s) rnorm: what a caller needs to re-create the normalised features)."""
    out = _episode(_BnTrunk, (x, gamma, beta, eps, use_bn), "gaussian", (y, sv, mean, noise, cls_weight, jitter0, max_tries))
    return out if full else out[:8]


def episode_loss_linear(z, y, sv, mean, noise, cls_weight, jitter0: float = 1e-6, max_tries: int = 3, unit_rows: bool = False):
    """z:[B,N,D] (already bn_out'ed + normalised).  Returns (obj, logp, alpha, info, jitter, e).
    unit_rows=True: z went through F.normalize (cossim / bncossim), |z| <= 1 element-wise -- the Gram kernels may then use
    the scaled 2-way f16 split (same fp32-level accuracy, less staging work).
    D <= 64 < N where it wins (lowrank_applies: the Conv4S / Omniglot episodes -- every 420-row batch, 105-row batches from 3072 episodes): the episode runs in
    feature space and E is None -- no N x N matrix exists."""
    return _episode(_LinearGram, (z, unit_rows), "gaussian", (y, sv, mean, noise, cls_weight, jitter0, max_tries))


