"""Every library call of dkt_amd.ops and dkt_amd.image_data inside a sentinel arena with guard bands (tests/guard_arena.py, docs/GUARD_BANDS.md): one case per
(entry point, shape, variant), at the smallest shapes at which a kernel's indexing changes.  A case fails when a call writes outside the blocks it was given
(footprint), leaves an element of a returned tensor unwritten (coverage), returns something that depends on the memory around its operands or on the
allocator (independence), or takes less workspace than the library's query asks for (placement).  Inputs are seeded and well conditioned (unit rows, noise
0.1 .. 0.3, |x| + 0.5 trunk outputs), so that no case meets the jitter ladder or a NaN by itself."""
import contextlib

import numpy as np
import pytest
import torch

import dkt_amd
from dkt_amd import _lib, image_data, ops

import dirichlet_lowrank_model
import dirichlet_model
import episode_routes as er
import guard_arena as ga
import lowrank_model
from test_image_data_gpu import MIXED
from test_inference_gpu import PREDICT_PER_CLASS, PREDICT_SHARED, VARIANCE_CASES
from test_laplace_grad_gpu import SHAPES as LAPLACE_SHAPES

pytestmark = pytest.mark.gpu

# Returned elements that may stay unwritten: only where a header says that their content is unspecified.  (entry point, output, the header's sentence)
EXEMPT = [
]

# Names of the signature tables that launch nothing: pure host queries
HOST_QUERIES = ("abi_version", "device_cu_count", "reload_env", "env_value", "workspace_bytes", "_supported", "_nsplit", "state_bytes", "augment_plan")


class Case:
    """outside: the returned tensors torch computes itself (or a callable that asks the library); zero: returned tensors that must be all zero besides every
    `info` / `jitter` entry of a returned dict (the status and the jitter rung where a call returns them in a tuple)."""

    def __init__(self, name, calls, make, outside=(), tol=None, env=None, hook=None, zero=()):
        self.name, self.calls, self.make, self.outside, self.tol, self.env, self.hook, self.zero = name, set(calls.split()), make, outside, tol, env or {}, hook, zero


CASES = []


def case(name, calls, make, **kw):
    CASES.append(Case(name, calls, make, **kw))


# ------------------------------------------------------------------------------------------------ inputs
def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _unit(seed, b, n, d, dev):
    return torch.nn.functional.normalize(_randn(seed, b, n, d), dim=2).to(dev)


def _hypers(c, n, dev):
    return dict(sv=torch.linspace(0.5, 2.0, c).to(dev), mean=torch.linspace(-0.2, 0.3, c).to(dev), noise=torch.linspace(0.1, 0.3, c).to(dev),
                cw=torch.linspace(0.5, 1.5, c).mul(-1.0 / (c * n)).to(dev))


def _pm1(c, n, dev, zero_one=False):
    cls = torch.arange(n) % max(c, 2)
    return torch.where(cls.unsqueeze(0) == torch.arange(c).unsqueeze(1), 1.0, 0.0 if zero_one else -1.0).contiguous().to(dev)


def _sym(w):
    return (0.5 * (w + w.transpose(-1, -2))).contiguous()


def _gram_of(z):
    return _sym(z @ z.transpose(1, 2))


def _per_class(e, c):
    """[B,C,N,N] RBF matrices of unit rows from their Gram: exp(-|zi - zj|^2 / (2 l_c^2)), |zi - zj|^2 = 2 - 2 e."""
    ls = torch.linspace(0.6, 1.5, c, device=e.device).reshape(1, c, 1, 1)
    return ((e.unsqueeze(1) - 1.0).clamp_max_(0.0) / ls ** 2).exp_()                  # (one temporary of e's size: the B = 130 case holds 209 MB here)


# ------------------------------------------------------------------------------------------------ ops.gram, ops.gram_bwd
GRAM_SYM = [(1, 1, 4), (2, 5, 7), (3, 17, 36), (2, 33, 65), (2, 65, 36), (1, 127, 100), (2, 128, 160), (1, 129, 64), (1, 130, 516), (1, 257, 100), (1, 447, 36),
            (1, 449, 20), (5, 19, 2916)]
GRAM_CROSS = [(1, 7, 3, 5), (2, 75, 25, 64), (1, 300, 100, 36), (1, 19, 5, 2916)]
KINDS = dict(linear=ops.KERNEL_LINEAR, unit=ops.KERNEL_LINEAR_UNIT, rbf=ops.KERNEL_RBF, sqdist=ops.KERNEL_SQDIST)


def _gram(b, m, n, d, kind):
    def make(dev):
        inp = dict(a=_unit(m + d, b, m, d, dev), ls=torch.tensor([0.8], device=dev))
        if n is not None:
            inp["bm"] = _unit(n + d + 1, b, n, d, dev)
        return inp, lambda p: ops.gram(p["a"], p.get("bm"), KINDS[kind], p["ls"])
    return make


for _b, _n, _d in GRAM_SYM:
    for _k in KINDS:
        case("gram-%s-B%d-N%d-D%d" % (_k, _b, _n, _d), "dkt_gram_f32", _gram(_b, _n, None, _d, _k))
for _b, _m, _n, _d in GRAM_CROSS:
    for _k in KINDS:
        case("gram-cross-%s-B%d-M%d-N%d-D%d" % (_k, _b, _m, _n, _d), "dkt_gram_f32", _gram(_b, _m, _n, _d, _k))


def _gram_bwd(b, n, d, scale, unit_rows, w_symmetric):
    def make(dev):
        inp = dict(w=_sym(_randn(n, b, n, n) / n).to(dev), z=_unit(n + d, b, n, d, dev))
        if scale:
            inp["g"] = torch.linspace(-2.0, 1.0, b).to(dev)
        return inp, lambda p: ops.gram_bwd(p["w"], p["z"], p.get("g"), unit_rows=unit_rows, w_symmetric=w_symmetric)
    return make


for _b, _n, _d in GRAM_SYM:
    for _s, _u, _w in ((False, False, False), (True, True, False), (True, False, True), (False, True, True)):
        case("gram_bwd-B%d-N%d-D%d%s%s%s" % (_b, _n, _d, "-scale" * _s, "-unit" * _u, "-wsym" * _w), "dkt_gram_bwd_f32", _gram_bwd(_b, _n, _d, _s, _u, _w))


# ------------------------------------------------------------------------------------------------ rbf_bwd, sqdist_bwd, class_kernel, class_kernel_bwd
CK_N, CK_C = (7, 33, 128, 130, 258, 131, 257), (1, 5, 20, 32)          # (131, 257: the 16-byte kernel of class_kernel_bwd at an odd N)
CK_MAPS = dict(rbf=(ops.CLASSMAP_RBF, 0), matern=(ops.CLASSMAP_MATERN25, 0), poli1=(ops.CLASSMAP_POLY, 1), poli2=(ops.CLASSMAP_POLY, 2))


def _sqdist(z):
    return (2.0 - 2.0 * _gram_of(z)).clamp_min(0.0)


def _elementwise_bwd(fn, n):
    def make(dev):
        u = _sqdist(_unit(n, 2, n, 16, dev)) / 0.8 ** 2
        inp = dict(w=_sym(_randn(n, 2, n, n) / n).to(dev), m=torch.exp(-0.5 * u) if fn == "rbf_bwd" else u, ls=torch.tensor([0.8], device=dev))
        return inp, lambda p: getattr(ops, fn)(p["w"], p["m"], p["ls"])
    return make


for _n in CK_N:
    case("rbf_bwd-N%d" % _n, "dkt_rbf_bwd_f32", _elementwise_bwd("rbf_bwd", _n))
    case("sqdist_bwd-N%d" % _n, "dkt_sqdist_bwd_f32", _elementwise_bwd("sqdist_bwd", _n))


def _class_base(kind, b, n, dev):
    z = _unit(n + b, b, n, 16, dev)
    return _gram_of(z) if kind.startswith("poli") else _sqdist(z)


def _class_kernel(kind, b, c, n):
    def make(dev):
        inp = dict(base=_class_base(kind, b, n, dev), param=torch.linspace(0.6, 1.5, c).to(dev))
        return inp, lambda p: ops.class_kernel(p["base"], CK_MAPS[kind][0], CK_MAPS[kind][1], p["param"])
    return make


def _class_kernel_bwd(kind, b, c, n):
    def make(dev):
        inp = dict(w=_sym(_randn(n + c, b, c, n, n) / n).to(dev), base=_class_base(kind, b, n, dev), param=torch.linspace(0.6, 1.5, c).to(dev))
        return inp, lambda p: ops.class_kernel_bwd(p["w"], p["base"], CK_MAPS[kind][0], CK_MAPS[kind][1], p["param"])
    return make


def _parts_summed_by_torch(b, n):
    """Beyond one split of the rows (dkt_class_kernel_bwd_nsplit), ops sums the parameter-gradient parts with torch: that output lies outside the arena."""
    return lambda: ("out[1]",) if int(_lib.load().dkt_class_kernel_bwd_nsplit(b, n)) > 1 else ()


_ck = [(k, n, CK_C[(i + j) % 4]) for i, k in enumerate(CK_MAPS) for j, n in enumerate(CK_N[:5])] + [(k, 33, c) for k in CK_MAPS for c in CK_C]
_ck += [(k, n, CK_C[(i + j) % 4]) for i, k in enumerate(CK_MAPS) for j, n in enumerate(CK_N[5:])]          # (last: every earlier case keeps its B and its C)
for _i, (_k, _n, _c) in enumerate(dict.fromkeys(_ck)):
    _b = (1, 3, 5)[_i % 3]
    case("class_kernel-%s-B%d-C%d-N%d" % (_k, _b, _c, _n), "dkt_class_kernel_f32", _class_kernel(_k, _b, _c, _n))
    case("class_kernel_bwd-%s-B%d-C%d-N%d" % (_k, _b, _c, _n), "dkt_class_kernel_bwd_f32", _class_kernel_bwd(_k, _b, _c, _n),
         outside=_parts_summed_by_torch(_b, _n))


# ------------------------------------------------------------------------------------------------ ops.mll
MLL_N = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 111, 112, 127, 128, 129, 143, 144, 257, 447, 448, 460)
MLL_VARIANTS = dict(                      # the flag, the N it accepts, whether DKT_MLL_WANT_CHOL combines with it, the C it accepts
    default=({}, lambda n: True, True, (1, 5, 20)),
    generic=(dict(force_generic=True), lambda n: True, True, (1, 5, 20)),
    blocked=(dict(force_blocked=True), lambda n: n > 127, True, (1, 5, 20)),
    tiled=(dict(force_tiled=True), lambda n: 128 <= n <= 447, False, (1, 5, 20)),
    band=(dict(force_band=True), lambda n: 128 <= n <= 432, False, (5, 20)),
    f32mfma=(dict(force_f32mfma=True), lambda n: n <= 127, True, (1, 5, 20)),
    per_class=({}, lambda n: True, False, (1, 5, 20)),
)


def _mll(variant, b, c, n, grad, chol, weighted):
    def make(dev):
        e = _gram_of(_unit(7 * n + b, b, n, 64, dev))
        h = _hypers(c, n, dev)
        inp = dict(e=_per_class(e, c) if variant == "per_class" else e, y=_pm1(c, n, dev), sv=h["sv"], mean=h["mean"], noise=h["noise"])
        if weighted:
            inp["cw"] = h["cw"]
        return inp, lambda p: ops.mll(p["e"], p["y"], p["sv"], p["mean"], p["noise"], want_grad=grad, want_chol=chol, cls_weight=p.get("cw"),
                                      **MLL_VARIANTS[variant][0])
    return make


# Every (variant, N) runs every flag set at B = 1 and at B = 3: want_grad with and without cls_weight, and where DKT_MLL_WANT_CHOL combines with the variant also
# want_chol alone and want_grad + want_chol + cls_weight.  C goes through the variant's values over these runs, starting one further at every N, so that each
# (B, flag set) meets every C at some N edge and every (variant, N) meets every C.
MLL_FLAG_SETS = ((True, False, True), (True, False, False), (False, True, False), (True, True, True))          # (want_grad, want_chol, cls_weight)
for _v, (_kw, _accepts, _chol_ok, _cs) in MLL_VARIANTS.items():
    for _j, _n in enumerate(n for n in MLL_N if _accepts(n)):
        _runs = [(b, f) for f in MLL_FLAG_SETS if _chol_ok or not f[1] for b in (1, 3)]
        for _k, (_b, (_grad, _chol, _w)) in enumerate(_runs):
            _c = _cs[(_j + _k) % len(_cs)]
            case("mll-%s-B%d-C%d-N%d%s%s%s" % (_v, _b, _c, _n, "-grad" * _grad, "-chol" * _chol, "-cw" * _w), "dkt_mll_f32", _mll(_v, _b, _c, _n, _grad, _chol, _w))
# the only place where the generic kernel's loop over workspace chunks runs: per-class workspace is sized for min(B, 128) episodes
case("mll-per_class-B130-C2-N448", "dkt_mll_f32", _mll("per_class", 130, 2, 448, False, False, True))


# ------------------------------------------------------------------------------------------------ objective, hyper_grads, bn_param_grads
def _objective(b, c, weighted):
    def make(dev):
        inp = dict(logp=_randn(b + c, b, c).to(dev))
        if weighted:
            inp["cw"] = _hypers(c, 25, dev)["cw"]
        return inp, lambda p: ops.objective(p["logp"], p.get("cw"))
    return make


def _hyper_grads(b, c, weighted, which):
    def make(dev):
        inp = dict(gobj=torch.linspace(-2.0, 1.0, b).to(dev), **{k: _randn(b + c + i, b, c).to(dev) for i, k in enumerate(("dsv", "dmean", "dnoise")) if k in which})
        if weighted:
            inp["cw"] = _hypers(c, 25, dev)["cw"]
        return inp, lambda p: ops.hyper_grads(p["gobj"], p.get("cw"), p.get("dsv"), p.get("dmean"), p.get("dnoise"), ((c,), (c,), (c,)))
    return make


for _b, _c in ((1, 1), (3, 5), (5, 17), (257, 32), (1024, 20)):
    for _w in (False, True):
        case("objective-B%d-C%d%s" % (_b, _c, "-cw" * _w), "dkt_objective_f32", _objective(_b, _c, _w))
        case("hyper_grads-B%d-C%d%s" % (_b, _c, "-cw" * _w), "dkt_hyper_grads_f32", _hyper_grads(_b, _c, _w, ("dsv", "dmean", "dnoise")))
    case("hyper_grads-B%d-C%d-sv-only" % (_b, _c), "dkt_hyper_grads_f32", _hyper_grads(_b, _c, True, ("dsv",)))
    case("hyper_grads-B%d-C%d-mean-noise" % (_b, _c), "dkt_hyper_grads_f32", _hyper_grads(_b, _c, False, ("dmean", "dnoise")))


def _bn_param_grads(b, d):
    def make(dev):
        return dict(dg=_randn(b + d, b, d).to(dev), db=_randn(b + d + 1, b, d).to(dev)), lambda p: ops.bn_param_grads(p["dg"], p["db"])
    return make


for _b in (1, 2, 256, 257):
    for _d in (36, 64, 1600):
        case("bn_param_grads-B%d-D%d" % (_b, _d), "dkt_bn_param_grads_f32" if _b > 1 else "", _bn_param_grads(_b, _d))      # (one episode: the parts ARE the sums, no launch)


# ------------------------------------------------------------------------------------------------ predict, predict_var
def _predict(b, c, m, n, per_class):
    def make(dev):
        h = _hypers(c, n, dev)
        ex = _unit(m + n, b * (c if per_class else 1), m, n, dev).reshape((b, c, m, n) if per_class else (b, m, n)).contiguous()
        return dict(ex=ex, alpha=_randn(m + n + c, b, c, n).to(dev), sv=h["sv"], mean=h["mean"]), lambda p: ops.predict(p["ex"], p["alpha"], p["sv"], p["mean"])
    return make


def _predict_var(b, c, m, n):
    def make(dev):
        z, zq = _unit(n + m, b, n, 64, dev), _unit(n + m + 1, b, m, 64, dev)
        h = _hypers(c, n, dev)
        chol = ops.mll(_gram_of(z), _pm1(c, n, dev), h["sv"], h["mean"], h["noise"], want_chol=True)["chol"]
        inp = dict(ex=(zq @ z.transpose(1, 2)).contiguous(), exx=torch.ones(b, m, device=dev), chol=chol, sv=h["sv"], noise=h["noise"])
        return inp, lambda p: ops.predict_var(p["ex"], p["exx"], p["chol"], p["sv"], p["noise"])
    return make


for _b, _c, _m, _n in PREDICT_SHARED:
    case("predict-B%d-C%d-M%d-N%d" % (_b, _c, _m, _n), "dkt_predict_f32", _predict(_b, _c, _m, _n, False))
for _b, _c, _m, _n in PREDICT_PER_CLASS:
    case("predict-per_class-B%d-C%d-M%d-N%d" % (_b, _c, _m, _n), "dkt_predict_per_class_f32", _predict(_b, _c, _m, _n, True))
for _b, _c, _m, _n in VARIANCE_CASES:
    case("predict_var-B%d-C%d-M%d-N%d" % (_b, _c, _m, _n), "dkt_predict_var_f32", _predict_var(_b, _c, _m, _n))


# ------------------------------------------------------------------------------------------------ the front-end calls, float32 / bfloat16 / float16
FRONT_SHAPES = [(2, 5, 12), (5, 1, 36), (2, 33, 8), (3, 25, 64), (1, 128, 100), (2, 129, 68), (1, 150, 512), (2, 19, 2916)]
X_DTYPES = dict(f32=torch.float32, bf16=torch.bfloat16, f16=torch.float16)


def _trunk(b, n, d, dtype, dev):
    return dict(x=(_randn(n + d, b, n, d).abs() + 0.5).to(dev, dtype), gamma=(1.0 + 0.2 * _randn(d, d)).to(dev), beta=(0.1 * _randn(d + 1, d)).to(dev))


def _front(what, b, n, d, dtype):
    def make(dev):
        inp = _trunk(b, n, d, dtype, dev)
        if what == "bn_stats":
            return inp, lambda p: ops.bn_stats(p["x"], p["gamma"], p["beta"])
        if what == "gram_bn_train":
            return inp, lambda p: ops.gram_bn_train(p["x"], p["gamma"], p["beta"])
        st = ops.bn_stats(inp["x"], inp["gamma"], inp["beta"])
        inp = dict(x=inp["x"], a=st["a"], s=st["s"])
        if what == "gram_bn":
            return inp, lambda p: ops.gram_bn(p["x"], p["a"], p["s"])
        if what == "affine_normalize":
            return inp, lambda p: ops.affine_normalize(p["x"], p["a"], p["s"])
        inp.update(mean=st["mean"], rstd=st["rstd"])
        if what == "gram_bn_bwd":
            e, rnorm = ops.gram_bn(inp["x"], st["a"], st["s"])
            inp.update(w=_sym(_randn(n, b, n, n) / n).to(dev), e=e, rnorm=rnorm, g=torch.linspace(-2.0, 1.0, b).to(dev))
            return inp, lambda p: ops.gram_bn_bwd(p["w"], p["e"], p["x"], p["a"], p["s"], p["rnorm"], p["mean"], p["rstd"], p["g"])
        zn, rnorm = ops.affine_normalize(inp["x"], st["a"], st["s"])
        inp.update(dzn=(_randn(n + 1, b, n, d) / n).to(dev), zn=zn, rnorm=rnorm)
        return inp, lambda p: ops.normalize_bn_bwd(p["dzn"], p["zn"], p["x"], p["a"], p["rnorm"], p["mean"], p["rstd"])
    return make


for _what in ("bn_stats", "gram_bn", "gram_bn_train", "gram_bn_bwd", "affine_normalize", "normalize_bn_bwd"):
    for _b, _n, _d in FRONT_SHAPES:
        if _n > ops.FUSED_EP_MAX_N and _what.startswith("gram_bn"):
            continue                                                       # (the episode-resident calls take up to 128 rows)
        for _t, _dt in X_DTYPES.items():
            case("%s-%s-B%d-N%d-D%d" % (_what, _t, _b, _n, _d), "dkt_%s_%s" % (_what, "f32" if _t == "f32" else "x16"), _front(_what, _b, _n, _d, _dt))


# ------------------------------------------------------------------------------------------------ spectral mixture
def _smk_inputs(b, m, n, d, q, dev, cross):
    inp = dict(x1=(0.2 * _randn(m + d, b, m, d)).to(dev), w=(_rand(q, q) + 0.2).to(dev), mu=(_rand(q + 1, q, d) * 0.8 + 0.05).to(dev),
               sg=(_rand(q + 2, q, d) * 0.8 + 0.05).to(dev))
    if cross:
        inp["x2"] = (0.2 * _randn(n + d + 1, b, n, d)).to(dev)
    return inp


def _smk(fn, b, m, n, d, q, cross, **kw):
    def make(dev):
        return _smk_inputs(b, m, n, d, q, dev, cross), lambda p: getattr(ops, fn)(p["x1"], p.get("x2"), p["w"], p["mu"], p["sg"], **kw)
    return make


def _smk_bwd(b, n, d, q, task):
    def make(dev):
        inp = _smk_inputs(b, n, n, d, q, dev, False)
        inp["ge"] = _randn(n + q, b, n, n).to(dev)                           # not symmetric on purpose
        if task:
            return inp, lambda p: ops.smk_task_bwd(p["ge"], p["x1"], p["w"], p["mu"], p["sg"])
        inp["eq"] = ops.smk(inp["x1"], None, inp["w"], inp["mu"], inp["sg"], want_terms=True)[1]
        return inp, lambda p: ops.smk_bwd(p["ge"], p["eq"], p["x1"], p["w"], p["mu"], p["sg"])
    return make


for _b, _m, _n, _d, _q, _x in ((2, 10, 10, 40, 4, False), (1, 33, 33, 3, 1, False), (3, 5, 5, 1, 8, False), (2, 65, 31, 40, 4, True), (1, 129, 5, 1, 2, True)):
    case("smk-%s-B%d-M%d-N%d-D%d-Q%d" % ("cross" if _x else "sym", _b, _m, _n, _d, _q), "dkt_smk_f32", _smk("smk", _b, _m, _n, _d, _q, _x, want_terms=not _x))
    if not _x:
        case("smk_bwd-B%d-N%d-D%d-Q%d" % (_b, _n, _d, _q), "dkt_smk_bwd_f32", _smk_bwd(_b, _n, _d, _q, False))
for _i, _n in enumerate((1, 5, 31, 32)):
    for _j, _q in enumerate((1, 4, 8)):
        _b, _d = (1, 3, 5)[(_i + _j) % 3], (1, 40, 64, 63)[(_i + _j) % 4]
        case("smk_task-sym-B%d-N%d-D%d-Q%d" % (_b, _n, _d, _q), "dkt_smk_task_f32", _smk("smk_task", _b, _n, _n, _d, _q, False))
        case("smk_task_bwd-B%d-N%d-D%d-Q%d" % (_b, _n, _d, _q), "dkt_smk_task_bwd_f32", _smk_bwd(_b, _n, _d, _q, True))
for _i, _m in enumerate((1, 255, 256)):
    for _j, _q in enumerate((1, 4, 8)):
        _b, _n, _d = (1, 3, 5)[(_i + _j) % 3], (1, 5, 31, 32)[(_i + 2 * _j) % 4], (1, 40, 64, 63)[(_i + _j) % 4]
        case("smk_task-cross-B%d-M%d-N%d-D%d-Q%d" % (_b, _m, _n, _d, _q), "dkt_smk_task_f32", _smk("smk_task", _b, _m, _n, _d, _q, True))


# ------------------------------------------------------------------------------------------------ Laplace
def _laplace_k(b, c, n, dev, per_class):
    e = _gram_of(_unit(31 * n + c, b, n, 16, dev))
    return _per_class(e, c) if per_class else torch.exp(-(1.0 - e).clamp_min(0.0)).contiguous()


def _laplace(what, b, c, n, per_class=False, scaled=False):
    def make(dev):
        k, y = _laplace_k(b, c, n, dev, per_class), _pm1(c, n, dev, True)
        if what == "mode":
            return dict(k=k, y=y), lambda p: ops.laplace_mode(p["k"], p["y"])
        h = _hypers(c, n, dev)
        if what == "predict":
            md = ops.laplace_mode(k, y)
            zq = 17
            inp = dict(ks=_unit(n + 1, b, zq, n, dev).mul(0.5).contiguous(), kss=torch.ones(b, zq, device=dev), g=md["g"], w_sr=md["w_sr"], chol=md["chol"])
            return inp, lambda p: ops.laplace_predict(p["ks"], p["kss"], dict(g=p["g"], w_sr=p["w_sr"], chol=p["chol"]))
        kc = k if not scaled else (k if per_class else k.unsqueeze(1)) * h["sv"].reshape(1, -1, 1, 1)
        inp = dict(k=k, y=y, f=ops.laplace_mode(kc.contiguous(), y)["f"], cw=h["cw"])
        if scaled:
            inp["sv"] = h["sv"]
        return inp, lambda p: ops.laplace_grad(p["k"], p["y"], p["f"], p["cw"], p.get("sv"))
    return make


for _i, (_b, _c, _n) in enumerate(LAPLACE_SHAPES):
    case("laplace_mode-B%d-C%d-N%d" % (_b, _c, _n), "dkt_gpc_mode_f32", _laplace("mode", _b, _c, _n))
    case("laplace_mode-per_class-B%d-C%d-N%d" % (_b, _c, _n), "dkt_gpc_mode_f32", _laplace("mode", _b, _c, _n, per_class=True))
    case("laplace_predict-B%d-C%d-N%d" % (_b, _c, _n), "dkt_gpc_predict_f32", _laplace("predict", _b, _c, _n))
    case("laplace_grad-B%d-C%d-N%d" % (_b, _c, _n), "dkt_laplace_grad_f32", _laplace("grad", _b, _c, _n, scaled=bool(_i % 2)))
    case("laplace_grad-per_class-B%d-C%d-N%d" % (_b, _c, _n), "dkt_laplace_grad_f32", _laplace("grad", _b, _c, _n, per_class=True, scaled=not _i % 2))
case("laplace_grad-B2-C32-N127", "dkt_laplace_grad_f32", _laplace("grad", 2, 32, 127, scaled=True))
case("laplace_mode-B2-C32-N127", "dkt_gpc_mode_f32", _laplace("mode", 2, 32, 127))


# ------------------------------------------------------------------------------------------------ Dirichlet
def _rownoise(b, c, n, grad, chol, per_class=False):
    def make(dev):
        e = _gram_of(_unit(13 * n + c, b, n, 64, dev))
        y, nr = ops.dirichlet_targets(_pm1(c, n, dev))
        h = _hypers(c, n, dev)
        inp = dict(e=_per_class(e, c) if per_class else e, y=y, nr=nr, sv=h["sv"], mean=h["mean"], cw=h["cw"])
        return inp, lambda p: ops.mll_rownoise(p["e"], p["y"], p["nr"], p["sv"], p["mean"], want_grad=grad, want_chol=chol, cls_weight=p["cw"])
    return make


for _b, _c, _n in dirichlet_model.SHAPES + [(2, 32, 127), (5, 17, 19)]:
    case("mll_rownoise-B%d-C%d-N%d" % (_b, _c, _n), "dkt_mll_rownoise_f32", _rownoise(_b, _c, _n, False, True))
    case("mll_rownoise-B%d-C%d-N%d-grad" % (_b, _c, _n), "dkt_mll_rownoise_f32", _rownoise(_b, _c, _n, True, False))
    case("mll_rownoise-per_class-B%d-C%d-N%d-grad" % (_b, _c, _n), "dkt_mll_rownoise_f32", _rownoise(_b, _c, _n, True, False, per_class=True))


def _proba(b, c, m, s):
    def make(dev):
        inp = dict(mu=_randn(m + c, b, c, m).to(dev), var=_rand(m + c + 1, b, c, m).to(dev), eps=_randn(s, s, c).to(dev))
        return inp, lambda p: ops.dirichlet_proba(p["mu"], p["var"], p["eps"])
    return make


for _b, _c, _m, _s in dirichlet_model.PROBA_SHAPES + [(3, 32, 257, 5), (1, 17, 300, 64)]:
    case("dirichlet_proba-B%d-C%d-M%d-S%d" % (_b, _c, _m, _s), "dkt_dirichlet_proba_f32", _proba(_b, _c, _m, _s))


def _rownoise_lowrank(what, b, c, n, d):
    def make(dev):
        y, nr = ops.dirichlet_targets(_pm1(c, n, dev))
        h = _hypers(c, n, dev)
        inp = dict(z=_unit(n + d, b, n, d, dev), y=y, nr=nr, sv=h["sv"], mean=h["mean"], cw=h["cw"])
        if what == "fwd":
            return inp, lambda p: ops.rownoise_lowrank(p["z"], p["y"], p["nr"], p["sv"], p["mean"], p["cw"], want_grad=True)
        inp["state"] = ops.rownoise_lowrank(inp["z"], y, nr, h["sv"], h["mean"], h["cw"])["state"]
        if what == "bwd":
            inp["g"] = torch.linspace(-2.0, 1.0, b).to(dev)
            return inp, lambda p: ops.rownoise_lowrank_bwd(p["z"], p["y"], p["nr"], p["sv"], p["mean"], p["cw"], p["state"], p["g"])
        inp = dict(zq=_unit(n + d + 1, b, 17 + n % 3, d, dev), state=inp["state"], sv=h["sv"], mean=h["mean"])
        return inp, lambda p: ops.rownoise_lowrank_predict(p["zq"], p["state"], p["sv"], p["mean"])
    return make


def _state_bytes(b, c):
    def hook(m, standin, report):
        report.queries.append(("dkt_rownoise_lowrank_state_bytes", int(_lib.load().dkt_rownoise_lowrank_state_bytes(b, c))))
    return hook


for _b, _c, _n, _d in dirichlet_lowrank_model.SHAPES:
    case("rownoise_lowrank-B%d-C%d-N%d-D%d" % (_b, _c, _n, _d), "dkt_rownoise_lowrank_f32", _rownoise_lowrank("fwd", _b, _c, _n, _d), hook=_state_bytes(_b, _c))
    case("rownoise_lowrank_bwd-B%d-C%d-N%d-D%d" % (_b, _c, _n, _d), "dkt_rownoise_lowrank_bwd_f32", _rownoise_lowrank("bwd", _b, _c, _n, _d))
    case("rownoise_lowrank_predict-B%d-C%d-N%d-D%d" % (_b, _c, _n, _d), "dkt_rownoise_lowrank_predict_f32", _rownoise_lowrank("predict", _b, _c, _n, _d))


# ------------------------------------------------------------------------------------------------ image_data.augment
def _augment(b, s, aug):
    def make(dev):
        rng = np.random.default_rng(100 * b + s)
        sizes = (MIXED * 2)[:b]
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
        offs = np.concatenate([[0], np.cumsum([a.size for a in imgs])[:-1]]).astype(np.int64)
        table, jit, flip = image_data.build_table(offs, np.array([h for h, _ in sizes]), np.array([w for _, w in sizes]), s, aug, rng)
        pool = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
        return dict(pool=pool), lambda p: image_data.augment(p["pool"], table, s, jit, flip)
    return make


for _b in (1, 7):
    for _s in (28, 84):
        for _aug in (True, False):
            case("augment-B%d-S%d-%s" % (_b, _s, "aug" if _aug else "eval"), "dkt_augment_plan dkt_augment_u8", _augment(_b, _s, _aug))


# ------------------------------------------------------------------------------------------------ the feature-space Gaussian episode and the episode routes
def _feature_space(b, c, n, d):
    def make(dev):
        h = _hypers(c, n, dev)
        inp = dict(z=_unit(n + d, b, n, d, dev).requires_grad_(), y=_pm1(c, n, dev), sv=h["sv"], mean=h["mean"], noise=h["noise"], cw=h["cw"],
                   g=torch.linspace(-2.0, 1.0, b).to(dev))

        def call(p):
            outs = ops.episode_loss_linear(p["z"], p["y"], p["sv"], p["mean"], p["noise"], p["cw"], unit_rows=True)
            (outs[0] * p["g"]).sum().backward()
            return outs, p["z"].grad
        return inp, call
    return make


_LOWRANK_CALLS = "dkt_lowrank_noise_floor_f32 dkt_lowrank_gram_f32 dkt_mll_f32 dkt_lowrank_finish_f32 dkt_lowrank_bwd_f32"
for _i, _d in enumerate((4, 36, 60, 64)):
    for _j, _n in enumerate((80, 97, 130)):
        _b, _c = (1, 3, 5)[(_i + _j) % 3], (1, 5, 17, 20, 32)[(_i + 2 * _j) % 5]
        case("feature-space-B%d-C%d-N%d-D%d" % (_b, _c, _n, _d), _LOWRANK_CALLS, _feature_space(_b, _c, _n, _d), env=dict(DKT_LOWRANK="force"), zero=("out[0][3]", "out[0][4]"))


def _lowrank_kernels(b, c, n, d):
    """The gram, finish and backward calls themselves (no ops-level gate: N < 80 too) at the edge shapes of tests/lowrank_model.py: masked last row tile, padded
    columns, every class-tile and class-step count."""
    def make(dev):
        inp = {k: torch.as_tensor(v).to(dev) for k, v in lowrank_model.inputs(c, n, d, b=b, y_per_episode=True).items()}

        def call(p):
            fwd = ops._lowrank_forward(p["z"], p["y"], p["sv"], p["mean"], p["noise"], p["cw"], 1e-6, 3, True)
            return fwd, ops._lowrank_backward(p["z"], fwd["v"], fwd["t"], fwd["wd"], p["g"])
        return inp, call
    return make


for _i, (_c, _n, _d) in enumerate(lowrank_model.GUARD_CASES):
    _b = 2 + _i % 2
    case("lowrank-kernels-B%d-C%d-N%d-D%d" % (_b, _c, _n, _d), _LOWRANK_CALLS, _lowrank_kernels(_b, _c, _n, _d))


def _route(route):
    def make(dev):
        def call(p):
            got = er.run(route, dev)
            return got["outs"], got["grads"]
        return {}, call

    def hook(m, standin, report):
        m.setattr(er, "_leaf", lambda t, dev, dtype=torch.float32, grad=True: standin.place(t, dtype).requires_grad_(grad))
    return make, hook


def _route_zero(route):
    """Where the outputs of a route carry the status (and the Gaussian objective its jitter): (obj, logp, alpha, info, jitter, ..) / (obj, logp, alpha, info, ..);
    the Laplace objective returns (obj, lml, iters, ..) and has neither."""
    if "laplace" in route.name:
        return ()
    return ("out[0][3]",) if "dirichlet" in route.name else ("out[0][3]", "out[0][4]")


# leaf gradients that torch computes itself behind the library calls (they lie outside the arena): `de * gobj` of a given E, `_sum_episodes` of the Laplace and
# Dirichlet objectives and of the class-kernel parameter
_E, _SV, _SV_MEAN = ("e",), ("sv",), ("sv", "mean")
ROUTE_OUTSIDE = {
    "mll_objective": _E, "laplace_objective": _E + ("scale",), "dirichlet-objective": _E + _SV_MEAN,
    "class-kernel-rbf": ("param",), "class-kernel-poli2": ("param",),
    "laplace-linear": _SV, "laplace-rbf": _SV + ("lengthscale",), "laplace-bn": _SV,
    "dirichlet-linear": _SV_MEAN, "dirichlet-class-kernel-rbf": _SV_MEAN + ("lengthscale",), "dirichlet-bn-resident": _SV_MEAN,
    "dirichlet-bn-resident-no-bn": _SV_MEAN, "dirichlet-bn-resident-bf16": _SV_MEAN, "dirichlet-linear-feature-space": _SV_MEAN,
    "dirichlet-bn-feature-space": _SV_MEAN,
}
for _r in er.ROUTES:
    _make, _hook = _route(_r)
    case("route-" + _r.name, " ".join(dict.fromkeys(_r.forward + _r.backward)) + (" dkt_lowrank_noise_floor_f32" if "dkt_lowrank_gram_f32" in _r.forward else ""),
         _make, hook=_hook, env=_r.env, zero=_route_zero(_r), outside=tuple("out[1].%s" % k for k in ROUTE_OUTSIDE.get(_r.name, ())))


# ------------------------------------------------------------------------------------------------ the test
class Recorder:
    def __init__(self):
        self.calls, self.outside = [], []


@contextlib.contextmanager
def _recording(kase, standin, report, rec, monkeypatch):
    """Around every run of a case: the names of the library calls (through _lib.check), the operands that reach ops._p / image_data._ptr from outside the arena,
    the values of the workspace queries, the environment and the patches of the case."""
    arena, pending = standin.arena, []
    real_p, real_ptr, real_check = ops._p, image_data._ptr, _lib.check

    def note(t):
        if t is not None and arena is not None and t.numel() and not arena.contains(t):
            pending.append("%s %s" % (tuple(t.shape), str(t.dtype).replace("torch.", "")))

    def p(t):
        note(t)
        return real_p(t)

    def ptr(t):
        note(t)
        return real_ptr(t)

    def check(status, what):
        if arena is not None:
            rec.calls.append(what)
            rec.outside += ["%s: %s" % (what, d) for d in pending]
        del pending[:]
        real_check(status, what)

    def query(name, fn):
        def wrapped(*args):
            value = fn(*args)
            if name == "dkt_augment_plan":                                  # (the size comes back through its last argument; image_data.augment takes at least 16 bytes)
                report.queries.append((name, max(16, int(args[3]._obj.value))))
            else:
                report.queries.append((name, int(value)))
            return value
        return wrapped

    with monkeypatch.context() as m, er._environment(kase.env):
        m.setattr(ops, "_p", p)
        m.setattr(image_data, "_ptr", ptr)
        m.setattr(_lib, "check", check)
        for lib in list(_lib._libs.values()):
            for name, fn in list(vars(lib).items()):
                if "workspace_bytes" in name or name == "dkt_augment_plan":
                    m.setattr(lib, name, query(name, fn))
        if kase.hook is not None:
            kase.hook(m, standin, report)
        yield


@pytest.mark.parametrize("kase", CASES, ids=lambda k: k.name)
def test_guard_bands(kase, cuda, monkeypatch):
    torch.cuda.reset_peak_memory_stats()
    inputs, call = kase.make(cuda)
    rec = Recorder()
    report = ga.check(call, inputs, cuda, monkeypatch, [ops, image_data], extra=lambda s, r: _recording(kase, s, r, rec, monkeypatch), tol=kase.tol)
    exempt = [out for entry, out, _ in EXEMPT if entry in kase.name]
    failures = report.failures(outside=kase.outside() if callable(kase.outside) else kase.outside, exempt=exempt)
    # no case meets a NaN, a poisoned problem or the jitter ladder by itself: independence is never a comparison of failures
    for name, t in report.results.items():
        if t.dtype.is_floating_point and not bool(torch.isfinite(t).all()):
            failures.append("clean run: %s %s of the ordinary run is not finite" % (name, tuple(t.shape)))
        if (name.endswith(".info") or name.endswith(".jitter") or name in kase.zero) and bool((t != 0).any()):
            failures.append("clean run: %s of the ordinary run is not zero (max %g)" % (name, float(t.double().abs().max())))
    missing = [name for name in kase.zero if name not in report.results]
    assert not missing, "the case names %s, the call returns %s" % (missing, sorted(report.results))
    print("GUARD %s calls=%s outside=%s operands-outside=%s blocks=%d peak=%dMB" % (kase.name, sorted(set(rec.calls)), report.outside(), sorted(set(rec.outside)),
                                                                                  len(report.blocks), torch.cuda.max_memory_allocated() >> 20))
    assert set(rec.calls) == kase.calls, "the case is there for %s and made %s" % (sorted(kase.calls), sorted(set(rec.calls)))
    assert not failures, "\n".join(failures + ["operands from outside the arena (not watched): %s" % sorted(set(rec.outside))])
    assert ops.torch is torch and image_data.torch is torch


def test_every_entry_point_that_launches_a_kernel_has_an_arena_case():
    """Every name of the signature tables that is no pure host query is among the calls of a case above (and each case asserts that it made exactly its calls):
    a new entry point without an arena case fails here."""
    tables = (_lib.SIGNATURES, _lib.SMK_SIGNATURES, _lib.GPC_SIGNATURES, _lib.X16_SIGNATURES, {"dkt_augment_u8": None})
    launching = {name for table in tables for name in table if not any(q in name for q in HOST_QUERIES)}
    reached = set().union(*(k.calls for k in CASES))
    assert launching - reached == set(), "no arena case reaches %s" % sorted(launching - reached)
