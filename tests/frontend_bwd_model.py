"""numpy restatement of the front-end backward: `dkt_gram_bn_bwd_f32 / _x16` (the fused bn_out + F.normalize + Gram backward of episodes with at most 128 rows)
and `dkt_normalize_bn_bwd_f32 / _x16` (its streaming twin behind dkt_gram_bwd_f32), and the case list both test files of this kernel pair run.

Fused call (the comment block above gram_bn_bwd_ep_kernel), one episode, W = d obj / d E, g = the episode's upstream scale:

    A    = g (W + W^T)
    Zn_i = rnorm_i (a x_i + s)
    dZn  = A Zn
    t_i  = sum_j A_ij E_ij
    dY_i = rnorm_i (dZn_i - Zn_i t_i)
    train mode:  dbeta = sum_i dY_i,  dgamma = sum_i dY_i xh_i,  xh = (x - mean) rstd,  dX = a (dY - dbeta / N - xh dgamma / N)
    eval mode (mean is None):  dX = a dY, no parts

Streaming call: dZn and Zn are given, t_i = Zn_i . dZn_i, the rest as above.

dtype=float64 is the reference; dtype=float32 runs every array and operation in fp32: its distance from the float64 run is the fp32 floor the GPU tests
scale their bound from.  The floor is that of plain fp32 -- the kernel's 22-bit MFMA operands (`split22`) are modelled only in the group of one- and two-row
batches, where the plain run returns an exact zero that no rounding kernel can (docs/FRONTEND_BWD.md).  `defect` injects one of the mistakes the host test proves detectable.

`make_case` computes every forward quantity the backward consumes (a, s, mean, rstd, rnorm, E, Zn) in float64 from X and rounds it ONCE to fp32, so the
model and the kernel receive bit-identical operands and the backward is isolated from the forward."""
import numpy as np
import torch

EPS = 1e-5
XDTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
QUANTITIES = ("dx", "dgamma", "dbeta")


def _r32(v):
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


def _rx(v, xdtype):
    """Round to the element type of X (float64 holding values of that type)."""
    return torch.tensor(np.asarray(v, np.float64), dtype=torch.float64).to(XDTYPES[xdtype]).double().numpy()


def _finish(dy, dyt, x, a, mean, rstd, dtype, defect, tile):
    """dY -> dict(dx, dgamma, dbeta, terms): the BatchNorm1d half shared by the two calls.  `tile`: rows per tile of the kernel (16 fused, 32 streaming).
    dyt: the size of dY's two terms before they cancel; `terms` carries it through to each quantity (see `errors`)."""
    n, d = x.shape
    xht = (np.abs(x) + np.abs(mean)) * rstd if mean is not None else np.zeros_like(x)       # (xh = x rstd - mean rstd: a difference of two products)
    terms = dict(dx=float(np.abs(a * dyt).max()), dbeta=float(dyt.sum(0).max()), dgamma=float((dyt * xht).sum(0).max()))
    if mean is None:
        out = dict(dx=a * dy, dgamma=None, dbeta=None)
    else:
        xh = (x - mean) * rstd
        rows = slice(0, n - 1) if (defect == "b" and n % tile == 0 and n > 1) else slice(0, n)
        dbeta = dy[rows].sum(0, dtype=dtype)
        dgamma = (dy[rows] * xh[rows]).sum(0, dtype=dtype)
        if defect == "d":                                  # the reduce-scatter's index permutation left out: features 4k+1 and 4k+2 change places
            perm = np.arange(d).reshape(-1, 4)[:, [0, 2, 1, 3]].reshape(-1)
            dbeta, dgamma = dbeta[perm], dgamma[perm]
        inv_n = dtype(1) / dtype(tile * ((n + tile - 1) // tile) if defect == "e" else n)
        out = dict(dx=a * (dy - dbeta * inv_n - xh * (dgamma * inv_n)), dgamma=dgamma, dbeta=dbeta)
    if defect == "c":                                      # the partial last slab never processed
        slab = 64 if tile == 16 else 32
        d0 = slab * (d // slab)
        for q in out.values():
            if q is not None:
                q[..., d0:] = 0
    out["terms"] = terms
    return out


def _two_planes(v, scale):
    """v under `scale` as the sum of two float16 numbers (the kernel's MFMA operands: 22 bits), back in v's type."""
    vs = v * scale
    hi = vs.astype(np.float16).astype(v.dtype)
    return (hi + (vs - hi).astype(np.float16).astype(v.dtype)) / scale


def backward(w, e, x, a, s, rnorm, mean, rstd, g, dtype=np.float64, defect=None, split22=False):
    """One episode of dkt_gram_bn_bwd: w, e [N,N]; x [N,D]; a, s [D]; rnorm [N]; mean, rstd [D] or None (eval mode); g scalar or None (= 1).
    split22: A under its per-row power-of-two scale (row maximum in [2^14, 2^15)) and the Zn of the product A Zn under 2^15 rounded to two f16 planes."""
    w, e, x, a, s, rnorm = (np.asarray(v, dtype) for v in (w, e, x, a, s, rnorm))
    mean, rstd = (None if v is None else np.asarray(v, dtype) for v in (mean, rstd))
    n = x.shape[0]
    g = dtype(1.0 if (g is None or defect == "f") else g)
    am = g * w if defect == "a" else g * (w + w.T)
    zn = rnorm[:, None] * (a * x + s)
    if split22:
        rmax = np.abs(am).max(1, keepdims=True)
        am = _two_planes(am, np.exp2(14.0 - np.floor(np.log2(np.where(rmax > 0, rmax, 1.0)))).astype(dtype))
        dzn = am @ _two_planes(zn, dtype(32768.0))
    else:
        dzn = am @ zn
    if defect == "g":                                      # the image's pad columns j in [N, KP) not zeroed: they hold other rows, and A reaches them
        kp = 32 * ((n + 31) // 32)
        m = min(kp - n, n)
        dzn = dzn + am[:, :m] @ zn[:m]
    t = (am * e).sum(1, dtype=dtype)
    dy = rnorm[:, None] * (dzn - zn * t[:, None])
    dyt = rnorm[:, None] * (np.abs(am) @ np.abs(zn) + np.abs(zn) * (np.abs(am) * np.abs(e)).sum(1, dtype=dtype)[:, None])
    return _finish(dy, dyt, x, a, mean, rstd, dtype, defect, 16)


def streaming_backward(dzn, zn, x, a, rnorm, mean, rstd, dtype=np.float64, defect=None):
    """One episode of dkt_normalize_bn_bwd: dzn, zn, x [N,D]; a [D]; rnorm [N]; mean, rstd [D] or None."""
    dzn, zn, x, a, rnorm = (np.asarray(v, dtype) for v in (dzn, zn, x, a, rnorm))
    mean, rstd = (None if v is None else np.asarray(v, dtype) for v in (mean, rstd))
    t = (zn * dzn).sum(1, dtype=dtype)
    dy = rnorm[:, None] * (dzn - zn * t[:, None])
    dyt = rnorm[:, None] * (np.abs(dzn) + np.abs(zn) * (np.abs(zn) * np.abs(dzn)).sum(1, dtype=dtype)[:, None])
    return _finish(dy, dyt, x, a, mean, rstd, dtype, defect, 32)


def run(case, dtype=np.float64, defect=None, split22=False):
    """Every episode of a case: a list of dict(dx, dgamma, dbeta)."""
    out = []
    for b in range(case["x"].shape[0]):
        ab = (lambda v: v if v.ndim == 1 else v[b])
        mean, rstd = (None, None) if case["mean"] is None else (case["mean"][b], case["rstd"][b])
        if case["call"] == "fused":
            g = None if case["g"] is None else case["g"][b]
            out.append(backward(case["w"][b], case["e"][b], case["x"][b], ab(case["a"]), ab(case["s"]), case["rnorm"][b], mean, rstd, g, dtype, defect, split22))
        else:
            out.append(streaming_backward(case["dzn"][b], case["zn"][b], case["x"][b], ab(case["a"]), case["rnorm"][b], mean, rstd, dtype, defect))
    return out


def rel_err(got, ref, scale=None):
    """max |got - ref| / max |ref| of one episode and quantity (element-wise, not a norm); a reference that is identically zero admits only zero."""
    err = float(np.abs(np.asarray(got, np.float64) - ref).max())
    scale = float(np.abs(ref).max()) if scale is None else scale
    if err == 0.0:
        return 0.0
    return err / scale if scale > 0.0 else float("inf")


TERM_SCALED = ("tiny-batch",)


def errors(got, ref, group=None):
    """Per quantity, the largest rel_err over the episodes of a case (`got`, `ref`: lists as `run` returns).  In the groups of TERM_SCALED the error is
    divided by the size of the quantity's terms before they cancel instead of max |ref| -- the same formulas evaluated on the absolute values of the
    operands the call receives (|a x| + |s| for y, (|x| + |mean|) rstd for xh, sums of absolute values for every product and reduction): with one row the
    fused call's true result is identically zero (E_00 = 1: dY = A zn - zn A; xh = 0), with two rows dX is a 1e-5 remainder, and an error relative to
    such a result measures the cancellation, not the kernel."""
    return {q: max(rel_err(gb[q], rb[q], rb["terms"][q] if group in TERM_SCALED else None) for gb, rb in zip(got, ref))
            for q in QUANTITIES if ref[0][q] is not None}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _relu_like(rng, b, n, d):
    """Trunk outputs as in tests/test_gpu_parity.py: non-negative, a large common offset per feature."""
    return np.abs(rng.standard_normal((b, n, d))) * rng.uniform(0.2, 3.0, (1, 1, d)) + rng.uniform(0.0, 5.0, (1, 1, d))


def _weights(rng, b, n, wkind):
    w = rng.standard_normal((b, n, n)) / n
    pre = None
    if wkind == "symmetric":                               # entries on a grid of 2^-16: the half-sum (W0 + W0^T) / 2 is exact in fp32; `w_pre` keeps W0
        pre = np.rint(w * 65536.0) / 65536.0
        w = 0.5 * (pre + pre.transpose(0, 2, 1))
    elif wkind == "triangular":
        w = np.triu(w, 1)
    elif wkind == "binades":                               # row i scaled by 2^(k_i), k_i cycling through -40 .. +20
        w = w * np.exp2(-40.0 + (np.arange(n) % 61))[None, :, None]
    elif wkind == "zero-row":
        z = n // 3
        w[:, z, :] = 0.0
        w[:, :, z] = 0.0
    return w, pre


def input_condition(case):
    """(smallest |y_i| / median_i |y_i| over the episodes, largest fp32 rnorm): the case list keeps the first >= 0.05 and the second far below 1e12."""
    worst = np.inf
    for b in range(case["x"].shape[0]):
        a, s = (v if v.ndim == 1 else v[b] for v in (case["a"], case["s"]))
        norms = np.linalg.norm(a * case["x"][b] + s, axis=1)
        worst = min(worst, float(norms.min() / np.median(norms)))
    return worst, float(case["rnorm"].max())


def make_case(call="fused", n=25, d=64, b=2, mode="train", scaled=False, xdtype="f32", wkind="plain", seed=0, rounded=True, group=None):
    """A case: float64 arrays holding fp32 values (X: values of `xdtype`).  mode: "train" (batch statistics, per-episode a / s and mean / rstd),
    "eval-shared" (one [D] a / s from the statistics pooled over the call, no mean / rstd) or "eval-episode" ([B,D] a / s, no mean / rstd).
    rounded=False leaves the forward quantities in float64 (the host test's comparison with autograd).  The seed is advanced until the input condition holds."""
    rnd = _r32 if rounded else (lambda v: np.asarray(v, np.float64))
    for attempt in range(64):
        rng = np.random.default_rng([seed, n, d, attempt])
        x = _rx(_relu_like(rng, b, n, d), xdtype)
        gamma, beta = rnd(rng.uniform(0.5, 1.5, d)), rnd(rng.normal(0.0, 0.2, d))
        if mode == "eval-shared":
            mean, rstd = x.reshape(-1, d).mean(0), 1.0 / np.sqrt(x.reshape(-1, d).var(0) + EPS)
        else:
            mean, rstd = x.mean(1), 1.0 / np.sqrt(x.var(1) + EPS)
        a = gamma * rstd
        s = beta - mean * a
        a, s, mean, rstd = rnd(a), rnd(s), rnd(mean), rnd(rstd)
        y = (a if a.ndim == 1 else a[:, None, :]) * x + (s if s.ndim == 1 else s[:, None, :])
        norms = np.linalg.norm(y, axis=2)
        if not (norms.min(1) >= 0.05 * np.median(norms, axis=1)).all():
            continue
        rnorm = 1.0 / np.maximum(norms, 1e-12)
        zn = y * rnorm[:, :, None]
        case = dict(call=call, n=n, d=d, b=b, mode=mode, scaled=scaled, xdtype=xdtype, wkind=wkind, group=group, x=x, gamma=gamma, beta=beta, a=a, s=s,
                    mean=mean if mode == "train" else None, rstd=rstd if mode == "train" else None, rnorm=rnd(rnorm),
                    g=rnd(np.linspace(-2.0, 1.0, b)) if scaled else None)
        if call == "fused":
            w, pre = _weights(rng, b, n, wkind)
            case.update(w=rnd(w), w_pre=None if pre is None else rnd(pre), e=rnd(zn @ zn.transpose(0, 2, 1)))
        else:
            case.update(zn=rnd(zn), dzn=rnd(rng.standard_normal((b, n, d))))
        return case
    raise AssertionError("no seed satisfies the input condition for %s" % ((call, n, d, b, mode, xdtype),))


# ---- the case list ----------------------------------------------------------------------------------------------------------------------------
TILE_EDGE_N = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128)
PER_NT_N = (13, 29, 45, 61, 77, 93, 109, 125)
MODES = ("train", "eval-shared", "eval-episode")


def case_specs():
    """name -> keyword arguments of make_case, `group` included.  Groups are the bullets of the case list; a batch of one or two rows is a group of its own:
    in train mode its result is what is left after a cancellation to (almost) nothing -- N = 1: E = [[1]], every output identically zero; N = 2:
    xh = +-(1 - eps / var), dX ~ 1e-5 dY -- so its fp32 floor relative to the result is orders of magnitude above that of every other N (or 0 / 0) and would
    blunt the bound of the whole group: these cases are measured against the size of the terms instead (`errors`)."""
    specs = {}

    def add(name, group, **kw):
        assert name not in specs, name
        specs[name] = dict(kw, group=group)

    for n in TILE_EDGE_N:
        add("tile-n%d" % n, "tiny-batch" if n <= 2 else "tile-edges", n=n, d=68)
    for n in PER_NT_N:
        for d in (4, 60, 64, 128, 132, 192):
            add("slab-n%d-d%d" % (n, d), "slab-edges", n=n, d=d)
    for n in (16, 29, 33, 61, 80, 96, 97, 112, 113, 128):   # (29 and 61: NT = 2 and 4, so that every NT is reached in eval mode too)
        for mode in MODES:
            for scaled in (False, True):
                add("mode-n%d-%s-%s" % (n, mode, "scaled" if scaled else "unscaled"), "modes", n=n, d=132, b=3, mode=mode, scaled=scaled)
    for xd in ("bf16", "f16"):
        for n in (17, 48, 81, 105, 128):
            for d in (68, 128):
                for mode in ("train", "eval-shared"):
                    add("x16-%s-n%d-d%d-%s" % (xd, n, d, mode), "x16", n=n, d=d, mode=mode, xdtype=xd)
    for n, d in ((45, 68), (105, 132)):
        for wkind in ("symmetric", "triangular", "binades", "zero-row"):
            add("w-%s-n%d" % (wkind, n), "w-structure", n=n, d=d, wkind=wkind, scaled=True)
    for n in (1, 31, 32, 33, 127, 128, 129, 160, 161, 320, 321, 1024):
        add("stream-n%d" % n, "stream-rows", call="stream", n=n, d=36)
    for d in (4, 28, 32, 64, 68):
        for mode in MODES:
            add("stream-d%d-%s" % (d, mode), "stream-slabs", call="stream", n=161, d=d, mode=mode)
    for xd in ("bf16", "f16"):
        add("stream-x16-%s" % xd, "stream-x16", call="stream", n=161, d=36, xdtype=xd)
    return specs


def instantiation(spec):
    """(NT, train, xdtype) of gram_bn_bwd_ep_kernel a fused case runs."""
    return (spec["n"] + 15) // 16, spec.get("mode", "train") == "train", spec.get("xdtype", "f32")


_built = {}


def build_reference():
    """dict(specs, cases, r64, r32, e32_case, e32): the cases, both runs of the model, the float32 floor per case and quantity and per group and quantity
    (the largest of its cases).  Built once per process."""
    if not _built:
        specs = case_specs()
        cases = {k: make_case(seed=i, **kw) for i, (k, kw) in enumerate(specs.items())}
        r64 = {k: run(c, np.float64) for k, c in cases.items()}
        # (TERM_SCALED groups: the 22-bit operands are modelled -- with one row the plain float32 run returns the exact zero, which no kernel that rounds can)
        r32 = {k: run(c, np.float32, split22=c["group"] in TERM_SCALED) for k, c in cases.items()}
        e32_case = {k: errors(r32[k], r64[k], c["group"]) for k, c in cases.items()}
        e32 = {}
        for k, c in cases.items():
            grp = e32.setdefault(c["group"], {})
            for q, v in e32_case[k].items():
                grp[q] = max(grp.get(q, 0.0), v)
        _built.update(specs=specs, cases=cases, r64=r64, r32=r32, e32_case=e32_case, e32=e32)
    return _built
