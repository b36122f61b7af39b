"""The launch geometry of the three wave-level marginal-likelihood kernels for N <= 127 -- mll_h2_kernel and mll_h2e_kernel (csrc/dkt_mll_h2.hip), mll_mfma_kernel
(csrc/dkt_mll_mfma.hip) -- restated in plain Python, the list of cases that walks it, and the float64 / float32 references of those cases.  No GPU and no
library is needed here: tests/test_mll_geometry_host.py checks this file against the built library's kernel list, tests/test_mll_geometry_gpu.py runs the cases.

`geometry()` restates the host arithmetic of mll_plan (csrc/dkt_mll.hip), launch_h2 (csrc/dkt_mll_h2.hip) and launch_mfma (csrc/dkt_mll_mfma.hip):
    NT = ceil((N + 1) / 16) tiles per side (the + 1: the augmented row), rounds = ceil(C / 5), wpg = ceil(C / rounds) waves per episode, EPW = 2 episodes per
    workgroup for NT <= 7 and 1 for NT = 8, grid = ceil(units / EPW); the wave-per-episode kernel runs one 64-thread workgroup per unit.
The PRODUCT library builds mll_mfma_kernel for the Cholesky output at N + 1 <= 32 only (dkt_mll_mfma_serves: larger requests take the generic kernel); the twins
library (-DDKT_TWINS, `force_f32mfma`) has it at every tile count.  The `chol` route therefore asks the product library up to N = 31 and the twins library, with
DKT_MLL_FORCE_F32MFMA next to DKT_MLL_WANT_CHOL, from N = 32 on -- the way test_mll_forward_and_gradients_vs_oracle reaches that kernel (path f32mfma)."""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import dkt_oracle as O

MAX_WPG = 5                      # dkt_wave_mll.h
MLL_H2_KAPPA_MAX = 5.0e3         # dkt_mll.hip: above it the generic kernel redoes the unit
H2E_MINB_NEVER = 1000000000      # DKT_MLL_H2E_MINB of the `default` route (as tests/test_gpu_parity.py sets it)
D = 24                           # columns of the random unit rows behind E

N_AXIS = (1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127)
C_AXIS = (1, 2, 3, 4, 5, 6, 9, 11, 32)
B_AXIS = (1, 2, 3)
ROUTES = ("default", "h2e", "per_class", "chol")
B_MAX = max(B_AXIS)

# The bounds of tests/test_gpu_parity.py for these kernels at these sizes (MLL_RTOL, GRAD_RTOL, and the alpha / chol figures of
# test_mll_forward_and_gradients_vs_oracle and test_mll_large_and_small_magnitude_base_matrices), restated: none is new.
MLL_RTOL = 1e-4
GRAD_RTOL = 1e-3
BOUNDS = dict(logp=MLL_RTOL, logp_max=MLL_RTOL, alpha=5e-4, chol=5e-5, w=GRAD_RTOL, dsv=GRAD_RTOL, dmean=GRAD_RTOL, dnoise=GRAD_RTOL)
OUTPUTS = ("logp", "alpha", "chol", "w", "dsv", "dmean", "dnoise")


def ceil_div(a: int, b: int) -> int:
    return (a + b - 1) // b


class Geometry(NamedTuple):
    family: str                  # h2 | h2e | mfma | generic (generic: not one of the three kernels; the product library's answer to want_chol at N >= 32)
    nt: int
    rounds: int                  # trips of the kernel's round loop (h2e: the class loop)
    wpg: int                     # waves per episode and round
    epw: int                     # episodes (units) per workgroup
    units: int                   # B, or B * C with per-class base matrices
    grid: int
    block: int                   # threads per workgroup
    partial_round: bool          # the last round has idle waves
    surplus_episode: bool        # the last workgroup has a unit slot beyond the batch
    instantiation: Optional[tuple]     # (kernel, NT, template booleans in the order of the template)


def geometry(n: int, c: int, b: int, per_class: bool, want_grad: bool, want_chol: bool, h2e_min_batch: int, twins: bool = False) -> Geometry:
    """What dkt_mll_f32 launches for B episodes of C class models on N <= 127 rows.  `twins`: the call carries DKT_MLL_FORCE_F32MFMA and goes to the twins library."""
    if not (1 <= n <= 127 and c >= 1 and b >= 1):
        raise ValueError("N in 1..127, C >= 1, B >= 1")
    if per_class and (want_chol or twins):
        raise ValueError("mll_plan: per-class base matrices combine with neither the Cholesky output nor the exact-fp32 request")
    nt = ceil_div(n + 1, 16)
    epw = 2 if nt <= 7 else 1
    units = b * c if per_class else b
    if want_chol or twins:                                   # dkt_mll_h2_serves() declines; dkt_mll_mfma_serves() decides
        if not twins and n + 1 > 32:
            return Geometry("generic", nt, 1, 1, 1, units, units, 256, False, False, None)
        rounds = ceil_div(c, MAX_WPG)
        wpg = ceil_div(c, rounds)
        inst = ("mll_mfma_kernel", nt, want_grad, want_chol, want_grad and wpg == 5)
        return Geometry("mfma", nt, ceil_div(c, wpg), wpg, epw, units, ceil_div(units, epw), 64 * wpg * epw, c % wpg != 0, epw == 2 and units % 2 == 1, inst)
    if nt <= 7 and (per_class or (want_grad and b >= h2e_min_batch)):
        # one wave per unit: every class in sequence (shared E), or one (episode, class) matrix each
        return Geometry("h2e", nt, 1 if per_class else c, 1, 1, units, units, 64, False, False, ("mll_h2e_kernel", nt))
    rounds = 1 if per_class else ceil_div(c, MAX_WPG)        # (NT = 8 with per-class matrices: one wave per workgroup, one workgroup per matrix)
    wpg = 1 if per_class else ceil_div(c, rounds)
    inst = ("mll_h2_kernel", nt, want_grad, want_grad and wpg == 5)
    return Geometry("h2", nt, 1 if per_class else ceil_div(c, wpg), wpg, epw, units, ceil_div(units, epw), 64 * wpg * epw,
                    (not per_class) and c % wpg != 0, epw == 2 and units % 2 == 1, inst)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    route: str
    n: int
    c: int
    b: int
    y_per_episode: bool          # targets [B,C,N] (a per-episode permutation of the rows) instead of [C,N]
    weighted: bool               # class weights of both signs with one zero (C >= 3), instead of None

    @property
    def per_class(self) -> bool:
        return self.route == "per_class"

    @property
    def want_chol(self) -> bool:
        return self.route == "chol"

    @property
    def twins(self) -> bool:
        """The chol route beyond what the product library builds mll_mfma_kernel for."""
        return self.route == "chol" and self.n + 1 > 32

    @property
    def h2e_min_batch(self) -> int:
        return 1 if self.route == "h2e" else H2E_MINB_NEVER

    @property
    def grads(self) -> tuple:
        """The want_grad settings the GPU test launches for this case: the h2e route is the training call alone (its forward-only call IS the default route's)."""
        return (True,) if self.route == "h2e" else (True, False)

    def geometry(self, want_grad: bool = True, b: Optional[int] = None) -> Geometry:
        return geometry(self.n, self.c, self.b if b is None else b, self.per_class, want_grad, self.want_chol, self.h2e_min_batch, self.twins)

    @property
    def name(self) -> str:
        return "%s-n%d-c%d-b%d%s%s" % (self.route, self.n, self.c, self.b, "-yb" if self.y_per_episode else "", "-cw" if self.weighted else "")


def route_ns(route: str) -> tuple:
    return tuple(n for n in N_AXIS if route != "h2e" or n <= 111)          # mll_h2e_kernel: NT <= 7


def cases_for(route: str, n: int) -> list:
    """One pytest parameter: every C at B = 3 (class weights on all but C = 2 and C = 6), B in {1, 2} at C in {5, 9} (the even batch and the one-episode
    workgroup next to the odd tail; C = 5 without class weights), per-episode targets at C in {1, 5, 11}."""
    out = [Case(route, n, c, 3, False, c not in (2, 6)) for c in C_AXIS]
    out += [Case(route, n, c, b, False, c == 9) for c in (5, 9) for b in (1, 2)]
    out += [Case(route, n, c, 3, True, c != 5) for c in (1, 5, 11)]
    return out


PARAMS = [(route, n) for n in N_AXIS for route in ROUTES if n in route_ns(route)]          # N-major: the routes of one N share inputs and references
ALL_CASES = [case for route, n in PARAMS for case in cases_for(route, n)]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------------
def _unit_gram(rng, n: int) -> np.ndarray:
    z = rng.standard_normal((n, D))
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    return (z @ z.T).astype(np.float32)          # float64 product, ONE rounding: the fp32 matrix both the kernel and the reference are given


@functools.lru_cache(maxsize=None)
def hypers(c: int) -> tuple:
    """(sv, mean, noise): sv in [0.7, 1.1], |mean| <= 0.1, noise in [0.1, 0.3], distinct per class, noise not monotone in the class index."""
    t = np.arange(c) / max(c - 1, 1)
    tn = (np.arange(c) * 7 % c) / max(c - 1, 1)          # (7 is coprime to every C of the axis)
    return ((0.7 + 0.4 * t).astype(np.float32), (-0.1 + 0.2 * t).astype(np.float32), (0.1 + 0.2 * tn).astype(np.float32))


def class_weights(c: int, n: int) -> np.ndarray:
    """Of the size of the training objective's -1 / (C N): negative on the even classes, positive and a quarter of that on the odd ones (so that the sum over
    the classes does not cancel), one exact zero from C = 3 on (class 0 at C = 3, class 1 above: never the last class, whose W the ragged round handles)."""
    k = np.arange(c)
    cw = np.where(k % 2 == 0, -1.0, 0.25) * (1.0 + 0.5 * k / c) / (c * n)
    if c >= 3:
        cw[0 if c == 3 else 1] = 0.0
    return cw.astype(np.float32)


# (N, C of a per-class set or 0) whose first draw made a case's own reference value too small for a RELATIVE bound -- another draw, never another bound.
# N = 95, shared E: episode 2 at C = 1 had dsv = 0.5 (alpha^T E alpha - tr K^-1 E) = -0.11 between two terms of ~ 30 (its neighbours: -5.6, -10.4), which
# float32 numpy itself resolves to 1.25e-3 only.
_SEED_SALT = {(95, 0): 1}


@functools.lru_cache(maxsize=8)
def _base(n: int, per_class_c: int) -> np.ndarray:
    """E for B_MAX episodes of size N: [B_MAX, N, N], or [B_MAX, C, N, N] (one matrix per class).  A case with fewer episodes takes the first ones, so the
    single-episode calls of the batch check see the batch's own matrices."""
    rng = np.random.default_rng(1000 * n + per_class_c + 500 * _SEED_SALT.get((n, per_class_c), 0))
    if per_class_c:
        return np.stack([np.stack([_unit_gram(rng, n) for _ in range(per_class_c)]) for _ in range(B_MAX)])
    return np.stack([_unit_gram(rng, n) for _ in range(B_MAX)])


def inputs(case: Case) -> dict:
    """fp32 numpy operands of ops.mll for the case: e, y, sv, mean, noise, cw (or None)."""
    n, c, b = case.n, case.c, case.b
    e = _base(n, c if case.per_class else 0)[:b]
    y = np.where(np.arange(n)[None, :] % c == np.arange(c)[:, None], 1.0, -1.0).astype(np.float32)          # [C,N]: +1 on the rows of the class
    if case.y_per_episode:
        rng = np.random.default_rng(77 * n + c)
        y = np.stack([y[:, rng.permutation(n)] for _ in range(B_MAX)])[:b]
    sv, mean, noise = hypers(c)
    return dict(e=e, y=y, sv=sv, mean=mean, noise=noise, cw=class_weights(c, n) if case.weighted else None)


def episode(x: dict, i: int) -> dict:
    """The operands of episode i alone (B = 1)."""
    return dict(x, e=x["e"][i:i + 1], y=x["y"][i:i + 1] if x["y"].ndim == 3 else x["y"])


def condition_bounds(case: Case) -> np.ndarray:
    """The a-priori bound 1 + sv trace(E) / noise the split kernels compare with MLL_H2_KAPPA_MAX, per (episode, class)."""
    x = inputs(case)
    tr = np.trace(x["e"].astype(np.float64), axis1=-2, axis2=-1)          # [B] or [B,C]
    tr = tr if case.per_class else tr[:, None]
    return 1.0 + x["sv"].astype(np.float64)[None, :] * tr / x["noise"].astype(np.float64)[None, :]


# ---- references ------------------------------------------------------------------------------------------------------------------------------------------
def _episode_class_loop(case: Case, x: dict, one_class):
    """Assemble the outputs in the kernels' layout from one_class(e [N,N], y [N], sv, mean, noise) -> (logp, alpha, chol, M = 0.5 (alpha alpha^T - K^-1), dsv, dmean, dnoise)."""
    n, c, b = case.n, case.c, case.b
    dt = x["e"].dtype
    out = dict(logp=np.zeros((b, c), dt), alpha=np.zeros((b, c, n), dt), chol=np.zeros((b, c, n, n), dt), w=np.zeros(x["e"].shape, dt),
               dsv=np.zeros((b, c), dt), dmean=np.zeros((b, c), dt), dnoise=np.zeros((b, c), dt))
    cw = np.ones(c, dt) if x["cw"] is None else x["cw"]
    for i in range(b):
        for k in range(c):
            e = x["e"][i, k] if case.per_class else x["e"][i]
            y = x["y"][i, k] if x["y"].ndim == 3 else x["y"][k]
            logp, alpha, chol, m, dsv, dmean, dnoise = one_class(e, y, x["sv"][k], x["mean"][k], x["noise"][k])
            out["logp"][i, k], out["alpha"][i, k], out["chol"][i, k] = logp, alpha, chol
            out["dsv"][i, k], out["dmean"][i, k], out["dnoise"][i, k] = dsv, dmean, dnoise
            if case.per_class:
                out["w"][i, k] = cw[k] * x["sv"][k] * m
            else:
                out["w"][i] += cw[k] * x["sv"][k] * m
    return out


def _one_class_oracle(e, y, sv, mean, noise):
    res = O.mll_terms(e, y[None, :], [sv], [mean], [noise])
    m, dsv, dmean, dnoise = O.mll_grads(e, res, [1.0], [noise], [1.0])          # (weight 1, sv 1: w_e IS 0.5 (alpha alpha^T - K^-1))
    assert res.jitter[0] == 0.0
    return res.logp[0], res.alpha[0], res.chol[0], m, dsv[0], dmean[0], dnoise[0]


def _one_class_f32(e, y, sv, mean, noise):
    """O.mll_terms / O.mll_grads line by line, every operand and every operation in float32."""
    import scipy.linalg as sla
    f = np.float32
    n = e.shape[0]
    eye = np.eye(n, dtype=f)
    k = sv * e + noise * eye
    l = np.linalg.cholesky(k)
    r = (y - mean).astype(f)
    w = sla.solve_triangular(l, r, lower=True).astype(f)
    a = sla.solve_triangular(l.T, w, lower=False).astype(f)
    quad, logdet = f(w @ w), f(2.0) * np.log(np.diag(l)).sum(dtype=f)
    logp = f(-0.5) * (quad + logdet + f(n * O.LOG_2PI))
    linv = sla.solve_triangular(l, eye, lower=True).astype(f)
    m = f(0.5) * (np.outer(a, a) - linv.T @ linv)
    assert l.dtype == f and m.dtype == f and a.dtype == f
    return logp, a, l, m, (m * e).sum(dtype=f), a.sum(dtype=f), np.trace(m, dtype=f)


@functools.lru_cache(maxsize=96)
def _reference(key: Case) -> dict:
    x = inputs(key)
    x64 = {k: (None if v is None else v.astype(np.float64)) for k, v in x.items()}
    return _episode_class_loop(key, x64, _one_class_oracle)


@functools.lru_cache(maxsize=96)
def _reference32(key: Case) -> dict:
    return _episode_class_loop(key, inputs(key), _one_class_f32)


def _data_key(case: Case) -> Case:
    """default, h2e and chol see the same operands: one reference for the three."""
    return case._replace(route="per_class" if case.per_class else "default")


def reference(case: Case) -> dict:
    """float64 (oracle.dkt_oracle.mll_terms / mll_grads per episode and class) on the fp32 operands of the case: logp [B,C], alpha [B,C,N], chol [B,C,N,N], w in
    the layout of E (with the class weights; summed over the classes for a shared E), dsv / dmean / dnoise [B,C] (without them, as the kernels write them).
    Shared between the tests: treat as read-only."""
    return _reference(_data_key(case))


def reference32(case: Case) -> dict:
    """The same formulas in numpy float32."""
    return _reference32(_data_key(case))


# ---- the bounds -------------------------------------------------------------------------------------------------------------------------------------------
def rel_l2(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def fractions(case: Case, out: dict, want_grad: bool = True, want_chol: Optional[bool] = None) -> dict:
    """The fraction of each bound of BOUNDS that `out` (numpy arrays under the names of OUTPUTS) uses against reference(case), worst episode: logp per class
    (relative) and in max norm per episode, alpha / dsv / dmean / dnoise as rel-L2 per episode, chol per episode, w per matrix of its layout -- what
    test_mll_forward_and_gradients_vs_oracle asserts.  A non-finite output gives inf."""
    ref = reference(case)
    want_chol = case.want_chol if want_chol is None else want_chol
    fr = {}

    def put(key, err):
        err = float(err) if np.isfinite(err) else float("inf")
        fr[key] = max(fr.get(key, 0.0), err / BOUNDS[key])

    for i in range(case.b):
        lp, lr = np.asarray(out["logp"][i], np.float64), ref["logp"][i]
        put("logp", np.abs((lp - lr) / lr).max())
        put("logp_max", np.abs(lp - lr).max() / np.abs(lr).max())
        put("alpha", rel_l2(out["alpha"][i], ref["alpha"][i]))
        if want_chol:
            put("chol", rel_l2(out["chol"][i], ref["chol"][i]))
        if want_grad:
            for k in (range(case.c) if case.per_class else (None,)):
                put("w", rel_l2(out["w"][i] if k is None else out["w"][i, k], ref["w"][i] if k is None else ref["w"][i, k]))
            for key in ("dsv", "dmean", "dnoise"):
                put(key, rel_l2(out[key][i], ref[key][i]))
    return fr


def measured_line(case: Case, want_grad: bool, kernel_fr: dict, f32_fr: dict) -> str:
    g = case.geometry(want_grad)
    keys = [k for k in BOUNDS if k in kernel_fr]
    return "MEASURED mll_geometry %s %s [%s NT %d rounds %d wpg %d EPW %d grid %d]: kernel %s of the bound; float32 numpy %s" % (
        case.name, "grad" if want_grad else "fwd", g.family, g.nt, g.rounds, g.wpg, g.epw, g.grid,
        " ".join("%s %.2g" % (k, kernel_fr[k]) for k in keys), " ".join("%s %.2g" % (k, f32_fr[k]) for k in keys))


# ---- seeded mistakes: what a wrong kernel would write, applied to a correct result ----------------------------------------------------------------------
def _copy(out: dict) -> dict:
    return {k: np.array(v, copy=True) for k, v in out.items()}


def seed_last_class_w_twice(case: Case, out: dict) -> dict:
    """W of the last class (the last wave of a ragged round) added twice."""
    ref, x, o = reference32(case), inputs(case), _copy(out)
    k = case.c - 1
    cw = 1.0 if x["cw"] is None else x["cw"][k]
    for i in range(case.b):
        a = ref["alpha"][i, k].astype(np.float64)
        l = ref["chol"][i, k].astype(np.float64)
        linv = np.linalg.inv(l)
        tgt = o["w"][i, k] if case.per_class else o["w"][i]
        tgt += (cw * x["sv"][k] * 0.5 * (np.outer(a, a) - linv.T @ linv)).astype(o["w"].dtype)
    return o


def seed_last_episode_over_previous(case: Case, out: dict) -> dict:
    """The clamped unit index of a surplus half-workgroup writing: the last episode's outputs land on the one before it."""
    o = _copy(out)
    for k in o:
        o[k][case.b - 2] = o[k][case.b - 1]
    return o


def seed_round2_alpha_from_round1(case: Case, out: dict) -> dict:
    """alpha of the second round's classes left at what the same waves wrote in round 1."""
    o, wpg = _copy(out), case.geometry().wpg
    for k in range(wpg, min(2 * wpg, case.c)):
        o["alpha"][:, k] = o["alpha"][:, k - wpg]
    return o
