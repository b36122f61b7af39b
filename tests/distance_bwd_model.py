"""CPU restatement of the distance-kernel backward -- `dkt_rbf_bwd_f32` / `dkt_sqdist_bwd_f32` (rbf_bwd_kernel, sqdist_bwd_kernel of csrc/dkt_gram.hip) and the
chain gram(z, RBF | SQDIST) -> ... -> rbf_bwd | sqdist_bwd -> gram_bwd(Wp, z) that `ops.base_matrix` / `ops.base_matrix_per_class` run under autograd --
with the bounds and the case lists that tests/test_distance_bwd_host.py (CPU) and tests/test_distance_bwd_gpu.py (GPU) share.

The two kernels, one episode; W = d obj / d E (any matrix, not symmetric in general), E or U the forward's fp32 output, l the lengthscale:

    Ws = (W + W^T) / 2
    RBF     A = -Ws o E / l^2     Wp = diag(A 1) - A     dl = sum_ij Ws o E o (-2 ln E) / l          (0 ln 0 := 0;  -2 ln E = d2 / l^2)
    SQDIST  A = 2 Ws / l^2        Wp = diag(A 1) - A     dl = -2 sum_ij Ws o U / l
    dz = gram_bwd(Wp, z) = (Wp + Wp^T) z = 2 Wp z

`*_ref` evaluate these in float64 ON THE fp32 INPUTS (E / U is an input, never recomputed from z): the reference of the kernel's own operation.
`*_f32` restate them in float32 numpy in the kernel's order of operations.

Bounds (u = 2^-24, the fp32 unit roundoff; every fp32 operation rounds once, relative error <= u; `bounds()` returns them)

  off-diagonal Wp_ij = -a_ij.  ws = 0.5 (W_ij + W_ji): one rounding (the halving is exact).  ws e: one.  inv_l2 = 1 / (l l): the product rounds once,
      the division is allowed 3 u (1.5 units in the last place).  (ws e) inv_l2: one.  (SQDIST: 2 ws inv_l2, one rounding fewer.)  In all <= 7 u, with the
      second-order terms  |Wp_ij - ref| <= 8 u |Ws_ij E_ij| / l^2  (SQDIST: 8 u |2 Ws_ij| / l^2)  + DENORM (1 + 1 / l^2)   -- `off`.
      DENORM = 2^-126 covers a product that lands in (or is flushed from) the subnormal range, where roundings are absolute.
  diagonal Wp_ii = (a_i0 + a_i1 + ... + a_i,N-1) - a_ii: the kernel adds the N terms of row i one after the other (the diagonal term included) and
      subtracts a_ii, which it recomputes bit-identically (0.5 (W_ii + W_ii) = W_ii exactly): N additions of numbers bounded by the running sum of |a_ij|,
      each rounding once, on terms that carry 7 u each:  |Wp_ii - ref| <= (N + 9) u sum_j |a_ij| + N DENORM (1 + 1 / l^2)   -- `diag` (per row; j runs
      over the whole row, j = i included).  An fma contraction of `rowsum += a` only removes roundings.  The same bound holds for |Wp 1|_i (the row sum
      of the returned matrix, true value 0): it is the same N-term sum minus the stored, once-more-rounded terms.
  dl[b].  One term t_ij = ws e (-2 logf(e)): ws one rounding, ws e one, logf LOGF_ULPS = 2 units in the last place = 4 u (the device library documents
      1), the doubling exact, the product one: 3 + 2 LOGF_ULPS = 7 u.  (SQDIST: t_ij = ws U_ij, 2 u.)  A thread owns the rows tid, tid + 256, ...:
      T = ceil(N / 256) rows of N terms added one after the other, T N roundings on partial sums bounded by the thread's sum of |t|; block_sum_256 adds
      6 shuffle levels and 3 additions of the four wave sums: depth 9; the division by l (and SQDIST's exact -2) one more:
          |dl - ref| <= (T N + 9 + 1 + 3 + 2 LOGF_ULPS + 1) u sum_ij |t_ij| / l + N^2 DENORM 256 / l   -- `dl` (one number per episode).
      (256 DENORM: |2 ln e| < 256 for every positive fp32 e.)

`chain_ref` is float64 torch autograd of sum G o K(z, l) through oracle.dkt_oracle_torch.base_matrix on the fp32-rounded z, `chain_f32` the same autograd in
float32 with the kernels' formula (rows shifted by row 0, d2 = |a|^2 + |b|^2 - 2 a.b clamped at 0, zero diagonal): its distance from `chain_ref` is the
fp32 floor the GPU test scales its second bound from."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import dkt_oracle_torch as OT  # noqa: E402

U32 = 2.0 ** -24
DENORM = 2.0 ** -126
LOGF_ULPS = 2
THREADS = 256
GRAD_RTOL = 1e-3            # the project's gradient tolerance (tests/test_gpu_parity.py)
FLOOR_MARGIN, FLOOR_MIN = 4.0, 1e-6

f32 = np.float32


def r32(v):
    """float64 array holding the fp32 rounding of v."""
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


# ---- the two kernels, float64 on the fp32 inputs ----------------------------------------------------------------------------------------------------
def _wp(a):
    wp = -a
    idx = np.arange(a.shape[-1])
    wp[..., idx, idx] = a.sum(-1) - a[..., idx, idx]
    return wp


def _neg2_log(e):
    """-2 ln e with 0 ln 0 := 0 (the kernel's `if (e > 0.f)`)."""
    pos = e > 0
    return np.where(pos, -2.0 * np.log(np.where(pos, e, 1.0)), 0.0)


def rbf_bwd_ref(w, e, l):
    """w, e: [B,N,N]; l scalar.  -> (Wp [B,N,N], dl [B]) in float64."""
    w, e, l = np.asarray(w, np.float64), np.asarray(e, np.float64), float(l)
    ws = 0.5 * (w + w.transpose(0, 2, 1))
    return _wp(-ws * e / l ** 2), (ws * e * _neg2_log(e)).sum((1, 2)) / l


def sqdist_bwd_ref(w, u, l):
    w, u, l = np.asarray(w, np.float64), np.asarray(u, np.float64), float(l)
    ws = 0.5 * (w + w.transpose(0, 2, 1))
    return _wp(2.0 * ws / l ** 2), -2.0 * (ws * u).sum((1, 2)) / l


def bounds(kind, w, m, l):
    """(off [B,N,N], diag [B,N], dl [B]) of the module docstring for the call kind ("rbf": m = E, "sqdist": m = U)."""
    w, m, l = np.asarray(w, np.float64), np.asarray(m, np.float64), float(l)
    n = w.shape[-1]
    ws = 0.5 * (w + w.transpose(0, 2, 1))
    if kind == "rbf":
        a, t, term = np.abs(ws * m) / l ** 2, np.abs(ws * m * _neg2_log(m)), 3 + 2 * LOGF_ULPS
    else:
        a, t, term = np.abs(2.0 * ws) / l ** 2, 2.0 * np.abs(ws * m), 2
    rows = (n + THREADS - 1) // THREADS
    off = 8.0 * U32 * a + DENORM * (1.0 + 1.0 / l ** 2)
    diag = (n + 9) * U32 * a.sum(-1) + n * DENORM * (1.0 + 1.0 / l ** 2)
    dl = (rows * n + 9 + 1 + term + 1) * U32 * t.sum((1, 2)) / l + n * n * DENORM * 256.0 / l
    return off, diag, dl


# ---- the same in float32, in the kernel's order -----------------------------------------------------------------------------------------------------
def _block_sum_256(part):
    """part [256] fp32 -> wave_sum (v += shfl_down(v, o), o = 32 .. 1: lane 0 holds the tree sum) of the four waves, then red[0] + red[1] + red[2] + red[3]."""
    v = part.reshape(4, 64).copy()
    o = 32
    while o:
        v[:, :o] = v[:, :o] + v[:, o:2 * o]
        o >>= 1
    return f32(f32(f32(v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0])


def _thread_partials(t):
    """t [N,N] fp32 terms -> [256]: thread tid adds the terms of rows tid, tid + 256, ... one after the other (np.cumsum accumulates sequentially)."""
    n = t.shape[0]
    rows = (n + THREADS - 1) // THREADS
    pad = np.zeros((rows * THREADS, n), f32)          # (adding an exact zero changes nothing)
    pad[:n] = t
    seq = pad.reshape(rows, THREADS, n).transpose(1, 0, 2).reshape(THREADS, rows * n)
    return np.cumsum(seq, axis=1, dtype=f32)[:, -1]


def _bwd_f32(kind, w, m, l):
    w, m, l = np.asarray(w, f32), np.asarray(m, f32), f32(l)
    b, n, _ = w.shape
    inv_l2 = f32(1.0) / f32(l * l)
    wp, dl = np.empty_like(w), np.empty(b, f32)
    idx = np.arange(n)
    for i in range(b):
        ws = f32(0.5) * (w[i] + w[i].T)
        if kind == "rbf":
            a = -(ws * m[i]) * inv_l2
            # (the float64 logarithm rounded once: within half a unit in the last place, whatever the host's libm)
            t = (ws * m[i]) * _neg2_log(m[i].astype(np.float64)).astype(f32)
        else:
            a = (f32(2.0) * ws) * inv_l2
            t = ws * m[i]
        rowsum = np.cumsum(a, axis=1, dtype=f32)[:, -1]
        wp[i] = -a
        wp[i][idx, idx] = rowsum - a[idx, idx]
        tot = _block_sum_256(_thread_partials(t))
        dl[i] = tot / l if kind == "rbf" else f32(-2.0) * tot / l
    return wp, dl


def rbf_bwd_f32(w, e, l):
    return _bwd_f32("rbf", w, e, l)


def sqdist_bwd_f32(w, u, l):
    return _bwd_f32("sqdist", w, u, l)


def fractions(kind, wp, dl, w, m, l):
    """Largest fraction of each bound that (wp, dl) uses against the float64 reference: dict(off, diag, dl, rowsum, finite)."""
    wp, dl = np.asarray(wp, np.float64), np.asarray(dl, np.float64)
    rwp, rdl = (rbf_bwd_ref if kind == "rbf" else sqdist_bwd_ref)(w, m, l)
    off, diag, dlb = bounds(kind, w, m, l)
    n = wp.shape[-1]
    idx = np.arange(n)
    err = np.abs(wp - rwp)
    eo = err / off
    eo[:, idx, idx] = 0.0
    return dict(off=float(eo.max()), diag=float((err[:, idx, idx] / diag).max()), dl=float((np.abs(dl - rdl) / dlb).max()),
                rowsum=float((np.abs(wp.sum(-1)) / diag).max()), finite=bool(np.isfinite(wp).all() and np.isfinite(dl).all()))


# ---- inputs of the kernel-alone cases ---------------------------------------------------------------------------------------------------------------
KERNEL_N = (1, 2, 19, 33, 63, 255, 256, 257, 450, 513)
KERNEL_B = (1, 3)
KERNEL_L = (0.05, 1.1, 30.0)
EDGE_N = (33, 257)


def kernel_case(kind, n, b, l, seed=0):
    """dict(kind, w, m, l) in fp32: W random and NOT symmetric, different data in every episode; U random symmetric with a zero diagonal, E = exp(-U / 2)."""
    rng = np.random.default_rng([seed, n, b, int(l * 100), kind == "rbf"])
    w = rng.standard_normal((b, n, n)) / n
    u = np.abs(rng.standard_normal((b, n, n))) * rng.uniform(0.5, 4.0, (b, 1, 1))
    u = np.triu(u, 1)
    u = u + u.transpose(0, 2, 1)
    m = np.exp(-0.5 * u) if kind == "rbf" else u
    return dict(kind=kind, w=w.astype(f32), m=m.astype(f32), l=f32(l))


def edge_case(n, l, seed=0):
    """RBF, B = 3.  Episode 0: off-diagonal entries that underflowed to exactly 0, one subnormal entry, off-diagonal entries exactly 1 (duplicate rows);
    episode 1: as kernel_case; episode 2: every entry in [1 - 1e-4, 1] (l large against every distance)."""
    c = kernel_case("rbf", n, 3, l, seed + 7)
    e = c["m"]

    def put(ep, i, j, v):
        e[ep, i, j] = e[ep, j, i] = v

    for k in range(0, n - 1, 3):
        put(0, k, (k + 5) % n if (k + 5) % n != k else k + 1, 0.0)
    put(0, 1, n - 1, f32(1e-40))
    for k in range(2, n - 2, 7):
        put(0, k, k + 2, 1.0)
    put(0, 0, n - 2, 1.0)
    rng = np.random.default_rng([seed, n, 99])
    near = np.triu(1.0 - rng.uniform(0.0, 1e-4, (n, n)), 1)
    e[2] = (near + near.T + np.eye(n)).astype(f32)
    assert (e == e.transpose(0, 2, 1)).all() and (e[0] == 0).sum() >= 2 and ((e[0] > 0) & (e[0] < 1e-38)).sum() == 2 and e[2].min() >= f32(1.0 - 1e-4)
    assert ((e[0] == 1).sum() - n) >= 4
    return c


def kernel_cases():
    """name -> case of the kernel-alone group (a): every (kind, N, B, l), then the edge group."""
    out = {}
    for kind in ("rbf", "sqdist"):
        for n in KERNEL_N:
            for b in KERNEL_B:
                for l in KERNEL_L:
                    out["%s-n%d-b%d-l%g" % (kind, n, b, l)] = kernel_case(kind, n, b, l)
    for n in EDGE_N:
        for l in KERNEL_L:
            out["rbf-edge-n%d-l%g" % (n, l)] = edge_case(n, l)
    return out


# ---- the chain through autograd ---------------------------------------------------------------------------------------------------------------------
# (B, N, D) -> (forward route of dkt_gram_f32 kind RBF / SQDIST, backward route of dkt_gram_bwd_f32 with no flag set), read off the *_launch conditions:
#   forward   small    dkt_gram_small_launch:    N <= 32 and D % 4 == 0 (RBF: rows beyond sixteen on the VALU at 17 <= N <= 20, a workgroup per task from
#                                                D >= 2048 at N > 16; SQDIST: always a wave per task, MFMA tiles)
#             dist-ep  dkt_gram_dist_ep_launch:  32 < N <= 128, D % 4 == 0, B >= 64
#             generic  gram_nt_kernel<KIND, true>: everything else (64 x 64 tiles)
#   backward  small    dkt_gram_small_bwd_launch: N <= 32 and D % 4 == 0 (a workgroup per task from D >= 1024)
#             ep<NT>   dkt_gram_bwd_ep_launch:   64 < N <= 128, D % 4 == 0, B >= 32: launch_bwd<ceil(N / 16)>, exact-fp32 MFMA below D = 1024, the 3-way bf16
#                                                split from there (rows of any norm: no DKT_GRAM_UNIT_ROWS)
#             generic  gram_bwd_kernel:          everything else (dkt_gram_bwd_big_launch needs both flags, which this chain never sets)
CHAIN_SHAPES = {
    (3, 1, 8): ("small <K,1,0>", "small wave/task"),
    (5, 16, 64): ("small <K,1,0>", "small wave/task"),
    (5, 17, 64): ("small, RBF rows 17.. on the VALU (XR 3)", "small wave/task"),
    (3, 19, 2916): ("small, RBF workgroup/task + XR 3; SQDIST wave/task", "small workgroup/task"),
    (4, 20, 2052): ("small, RBF workgroup/task + XR 4; SQDIST wave/task", "small workgroup/task"),
    (3, 32, 36): ("small <K,2,0>", "small wave/task"),
    (2, 19, 30): ("generic (D % 4 != 0)", "generic (D % 4 != 0)"),
    (2, 33, 64): ("generic (B < 64), one tile", "generic, one tile"),
    (64, 33, 32): ("dist-ep NT 3", "generic"),
    (64, 64, 36): ("dist-ep NT 4", "generic (N <= 64)"),
    (32, 100, 64): ("generic (B < 64), 2 x 2 tiles", "ep<7> exact fp32"),
    (64, 65, 64): ("dist-ep NT 5", "ep<5> exact fp32"),
    (64, 90, 32): ("dist-ep NT 6", "ep<6> exact fp32"),
    (64, 128, 64): ("dist-ep NT 8", "ep<8> exact fp32"),
    (64, 100, 1024): ("dist-ep NT 7", "ep<7> bf16 x 3 split"),
    (2, 129, 36): ("generic, 3 x 3 tiles", "generic"),
    (1, 257, 30): ("generic, D % 4 != 0", "generic; rbf_bwd: two rows per thread"),
    (1, 450, 16): ("generic", "generic; rbf_bwd: two rows per thread"),
}
CHAIN_VARIANTS = (("rbf", False), ("matern", False), ("rbf", True), ("matern", True))     # (kernel, one lengthscale per class)
N_CLASS = 3


def routes(b, n, d):
    """(forward, backward) route names from the launch conditions above -- the host test checks CHAIN_SHAPES against it."""
    v4 = d % 4 == 0
    fwd = "small" if (n <= 32 and v4) else "dist-ep" if (32 < n <= 128 and v4 and b >= 64) else "generic"
    bwd = "small" if (n <= 32 and v4) else ("ep<%d>" % ((n + 15) // 16)) + (" bf16" if d >= 1024 else " exact") if (64 < n <= 128 and v4 and b >= 32) else "generic"
    return fwd, bwd


def chain_inputs(b, n, d, per_class=False, scale=1.0, plain=False, seed=0):
    """dict(z [B,N,D], l ([1] or [C]), g ([B,N,N] or [B,C,N,N])) as float64 arrays of fp32 values.  ReLU-like features with a common offset, distances of
    the order of l; in every episode one pair of duplicate rows (N >= 4) and one far outlier row (N >= 3: d2 / l^2 ~ 36 from the others), unless `plain`;
    a different G in every episode, not symmetric."""
    rng = np.random.default_rng([seed, b, n, d, int(per_class)])
    z = np.abs(rng.standard_normal((b, n, d))) * 0.3 + rng.uniform(0.0, 2.0, (1, 1, d))
    l = 1.7 * math.sqrt(d) * 0.3
    if not plain:
        for i in range(b):
            if n >= 3:
                z[i, (2 * i + 1) % n] += 6.0 * l / math.sqrt(d)
            if n >= 4:
                z[i, (2 * i + 3) % n] = z[i, (2 * i) % n]
    ls = l * np.array([0.7, 1.0, 1.6]) if per_class else np.array([l])
    g = rng.standard_normal((b, N_CLASS, n, n) if per_class else (b, n, n)) / n
    return dict(z=r32(z * scale), l=r32(ls * scale), g=r32(g))


def chain_ref(z, g, kernel, l):
    """float64 autograd of sum_b sum G o K(z_b, l) through the oracle's base_matrix.  -> (dz [B,N,D], dl like l) as numpy float64."""
    zt = torch.tensor(np.asarray(z, np.float64), requires_grad=True)
    lt = torch.tensor(np.asarray(l, np.float64), requires_grad=True)
    gt = torch.tensor(np.asarray(g, np.float64))
    total = 0.0
    for b in range(zt.shape[0]):
        if gt.dim() == 4:
            for c in range(lt.numel()):
                total = total + (gt[b, c] * OT.base_matrix(zt[b], None, kernel, lt[c])).sum()
        else:
            total = total + (gt[b] * OT.base_matrix(zt[b], None, kernel, lt[0])).sum()
    total.backward()
    return zt.grad.numpy(), lt.grad.numpy()


def _d2_shifted(zt):
    """Squared distances as the kernels form them (any dtype): rows shifted by row 0, norm expansion, clamp at 0, zero diagonal."""
    zs = zt - zt[:, :1]
    nrm = (zs * zs).sum(-1)
    d2 = (nrm[:, :, None] + nrm[:, None, :] - 2.0 * zs @ zs.transpose(1, 2)).clamp_min(0.0)
    return d2 * (1.0 - torch.eye(zt.shape[1], dtype=zt.dtype))


def _map(d2, lt, kernel, per_class):
    u = d2.unsqueeze(1) / lt.reshape(1, -1, 1, 1) ** 2 if per_class else d2 / lt.reshape(()) ** 2
    if kernel == "matern":
        r = torch.sqrt(5.0 * u.clamp_min(1e-30))
        return (1.0 + r + r * r / 3.0) * torch.exp(-r)
    return torch.exp(-0.5 * u)


def _forward_f32(zt, lt, kernel, per_class):
    """The kernels' formula in torch (any dtype; float32 here)."""
    return _map(_d2_shifted(zt), lt, kernel, per_class)


def chain_terms(z, g, kernel, l):
    """T[b,d] = sum_ij 2 |a_ij| (|z_jd| + |z_id|), a = H + H^T with H = d obj / d d2 (float64): the size of the terms 2 Wp_ij z_jd whose sum over i and j is
    sum_i dz_id = 0, the diagonal of Wp counted through the terms it is the sum of (|Wp_ii| <= sum_j |a_ij|, and that is what its rounding error scales with)."""
    zt, lt, gt = (torch.tensor(np.asarray(v, np.float64)) for v in (z, l, g))
    d2 = _d2_shifted(zt).requires_grad_(True)
    (gt * _map(d2, lt, kernel, gt.dim() == 4)).sum().backward()
    a = np.abs(d2.grad.numpy() + d2.grad.numpy().transpose(0, 2, 1))
    az = np.abs(np.asarray(z, np.float64))
    return 2.0 * (np.einsum("bij,bjd->bd", a, az) + np.einsum("bij,bid->bd", a, az))


def chain_f32(z, g, kernel, l):
    """The same autograd in float32 on the CPU with the kernels' formula.  -> (dz, dl) as numpy float64 holding fp32 values."""
    zt = torch.tensor(np.asarray(z), dtype=torch.float32, requires_grad=True)
    lt = torch.tensor(np.asarray(l), dtype=torch.float32, requires_grad=True)
    gt = torch.tensor(np.asarray(g), dtype=torch.float32)
    (gt * _forward_f32(zt, lt, kernel, gt.dim() == 4)).sum().backward()
    return zt.grad.double().numpy(), lt.grad.double().numpy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b))


def identity_residuals(z, l, dz, dl, terms):
    """The two identities on a (dz, dl) pair, evaluated in float64; returns (sum-to-zero residual / bound, the same / N u sum_i |dz_id|, homogeneity
    residual / bound).

    1. sum_i dz_id = 0 per episode and feature (K depends on differences of rows only).  dz_id = sum_j 2 Wp_ij z_jd: gram_bwd adds N terms per element
       (N roundings on partial sums bounded by sum_j |2 Wp_ij z_jd|) of a Wp whose entries carry 8 u and whose diagonal (N + 9) u sum_j |a_ij|, so
       |sum_i dz_id| <= (2 N + 9) u T_bd with T = `terms` (chain_terms: the terms with their absolute values).  gram_bwd does not shift the rows, so with
       features that share an offset the terms are several times larger than the dz_id they cancel to: N u sum_i |dz_id| -- the second number, printed
       next to the first -- is NOT a bound of the computation (the fp32 CPU autograd stays near 0.05 of it, the kernels reach 0.1 .. 1.4).
    2. sum_c l_c dl_c + sum_b <z_b - r_b, dz_b> = 0 for any rows r_b (K depends on z / l only; r_b = row 0: by 1. the choice of r does not matter),
       against N u (sum |z - r| o |dz| + sum_c |l_c dl_c|): one N-term fp32 sum of the terms whose true total is zero."""
    z, l, dz, dl = (np.asarray(v, np.float64) for v in (z, l, dz, dl))
    n = z.shape[1]
    tot, nz = np.abs(dz.sum(1)), terms > 0
    assert (tot[~nz] == 0).all()
    r1 = float((tot[nz] / ((2 * n + 9) * U32 * terms[nz])).max()) if nz.any() else 0.0
    sz = np.abs(dz).sum(1)
    r1_dz = float((tot[sz > 0] / (n * U32 * sz[sz > 0])).max()) if (sz > 0).any() else 0.0
    zr = z - z[:, :1]
    res = (l.reshape(-1) * dl.reshape(-1)).sum() + (zr * dz).sum()
    scale = n * U32 * ((np.abs(zr) * np.abs(dz)).sum() + np.abs(l.reshape(-1) * dl.reshape(-1)).sum())
    return r1, r1_dz, (float(abs(res) / scale) if scale > 0 else float(abs(res)))


_chain = {}


def chain_reference(shape, kernel, per_class):
    """dict(inp, dz64, dl64, dz32, dl32, e32_dz, e32_dl, terms) of one chain case, computed once per process."""
    key = (shape, kernel, per_class)
    if key not in _chain:
        inp = chain_inputs(*shape, per_class=per_class)
        dz64, dl64 = chain_ref(inp["z"], inp["g"], kernel, inp["l"])
        dz32, dl32 = chain_f32(inp["z"], inp["g"], kernel, inp["l"])
        _chain[key] = dict(inp=inp, dz64=dz64, dl64=dl64, dz32=dz32, dl32=dl32, e32_dz=rel_l2(dz32, dz64), e32_dl=rel_l2(dl32, dl64),
                           terms=chain_terms(inp["z"], inp["g"], kernel, inp["l"]))
    return _chain[key]


# ---- the small-distance regime of dlengthscale ------------------------------------------------------------------------------------------------------
SMALL_SHAPES = ((3, 19, 2916), (2, 105, 64))
SMALL_TARGETS = (1.0, 1e-2, 1e-4, 1e-6)


def small_distance_case(shape, target, seed=3):
    """Plain chain inputs (no duplicate, no outlier) with the features scaled so that the largest d2 / l^2 of the call is `target`."""
    inp = chain_inputs(*shape, plain=True, seed=seed)
    z, l = inp["z"], float(inp["l"][0])
    d2 = ((z[:, :, None, :] - z[:, None, :, :]) ** 2).sum(-1).max()
    inp["z"] = r32(z * math.sqrt(target / (d2 / l ** 2)))
    return inp


def qmul_case():
    """The scale of the QMUL head: features of make_golden.cfg0_features and the lengthscale of tests/golden/cfg0_qmul_regression_rbf.npz."""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    if gold not in sys.path:
        sys.path.insert(0, gold)
    from make_golden import cfg0_features
    g = np.load(os.path.join(gold, "cfg0_qmul_regression_rbf.npz"))
    z, _ = cfg0_features(int(g["seed"]), int(g["n"]), int(g["d"]))
    rng = np.random.default_rng(11)
    n = z.shape[0]
    return dict(z=r32(z[None]), l=r32(np.array([float(g["lengthscale"])])), g=r32(rng.standard_normal((1, n, n)) / n))


def dl_three_ways(inp, e32=None):
    """RBF dlengthscale of a case: dict(ref, formula32, homog32, umax) -- float64; the fp32 restatement of the kernel's formula, the logarithm of the ROUNDED
    E (rbf_bwd_f32), on `e32` -- the fp32 E the kernel itself was given (the GPU test passes the forward's output, so that the restatement and the kernel
    differ in the order of their sums only) or, by default, the fp32 forward restated on the CPU; the fp32 restatement of dl = -<z - r, dz> / l (dz of chain_f32)."""
    z, l, g = inp["z"], inp["l"], inp["g"]
    _, dl64 = chain_ref(z, g, "rbf", l)
    if e32 is None:
        with torch.no_grad():
            e32 = _forward_f32(torch.tensor(z, dtype=torch.float32), torch.tensor(l, dtype=torch.float32), "rbf", False).numpy()
    e32 = np.asarray(e32, f32)
    _, dlb = rbf_bwd_f32(g.astype(f32), e32, f32(l[0]))
    dz32, _ = chain_f32(z, g, "rbf", l)
    z32 = z.astype(f32)
    hom = -np.sum((z32 - z32[:, :1]) * dz32.astype(f32), dtype=f32) / f32(l[0])
    umax = float(_neg2_log(e32.astype(np.float64)).max())
    return dict(ref=float(dl64[0]), formula32=float(np.sum(dlb, dtype=f32)), homog32=float(hom), umax=umax)
