"""CPU restatement of the per-class kernel maps and their chain rule -- `dkt_class_kernel_f32` / `dkt_class_kernel_bwd_f32` (class_kernel_fwd, class_kernel_bwd,
class_kernel_bwd_n128, class_kernel_bwd_v4 of csrc/dkt_classkernel.hip) -- with the bounds, the route table and the case lists that
tests/test_class_kernel_host.py (CPU) and tests/test_class_kernel_gpu.py (GPU) share.

One episode; v = base_ij (squared distance or Gram entry), p_c the parameter of class c (lengthscale l_c or offset), w_c = W[c]_ij = d obj / d E[c]_ij
(bitwise symmetric per matrix):

    RBF       u = v / p^2                       f = exp(-u / 2)                  f' = -f / 2
    MATERN25  u = v / p^2, r = sqrt(5 max(u, 1e-30))   f = (1 + r + r^2 / 3) exp(-r)    f' = -(5 / 6)(1 + r) exp(-r)        (f' = d f / d u)
    POLY      t = v + p                         f = t^k (k = 1, 2)               f' = k t^(k - 1)

    E[c] = f                                                                                         (forward)
    distance kinds:  tau_c = 2 w_c f'(u_c) / p_c^2,  A = sum_c tau_c,  Wp = diag(A 1) - A            (Wp_ii = sum_{j != i} A_ij: a_ii drops out)
                     theta_c = w_c f'(u_c) (-2 u_c / p_c),  dparam[c] = sum_ij theta_c
    poly:            tau_c = theta_c = w_c f'(t_c),  Wp = sum_c tau_c,  dparam[c] = sum_ij theta_c

`reference` evaluates these in float64 ON THE fp32 INPUTS (closed forms, no autograd); `restate_f32` / `forward_f32` restate the kernels in float32 numpy
in their order of operations (the reciprocal il2 = 1 / (p p) and m2p = -2 / p of the backward, v / (p p) of the forward, explicit fused multiply-adds where
the kernels have them, each route's own lane-to-column map, wave tree, 8-wave tree and row split; expf as the float64 exponential rounded once).

Routes (`route`), as dkt_class_kernel_bwd_f32 dispatches:
    n128   64 < N <= 128 and C <= 8     a wave per row, lanes own the columns lane and lane + 64
    v4     128 < N <= 512               a lane owns 4 consecutive columns of each group of 256 columns (one or two groups), classes in groups of four
    dword  everything else              lanes stride over the columns by 64
    ns = 1; while ns < 16 and B ns < 256 and N >= 16 ns: ns *= 2;  rows per split = ceil(N / ns)   (the last split can be empty: 129 <= N <= 135 at B = 1)

Bounds (u = 2^-24, the fp32 unit roundoff; one fp32 operation rounds once, relative error <= u; counts below are multiples of u; `+ 1` at the end of each
count pays for the second-order terms)

  the argument.  p p: 1.  The forward's v / (p p): DIV_U = 3 (1.5 units in the last place; a correctly rounded division needs 1).  The backward's
      il2 = 1 / (p p): 1 + DIV_U, and u = v il2: 1 more.  ARG_U = 5 covers both.
  expf, sqrtf.  The device library's figures are not documented in this tree: EXPF_ULPS = 2 and SQRTF_ULPS = 2 units in the last place (4 u each) are
      ALLOWED here (the published figure for both is 1).
  f and f'.
      RBF     exp(-u / 2) with an argument that carries ARG_U: amplified by |u| / 2.  f: 2 EXPF_ULPS + ARG_U |u| / 2 + 1.  f' = -0.5 f: the same (exact halving).
      MATERN  5 u: 1; the square root halves the relative error: RHO = (ARG_U + 1) / 2 + 2 SQRTF_ULPS = 7 on r.  exp(-r): r RHO + 2 EXPF_ULPS.
              1 + r + r r (1/3), all terms positive: r r 2 RHO + 1, times the rounded constant 2 more, the two additions 2 more: <= 2 RHO + 5.
              f = (...) exp(-r): 1 more:  2 RHO + 5 + r RHO + 2 EXPF_ULPS + 1 + 1 = 25 + 7 r.
              f' = (-(5/6) (1 + r)) exp(-r): the constant 1, 1 + r RHO + 1, two products 2:  RHO + 4 + r RHO + 2 EXPF_ULPS + 1 = 16 + 7 r.
      POLY    t = v + p: 1.  f = t: 1 + 1;  f = t t: 2 + 1 + 1.  f' = 1: 0;  f' = 2 t: 1 (the doubling is exact).
      `E` per element:  |E - ref| <= D_f u |f| + DENORM amp.   DENORM = 2^-126, the smallest NORMAL fp32, is the absolute floor: a result or a factor in
      (or flushed from) the subnormal range has an absolute error below it, so the test does not decide whether subnormals are flushed; amp is what such
      a factor is multiplied by afterwards (MATERN: 1 + r + r^2 / 3 for f, 1 + r for f'; 1 otherwise).
  one term.  g = w f': D_f' + 1.  tau = fma(2 g, il2, a): the product is exact inside the fma, il2 carries 1 + DIV_U:  D_tau = D_f' + 5  (POLY: D_f' + 1).
      theta = fma(g, u m2p, dp): u ARG_U, m2p = -2 / p DIV_U, their product 1, one more where `g * (-2 u / p)` is not contracted into the
      accumulation (the dword kernel):  D_theta = D_f' + 1 + ARG_U + DIV_U + 2 = D_f' + 11  (POLY: D_f' + 1).
  `Wp` off the diagonal (POLY: every element) = -a, a = the C-term sum over the classes, one rounding per class (fma, or `a += g` -- contracting it into an
      fma only removes the rounding of g), partial sums bounded by sum_c |tau_c|:
          |Wp_ij - ref| <= sum_c (D_tau,c + C + 1) u |tau_c| + DENORM sum_c (1 + |w_c|) amp_c (1 + 2 / p_c^2)                       -- `off`
  `Wp` on the diagonal (distance kinds) = rowsum - adiag: rowsum adds the row's a_ij, a_ii included, adiag is the same a_ii bit for bit.  A lane adds its
      columns one after the other -- ceil(N / 64) in the dword kernel, 2 in n128, 8 in v4 --, the wave tree adds 6 levels, the subtraction 1; partial
      sums bounded by T_i = sum_j sum_c |tau_c,ij| (j = i included: a_ii is in every partial sum it passed through), the terms j != i carry `off`:
          |Wp_ii - ref| <= sum_{j != i} off_ij + (max(ceil(N / 64), 8) + 6 + 1 + 1) u T_i                                         -- `diag`
  `dparam[b, c]`: the longest chain of additions a partial goes through in any of the three kernels: a lane visits ceil(rows per split / 8) rows and adds
      max(ceil(N / 64), 8) terms per row one after the other, then 6 levels of the wave tree, 3 of the 8 waves, and at most ns - 1 additions of the
      splits (ops sums them with torch; any order):  K = ceil(rows per split / 8) max(ceil(N / 64), 8) + 6 + 3 + ns  (not N^2):
          |dparam - ref| <= sum_ij (D_theta + K + 1) u |theta_ij| + DENORM sum_ij (1 + |w|) amp (1 + 2 |u| / p)                      -- `dparam`
"""
import numpy as np

U32 = 2.0 ** -24
DENORM = 2.0 ** -126
DIV_U = 3
ARG_U = 1 + DIV_U + 1
EXPF_ULPS = 2
SQRTF_ULPS = 2
RHO = (ARG_U + 1) / 2.0 + 2 * SQRTF_ULPS
KINDS = ("rbf", "matern", "poli1", "poli2")
MAX_C = 32

f32 = np.float32
f64 = np.float64


def is_poly(kind):
    return kind.startswith("poli")


def power_of(kind):
    return {"poli1": 1, "poli2": 2}.get(kind, 0)


# ---- the dispatch ---------------------------------------------------------------------------------------------------------------------------------------
def nsplit(b, n):
    ns = 1
    while ns < 16 and b * ns < 256 and n >= 16 * ns:
        ns *= 2
    return ns


def route(b, c, n):
    """(kernel name, nsplit, rows per split) of dkt_class_kernel_bwd_f32 at [B, C, N, N]."""
    ns = nsplit(b, n)
    name = "n128" if (64 < n <= 128 and c <= 8) else "v4" if 128 < n <= 512 else "dword"
    return name, ns, -(-n // ns)


def last_split_rows(b, c, n):
    """(first, end) rows of the last split that has any."""
    _, ns, rp = route(b, c, n)
    last = (n - 1) // rp
    return last * rp, n


def has_empty_split(b, c, n):
    _, ns, rp = route(b, c, n)
    return (ns - 1) * rp >= n


def _lane_columns(name, n):
    """[64, S] column of lane l at its s-th step within a row (n: none -- a padding slot)."""
    lane = np.arange(64)[:, None]
    if name == "v4":
        s = np.arange(4 * ((n + 255) // 256))[None, :]
        col = 256 * (s // 4) + 4 * lane + s % 4
    else:
        s = np.arange(2 if name == "n128" else (n + 63) // 64)[None, :]
        col = lane + 64 * s
    return np.where(col < n, col, n)


def _wave_rows(n, ns, rp):
    """[ns, 8, K] row of wave w of split sp at its k-th trip (n: none)."""
    k = -(-rp // 8)
    row = (np.arange(ns) * rp)[:, None, None] + np.arange(8)[None, :, None] + 8 * np.arange(k)[None, None, :]
    end = np.minimum(n, (np.arange(ns) + 1) * rp)[:, None, None]
    return np.where(row < end, row, n)


def chain_length(b, c, n):
    _, ns, rp = route(b, c, n)
    return -(-rp // 8) * max(-(-n // 64), 8) + 6 + 3 + ns


def row_chain_length(n):
    return max(-(-n // 64), 8) + 6 + 1 + 1


# ---- float64 closed forms -------------------------------------------------------------------------------------------------------------------------------
def _map64(kind, v, p, defect=None):
    """v [...], p [C] float64 -> (arg, f, f', D_f, D_f', amp_f, amp_f') each [C, ...]; arg = u (distance kinds) or t (poly)."""
    pc = p.reshape((-1,) + (1,) * v.ndim)
    with np.errstate(all="ignore"):
        if is_poly(kind):
            t = v[None] + pc
            one = np.ones_like(t)
            if kind == "poli1":
                return t, t, one, 2.0 * one, 0.0 * one, one, one
            return t, t * t, (t if defect == "poli2-f'=t" else 2.0 * t), 4.0 * one, one, one, one
        u = v[None] / pc ** 2
        if kind == "rbf":
            f = np.exp(-0.5 * u)
            d = 2 * EXPF_ULPS + ARG_U * np.abs(u) / 2.0 + 1.0
            return u, f, -0.5 * f, d, d, np.ones_like(u), np.ones_like(u)
        if defect == "no-matern-clamp":          # f' as the chain rule through the square root gives it, d f / d r . d r / d u, with r = 0 at u = 0: 0 . inf
            r = np.sqrt(5.0 * u)
            er = np.exp(-r)
            df = (-(r / 3.0) * (1.0 + r) * er) * (5.0 / (2.0 * r))
        else:
            r = np.sqrt(5.0 * np.maximum(u, 1e-30))
            er = np.exp(-r)
            df = -(5.0 / 6.0) * (1.0 + r) * er
        f = (1.0 + r + r * r / 3.0) * er
        return u, f, df, 2 * RHO + 5 + r * RHO + 2 * EXPF_ULPS + 2, RHO + 4 + r * RHO + 2 * EXPF_ULPS + 1, 1.0 + r + r * r / 3.0, 1.0 + r


def forward_ref(kind, base, p):
    """base [B, ...] fp32, p [C] fp32 -> (E [B, C, ...] float64, bound of the same shape)."""
    base, p = np.asarray(base, f64), np.asarray(p, f64)
    e, bd = [], []
    for v in base:
        _, f, _, d_f, _, amp, _ = _map64(kind, v, p)
        e.append(f)
        bd.append(d_f * U32 * np.abs(f) + DENORM * amp)
    return np.stack(e), np.stack(bd)


DEFECTS = ("v4-tail-not-masked", "last-class-group-dropped", "second-column-group-dropped", "diagonal-keeps-a_ii", "no-diagonal-from-row-64",
           "last-split-rows-lost", "-2u/p^2", "poli2-f'=t", "param[0]-for-every-class", "dparam-parts-transposed", "no-matern-clamp")


def reference(kind, w, base, p, defect=None):
    """w [B,C,N,N], base [B,N,N], p [C] (fp32 values) -> dict(wp [B,N,N], dparam [B,C], parts [B,ns,C]) in float64 and, without a defect, the bounds
    off [B,N,N], diag [B,N] (distance kinds; poly: zeros, every element is under `off`), dparam_b [B,C].  `defect`: one of DEFECTS -- what a kernel with
    that mistake would return, up to its own rounding."""
    w, base, p = np.asarray(w, f64), np.asarray(base, f64), np.asarray(p, f64)
    b, c, n, _ = w.shape
    name, ns, rp = route(b, c, n)
    poly = is_poly(kind)
    idx = np.arange(n)
    pc = p.reshape(-1, 1, 1)
    pu = np.full_like(p, p[0]) if defect == "param[0]-for-every-class" else p
    split_of = np.minimum(idx // rp, ns - 1)
    out = dict(wp=np.zeros((b, n, n)), dparam=np.zeros((b, c)), parts=np.zeros((b, ns, c)), off=np.zeros((b, n, n)), diag=np.zeros((b, n)), dparam_b=np.zeros((b, c)))
    k_dp, k_row = chain_length(b, c, n), row_chain_length(n)
    for e in range(b):
        arg, _, df, _, d_df, _, amp = _map64(kind, base[e], pu, defect)
        with np.errstate(all="ignore"):
            g = w[e] * df
            if poly:
                tau, theta = g, g
                d_tau, d_theta = d_df + 1, d_df + 1
                fl_tau, fl_theta = (1 + np.abs(w[e])), (1 + np.abs(w[e]))
            else:
                tau = 2.0 * g / pu.reshape(-1, 1, 1) ** 2
                theta = g * (-2.0 * arg / (pu.reshape(-1, 1, 1) ** 2 if defect == "-2u/p^2" else pu.reshape(-1, 1, 1)))
                d_tau, d_theta = d_df + 1 + (1 + DIV_U), d_df + 1 + ARG_U + DIV_U + 2
                fl_tau, fl_theta = (1 + np.abs(w[e])) * amp * (1 + 2.0 / pc ** 2), (1 + np.abs(w[e])) * amp * (1 + 2.0 * np.abs(arg) / pc)
        if defect is None:
            off = ((d_tau + c + 1) * U32 * np.abs(tau)).sum(0) + DENORM * fl_tau.sum(0)
            out["off"][e] = off
            if not poly:
                t_row = np.abs(tau).sum((0, 2))
                out["diag"][e] = off.sum(1) - off[idx, idx] + k_row * U32 * t_row
            out["dparam_b"][e] = ((d_theta + k_dp + 1) * U32 * np.abs(theta)).sum((1, 2)) + DENORM * fl_theta.sum((1, 2))
        keep = np.ones((c, n, n))
        written = np.ones((n, n), bool)
        if defect == "last-class-group-dropped" and name == "v4" and c % 4:
            keep[4 * (c // 4):] = 0.0
        if defect == "second-column-group-dropped" and name == "v4" and n > 256:
            keep[:, :, 256:] = 0.0
            written[:, 256:] = False
        if defect == "last-split-rows-lost" and ns > 1:
            keep[:, ns * (n // ns):, :] = 0.0
            written[ns * (n // ns):, :] = False
        tau, theta = tau * keep, theta * keep
        a = tau.sum(0)
        row_extra, par = np.zeros(n), theta.sum(2)                   # par [C, N]: the parameter terms of row i
        if defect == "v4-tail-not-masked" and name == "v4" and n % 4:
            m = 4 - n % 4                                            # the 16-byte load that holds the row end also holds the next row's first m values
            row_extra[:-1] = tau[:, 1:, :m].sum((0, 2))
            par = par.copy()
            par[:, :-1] += theta[:, 1:, :m].sum(2)
        if poly:
            wp = a
        else:
            wp = -a
            rowsum = a.sum(1) + row_extra
            wp[idx, idx] = rowsum if defect == "diagonal-keeps-a_ii" else rowsum - a[idx, idx]
            if defect == "no-diagonal-from-row-64" and name == "n128":
                wp[idx[64:], idx[64:]] = -a[idx[64:], idx[64:]]
        out["wp"][e] = np.where(written, wp, 0.0)
        for sp in range(ns):
            out["parts"][e, sp] = par[:, split_of == sp].sum(1) if (split_of == sp).any() else 0.0
        parts = out["parts"][e]
        if defect == "dparam-parts-transposed":                      # written [C, ns], read [ns, C]
            parts = parts.T.reshape(ns, c)
        out["dparam"][e] = parts.sum(0)
    return out


# ---- the same in float32, in the kernels' order ---------------------------------------------------------------------------------------------------------
def _exp32(x):
    """expf: the float64 exponential rounded once (within half a unit in the last place, whatever the host's libm)."""
    with np.errstate(all="ignore"):
        return np.exp(x.astype(f64)).astype(f32)


def _map32(kind, t):
    """class_map<KIND>: t fp32 array -> (f, f') fp32."""
    if kind == "rbf":
        f = _exp32(f32(-0.5) * t)
        return f, f32(-0.5) * f
    if kind == "matern":
        r = np.sqrt(f32(5.0) * np.maximum(t, f32(1e-30)))
        er = _exp32(-r)
        f = (f32(1.0) + r + r * r * (f32(1.0) / f32(3.0))) * er
        return f, -(f32(5.0) / f32(6.0)) * (f32(1.0) + r) * er
    if kind == "poli2":
        return t * t, f32(2.0) * t
    return t, np.ones_like(t)


def forward_f32(kind, base, p):
    """class_kernel_fwd: t = v / (p p) or v + p."""
    base, p = np.asarray(base, f32), np.asarray(p, f32)
    out = np.empty((base.shape[0], p.size) + base.shape[1:], f32)
    with np.errstate(all="ignore"):
        for c in range(p.size):
            t = base + p[c] if is_poly(kind) else base / f32(p[c] * p[c])
            out[:, c] = _map32(kind, t)[0]
    return out


def _fma32(x, y, z):
    """fl32(x y + z) for fp32 arrays: the product of two fp32 numbers is exact in float64; the float64 addition rounds at 2^-53 before the fp32 rounding."""
    return (x.astype(f64) * y.astype(f64) + z.astype(f64)).astype(f32)


def _wave_tree(v):
    """wave_allsum over the last axis (64 lanes): v += shfl_xor(v, o), o = 32 .. 1 -- every lane ends with the same tree sum."""
    o = 32
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o >>= 1
    return v[..., 0]


def _sequential(addends):
    """Sum over the last axis one addend after the other, one fp32 rounding per step; addends float64 (fp32 values, or exact products: a fused multiply-add)."""
    s = np.zeros(addends.shape[:-1], f32)
    for k in range(addends.shape[-1]):
        s = (s.astype(f64) + addends[..., k]).astype(f32)
    return s


def restate_f32(kind, w, base, p):
    """The backward in float32 numpy, in the order of the kernel `route` names.  -> (wp [B,N,N], dparam [B,C]) fp32."""
    w, base, p = np.asarray(w, f32), np.asarray(base, f32), np.asarray(p, f32)
    b, c, n, _ = w.shape
    name, ns, rp = route(b, c, n)
    poly = is_poly(kind)
    cols, rows = _lane_columns(name, n), _wave_rows(n, ns, rp)
    idx = np.arange(n)
    wp, dparam = np.empty((b, n, n), f32), np.empty((b, c), f32)
    with np.errstate(all="ignore"):
        for e in range(b):
            v = base[e]
            a = np.zeros((n, n), f32)
            add = np.zeros((c, n + 1, n + 1), f64)                   # (row n, column n: the padding slots, exact zeros)
            for k in range(c):
                if poly:
                    _, df = _map32(kind, v + p[k])
                    g = w[e, k] * df
                    a = a + g
                    add[k, :n, :n] = g
                else:
                    il2 = f32(1.0) / f32(p[k] * p[k])
                    u = v * il2
                    _, df = _map32(kind, u)
                    g = w[e, k] * df
                    a = _fma32(f32(2.0) * g, np.full_like(g, il2), a)
                    if name == "dword":
                        add[k, :n, :n] = g * (f32(-2.0) * u / p[k])
                    else:
                        add[k, :n, :n] = g.astype(f64) * (u * (f32(-2.0) / p[k])).astype(f64)
            if poly:
                wp[e] = a
            else:
                ap = np.concatenate([a, np.zeros((n, 1), f32)], 1)[:, cols]          # [N, 64, S]
                rowsum = _wave_tree(_sequential(ap.astype(f64)))
                wp[e] = -a
                wp[e][idx, idx] = rowsum - a[idx, idx]
            seq = add[:, rows][:, :, :, :, cols]                                      # [C, ns, 8, K, 64, S]
            seq = seq.transpose(0, 1, 2, 4, 3, 5).reshape(c, ns, 8, 64, -1)
            d = _wave_tree(_sequential(seq))                                          # [C, ns, 8]
            parts = ((d[..., 0] + d[..., 1]) + (d[..., 2] + d[..., 3])) + ((d[..., 4] + d[..., 5]) + (d[..., 6] + d[..., 7]))
            dparam[e] = _sequential(parts.astype(f64))
    return wp, dparam


def fractions(kind, wp, dparam, ref):
    """Largest fraction of each bound that (wp, dparam) uses against `ref` (reference(...) without a defect): dict(off, diag, dparam, finite)."""
    wp, dparam = np.asarray(wp, f64), np.asarray(dparam, f64)
    n = wp.shape[-1]
    idx = np.arange(n)
    finite = bool(np.isfinite(wp).all() and np.isfinite(dparam).all())
    with np.errstate(all="ignore"):
        eo = np.abs(wp - ref["wp"]) / ref["off"]
        ed = np.zeros((1,))
        if not is_poly(kind):
            ed = eo[:, idx, idx] * ref["off"][:, idx, idx] / ref["diag"]
            eo[:, idx, idx] = 0.0
        ep = np.abs(dparam - ref["dparam"]) / ref["dparam_b"]
    worst = lambda x: float(np.where(np.isfinite(x), x, np.inf).max())          # noqa: E731  (a NaN or an infinity is outside every bound)
    return dict(off=worst(eo), diag=worst(ed), dparam=worst(ep), finite=finite)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------------
LENGTHSCALES = (1.1, 0.05, 30.0, 0.4, 3.0, 0.15, 10.0, 0.7)          # 0.05: d2 / l^2 in the hundreds, exp underflows to 0;  30: every entry of E near 1
OFFSETS = (1.1, -0.3, 0.05, 2.0, -1.0, 0.4, 30.0, -0.05)             # the negative ones: g + offset crosses zero within a matrix
EDGE_WEIGHT = 64.0
EDGE_COLUMNS = (63, 64, 65, 255, 256, 257)
D_FEAT = 8


def params(kind, c):
    """[C] fp32, distinct per class: the list above, each further round of it 3 % larger."""
    src = OFFSETS if is_poly(kind) else LENGTHSCALES
    return np.array([src[k % 8] * (1.0 + 0.03 * (k // 8)) for k in range(c)], f32)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def square_base(kind, b, n, rng):
    """[B,N,N] fp32, bitwise symmetric.  Distance kinds: squared distances of ReLU-like features with a common offset (median ~ 0.5), an exactly zero
    diagonal and duplicate rows (off-diagonal exact zeros) from N = 4.  Poly: the Gram of zero-mean features (entries of both signs, diagonal ~ 2)."""
    if is_poly(kind):
        z = 0.5 * rng.standard_normal((b, n, D_FEAT))
        return (z[:, :, None, :] * z[:, None, :, :]).sum(-1).astype(f32)
    z = np.abs(rng.standard_normal((b, n, D_FEAT))) * 0.3 + rng.uniform(0.0, 2.0, (1, 1, D_FEAT))
    if n >= 4:
        z[:, n // 2] = z[:, 1]
    if n >= 70:
        z[:, n - 1] = z[:, 64]
        z[:, 66] = z[:, 3]
    d = z[:, :, None, :] - z[:, None, :, :]
    return (d * d).sum(-1).astype(f32)


def edge_rows(b, c, n):
    """Rows (and, W being symmetric, columns) that carry EDGE_WEIGHT: the last three, 63 .. 65, 255 .. 257, the rows of the last non-empty split."""
    edge = np.zeros(n, bool)
    edge[max(0, n - 3):] = True
    for k in EDGE_COLUMNS:
        if k < n:
            edge[k] = True
    if route(b, c, n)[1] > 1:
        first, end = last_split_rows(b, c, n)
        edge[first:end] = True
    return edge


def weights(b, c, n, rng):
    """W [B,C,N,N] fp32, bitwise symmetric per matrix, entries O(1); EDGE_WEIGHT times that on the edge rows and columns, on the diagonal and in the whole
    last class (C > 1): a lost or leaked edge term shows in dparam and in the row sums."""
    w = rng.standard_normal((b, c, n, n))
    w = np.triu(w) + np.triu(w, 1).transpose(0, 1, 3, 2)
    edge = edge_rows(b, c, n)
    scale = np.where(edge[:, None] | edge[None, :] | np.eye(n, dtype=bool), EDGE_WEIGHT, 1.0)
    w = w * scale
    if c > 1:
        w[:, -1] *= EDGE_WEIGHT / scale
    return w.astype(f32)


def bwd_case(kind, b, c, n, seed=0):
    rng = _rng(seed, b, c, n, KINDS.index(kind))
    case = dict(kind=kind, base=square_base(kind, b, n, rng), w=weights(b, c, n, rng), p=params(kind, c))
    assert np.array_equal(case["base"], case["base"].transpose(0, 2, 1)) and np.array_equal(case["w"], case["w"].transpose(0, 1, 3, 2))
    return case


# (B, C, N) of the backward, by the route they take
BWD_DWORD = ((1, 1, 1), (2, 5, 7), (1, 3, 15), (1, 3, 16), (3, 5, 63), (2, 32, 64), (1, 9, 65), (2, 9, 128), (1, 2, 513))
BWD_N128 = ((1, 1, 65), (1, 8, 65), (3, 5, 100), (2, 8, 127), (1, 5, 128))
BWD_V4 = ((1, 1, 129), (1, 5, 131), (2, 3, 255), (1, 4, 256), (1, 9, 257), (1, 20, 259), (1, 20, 447), (1, 2, 511), (1, 32, 512))
BWD_SHAPES = BWD_DWORD + BWD_N128 + BWD_V4
SPLIT_SHAPES = {(127, 2, 65): 4, (128, 2, 65): 2, (255, 2, 65): 2, (256, 2, 65): 1}          # (B, C, N) -> nsplit
SPLIT_KINDS = ("rbf", "poli2")


def bwd_cases():
    """[(kind, (B, C, N))] of every backward case of the GPU test."""
    return [(k, s) for s in BWD_SHAPES for k in KINDS] + [(k, s) for s in SPLIT_SHAPES for k in SPLIT_KINDS]


_bwd = {}


def bwd_reference(kind, shape):
    """dict(case, ref, f32 = fractions of the float32 restatement) of one backward case, computed once per process and left unchanged."""
    key = (kind, shape)
    if key not in _bwd:
        case = bwd_case(kind, *shape)
        ref = reference(kind, case["w"], case["base"], case["p"])
        wp, dp = restate_f32(kind, case["w"], case["base"], case["p"])
        _bwd[key] = dict(case=case, ref=ref, f32=fractions(kind, wp, dp, ref), f32_out=(wp, dp))
    return _bwd[key]


FWD_SHAPES = ((1, 1), (2, 255), (2, 256), (3, 257), (2, 7, 33), (1, 513, 513))          # base [B, NN] or [B, M, N]
FWD_C = (1, 5, 32)


def fwd_case(kind, shape, c, seed=0):
    """dict(kind, base, p).  Flat bases: positive values with exact zeros (distance kinds) or values of both signs (poly); [2, 7, 33]: the first 7 rows
    against all 33 of a square base (the cross matrix of test time; its leading 7 x 7 block holds the zero diagonal); [1, 513, 513]: a square base."""
    rng = _rng(seed, 77, c, KINDS.index(kind), *shape)
    if len(shape) == 2:
        base = rng.standard_normal(shape) * 0.7 if is_poly(kind) else rng.exponential(1.0, shape) * (rng.uniform(0, 1, shape) > 0.15)
        if not is_poly(kind):
            base[:, 0] = 0.0
        base = base.astype(f32)
    elif shape[1] != shape[2]:
        base = np.ascontiguousarray(square_base(kind, shape[0], shape[2], rng)[:, :shape[1]])
    else:
        base = square_base(kind, shape[0], shape[1], rng)
    return dict(kind=kind, base=base, p=params(kind, c))
