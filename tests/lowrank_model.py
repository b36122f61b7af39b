"""The linear-kernel episode in feature space (csrc/dkt_lowrank.hip: dkt_lowrank_gram_f32 -> dkt_mll_f32 on the 64 x 64 models -> dkt_lowrank_finish_f32 ->
dkt_lowrank_bwd_f32) restated in float64, kernel by kernel, independent of dkt_amd (a helper, not a test):

  gram       A = Zp^T Zp (64 x 64), P_c = Zp^T (y_c - m_c)                         Zp = Z zero-padded to 64 columns
  inner      K'_c = sv_c A + nz_c I:  t_c = K'_c^-1 p_c, K'_c^-1, W' = 0.5 sum_c cw_c sv_c (t_c t_c^T - K'_c^-1), and what dkt_mll_f32 hands on: logp_d, dnoise_d
  finish     S = Zp T^T, alpha = (r - sv S) / nz, V = cw sv (alpha - S), logp, dsv, dmean, dnoise (raw, without cw), obj = sum_c cw_c logp_c
  backward   dZ = g_b (V^T T + 2 Zp W')

Every stage takes its operands as arguments, so a test can feed it the DEVICE outputs of the stage before it, and returns next to each value the first-order
rounding bound of the float32 kernel that computes it (`*_bound`), written out beside the formula.  u = 2^-24; a sum of k products that are exact in fp32
(v_mfma_f32_16x16x4_f32) is off by at most gamma(k) = 2 (k + 4) u times the sum of the magnitudes -- the factor 2 covers the order inside the MFMA and the
reduction across lanes, the 4 the roundings of the operands (y - m, g t, 2 g W').

The model owns the feature order of the device: index d' = 16 q + m of A, P, t and W' stands for column 4 m + q (PERM[d'] = column).

The shape lists of the GPU comparison (tests/test_lowrank_gpu.py) and of the guard-band cases (tests/test_guard_bands_gpu.py) are plain data at the end."""
import numpy as np

DP = 64                                          # DKT_LOWRANK_DP
U = 2.0 ** -24
LOG_2PI = float(np.log(2.0 * np.pi))
PERM = np.array([4 * (dp % 16) + dp // 16 for dp in range(DP)])          # device index d' -> column
INV = np.argsort(PERM)                                                    # column -> device index d'


def gamma(k):
    return 2.0 * (k + 4) * U


def to_device(x, axes=(-1,)):
    """natural (column) order -> the device's order, along every axis of `axes` (each of length 64)"""
    x = np.asarray(x)
    for ax in axes:
        x = np.take(x, PERM, axis=ax)
    return x


def to_natural(x, axes=(-1,)):
    x = np.asarray(x)
    for ax in axes:
        x = np.take(x, INV, axis=ax)
    return x


def pad(z):
    """Z [B,N,D] -> float64 [B,N,64], zero columns from D on"""
    z = np.asarray(z, np.float64)
    out = np.zeros(z.shape[:-1] + (DP,))
    out[..., :z.shape[-1]] = z
    return out


def padded_device_indices(d):
    """the positions d' of A, P, t and W' that belong to the zero columns D .. 63"""
    return np.nonzero(PERM >= d)[0]


def _y3(y, b):
    y = np.asarray(y, np.float64)
    return y if y.ndim == 3 else np.broadcast_to(y[None], (b,) + y.shape)


def nct_of(c):
    """class tiles of 16 of the gram and finish kernels (lowrank_gram_kernel<NCT>, lowrank_finish_kernel<NCT>)"""
    return 1 if c <= 16 else 2


def nkc_of(c):
    """K steps of 4 classes of lowrank_bwd_kernel<NKC>, as dkt_lowrank_bwd_f32 selects it"""
    k = (c + 3) // 4
    return 2 if k <= 2 else 4 if k <= 4 else 5 if k <= 5 else 8


# ---- the stages ---------------------------------------------------------------------------------------------------------------------------------
def gram(z, y, mean):
    """natural order: A [B,64,64], P [B,C,64] and their bounds.  N products per element, exact in fp32; r = y - m is one rounding."""
    zp = pad(z)
    b_, n, _ = zp.shape
    r = _y3(y, b_) - np.asarray(mean, np.float64)[None, :, None]
    az = np.abs(zp)
    return dict(A=np.einsum("bnd,bne->bde", zp, zp), P=np.einsum("bnd,bcn->bcd", zp, r),
                A_bound=gamma(n) * np.einsum("bnd,bne->bde", az, az), P_bound=gamma(n) * np.einsum("bnd,bcn->bcd", az, np.abs(r)))


def inner(a, p, sv, nz, cw):
    """dkt_mll_f32 on (A, P) with zero mean, N' = 64 (any one feature order): t [B,C,64], kinv [B,C,64,64], wd [B,64,64], logp_d, dnoise_d [B,C] (raw),
    logdet_d.  nz = noise + jitter, [C] or [B,C]."""
    a, p, sv, cw = (np.asarray(x, np.float64) for x in (a, p, sv, cw))
    b_, c_ = p.shape[:2]
    nz = np.broadcast_to(np.asarray(nz, np.float64), (b_, c_))
    k = sv[None, :, None, None] * a[:, None] + nz[..., None, None] * np.eye(DP)
    kinv = np.linalg.inv(k)
    kinv = 0.5 * (kinv + np.swapaxes(kinv, -1, -2))
    t = np.einsum("bcde,bce->bcd", kinv, p)
    logdet = np.linalg.slogdet(k)[1]
    m = 0.5 * (t[..., :, None] * t[..., None, :] - kinv)
    return dict(t=t, kinv=kinv, wd=np.einsum("c,bcde->bde", cw * sv, m), logdet_d=logdet,
                logp_d=-0.5 * (np.einsum("bcd,bcd->bc", p, t) + logdet + DP * LOG_2PI), dnoise_d=np.einsum("bcdd->bc", m))


def finish(z, y, sv, mean, nz, cw, t, logp_d, dnoise_d):
    """The second pass over Z, from the t, logp_d and dnoise_d it is GIVEN (natural order).  Returns the values and `<name>_bound` for each.
        S       = Zp t^T                                     64 exact products                       eS   = gamma(64) |Zp| |t|^T
        alpha   = (r - sv S) / nz                            r, sv S, -, /, nz: <= 6 roundings       eal  = (sv eS + 6 u (|r| + sv |S|)) / nz
        V       = (cw sv) (alpha - S)                        cw sv, -, x                             eV   = |cw sv| (eal + eS + 3 u (|alpha| + |S|))
        a1 = sum alpha, a2 = sum alpha^2, r2 = sum r^2, rs = sum r S  (N terms), tt = |t|^2 (64 terms)
        logdet' = -2 logp_d - rs - 64 log 2 pi
        quad    = (r2 - sv rs) / nz
        trk'    = tt - 2 dnoise_d,  trk = (N - 64) / nz + trk'
        logp    = -quad / 2 - ((N - 64) log nz + logdet') / 2 - N / 2 log 2 pi
        dmean   = a1,  dnoise = (a2 - trk) / 2,  dsv = (tt - (64 - nz trk') / sv) / 2,  obj = sum_c cw_c logp_c
    each bound: the bounds of the operands carried through the expression, plus u times the magnitude of every term per rounding of the expression itself
    (the cancelling terms keep their magnitudes: |r| + sv |S|, |a2| + |trk|, ...)."""
    zp = pad(z)
    b_, n, _ = zp.shape
    sv, mean, cw, t, logp_d, dnoise_d = (np.asarray(x, np.float64) for x in (sv, mean, cw, t, logp_d, dnoise_d))
    c_ = t.shape[1]
    nzb = np.broadcast_to(np.asarray(nz, np.float64), (b_, c_))
    nz3, sv3, sv2 = nzb[..., None], sv[None, :, None], sv[None, :]
    r = _y3(y, b_) - mean[None, :, None]
    gn, g64 = gamma(n), gamma(DP)
    s = np.einsum("bnd,bcd->bcn", zp, t)
    e_s = g64 * np.einsum("bnd,bcd->bcn", np.abs(zp), np.abs(t))
    alpha = (r - sv3 * s) / nz3
    e_al = (sv3 * e_s + 6 * U * (np.abs(r) + sv3 * np.abs(s))) / nz3
    cws = (cw * sv)[None, :, None]
    v = cws * (alpha - s)
    e_v = np.abs(cws) * (e_al + e_s + 3 * U * (np.abs(alpha) + np.abs(s)))
    a1, e_a1 = alpha.sum(-1), e_al.sum(-1) + gn * np.abs(alpha).sum(-1)
    a2, e_a2 = (alpha * alpha).sum(-1), (2 * np.abs(alpha) * e_al).sum(-1) + gn * (alpha * alpha).sum(-1)
    r2, e_r2 = (r * r).sum(-1), (gn + 4 * U) * (r * r).sum(-1)
    rs, e_rs = (r * s).sum(-1), (np.abs(r) * e_s).sum(-1) + (gn + 4 * U) * np.abs(r * s).sum(-1)
    tt = (t * t).sum(-1)
    e_tt = g64 * tt
    logdet = -2.0 * logp_d - rs - DP * LOG_2PI
    e_logdet = e_rs + 4 * U * (2 * np.abs(logp_d) + np.abs(rs) + DP * LOG_2PI)
    quad = (r2 - sv2 * rs) / nzb
    e_quad = (e_r2 + sv2 * e_rs + 4 * U * (np.abs(r2) + sv2 * np.abs(rs))) / nzb
    trkd = tt - 2.0 * dnoise_d
    e_trkd = e_tt + 2 * U * (np.abs(tt) + 2 * np.abs(dnoise_d))
    trk = (n - DP) / nzb + trkd
    e_trk = e_trkd + 3 * U * (abs(n - DP) / nzb + np.abs(trkd))
    lognz = np.log(nzb)
    logp = -0.5 * quad - 0.5 * ((n - DP) * lognz + logdet) - 0.5 * n * LOG_2PI
    e_logp = (0.5 * e_quad + 0.5 * e_logdet + 0.5 * abs(n - DP) * U * (1 + 4 * np.abs(lognz))            # logf within 2 ulp of log(fl(nz))
              + 6 * U * (0.5 * np.abs(quad) + 0.5 * abs(n - DP) * np.abs(lognz) + 0.5 * np.abs(logdet) + 0.5 * n * LOG_2PI))
    dnoise = 0.5 * (a2 - trk)
    e_dnoise = 0.5 * (e_a2 + e_trk + 2 * U * (np.abs(a2) + np.abs(trk)))
    inner_ = DP - nzb * trkd
    dsv = 0.5 * (tt - inner_ / sv2)
    e_dsv = 0.5 * (e_tt + (nzb * e_trkd + 4 * U * (DP + nzb * np.abs(trkd))) / sv2 + 2 * U * (np.abs(tt) + np.abs(inner_) / sv2))
    obj = (cw[None] * logp).sum(-1)
    e_obj = (np.abs(cw)[None] * e_logp).sum(-1) + gamma(c_) * np.abs(cw[None] * logp).sum(-1)
    return dict(s=s, alpha=alpha, v=v, logp=logp, dsv=dsv, dmean=a1, dnoise=dnoise, obj=obj,
                alpha_bound=e_al, v_bound=e_v, logp_bound=e_logp, dsv_bound=e_dsv, dmean_bound=e_a1, dnoise_bound=e_dnoise, obj_bound=e_obj)


def backward(z, v, t, wd, g):
    """dZ [B,N,D] = g_b (V^T T + 2 Zp W') (natural order), C + 64 products per element; the operands g t and 2 g W' are one rounding each."""
    zp = pad(z)
    d = np.asarray(z).shape[-1]
    v, t, wd, g = (np.asarray(x, np.float64) for x in (v, t, wd, g))
    c_ = t.shape[1]
    dz = g[:, None, None] * (np.einsum("bcn,bcd->bnd", v, t) + 2.0 * np.einsum("bnd,bde->bne", zp, wd))
    mag = np.abs(g)[:, None, None] * (np.einsum("bcn,bcd->bnd", np.abs(v), np.abs(t)) + 2.0 * np.einsum("bnd,bde->bne", np.abs(zp), np.abs(wd)))
    return dict(dz=dz[..., :d], dz_bound=(2.0 * (c_ + DP + 2) * U * mag)[..., :d])


def episode(z, y, sv, mean, noise, cw, g):
    """The whole episode in float64, every stage fed by the one before it.  Natural order, and A, P, t, W' in the device's order as `<name>_dev`."""
    gr = gram(z, y, mean)
    inn = inner(gr["A"], gr["P"], sv, noise, cw)
    fin = finish(z, y, sv, mean, noise, cw, inn["t"], inn["logp_d"], inn["dnoise_d"])
    bw = backward(z, fin["v"], inn["t"], inn["wd"], g)
    out = dict(A=gr["A"], P=gr["P"], t=inn["t"], kinv=inn["kinv"], wd=inn["wd"], logp_d=inn["logp_d"], dnoise_d=inn["dnoise_d"], dz=bw["dz"])
    out.update({k: fin[k] for k in ("alpha", "v", "logp", "dsv", "dmean", "dnoise", "obj")})
    out.update(A_dev=to_device(gr["A"], (-1, -2)), P_dev=to_device(gr["P"]), t_dev=to_device(inn["t"]), wd_dev=to_device(inn["wd"], (-1, -2)))
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


def inputs(c, n, d, b=2, y_per_episode=False, seed=None):
    """fp32-representable inputs of one call: unit rows Z [B,N,D] around max(c, 2) class centres, targets +-1 ([C,N], or [B,C,N] with distinct class
    assignments per episode), sv in 0.5 .. 2, mean, noise 0.1 .. 0.3, class weights of both signs, an upstream gradient per episode."""
    rng = np.random.default_rng(100000 * d + 1000 * n + 10 * c + b if seed is None else seed)
    cc = max(c, 2)
    z = rng.standard_normal((cc, d))[rng.integers(0, cc, (b, n))] * 0.5 + rng.standard_normal((b, n, d))
    z /= np.linalg.norm(z, axis=-1, keepdims=True)
    cls = rng.integers(0, cc, (b, n)) if y_per_episode else np.arange(n) % cc
    y = np.where(cls[..., None, :] == np.arange(c)[:, None], 1.0, -1.0)
    cw = -np.linspace(0.5, 1.5, c) / (c * n)
    cw[c // 2::3] *= -1.5
    return dict(z=f32(z), y=f32(y), sv=f32(np.linspace(0.5, 2.0, c)), mean=f32(np.linspace(-0.2, 0.3, c)), noise=f32(np.linspace(0.1, 0.3, c)),
                cw=f32(cw), g=f32(np.linspace(-1.5, 2.0, b)))


def aligned_rows(seed, c, per, d, shift):
    """Non-negative, strongly aligned unit rows (a ReLU trunk under the plain cossim kernel): [N = c per, D] float64"""
    from oracle import dkt_oracle as O
    rng = np.random.default_rng(seed)
    cm = rng.standard_normal((c, d))
    return O.l2_normalize(np.maximum(0.7 * np.repeat(cm, per, axis=0) + 0.7 * rng.standard_normal((c * per, d)) + shift, 0.0) + 1e-3)


def cond_k(z, sv, noise):
    """cond(sv Z Z^T + noise I) for N > D: 1 + sv lambda_max(Z^T Z) / noise"""
    z = np.asarray(z, np.float64)
    return 1.0 + sv * float(np.linalg.eigvalsh(z.T @ z)[-1]) / noise


# ---- the cases, (C, N, D) ------------------------------------------------------------------------------------------------------------------------
CLASS_COUNTS = (1, 4, 5, 8, 9, 12, 16, 17, 20, 21, 32)          # every NKC (2: 1-8, 4: 9-16, 5: 17-20, 8: 21-32) and NCT (1: 1-16, 2: 17-32) at its first and last C
N_EDGES = (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 35, 63, 64, 65, 127, 128, 129)      # the 4-row K step, the 16-row tile, the 32-row chunk of LR_U = 8 K steps
D_EDGES = (4, 12, 16, 20, 36, 48, 52, 60, 64)
CLASS_CASES = [(c, n, d) for c in CLASS_COUNTS for n, d in ((37, 64), (80, 20))]
N_CASES = [(c, n, d) for n in N_EDGES for c, d in ((5, 64), (17, 12))]
D_CASES = [(9, 35, d) for d in D_EDGES]
CASES = CLASS_CASES + N_CASES + D_CASES
END_TO_END_EXTRA = [(9, 84, 64), (12, 96, 20), (16, 84, 52), (21, 96, 64)]
END_TO_END = [k for k in CASES if k[1] >= 80] + END_TO_END_EXTRA      # what the ops-level gate (N >= 80) lets through
GUARD_CASES = [(9, 35, 12), (16, 33, 52), (21, 17, 4), (32, 129, 64)]
ALIGNED_SEED = 5
ALIGNED_SHAPES = [(20, 21, 64), (5, 21, 64)]                    # (C, per, D): N = 420 and 105
ALIGNED_SHIFTS = (0, 1, 2)
ALIGNED_SV = (1.0, 3.0)
ALIGNED_NOISE, ALIGNED_MEAN = 0.1, 0.05


def case_flags(index):
    """(B, y per episode) of CASES[index]: B = 2 or 3, every third case with targets of its own per episode"""
    return 2 + index % 2, index % 3 == 1
