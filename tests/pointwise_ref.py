"""Plain restatements and exact references of the ViT's pointwise arithmetic (numpy only, no GPU).

Three layers, used by tests/test_pointwise_cpu.py and tests/test_gpu_pointwise.py:

* exact references in fp64: gelu (Phi through erfc on the negative side), silu, LayerNorm;
* fp32 restatements, operation for operation, of gelu_pk / gelu_pk9 / gelu_erf_pk (csrc/gemm_kernel.hpp, coefficients copied by
  value), the exp2- and expf-form SiLU, the erff GELU of f32_tile.hip, and the two LayerNorm algorithms (two-pass: layernorm_kernel;
  single-pass: the residual GEMM's partial sums + ln_finalize_kernel).  An fma is the fp64 product and sum rounded once to fp32;
  v_rcp_f32, v_exp_f32 and rsqrtf are CORRECTLY ROUNDED here (the hardware ones are 1-ulp approximations: every bar that is a
  multiple of a restatement's error says which multiple covers that);
* the input generators and the checks themselves.  A check takes the inputs and an output array, returns (ok, measured, bar, text):
  the GPU test feeds it the kernels' outputs, the CPU test feeds it the restatements' outputs -- faithful ones must pass, and each
  imitated fault (a `fault=` argument of a restatement) must fail at least one of them.

Every restatement takes `fault`: None or a string naming one deliberate defect (see FAULTS_*).
"""

import math

import numpy as np

F32 = np.float32
U24, U23 = 2.0 ** -24, 2.0 ** -23
LN_EPS = 1e-6
CLAMP_PK, CLAMP_PK9 = 3.9, 4.4

_erfc = np.frompyfunc(math.erfc, 1, 1)
_erf = np.frompyfunc(math.erf, 1, 1)


# ------------------------------------------------------------------------------------------------ exact references (fp64)
def phi(x):
    """Phi(x) in fp64; erfc on both sides so neither tail cancels (x < 0: Phi = erfc(-x / sqrt 2) / 2; x >= 0: 1 - erfc(x / sqrt 2) / 2)."""
    x = np.asarray(x, np.float64)
    t = 0.5 * np.asarray(_erfc(np.abs(x) / math.sqrt(2.0)), np.float64)
    return np.where(x < 0, t, 1.0 - t)


def gelu(x):
    """x Phi(x) in fp64; the negative tail is x erfc(|x| / sqrt 2) / 2, no cancellation."""
    x = np.asarray(x, np.float64)
    return x * phi(x)


def silu(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def layernorm(x, weight=None, bias=None, eps=LN_EPS):
    """LayerNorm in fp64 of the fp64 VALUE of x (no re-rounding of the input).  -> (y, mean, var)."""
    x = np.asarray(x).astype(np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps)
    if weight is not None:
        y = y * np.asarray(weight, np.float64) + np.asarray(bias, np.float64)
    return y, mu[..., 0], var[..., 0]


# ------------------------------------------------------------------------------------------------ fp32 primitives
def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _mul(a, b):
    return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)


def rcp(x):      # v_rcp_f32, correctly rounded here (hardware: 1 ulp)
    with np.errstate(divide="ignore"):
        return (1.0 / np.asarray(x, np.float64)).astype(F32)


def exp2(x):     # v_exp_f32, correctly rounded here (hardware: 1 ulp)
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2(np.asarray(x, np.float64)).astype(F32)


def rsqrt(x):    # rsqrtf, correctly rounded here
    with np.errstate(divide="ignore"):
        return (1.0 / np.sqrt(np.asarray(x, np.float64))).astype(F32)


def round_bf16(x, trunc=False):
    """fp32 -> bf16 (returned as the fp32 value), round to nearest even; trunc: the imitated fault."""
    b = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    if not trunc:
        b = b + 0x7FFF + ((b >> 16) & 1)
    return (b & 0xFFFF0000).astype(np.uint32).view(F32)


def round_f16(x, trunc=False):
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    if trunc:
        hf = h.astype(F32)
        over = (np.abs(hf) > np.abs(x)) & np.isfinite(hf)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(F32)


def round_e4m3(x):
    """Nearest e4m3 value (ties to even), saturating at +-448; subnormals in steps of 2^-9."""
    x = np.asarray(x, np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -9)))
    step = 2.0 ** (np.maximum(e, -6.0) - 3.0)
    return np.clip(np.rint(x / step) * step, -448.0, 448.0)


def round_to(fmt, x, trunc=False):
    return {"bf16": round_bf16, "f16": round_f16}[fmt](x, trunc)


# ------------------------------------------------------------------------------------------------ GELU restatements
PK_COEF = [3.214934915e-08, -2.075321994e-06, 5.740229389e-05, -9.056365499e-04, 9.218766509e-03, -6.556460516e-02, 3.986083959e-01]
PK9_COEF = [3.569422188e-11, -3.754043298e-09, 1.740845335e-07, -4.724864539e-06, 8.429298032e-05, -1.054992317e-03, 9.643027559e-03,
            -6.607642770e-02, 3.987614810e-01]
ERF_COEF = [-0.29844723923966754, 1.5048025775340452, -2.0855161249300567, 2.040068178110667, -0.7490454190655901, 0.4310967998728252,
            0.15704123123125485]

FAULTS_GELU_POLY = ["coef0", "coef3", "coef_last", "clamp3", "noclamp", "tanh"]
FAULTS_GELU_ERF = ["coef0", "coef3", "coef_last", "tanh"]


def _coefs(c, fault):
    c = list(c)
    if fault in ("coef0", "coef3", "coef_last"):
        i = {"coef0": 0, "coef3": 3, "coef_last": len(c) - 1}[fault]
        c[i] *= 1.01
    return [F32(v) for v in c]


def gelu_tanh_f32(x):
    """The tanh-form GELU (the imitated fault "tanh"), in fp64 rounded once: the best any fp32 kernel of that form could do."""
    x = np.asarray(x, np.float64)
    return (0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))).astype(F32)


def _phi_poly(x, coef, clamp, fault):
    x = np.asarray(x, F32)
    X = {"clamp3": 3.0, "noclamp": None}.get(fault, clamp)
    xc = x if X is None else np.clip(x, F32(-X), F32(X))
    with np.errstate(over="ignore", invalid="ignore"):
        s = _mul(xc, xc)
        c = _coefs(coef, fault)
        q = np.full(x.shape, c[0], F32)
        for ci in c[1:]:
            q = fma(q, s, ci)
        return fma(xc, q, F32(0.5))


def phi_pk(x, fault=None):
    return _phi_poly(x, PK_COEF, CLAMP_PK, fault)


def phi_pk9(x, fault=None):
    return _phi_poly(x, PK9_COEF, CLAMP_PK9, fault)


def gelu_pk(x, fault=None):
    if fault == "tanh":
        return gelu_tanh_f32(x)
    with np.errstate(over="ignore", invalid="ignore"):
        return _mul(x, phi_pk(x, fault))


def gelu_pk9(x, fault=None):
    if fault == "tanh":
        return gelu_tanh_f32(x)
    with np.errstate(over="ignore", invalid="ignore"):
        return _mul(x, phi_pk9(x, fault))


def gelu_erf_pk(x, fault=None):
    if fault == "tanh":
        return gelu_tanh_f32(x)
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        hx = _mul(x, F32(0.5))
        hax = np.abs(hx)
        z = _mul(hax, F32(1.41421356237309504880))
        den = fma(z, F32(0.3275911), F32(1.0))
        t = rcp(den)
        c = _coefs(ERF_COEF, fault)
        q = np.full(x.shape, c[0], F32)
        for ci in c[1:]:
            q = fma(q, t, ci)
        q = _mul(q, t)
        a = _mul(z, _mul(z, F32(-1.44269504088896340736)))
        e = exp2(a)
        erfz = fma(-q, e, F32(1.0))
        return fma(hax, erfz, hx)


def gelu_erff(x, fault=None):
    """f32_tile.hip: 0.5f * x * (1.f + erff(x * 0.70710678f)), erff correctly rounded here (ocml: 2 ulps at the worst)."""
    if fault == "tanh":
        return gelu_tanh_f32(x)
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = _mul(x, F32(0.70710678118654752440))
        er = np.asarray(_erf(t.astype(np.float64)), np.float64).astype(F32)
        return _mul(_mul(F32(0.5), x), (F32(1.0) + er).astype(F32))


GELU_FORMS = {"pk": gelu_pk, "pk9": gelu_pk9, "erf_pk": gelu_erf_pk, "erff": gelu_erff}

# What the source states (gemm_kernel.hpp): gelu_pk max |dPhi| 8.3e-5 -> |x| x that; gelu_pk9 3.8e-5 absolute inside its clamp;
# gelu_erf_pk 4.2e-7 absolute.  test_pointwise_cpu.py confirms each on >= 2 million points with the restatement before the GPU test
# relies on it (measured there: 8.25e-5 |x|, 3.82e-5 -> see STATED_PK9, 3.0e-7).
STATED_PK_REL = 8.3e-5
STATED_PK9_ABS = 3.8e-5
STATED_ERF_ABS = 4.2e-7


def _half_ulp(fmt, y, scale=1.0):
    """Half a unit in the last place of the stored format at |y| (one correct rounding of the stored result)."""
    ay = np.abs(np.asarray(y, np.float64))
    e = np.floor(np.log2(np.maximum(ay, 1e-300)))
    if fmt == "bf16":
        return 2.0 ** (np.maximum(e, -126.0) - 8.0)
    if fmt == "f16":
        return 2.0 ** (np.maximum(e, -14.0) - 11.0)
    if fmt == "f32":
        return 2.0 ** (np.maximum(e, -126.0) - 24.0)
    if fmt == "split16":   # hi = f16(s y), lo = f16(s y - hi): each half an fp16 ulp of what it rounds; lo's subnormal step is 2^-24
        return (2.0 ** -22 * ay * scale + 2.0 ** -25) / scale
    if fmt == "splitx":    # lo is kept as e4m3(lo 2^4): 2^-4 relative of |lo| <= 2^-11 |s y|, subnormal step 2^-9 / 2^4
        return (2.0 ** -15 * ay * scale + 2.0 ** -14) / scale
    raise ValueError(fmt)


def gelu_approx_bound(form, x):
    """|approximation - gelu| allowed at x, from the source-stated bounds inside the clamps and from the RESTATEMENT at the clamp
    outside them: there the kernel computes x Phi_poly(+-X), so its error is |x| |Phi_poly(+-X) - Phi(x)| <=
    |x| (|Phi_poly(+-X) - limit| + |limit - Phi(x)|) with limit = 0 or 1.  Plus the fp32 evaluation's own rounding, 2^-23 |gelu|."""
    x = np.asarray(x, np.float64)
    ax = np.abs(x)
    y = np.abs(gelu(x))
    if form in ("pk", "pk9"):
        X = CLAMP_PK if form == "pk" else CLAMP_PK9
        pf = phi_pk if form == "pk" else phi_pk9
        lim = np.where(x < 0, 0.0, 1.0)
        edge = np.where(x < 0, float(pf(F32(-X))), float(pf(F32(X))))
        outside = ax * (np.abs(edge - lim) + np.abs(lim - phi(x)))
        inside = STATED_PK_REL * ax if form == "pk" else np.full(x.shape, STATED_PK9_ABS)
        b = np.where(ax > X, outside, inside)
        return b + U23 * (y + b)
    if form == "erf_pk":
        return STATED_ERF_ABS + U23 * y
    if form == "erff":
        # erff (<= 2 ulps of a value <= 1: 2 x 2^-24), the rounding of 1 + erf (2^-24) -> 3 x 2^-24 on a factor that multiplies x / 2;
        # the argument's rounding moves erf by <= 2^-24 |t| erf'(t) <= 0.5 x 2^-24 more; two roundings of the products
        return 3.5 * U24 * ax / 2 + 2 * U24 * y
    raise ValueError(form)


def check_gelu(form, fmt, x, out, scale=1.0):
    """out: the stored result as fp64 values, x: the fp32 pre-activation.  Element-wise |out - gelu(x)| <= approximation bound(x) +
    one rounding of the stored format (taken at |gelu| + the bound: the approximation may sit in the next binade)."""
    x64, out = np.asarray(x, np.float64), np.asarray(out, np.float64)
    y = gelu(x64)
    ab = gelu_approx_bound(form, x64)
    bar = ab + _half_ulp(fmt, np.abs(y) + ab, scale)
    finite = np.isfinite(out)
    err = np.where(finite, np.abs(out - y), np.inf)
    ratio = err / bar
    i = int(np.argmax(ratio))
    ok = bool(finite.all() and (ratio <= 1.0).all())
    return ok, float(ratio.flat[i]), 1.0, f"gelu {form}/{fmt}: max err/bar {ratio.flat[i]:.3f} at x={x64.flat[i]:.9g} (err {err.flat[i]:.3e}, bar {bar.flat[i]:.3e}); max |err| {np.max(err):.3e}"


TAIL_X = [-8.0, -12.0, -30.0, -100.0, -1000.0]


def gelu_tail_expect(form):
    """(lo, hi) the output at each TAIL_X must lie in, before the stored format's rounding (added by the check).
    gelu_pk: POSITIVE, x Phi_poly(-3.9) from the restatement (+3.4e-5 |x|: the pinned defect of the seven-coefficient form);
    gelu_pk9: x Phi_poly9(-4.4), positive too and 1300 times smaller (+2.6e-8 |x|); erf forms: between gelu(x) - bound and +0."""
    res = []
    for xv in TAIL_X:
        if form in ("pk", "pk9"):
            p = float((phi_pk if form == "pk" else phi_pk9)(F32(xv)))
            v = xv * p
            res.append((v - abs(v) * 4 * U23, v + abs(v) * 4 * U23))
        else:
            b = float(gelu_approx_bound(form, np.float64(xv)))
            res.append((float(gelu(xv)) - b, 0.0))
    return res


def check_gelu_tails(form, fmt, x, out, scale=1.0):
    """Sign and magnitude at x = -8 ... -1000 (every occurrence in x)."""
    x, out = np.asarray(x, np.float64).ravel(), np.asarray(out, np.float64).ravel()
    ok, lines, found = True, [], 0
    for xv, (lo, hi) in zip(TAIL_X, gelu_tail_expect(form)):
        m = x == xv
        found += int(m.any())
        if not m.any():
            continue
        o = out[m]
        slack = float(_half_ulp(fmt, max(abs(lo), abs(hi)), scale))
        good = bool(np.all((o >= lo - slack) & (o <= hi + slack)))
        if form in ("pk", "pk9"):
            good = good and bool(np.all(o > 0))           # the pinned wrong sign: Phi_poly(-X) < 0 in both polynomial forms
        else:
            good = good and bool(np.all(o <= 0))
        ok = ok and good
        lines.append(f"x={xv:g}: out in [{o.min():.4e}, {o.max():.4e}] expect [{lo:.4e}, {hi:.4e}] +- {slack:.1e}")
    return ok and found == len(TAIL_X), float(found), float(len(TAIL_X)), f"gelu tails {form}/{fmt}: " + "; ".join(lines)


# ------------------------------------------------------------------------------------------------ SiLU restatements
FAULTS_SILU = ["exp_scale"]
LOG2E = 1.44269504088896340736


def silu_gate_exp2(x1, x2, fault=None):
    """v0 / (1.f + exp2(-v0 * log2 e)) * v1 (the bf16 / fp16 / fp8 epilogues).  fault exp_scale: the scale of exp in place of exp2's (1)."""
    x1, x2 = np.asarray(x1, F32), np.asarray(x2, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        t = _mul(-x1, F32(1.0 if fault == "exp_scale" else LOG2E))
        d = (F32(1.0) + exp2(t)).astype(F32)
        return _mul((x1.astype(np.float64) / d.astype(np.float64)).astype(F32), x2)


def silu_gate_expf(x1, x2, fault=None):
    """v0 / (1.f + expf(-v0)) * v1 (split formats, gemm_f32); expf correctly rounded here (ocml: 1 ulp)."""
    x1, x2 = np.asarray(x1, F32), np.asarray(x2, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        e = np.exp(-x1.astype(np.float64)).astype(F32) if fault != "exp_scale" else np.exp2(-x1.astype(np.float64)).astype(F32)
        d = (F32(1.0) + e).astype(F32)
        return _mul((x1.astype(np.float64) / d.astype(np.float64)).astype(F32), x2)


def silu_bar_rel(form, x1):
    """Relative bar on silu(x1) x2 in units of 2^-23 ("fp32 ulps", an ulp taken at its largest, 2^-23 of the value).
    expf form: 2 (exp 1 ulp, then 1 + e, the quotient and the product at half an ulp each: 2^-23 + 1.5 x 2^-24 < 2 x 2^-23).
    exp2 form: the restatement shows it needs more for large |x1| -- the argument -x1 log2 e is rounded to fp32 (2^-24 |t|) and so is
    the constant (2^-25 |t| at the worst), which moves exp2 by ln 2 x |t| x 1.5 x 2^-24 = 0.75 |x1| x 2^-23 relative, and where
    exp dominates the denominator (x1 << 0) all of it reaches the result: 2 + 0.75 |x1| fp32 ulps.  test_pointwise_cpu.py holds the
    restatement to this bar / 1.25 (the margin for the 1-ulp hardware exp2)."""
    ax = np.abs(np.asarray(x1, np.float64))
    return (2.0 + (0.75 * ax if form == "exp2" else 0.0)) * U23


def check_silu(form, fmt, x1, x2, out, scale=1.0, margin=1.0):
    x1, x2, out = np.asarray(x1, np.float64), np.asarray(x2, np.float64), np.asarray(out, np.float64)
    y = silu(x1) * x2
    # + the floor where exp(-x1) overflows fp32 (x1 < -88.72) and the kernel returns a zero: |silu| < 89 x 2^-128 there
    ab = silu_bar_rel(form, x1) * np.abs(y) / margin + 89.0 * 2.0 ** -128 * np.abs(x2)
    bar = ab + (_half_ulp(fmt, np.abs(y) + ab, scale) if fmt else 0.0)
    finite = np.isfinite(out)
    err = np.where(finite, np.abs(out - y), np.inf)
    ratio = err / bar
    i = int(np.argmax(ratio))
    ok = bool(finite.all() and (ratio <= 1.0).all())
    # x1 <= -90: exp2 / expf overflow to inf and the quotient must be a zero (of the sign of -x2), never NaN
    far = x1 <= -90.0
    zeros_ok = bool(np.all(out[far] == 0.0)) if far.any() else True
    return ok and zeros_ok, float(ratio.flat[i]), 1.0, (f"silu {form}/{fmt}: max err/bar {ratio.flat[i]:.3f} at x1={x1.flat[i]:.9g} x2={x2.flat[i]:g} "
                                                        f"(err {err.flat[i]:.3e}, bar {bar.flat[i]:.3e}); x1 <= -90 all zero: {zeros_ok}")


# ------------------------------------------------------------------------------------------------ LayerNorm restatements
FAULTS_LN2 = ["eps_outside", "unbiased", "mean_len"]
FAULTS_FOLD = ["no_fmax", "eps_outside", "unbiased", "mean_len"]


def _butterfly(v):
    """Sum over the last axis (a power of two) by xor-butterfly, fp32: every lane ends with the same total."""
    n = v.shape[-1]
    idx = np.arange(n)
    off = 1
    while off < n:
        v = (v + v[..., idx ^ off]).astype(F32)
        off *= 2
    return v[..., 0]


def _rstd(var, eps, fault, D):
    var = np.asarray(var, F32)
    if fault == "unbiased":
        var = (var * F32(D / (D - 1.0))).astype(F32)
    if fault == "eps_outside":
        with np.errstate(divide="ignore"):
            return (1.0 / (np.sqrt(var.astype(np.float64)).astype(F32) + F32(eps)).astype(np.float64)).astype(F32)
    return rsqrt((var + F32(eps)).astype(F32))


def layernorm_two_pass_f32(x, weight, bias, eps=LN_EPS, vec=None, fault=None):
    """layernorm_kernel: a lane holds VEC consecutive floats of every 64 x VEC chunk, sums its own sequentially, then a wave butterfly."""
    x = np.asarray(x, F32)
    rows, D = x.shape
    vec = vec or (4 if D % 256 == 0 else 2)
    nv = D // (64 * vec)
    v = x.reshape(rows, nv, 64, vec)
    Dm = F32(D + 1 if fault == "mean_len" else D)
    s = np.zeros((rows, 64), F32)
    for i in range(nv):
        for e in range(vec):
            s = (s + v[:, i, :, e]).astype(F32)
    mean = (_butterfly(s) / Dm).astype(F32)
    ss = np.zeros((rows, 64), F32)
    for i in range(nv):
        for e in range(vec):
            d = (v[:, i, :, e] - mean[:, None]).astype(F32)
            ss = fma(d, d, ss)
    rstd = _rstd((_butterfly(ss) / F32(D)).astype(F32), eps, fault, D)
    d = (x - mean[:, None]).astype(F32)
    return fma(_mul(d, rstd[:, None]), np.asarray(weight, F32)[None], np.asarray(bias, F32)[None]), mean, rstd


def fold_partials_f32(x):
    """Epilogue 7's share of the statistics: per 128 columns, 32 lanes x float4 -- (x + y) + (z + w) and fma(x, x, y y) + fma(z, z, w w)
    per lane, then a 32-lane butterfly.  -> [parts, rows, 2]."""
    x = np.asarray(x, F32)
    rows, D = x.shape
    v = x.reshape(rows, D // 128, 32, 4)
    s1 = ((v[..., 0] + v[..., 1]).astype(F32) + (v[..., 2] + v[..., 3]).astype(F32)).astype(F32)
    s2 = (fma(v[..., 0], v[..., 0], _mul(v[..., 1], v[..., 1])) + fma(v[..., 2], v[..., 2], _mul(v[..., 3], v[..., 3]))).astype(F32)
    return np.stack([_butterfly(s1), _butterfly(s2)], -1).transpose(1, 0, 2)


def ln_finalize_f32(stats, D, eps=LN_EPS, fault=None):
    """ln_finalize_kernel: add the parts in slot order; mu = s1 / D; rstd = rsqrt(fmaxf(s2 / D - mu^2, 0) + eps) -> (rstd, mu rstd)."""
    stats = np.asarray(stats, F32)
    s1 = np.zeros(stats.shape[1], F32)
    s2 = np.zeros(stats.shape[1], F32)
    for p in range(stats.shape[0]):
        s1 = (s1 + stats[p, :, 0]).astype(F32)
        s2 = (s2 + stats[p, :, 1]).astype(F32)
    inv = F32(1.0) / F32(D)
    inv_m = F32(1.0) / F32(D + 1) if fault == "mean_len" else inv
    mu = _mul(s1, inv_m)
    var = (_mul(s2, inv) - _mul(mu, mu)).astype(F32)
    if fault != "no_fmax":
        var = np.maximum(var, F32(0))
    with np.errstate(invalid="ignore"):
        rs = _rstd(var, eps, fault, D)
    return np.stack([rs, _mul(mu, rs)], -1)


def kappa_of(x):
    """E[x^2] / var of each row in fp64 (inf for a constant row): what the single-pass variance loses, in units of the fp32 unit."""
    x = np.asarray(x).astype(np.float64)
    _, mu, var = layernorm(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(var > 0, (x ** 2).mean(-1) / var, np.inf)


# ------------------------------------------------------------------------------------------------ input generators
SPECIAL_COLS = 64
NEGZERO_SPECIAL = 19   # index of the second 0.0 among the specials: the fp8 epilogue, (acc + bias) * col_scale, turns it into -0 through a negative
                       # col_scale; every other epilogue adds the bias to a +0 accumulator, which can give +0 only (-0 is unreachable there)


def specials(fmt):
    """The 64 pre-activations every row meets through the bias alone (fp32, exact): both sides of each clamp to one fp32 step, +0, tiny
    values of both signs, the tails, and for the 16-bit formats values whose result sits near the largest finite output."""
    v = []
    for c in (CLAMP_PK, CLAMP_PK9, 3.0):
        c32 = F32(c)
        for s in (1, -1):
            v += [s * c32, s * np.nextafter(c32, F32(10)), s * np.nextafter(c32, F32(0))]
    v += [0.0, 0.0, 1e-30, -1e-30, 2.0 ** -140, -2.0 ** -140, 1e-6, -1e-6]
    for m in (8.0, 12.0, 30.0, 100.0, 1000.0):
        v += [m, -m]
    v += [-90.0, -88.0, -87.0, -104.0, 88.5, 5.0, -5.0, 6.0, -6.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 0.7978846, -0.7517916]
    # ties of the two 16-bit formats (to even: down, then up) and values that round up to a power of two
    v += [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.9999, 0.99999, -1.9999]
    if fmt == "bf16":
        v += [3.0e38, -3.0e38, 1.0e30]
    elif fmt == "f16":
        v += [65000.0, 60000.0, -65000.0]
    else:
        v += [20.0, -20.0, 50.0]
    v = np.asarray(v, F32)
    assert v.size <= SPECIAL_COLS and v[NEGZERO_SPECIAL] == 0 and v[NEGZERO_SPECIAL - 1] == 0, v.size
    return np.concatenate([v, np.linspace(-4.5, 4.5, SPECIAL_COLS - v.size).astype(F32)])


# pieces per value and K of the exactness construction, per operand format
PIECES = {"bf16": 2, "f16": 2, "fp8": 4, "split16": 1, "splitx": 1, "f32": 1}
GRID_K = {"bf16": 128, "f16": 128, "fp8": 128, "split16": 64, "splitx": 64, "f32": 64}
FP8_COL_SCALE = 2.0 ** -5   # e4m3 pieces span +-448 in steps >= 2^-9: x (acc x 2^-5) reaches +-14 in steps of 2^-14


def _pieces(fmt, t):
    """Target fp64 values t -> (pieces [..., P] as fp64 values each representable in the operand format, realised exact sum)."""
    t = np.asarray(t, np.float64).astype(F32).astype(np.float64)      # an fp32 target: every piece then lies inside its 24-bit span
    if fmt in ("bf16", "f16"):
        r = round_bf16 if fmt == "bf16" else round_f16
        hi = r(t.astype(F32)).astype(np.float64)
        lo = r((t - hi).astype(F32)).astype(np.float64)
        return np.stack([hi, lo], -1), hi + lo
    if fmt == "fp8":
        # The fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4) does NOT add its 64 products exactly: measured on the MI355X with these very operands, every
        # product is aligned to the largest one of the instruction and what lies below 2^-13 of that one's binade is cut off (toward zero) -- the model
        # "truncate each piece at 2^(e_max - 13)" reproduces all 65 536 outputs bit for bit.  So the value is first rounded to 12 bits below its leading
        # piece's binade (one bit to spare); every e4m3 piece of it is then a multiple of that step and the sum is exact in the instruction too.
        u = t / FP8_COL_SCALE
        e1 = np.floor(np.log2(np.maximum(np.abs(round_e4m3(u)), 2.0 ** -9)))
        step = 2.0 ** np.maximum(e1 - 12.0, -9.0)
        u = np.rint(u / step) * step
        ps, rem = [], u.copy()
        for _ in range(4):
            p = round_e4m3(rem)
            ps.append(p)
            rem = rem - p
        assert not rem.any(), "four e4m3 pieces hold a 13-bit value"
        ps = np.stack(ps, -1)
        assert np.all(np.abs(ps) % step[..., None] == 0)
        return ps, ps.sum(-1) * FP8_COL_SCALE
    if fmt in ("split16", "splitx"):
        # one fp32 value per k; the packers split it.  Kept to 15 significant bits (and a multiple of 2^-19) so that hi + lo -- fp16 + fp16,
        # or fp16 + e4m3 -- holds it exactly at the packing scales the tests use (asserted there on the packed operand itself)
        e = np.floor(np.log2(np.maximum(np.abs(t), 2.0 ** -5)))
        step = 2.0 ** (e - 14)
        v = np.rint(t / step) * step
        return v[..., None], v
    v = t.astype(F32).astype(np.float64)
    return v[..., None], v


def preact_grid(fmt, swiglu=False):
    """The operands of one 256 x 256 launch whose fp32 pre-activations are known exactly, and those pre-activations.

    -> dict(a [256, K] fp64 values (each representable in the operand format), w [256, K] 0/1, bias [256] fp32, x [256, L] fp32,
            x2 [256, L] fp32 or None, col_scale).  L = 256 logical columns (SwiGLU: 128 pairs, N = 256 interleaved (x1, x2)).
    Logical column c < L - 64 selects slot c % S of the row (S = K / pieces values per row, each in `pieces` k positions); its bias is 0
    for c < S and a small fp32 offset beyond (the fp32 add of the epilogue then lands on values with full mantissas).  The last 64
    logical columns select nothing and carry specials(fmt) in the bias: every row, so every lane position, meets every special.
    Slot values: dense on [-6, 6] (the first 192 rows x S slots, stratified), then [-12, 12], then log-spaced magnitudes 2^-20 .. 16."""
    P, K = PIECES[fmt], GRID_K[fmt]
    S = K // P
    L = 128 if swiglu else 256
    rng = np.random.default_rng(1234 + P + K)
    n = 256 * S
    u = (np.arange(n) + rng.random(n)) / n
    t = np.empty(n)
    nd = 192 * S
    t[:nd] = -6.0 + 12.0 * (np.arange(nd) + rng.random(nd)) / nd
    nw = 32 * S
    t[nd:nd + nw] = -12.0 + 24.0 * (np.arange(nw) + rng.random(nw)) / nw
    nl = n - nd - nw
    t[nd + nw:] = np.where(np.arange(nl) % 2 == 0, 1.0, -1.0) * 2.0 ** (-20.0 + 24.0 * u[:nl])
    t = t[rng.permutation(n)].reshape(256, S)
    pieces, real = _pieces(fmt, t)
    a = pieces.reshape(256, K)
    sel = np.zeros((L, K))
    cols = np.arange(L - SPECIAL_COLS)
    for p in range(P):
        sel[cols, (cols % S) * P + p] = 1.0
    bias = np.zeros(L, F32)
    off = cols >= S
    bias[:L - SPECIAL_COLS][off] = ((cols[off] - S + 1) * F32(0.0123457)).astype(F32) * np.where(cols[off] % 2 == 0, 1, -1).astype(F32)
    bias[L - SPECIAL_COLS:] = specials(fmt)
    acc = np.zeros((256, L))
    acc[:, :L - SPECIAL_COLS] = real[:, cols % S]
    acc32 = acc.astype(F32)
    assert np.array_equal(acc32.astype(np.float64), acc), "the accumulator must be exact in fp32"
    with np.errstate(over="ignore"):
        x = (acc32 + bias[None, :]).astype(F32)      # the epilogue's fp32 add (an fma with a power-of-two scale rounds the same)
    cscale = np.full(L, FP8_COL_SCALE if fmt == "fp8" else 1.0, F32)
    out = dict(fmt=fmt, a=a, x=x, x2=None, col_scale=cscale, S=S, P=P, K=K)
    if fmt == "fp8":
        cscale[L - SPECIAL_COLS + NEGZERO_SPECIAL] *= -1
        x[:, L - SPECIAL_COLS + NEGZERO_SPECIAL] = -0.0                                 # the epilogue computes (acc + bias) * col_scale: bias pre-divided, both exact (power of two)
        bias = (bias.astype(np.float64) / FP8_COL_SCALE).astype(F32)
    if not swiglu:
        out.update(w=sel, bias=bias)
        return out
    x2v = np.asarray([1.0, -1.0, 3.5], F32)[np.arange(L) % 3]
    w = np.zeros((256, K))
    w[0::2] = sel
    b = np.zeros(256, F32)
    b[0::2] = bias
    b[1::2] = x2v / F32(FP8_COL_SCALE if fmt == "fp8" else 1.0)
    cs2 = np.full(256, FP8_COL_SCALE if fmt == "fp8" else 1.0, F32)
    cs2[0::2] = cscale
    out.update(w=w, bias=b, col_scale=cs2, x2=np.broadcast_to(x2v[None, :], (256, L)).copy())
    return out


LN_CLASSES = ["offset0", "offset1", "offset10", "offset100", "offset1000", "massive", "constant", "std1e-3", "alternating", "zero"]


def ln_rows(D, rows=67, seed=0):
    """-> (x [rows, D] fp32, classes [rows] of LN_CLASSES).  The rows that decide: Gaussian rows offset by {0, 1, 10, 100, 1000} std, one
    massive channel (200 to 2000 times the rest), a constant row (var = 0), a row of std 1e-3 around 1, alternating +-c, a zero row."""
    rng = np.random.default_rng(seed + D)
    x = np.zeros((rows, D), F32)
    cls = []
    for r in range(rows):
        c = LN_CLASSES[r % len(LN_CLASSES)]
        g = rng.standard_normal(D)
        std = float(2.0 ** rng.integers(-2, 3))
        if c.startswith("offset"):
            v = std * (g + float(c[6:]) * (1 if r % 20 < 10 else -1))
        elif c == "massive":
            v = std * g
            v[int(rng.integers(0, D))] = std * float(rng.uniform(200, 2000)) * (1 if r % 20 < 10 else -1)
        elif c == "constant":
            # the first three have few significant bits: every fp32 sum, so the mean, is exact in any order (the two-pass kernel then gives `bias`
            # exactly, the fold a variance of exactly 0); the others round, so the single-pass variance comes out at +-1e-1: negative for some -> fmaxf
            v = np.full(D, [3.25, -0.125, 1000.0, 1000.1, -517.3, 2.0 ** -9, 77.7][(r // 10) % 7])
        elif c == "std1e-3":
            v = 1.0 + 1e-3 * g
        elif c == "alternating":
            v = np.where(np.arange(D) % 2 == 0, 1.0, -1.0) * [0.37, 5.0, 1e-3][(r // 10) % 3]
        else:
            v = np.zeros(D)
        x[r] = v.astype(F32)
        cls.append(c)
    return x, np.asarray(cls)


# ------------------------------------------------------------------------------------------------ LayerNorm checks
LN_TREE_FACTOR = 4.0     # the kernel's summation tree is not the restatement's: 4 x the restatement's own error on the same rows


def ln_err_units(y, x, weight, bias, eps=LN_EPS):
    """Per-element |y - LayerNorm_fp64(x)| in units of what fp32 two-pass arithmetic owes there, 2^-24 x (|w| (1 + |mean| / std + |xn|) + |y|):
    x - mean carries 2^-24 (|x| + |mean|), i.e. 2^-24 std (|xn| + 2 |mean| / std), before rstd w scales it; rstd's own relative error scales
    |w xn|; the last fma rounds at |y|.  -> (units [rows, D], mean, var)."""
    ref, mu, var = layernorm(x, weight, bias, eps)
    std = np.sqrt(var + eps)
    xn = (np.asarray(x).astype(np.float64) - mu[:, None]) / std[:, None]
    w = np.abs(np.asarray(weight, np.float64))[None, :]
    shape = U24 * (w * (1.0 + (np.abs(mu) / std)[:, None] + np.abs(xn)) + np.abs(ref))
    return np.abs(np.asarray(y, np.float64) - ref) / shape, mu, var


def check_layernorm_two_pass(x, weight, bias, y, eps=LN_EPS):
    """y: the kernel's fp32 output.  Per element, error <= C x the unit of ln_err_units -- the form (1 + |mean| / std) 2^-24 grows in, with the
    element's own magnitude added -- where C = LN_TREE_FACTOR x the restatement's own constant on the same rows (measured, not assumed);
    constant rows whose sums are exact in fp32 (few significant bits) and zero rows give `bias` exactly."""
    units, mu, var = ln_err_units(y, x, weight, bias, eps)
    y_r, _, _ = layernorm_two_pass_f32(x, weight, bias, eps)
    units_r, _, _ = ln_err_units(y_r, x, weight, bias, eps)
    C = LN_TREE_FACTOR * float(units_r.max())
    # constant rows of at most 10 significant bits: every partial sum of <= 2048 of them is exact in fp32, whatever the tree
    const = np.all(np.asarray(x) == np.asarray(x)[:, :1], axis=1) & ((np.asarray(x, F32)[:, 0].view(np.uint32) & 0x3FFF) == 0)
    exact = bool(np.array_equal(np.asarray(y, F32)[const], np.broadcast_to(np.asarray(bias, F32), y.shape)[const]))
    rows = units.max(1)
    i = int(np.argmax(rows))
    ok = bool(np.isfinite(np.asarray(y, np.float64)).all() and (rows <= C).all() and exact)
    return ok, float(rows[i] / C), 1.0, (f"layernorm two-pass D={x.shape[1]}: max error {rows[i]:.2f} units (row {i}) against C = {C:.2f} = {LN_TREE_FACTOR:g} x the "
                                         f"restatement's {C / LN_TREE_FACTOR:.2f}; unit = 2^-24 (|w| (1 + |mean| / std + |xn|) + |y|); exact constant rows give bias exactly: {exact}")


def check_fold_partials(x, stats):
    """stats [parts, rows, 2] against fp64 sums of the fp32 stream: relative 2^-20 (of the sum of |addends| for the plain sums, which cancel)."""
    x64 = np.asarray(x).astype(np.float64)
    rows, D = x64.shape
    p = x64.reshape(rows, D // 128, 128)
    s1, s1a, s2 = p.sum(-1).T, np.abs(p).sum(-1).T, (p ** 2).sum(-1).T
    st = np.asarray(stats, np.float64)
    r1 = np.abs(st[..., 0] - s1) / np.maximum(s1a, 1e-300)
    r2 = np.abs(st[..., 1] - s2) / np.maximum(s2, 1e-300)
    r1, r2 = np.where(s1a == 0, np.abs(st[..., 0]), r1), np.where(s2 == 0, np.abs(st[..., 1]), r2)
    m = float(max(r1.max(), r2.max()))
    return m <= 2.0 ** -20, m, 2.0 ** -20, f"fold partial sums: max relative error {m:.3e} (bar 2^-20 = {2.0 ** -20:.3e})"


def fold_rstd_errors(x, ln_row, eps=LN_EPS):
    """Per row: (|rstd / rstd_exact - 1|, |mean rstd - exact| / (1 + |exact|), kappa)."""
    _, mu, var = layernorm(x, eps=eps)
    rs = 1.0 / np.sqrt(var + eps)
    lr = np.asarray(ln_row, np.float64)
    kap = ((np.asarray(x).astype(np.float64) ** 2).mean(-1) + eps) / (var + eps)     # eps keeps the constant rows' kappa finite: what the formula sees
    return np.abs(lr[:, 0] / rs - 1.0), np.abs(lr[:, 1] - mu * rs) / (1.0 + np.abs(mu * rs)), kap


def check_fold_rstd(x, ln_row, eps=LN_EPS):
    """rstd and mean x rstd of the single-pass statistics against fp64: bar C kappa 2^-24, C = LN_TREE_FACTOR x the single-pass
    restatement's constant on the same rows (emulated 1.2 to 2.3, so C near 8).  A constant row c gives rstd = eps^-1/2 within 1e-6
    where the algorithm's own bound allows it, (c^2 / eps) 2^-24 <= 2.5e-7 (|c| <= 2^-9 at eps = 1e-6): s2 / D and mu^2 are both c^2 to one
    rounding each, so the variance comes out at +-c^2 2^-24, not at 0, whenever 1 / D is not a power of two (measured on the GPU at D = 384,
    c = -0.125: rstd 2.3e-4 off).  Those rows are asserted for it; the others are printed."""
    x = np.asarray(x, F32)
    D = x.shape[1]
    e_rs, e_mrs, kap = fold_rstd_errors(x, ln_row, eps)
    lr_r = ln_finalize_f32(fold_partials_f32(x), D, eps)
    r_rs, r_mrs, _ = fold_rstd_errors(x, lr_r, eps)
    unit = kap * U24
    C = LN_TREE_FACTOR * float(max(np.max(r_rs / unit), np.max(r_mrs / unit)))
    ratio = np.maximum(e_rs, e_mrs) / (C * unit)
    i = int(np.argmax(ratio))
    finite = bool(np.isfinite(np.asarray(ln_row, np.float64)).all())
    const_all = np.all(x == x[:, :1], axis=1) & (x[:, 0] != 0)
    const = const_all & (x[:, 0].astype(np.float64) ** 2 / eps * U24 <= 2.5e-7)
    c_all = np.abs(np.asarray(ln_row, np.float64)[:, 0] * math.sqrt(eps) - 1.0)
    c_err = float(np.max(c_all[const])) if const.any() else 0.0
    others = ", ".join(f"c={x[i, 0]:g}: {c_all[i]:.1e}" for i in np.nonzero(const_all & ~const)[0])
    ok = finite and bool((ratio <= 1.0).all()) and c_err <= 1e-6
    return ok, float(ratio[i]), 1.0, (f"folded rstd D={D}: max err/bar {ratio[i]:.3f} (row {i}, kappa {kap[i]:.3g}, rstd err {e_rs[i]:.3e}), C = {C:.2f} = "
                                      f"{LN_TREE_FACTOR:g} x restatement's {C / LN_TREE_FACTOR:.2f}; small constant rows: |rstd sqrt(eps) - 1| = {c_err:.2e} (bar 1e-6); the other constant rows: {others}")


def fold_consumer_f32(xb, w, bias, colsum, ln_row):
    """The consumer's epilogue 0 in fp32 on an exact accumulator: fma(rstd, acc, fma(-mean rstd, colsum, bias))."""
    acc = (np.asarray(xb, np.float64) @ np.asarray(w, np.float64).T).astype(F32)
    t = fma(-np.asarray(ln_row, F32)[:, 1:2], np.asarray(colsum, F32)[None], np.asarray(bias, F32)[None])
    return fma(np.asarray(ln_row, F32)[:, 0:1], acc, t)


def check_fold_consumer(xb, stream, w, bias, out, kappa_max=200.0, eps=LN_EPS):
    """out (bf16 values) against Linear(LayerNorm_exact(xb)), the statistics being those of the fp32 `stream`, for the rows with
    kappa <= kappa_max.  Bar: one bf16 rounding (half an ulp at the exact value) + what the algorithm's own rstd error moves the
    result by: C kappa 2^-24 (C = 8, the bar of check_fold_rstd) x (|rstd acc| + |mean rstd colsum|) + 2^-22 of those terms for the
    fp32 epilogue.  All rows must be finite."""
    xb64, w64 = np.asarray(xb, np.float64), np.asarray(w, np.float64)
    _, mu, var = layernorm(stream, eps=eps)
    rs = 1.0 / np.sqrt(var + eps)
    acc = xb64 @ w64.T
    cs = w64.sum(1)
    ref = rs[:, None] * acc - (mu * rs)[:, None] * cs[None, :] + np.asarray(bias, np.float64)[None, :]
    mag = np.abs(rs[:, None] * acc) + np.abs((mu * rs)[:, None] * cs[None, :])
    kap = ((np.asarray(stream).astype(np.float64) ** 2).mean(-1) + eps) / (var + eps)
    ab = (8.0 * kap[:, None] * U24 + 2.0 ** -22) * mag
    bar = _half_ulp("bf16", np.abs(ref) + ab) + ab
    out = np.asarray(out, np.float64)
    sel = kap <= kappa_max
    ratio = np.abs(out - ref) / bar
    finite = bool(np.isfinite(out).all())
    m = float(ratio[sel].max())
    return finite and m <= 1.0, m, 1.0, f"folded consumer: max err/bar {m:.3f} over {int(sel.sum())} rows with kappa <= {kappa_max:g}; all finite: {finite}"
