"""The counter-based generator of csrc/las_common.h (las_mix32, las_uniform, las_normal) and every entry point that draws from it
(csrc/rng.hip, sample_features_kernel of csrc/decoder.hip) restated in NumPy from their contracts in include/las_hip.h.

The generator is 32-bit integer arithmetic followed by an exact scaling, (h >> 8) * 2^-24, so it is restated bit for bit; every
threshold decision (u < keep, u < prob) is then exact too.  The fp32 arithmetic around it follows each kernel's own operations:
the forward dropout multiplies by the fp32 reciprocal 1/keep, las_add_masked divides by keep, las_dropout_bwd forms
a * m_a and then fma(b, m_b, .) (the compiler contracts that sum).  bf16 stores round to nearest even, as the (__bf16) cast of
las_f2bf does (v_cvt_pk_bf16_f32).  The transcendental parts (Box-Muller, the Gumbel perturbation, the sigmoid) are restated in
float64; the device uses fast fp32 approximations, so those are compared with a margin.  Imports nothing from the project."""
import numpy as np

U32 = np.uint32
F32 = np.float32
M32 = 0xFFFFFFFF
TWO_M24 = F32(1.0 / 16777216.0)
NORMAL_CLAMP = F32(1e-12)                       # fmaxf(u1, 1e-12f) of las_normal and of the Gumbel step
Z_MAX = float(np.sqrt(-2.0 * np.log(np.float64(NORMAL_CLAMP))))    # the largest |z| Box-Muller can give

SELECT_STREAM = 0x5e1ec7        # "sample at this step?" of las_sample_tokens / las_sample_features, index step*B + b
GUMBEL_STREAM = 0x9a3b1e        # las_sample_tokens' Gumbel draws, index (step*B + b)*V + v
FEATURE_STREAM = 0xb17f00d      # las_sample_features' Bernoulli draws, index (step*B + b)*nf + f


def mix32(x):
    x = np.asarray(x, dtype=U32).copy()
    x ^= x >> U32(16)
    x *= U32(0x7feb352d)
    x ^= x >> U32(15)
    x *= U32(0x846ca68b)
    x ^= x >> U32(16)
    return x


def uniform_bits(seed, stream, idx):
    """The 24-bit integer h >> 8 behind las_uniform(seed, stream, idx); idx: anything castable to uint64."""
    idx = np.asarray(idx, dtype=np.uint64)
    key = U32((int(seed) ^ ((int(stream) * 0x9E3779B9) & M32)) & M32)
    with np.errstate(over='ignore'):
        h = mix32(np.full(idx.shape, key, dtype=U32))
        h = mix32(h ^ (idx & np.uint64(M32)).astype(U32))
        hi = (idx >> np.uint64(32)).astype(U32)
        h = mix32(h + hi * U32(0x85EBCA6B) + U32(0x632BE5AB))
    return h >> U32(8)


def uniform(seed, stream, idx):
    """las_uniform: float32 in [0, 1) on the 2^-24 grid (the scaling is exact)."""
    return uniform_bits(seed, stream, idx).astype(F32) * TWO_M24


def normal(seed, stream, i):
    """las_normal draw(s) i in float64: Box-Muller on the uniforms 2i and 2i+1, u1 clamped at 1e-12f, 2*pi as the fp32
    constant the kernel multiplies by."""
    i = np.asarray(i, dtype=np.uint64)
    u1 = np.maximum(uniform(seed, stream, 2 * i), NORMAL_CLAMP).astype(np.float64)
    u2 = uniform(seed, stream, 2 * i + 1).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(np.float64(F32(6.2831853)) * u2)


# ---- fp32 / bf16 arithmetic -------------------------------------------------------------------------------------------------
def f2bf(x):
    """fp32 -> bf16 bits, round to nearest even (NaN stays a quiet NaN of the same sign)."""
    x = np.asarray(x, dtype=F32)
    b = x.view(U32)
    with np.errstate(over='ignore'):
        r = (b + U32(0x7FFF) + ((b >> U32(16)) & U32(1))) >> U32(16)
    nan = np.isnan(x)
    r = np.where(nan, (b >> U32(16)) | U32(0x40), r)
    return r.astype(np.uint16)


def bf2f(u):
    return (np.asarray(u, dtype=np.uint16).astype(U32) << U32(16)).view(F32)


def fma32(x, y, z):
    """fp32 fma(x, y, z), one rounding: x*y is exact in float64, and a float64 sum that lands on an fp32 midpoint is
    resolved by the sign of its TwoSum error (the only case where rounding twice differs from rounding once)."""
    x, y, z = (np.asarray(a, dtype=F32) for a in (x, y, z))
    p = x.astype(np.float64) * y.astype(np.float64)
    zz = z.astype(np.float64)
    s = p + zz
    bb = s - p
    err = (p - (s - bb)) + (zz - bb)
    r = s.astype(F32)
    toward = np.nextafter(r, np.where(s > r.astype(np.float64), F32(np.inf), F32(-np.inf)))
    mid = (s != r.astype(np.float64)) & (2.0 * s == r.astype(np.float64) + toward.astype(np.float64))
    fix = mid & (err != 0) & ((err > 0) == (s > r.astype(np.float64)))
    return np.where(fix, toward, r)


def keep_factor(u, keep):
    """(u < keep ? 1/keep : 0) in fp32, the reciprocal formed as the kernels form it (IEEE fp32 division)."""
    keep = F32(keep)
    return np.where(u < keep, F32(1.0) / keep, F32(0.0)).astype(F32)


# ---- the entry points -------------------------------------------------------------------------------------------------------
def dropout_mask(total, keep, seed, stream):
    """las_dropout_mask: out[i] = (u_i < keep) / keep, fp32."""
    return keep_factor(uniform(seed, stream, np.arange(total, dtype=np.uint64)), keep)


def dropout_bf16(x, keep, seed, stream):
    """las_dropout_bf16 on the logical [rows, cols] bf16 bits x (the row strides only place the rows): element (r, c) is draw
    r*cols + c, y = bf16(f32(x) * (1/keep or 0))."""
    x = np.asarray(x, dtype=np.uint16)
    rows, cols = x.shape
    m = dropout_mask(rows * cols, keep, seed, stream).reshape(rows, cols)
    return f2bf(bf2f(x) * m)


def dropout_bf16_pair(x, keep, seed, stream0, stream1):
    """las_dropout_bf16_pair: the two streams' las_dropout_bf16 of the same input."""
    return dropout_bf16(x, keep, seed, stream0), dropout_bf16(x, keep, seed, stream1)


def dropout_bf16_steps(x, keep, seed, stream0, idx_cols=0):
    """las_dropout_bf16_steps on the logical [B, U, cols] bits x: element (b, t, c) is draw (stream0 + t, b*idx_cols + c)."""
    x = np.asarray(x, dtype=np.uint16)
    B, U, cols = x.shape
    idx_cols = idx_cols if idx_cols > 0 else cols
    out = np.empty_like(x)
    idx = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(idx_cols) + np.arange(cols, dtype=np.uint64)[None, :])
    for t in range(U):
        m = keep_factor(uniform(seed, (stream0 + t) & M32, idx), keep)
        out[:, t] = f2bf(bf2f(x[:, t]) * m)
    return out


def dropout_bwd(a, b, keep, seed, stream_a, stream_b):
    """las_dropout_bwd on contiguous fp32 [rows, cols]: a*m_a, then fma(b, m_b, that) when b is given."""
    a = np.asarray(a, dtype=F32)
    n = a.size
    ma = dropout_mask(n, keep, seed, stream_a).reshape(a.shape)
    v = (a * ma).astype(F32)
    if b is None:
        return v
    mb = dropout_mask(n, keep, seed, stream_b).reshape(a.shape)
    return fma32(np.asarray(b, dtype=F32), mb, v)


def onehot_bf16(ids, V, ldo, keep, seed, stream, feed_width):
    """las_onehot_bf16: ids [B, U] int; out [B*U, ldo] bf16 bits, row b*U + t holds bf16(scale) at column ids[b, t] when
    0 <= id < V (else the row stays zero), scale = 1 if keep >= 1 else (u < keep ? 1/keep : 0) of draw
    ((t*B + b)*feed_width + id) (the token scale of dec_step_fwd)."""
    ids = np.asarray(ids, dtype=np.int64)
    B, U = ids.shape
    out = np.zeros((B * U, ldo), dtype=np.uint16)
    for b in range(B):
        for t in range(U):
            i = int(ids[b, t])
            if not 0 <= i < V:
                continue
            sc = F32(1.0)
            if F32(keep) < F32(1.0):
                idx = ((t * B + b) * feed_width + i) & 0xFFFFFFFFFFFFFFFF
                sc = keep_factor(uniform(seed, stream, np.uint64(idx)), keep)
            out[b * U + t, i] = f2bf(F32(sc))
    return out


def add_masked(a, b, keep, seed, stream, idx_base, idx_ld):
    """las_add_masked on the logical [rows, cols] fp32 b (and a, None = zero): v = b, masked as (u < keep ? v / keep : 0) at
    draw idx_base + r*idx_ld + c when keep < 1, then v + a."""
    b = np.asarray(b, dtype=F32)
    rows, cols = b.shape
    v = b.copy()
    if F32(keep) < F32(1.0):
        idx = (np.uint64(idx_base) + np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(idx_ld)
               + np.arange(cols, dtype=np.uint64)[None, :])
        u = uniform(seed, stream, idx)
        v = np.where(u < F32(keep), (v / F32(keep)).astype(F32), F32(0.0)).astype(F32)
    if a is not None:
        v = (v + np.asarray(a, dtype=F32)).astype(F32)
    return v


def select(B, prob, seed, step):
    """The per-utterance decision of both samplers: u(seed, 0x5e1ec7, step*B + b) < prob."""
    return uniform(seed, SELECT_STREAM, np.uint64(step) * np.uint64(B) + np.arange(B, dtype=np.uint64)) < F32(prob)


def gumbel_scores(logits, seed, step):
    """float64 logits[b, v] - log(-log(max(u, 1e-12))) of las_sample_tokens' draws (step*B + b)*V + v."""
    logits = np.asarray(logits, dtype=F32)
    B, V = logits.shape
    idx = ((np.uint64(step) * np.uint64(B) + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(V)
           + np.arange(V, dtype=np.uint64)[None, :])
    u = np.maximum(uniform(seed, GUMBEL_STREAM, idx), NORMAL_CLAMP).astype(np.float64)
    return logits.astype(np.float64) - np.log(-np.log(u))


def sample_tokens(logits, teacher, prob, seed, step):
    """las_sample_tokens: returns (next [B] int64, selected [B] bool, margin [B]): next = the Gumbel argmax (ties to the lower
    v) where selected, else teacher[b] (0 when teacher is None); margin = the gap between the two best perturbed scores
    (inf when V == 1), the cells where the device's fast logarithms may pick the other token."""
    logits = np.asarray(logits, dtype=F32)
    B, V = logits.shape
    sel = select(B, prob, seed, step)
    g = gumbel_scores(logits, seed, step)
    arg = np.argmax(g, axis=1)
    if V > 1:
        top2 = np.sort(g, axis=1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]
    else:
        margin = np.full(B, np.inf)
    base = np.zeros(B, dtype=np.int64) if teacher is None else np.asarray(teacher, dtype=np.int64)
    return np.where(sel, arg, base), sel, margin


def sample_features(logits, teacher, prob, seed, step):
    """las_sample_features: returns (next [B, nf] bf16 bits, selected [B], margin [B, nf]): a selected row draws
    u(seed, 0xb17f00d, (step*B + b)*nf + f) < sigmoid(logits) -> bf16 1.0 / 0.0, else the teacher's bits (zeros when None);
    margin = |u - sigmoid(x)| in float64 (the device's sigmoid is rcp(1 + exp(-x)) in fast fp32)."""
    logits = np.asarray(logits, dtype=F32)
    B, nf = logits.shape
    sel = select(B, prob, seed, step)
    idx = ((np.uint64(step) * np.uint64(B) + np.arange(B, dtype=np.uint64))[:, None] * np.uint64(nf)
           + np.arange(nf, dtype=np.uint64)[None, :])
    u = uniform(seed, FEATURE_STREAM, idx).astype(np.float64)
    sig = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    drawn = np.where(u < sig, np.uint16(0x3F80), np.uint16(0)).astype(np.uint16)
    base = np.zeros((B, nf), dtype=np.uint16) if teacher is None else np.asarray(teacher, dtype=np.uint16)
    return np.where(sel[:, None], drawn, base), sel, np.abs(u - sig)


def normal_fill(n, seed, stream):
    """las_normal_fill: draws 0 .. n-1, float64."""
    return normal(seed, stream, np.arange(n, dtype=np.uint64))


def add_noise(p, std, seed, stream):
    """las_add_noise: p + std * N(0,1) draw i, float64."""
    p = np.asarray(p, dtype=F32)
    return p.astype(np.float64) + np.float64(F32(std)) * normal_fill(p.size, seed, stream).reshape(p.shape)


def relu_bf16(x):
    """las_relu_bf16 on bf16 bits: every value with the sign bit set (negatives, -0, -inf, negative NaNs) becomes +0; the rest
    (+0, positives, +inf, positive NaNs) is kept bit for bit."""
    x = np.asarray(x, dtype=np.uint16)
    return np.where(x & np.uint16(0x8000), np.uint16(0), x).astype(np.uint16)


def relu_bwd(d, y):
    """las_relu_bwd: d kept where the bf16 forward output y is > 0 (positive denormals included), else +0 -- so zero for
    y = +-0, negatives and NaN of either sign."""
    d = np.asarray(d, dtype=F32)
    keep = bf2f(y) > F32(0.0)
    return np.where(keep, d, F32(0.0)).astype(F32)
