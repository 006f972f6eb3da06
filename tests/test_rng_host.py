"""Properties of the counter-based generator, established on its NumPy restatement (tests/rng_restated.py): the device inherits
them through the bit-equality that tests/test_gpu_rng_kernels.py checks.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import tests.rng_restated as R


def _chi2_sf(x, df):
    """P(chi2_df > x): the regularised upper incomplete gamma Q(df/2, x/2) (series below a + 1, continued fraction above)."""
    a, x = 0.5 * df, 0.5 * x
    if x <= 0:
        return 1.0
    lg = math.lgamma(a)
    if x < a + 1:
        term = s = 1.0 / a
        n = a
        while abs(term) > 1e-15 * abs(s):
            n += 1
            term *= x / n
            s += term
        return 1.0 - s * math.exp(-x + a * math.log(x) - lg)
    b = x + 1 - a
    c, d = 1e300, 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = 1e-300 if abs(d) < 1e-300 else d
        c = b + an / c
        c = 1e-300 if abs(c) < 1e-300 else c
        d = 1.0 / d
        h *= d * c
        if abs(d * c - 1) < 1e-15:
            break
    return h * math.exp(-x + a * math.log(x) - lg)


def test_chi2_tail_matches_known_values():
    assert abs(_chi2_sf(3.841458820694124, 1) - 0.05) < 1e-9
    assert abs(_chi2_sf(18.307038053275146, 10) - 0.05) < 1e-9
    assert abs(_chi2_sf(88.3794, 60) - 0.01) < 1e-5


def test_mix32_known_values():
    # lowbias32 (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16), worked by hand in Python ints
    def ref(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)
    xs = np.array([0, 1, 2, 0x7fffffff, 0x80000000, 0xFFFFFFFF, 0x12345678, 0x9E3779B9], dtype=np.uint32)
    assert [int(v) for v in R.mix32(xs)] == [ref(int(x)) for x in xs]
    assert int(R.mix32(np.uint32(0))) == 0


def test_uniform_is_the_scalar_formula_including_the_high_index_word():
    def ref(seed, stream, idx):
        def mix(x):
            return int(R.mix32(np.uint32(x & 0xFFFFFFFF)))
        h = mix(seed ^ ((stream * 0x9E3779B9) & 0xFFFFFFFF))
        h = mix(h ^ (idx & 0xFFFFFFFF))
        h = mix(h + ((idx >> 32) * 0x85EBCA6B) + 0x632BE5AB)
        return (h >> 8) / 16777216.0
    for seed, stream, idx in [(0, 0, 0), (7, 1, 5), (0x7fffffff, 0x5e1ec7, (1 << 32) + 3), (3, 4160, (5 << 40) + 17),
                              (1, 0xb17f00d, (1 << 64) - 1)]:
        assert float(R.uniform(seed, stream, np.uint64(idx))) == ref(seed, stream, idx)
    # the high word matters: the same low word above 2^32 is another draw
    lo = R.uniform_bits(5, 9, np.arange(4096, dtype=np.uint64))
    hi = R.uniform_bits(5, 9, np.arange(4096, dtype=np.uint64) + np.uint64(1 << 32))
    assert (lo != hi).mean() > 0.99


def test_uniform_values_lie_on_the_24_bit_grid_in_0_1():
    u = R.uniform(20240611, 17, np.arange(1 << 22, dtype=np.uint64))
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    k = u.astype(np.float64) * 16777216.0
    assert np.array_equal(k, np.floor(k))
    assert float(R.uniform(0, 0, np.uint64(0))) * 16777216 == float(R.uniform_bits(0, 0, np.uint64(0)))


@pytest.mark.parametrize('keep', [0.5, 0.8, 0.9])
def test_bernoulli_rate_of_the_dropout_threshold(keep):
    n = 1 << 22
    rate = float((R.uniform(4321, 16, np.arange(n, dtype=np.uint64)) < np.float32(keep)).mean())
    # u < keep on the 2^-24 grid: P = ceil(keep * 2^24) / 2^24, within 2^-24 of keep
    assert abs(rate - keep) < 5 * math.sqrt(keep * (1 - keep) / n) + 2.0 ** -24


# the streams one train step uses together: listener layers 0..2 (16 + 2l, 17 + 2l), the decoder's token scale / dense feed (1),
# the monotonic-attention noise (3), the per-cell input masks 64 + 4096 l + t, the samplers and weight noise 1000 + i
STEP_STREAMS = [16, 17, 18, 19, 20, 21, 1, 3, 64, 65, 66, 4160, 4161, R.SELECT_STREAM, R.GUMBEL_STREAM, R.FEATURE_STREAM,
                1000, 1001, 1017]


def test_streams_used_together_are_uncorrelated():
    n = 1 << 19
    idx = np.arange(n, dtype=np.uint64)
    for seed in (0x2468ace, 0x7fffffff):
        u = np.stack([R.uniform(seed, s, idx).astype(np.float64) for s in STEP_STREAMS])
        r = np.corrcoef(u)
        off = r[~np.eye(len(STEP_STREAMS), dtype=bool)]
        assert float(np.abs(off).max()) < 5 / math.sqrt(n)
        # and the draws of one stream at neighbouring indices (the elements of one row)
        lag = np.corrcoef(u[:, :-1].ravel(), u[:, 1:].ravel())[0, 1]
        assert abs(lag) < 5 / math.sqrt(u[:, 1:].size)


def test_streams_of_one_seed_are_xor_permutations_of_each_other():
    """Known property: below 2^32 the index only enters through h ^ idx, so stream B at index i ^ D is stream A at
    index i, D = key_A ^ key_B.  Two users of one seed draw the same numbers at permuted positions: harmless as long as no user
    reads another's stream at the permuted indices, which is why the stream map keeps their (stream, index) ranges apart."""
    def key(seed, stream):
        return int(R.mix32(np.uint32((seed ^ ((stream * 0x9E3779B9) & 0xFFFFFFFF)) & 0xFFFFFFFF)))
    seed, a, b = 99, 16, 17
    D = np.uint64(key(seed, a) ^ key(seed, b))
    i = np.arange(1000, dtype=np.uint64)
    assert np.array_equal(R.uniform_bits(seed, b, i ^ D), R.uniform_bits(seed, a, i))


def _gumbel_counts(logits, n_draws, seed=77):
    logits = np.asarray(logits, dtype=np.float32)
    V = logits.size
    counts = np.zeros(V, dtype=np.int64)
    step_rows = 1 << 14
    for step in range(-(-n_draws // step_rows)):
        rows = min(step_rows, n_draws - step * step_rows)
        g = R.gumbel_scores(np.broadcast_to(logits, (step_rows, V)), seed, step)[:rows]
        counts += np.bincount(np.argmax(g, axis=1), minlength=V)
    return counts


@pytest.mark.parametrize('logits', [
    [0.0, 1.0],
    [0.5, -1.0, 2.0, 0.0, 3.0, -2.0, 1.0, 0.25],
    list(np.linspace(-3.0, 3.0, 61)),
    [0.0, 8.0, 2.0, -1.0, 1.0, 0.0, 0.0, 4.0],                 # a gap of 8: the rarest cells still expect ~5 draws
], ids=['V2', 'V8', 'V61', 'V8_gap8'])
def test_gumbel_max_reproduces_the_softmax(logits):
    V = len(logits)
    n = (1 << 22) // V                                           # 2^22 uniform draws per case
    counts = _gumbel_counts(logits, n)
    p = np.exp(np.array(logits) - max(logits))
    p /= p.sum()
    expected = n * p
    assert expected.min() >= 5
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    assert _chi2_sf(chi2, V - 1) > 1e-3, (chi2, counts, expected)


def test_gumbel_max_under_a_logit_gap_of_20():
    """On 24-bit uniforms the perturbation -log(-log(u)) lies in [-log(-log(1e-12)), -log(-log(1 - 2^-24))] = [-3.32, 16.63]: a token
    trailing by 20 can never win.  Softmax gives it e^-20 = 2.1e-9 -- the truncation costs that much probability mass."""
    lo = -math.log(-math.log(float(np.float32(1e-12))))
    hi = -math.log(-math.log(1 - 2.0 ** -24))
    assert hi - lo < 20.0
    counts = _gumbel_counts([0.0, 20.0], 1 << 21)
    assert counts[0] == 0 and counts[1] == 1 << 21
    counts = _gumbel_counts([20.0] + [0.0] * 7, 1 << 19)
    assert counts[0] == 1 << 19


@pytest.mark.parametrize('x', [-4.0, -1.0, 0.0, 0.3, 2.5])
def test_feature_draws_follow_the_sigmoid(x):
    n = 1 << 20
    B = 1 << 10
    nxt = np.concatenate([R.sample_features(np.full((B, 1), x, np.float32), None, 1.0, 31, s)[0][:, 0]
                          for s in range(n // B)])
    rate = float((nxt == 0x3F80).mean())
    p = 1 / (1 + math.exp(-x))
    assert abs(rate - p) < 5 * math.sqrt(p * (1 - p) / n) + 2.0 ** -24


def test_normal_draws_moments_and_bounds():
    n = 1 << 22
    z = R.normal_fill(n, 20240611, 3)
    assert np.isfinite(z).all() and float(np.abs(z).max()) <= R.Z_MAX
    m, v = float(z.mean()), float(z.var())
    kurt = float(((z - m) ** 4).mean() / v ** 2 - 3)
    assert abs(m) < 5 / math.sqrt(n)
    assert abs(v - 1) < 5 * math.sqrt(2 / n)
    assert abs(kurt) < 5 * math.sqrt(24 / n)


def test_normal_at_the_extreme_uniforms():
    # seed 20240611, stream 0: u1 of draw 4049763 is 0 (clamped to 1e-12f), of draw 81983 it is 1 - 2^-24
    seed, stream = 20240611, 0
    assert int(R.uniform_bits(seed, stream, np.uint64(2 * 4049763))) == 0
    assert int(R.uniform_bits(seed, stream, np.uint64(2 * 81983))) == 0xFFFFFF
    z = R.normal(seed, stream, np.array([4049763, 81983], dtype=np.uint64))
    assert abs(abs(z[0]) - R.Z_MAX * abs(math.cos(float(np.float32(6.2831853)) * float(R.uniform(seed, stream, np.uint64(2 * 4049763 + 1)))))) < 1e-9
    assert 0 < abs(z[1]) < 4e-4


def test_fma32_rounds_once():
    rng = np.random.default_rng(3)
    x = rng.standard_normal(4000).astype(np.float32)
    y = np.where(rng.random(4000) < 0.5, np.float32(1.25), np.float32(1 / 0.3)).astype(np.float32)
    z = (rng.standard_normal(4000) * np.exp2(rng.integers(-30, 30, 4000))).astype(np.float32)
    # cases built to land on an fp32 midpoint after a float64 rounding: z = 1, x*y = 2^-24 + 2^-60
    x = np.append(x, [np.float32(2.0 ** -24 + 2.0 ** -47)])
    y = np.append(y, [np.float32(1 + 2.0 ** -13)])
    z = np.append(z, [np.float32(1.0)])
    got = R.fma32(x, y, z)
    for a, b, c, g in zip(x, y, z, got):
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        # round the exact value to fp32, nearest even, through the two neighbours of the float64 guess
        r = np.float32(float(exact))
        cands = [np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))]
        best = min(cands, key=lambda q: (abs(Fraction(float(q)) - exact), int(np.array(q).view(np.uint32)) & 1))
        assert g == best, (a, b, c, g, best)


def test_bf16_rounding_is_nearest_even():
    f = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -2.5, 3.0e38, np.inf, -0.0],
                 dtype=np.float32)
    got = R.f2bf(f)
    assert [hex(int(v)) for v in got] == ['0x3f80', '0x3f80', '0x3f82', '0x3f81', '0xc020', '0x7f62', '0x7f80', '0x8000']
    assert np.isnan(R.bf2f(R.f2bf(np.array([np.nan], np.float32))))[0]


# ---- the stream map -----------------------------------------------------------------------------------------------------------
def stream_map(cfg, speller_seeds):
    """Every user of the generator in one train step: (name, seed, first stream, last stream, first index, end index).  cfg:
    B, T (listener input frames), F (padded feature width), L, H, pyramidal (listener), U (decoder steps), V, M (memory width), A (attention
    width), Hd, dec_layers, kernels (number of '*kernel' variables; noise stream 1000 + i counts every variable before it, so
    this is the last one's table index + 1), kernel_numel (the largest), Tm (memory frames), and per decoder k its seed
    speller_seeds[k].  Weight noise draws with the noise seed, which on rank 0 equals the step seed."""
    B, U = cfg['B'], cfg['U']
    users = []
    T, D = cfg['T'], cfg['F']
    for l in range(cfg['L']):                            # las/ops.py bilstm: rng = (seed, 16 + 2l), one stream per direction
        users.append(('listener %d fw' % l, 'step', 16 + 2 * l, 16 + 2 * l, 0, B * T * D))
        users.append(('listener %d bw' % l, 'step', 17 + 2 * l, 17 + 2 * l, 0, B * T * D))
        pyr = cfg.get('pyramidal', True)
        if l > 0 and pyr:
            T //= 2                                      # pyramidal: half the frames, twice the width
        D = 2 * cfg['H'] * (2 if (l > 0 and pyr) else 1)
    for k, seed in enumerate(speller_seeds):
        fw = cfg['V'] + cfg['M']
        users.append(('speller %d token scale / dense feed' % k, seed, 1, 1, 0, U * B * fw))
        users.append(('speller %d monotonic noise' % k, seed, 3, 3, 0, U * B * cfg['Tm']))
        for l in range(cfg['dec_layers']):
            win = cfg['A'] + cfg['Hd'] + fw
            users.append(('speller %d cell %d input masks' % (k, l), seed, 64 + 4096 * l, 64 + 4096 * l + U - 1, 0, B * win))
        users.append(('speller %d sample select' % k, seed, R.SELECT_STREAM, R.SELECT_STREAM, 0, U * B))
        users.append(('speller %d Gumbel' % k, seed, R.GUMBEL_STREAM, R.GUMBEL_STREAM, 0, U * B * cfg['V']))
        users.append(('speller %d feature draws' % k, seed, R.FEATURE_STREAM, R.FEATURE_STREAM, 0, U * B * cfg['V']))
    users.append(('weight noise', 'step', 1000, 1000 + cfg['kernels'] - 1, 0, 2 * cfg['kernel_numel']))
    return users


def _clashes(users):
    out = []
    for i, a in enumerate(users):
        for b in users[i + 1:]:
            if a[1] == b[1] and a[2] <= b[3] and b[2] <= a[3] and a[4] < b[5] and b[4] < a[5]:
                out.append((a[0], b[0]))
    return out


def _speller_seed(step_seed, k):
    from phones_las_amd import model_helper as mh
    return mh.speller_seed(step_seed, k)


DEFAULT_ARCH = dict(B=64, T=800, F=40, L=3, H=128, U=100, V=61, M=256, A=256, Hd=128, dec_layers=2, kernels=24, kernel_numel=640 * 512,
                   Tm=200)


@pytest.mark.parametrize('multitask', [False, True])
def test_no_two_users_of_one_step_draw_the_same_numbers(multitask):
    step_seed = 0x1234567
    seeds = [_speller_seed(step_seed, k) for k in range(2 if multitask else 1)]
    assert seeds[0] == step_seed                 # decoder 0 keeps the step's seed: recorded draws stay where they were
    names = ['step' if s == step_seed else 'speller %d' % k for k, s in enumerate(seeds)]
    assert len(set(names)) == len(names)         # every further decoder draws under a seed of its own
    for cfg in (DEFAULT_ARCH, dict(DEFAULT_ARCH, U=936, L=5, dec_layers=4)):
        assert _clashes(stream_map(cfg, names)) == []


def test_stream_map_limits():
    """The two places where the map runs out, recorded rather than changed (every recorded draw would move): the input masks of
    decoder cell 0 (64 + t) reach the weight noise (1000 + i, the same seed on rank 0) from U = 937 steps on, and a listener of
    more than 24 layers reaches stream 64."""
    assert ('speller 0 cell 0 input masks', 'weight noise') in _clashes(stream_map(dict(DEFAULT_ARCH, U=937), ['step']))
    assert _clashes(stream_map(dict(DEFAULT_ARCH, U=936), ['step'])) == []
    assert any('listener' in a and 'cell 0' in b for a, b in _clashes(stream_map(dict(DEFAULT_ARCH, L=25, pyramidal=False), ['step'])))
    assert _clashes(stream_map(dict(DEFAULT_ARCH, L=24, pyramidal=False), ['step'])) == []


def test_speller_seeds_are_distinct_and_keep_decoder_0():
    rng = np.random.default_rng(0)
    for s in [0, 1, 0x7fffffff] + [int(v) for v in rng.integers(0, 1 << 31, 200)]:
        seeds = [_speller_seed(s, k) for k in range(4)]
        assert seeds[0] == s and len(set(seeds)) == 4
        assert all(0 <= v < (1 << 31) for v in seeds)


def test_listener_backward_refuses_dx_through_masks_drawn_at_another_width():
    """The forward draws a layer's input masks over [B*T, Dp] (index r*Dp + c); las_gemm_nt_masked / las_dropout_bwd regenerate
    them over [B*T, D].  No layer whose dX is formed has D < Dp (only the bottom one, whose dX nobody needs): the backward
    refuses the combination before it launches anything, so a future change cannot silently desynchronise the masks."""
    from phones_las_amd.las import ops
    rec = dict(B=2, T=4, H=64, D=13, Dp=16, nd=2, keep=0.8, dropped=[(None, 16), (None, 16)], rng=(1, 16))
    with pytest.raises(ValueError, match='D == Dp'):
        ops.bilstm_backward(rec, None, None, {}, need_dx=True)
