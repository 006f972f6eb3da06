"""The random-draw kernels (csrc/rng.hip, las_sample_features of csrc/decoder.hip, the masked epilogue of las_gemm_nt_masked)
through the C-ABI against tests/rng_restated.py.  The threshold decisions and every pure-fp32 result must match bit for bit; the
Gumbel argmax and the feature draws outside a small margin (the device's fast logarithms / sigmoid against float64); the normal
draws to a tolerance.  Shapes: below and above 524 288 elements (the grid-stride loops' second lap), ragged columns, row strides
wider than the row, keep = 1 and a small keep, an index base above 2^32."""
import numpy as np
import pytest
import torch

import tests.rng_restated as R

pytestmark = pytest.mark.gpu


def _lib():
    from phones_las_amd import hip
    return hip, hip.lib()


def _bits16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bf16_from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def _rand_bf16_bits(rng, shape):
    return R.f2bf((rng.standard_normal(shape) * 2).astype(np.float32))


SHAPES = [(37, 61), (1031, 600)]            # 2 257 and 618 600 elements
KEEPS = [1.0, 0.8, 0.05, 'tie']


def _keep(keep, seed, stream, idx):
    """'tie': keep = the uniform of draw idx itself, so that one element sits exactly on the threshold (u < keep is false there;
    a kernel that tested u <= keep would keep it)."""
    if keep != 'tie':
        return keep
    u = float(R.uniform(seed, stream, np.uint64(idx)))
    assert 0.0 < u < 1.0
    return u


@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_dropout_bf16_bits(rows, cols, keep):
    hip, lib = _lib()
    rng = np.random.default_rng(rows + cols)
    ldx, ldy = cols + 5, cols + 3
    xb = _rand_bf16_bits(rng, (rows, ldx))
    x = _bf16_from_bits(xb)
    y = torch.full((rows * ldy,), -3.0, dtype=torch.bfloat16, device='cuda')
    keep = _keep(keep, 1234567, 16, rows * cols // 2)
    hip.check(lib.las_dropout_bf16(hip.p(x), ldx, hip.p(y), ldy, rows, cols, keep, 1234567, 16, hip.stream()))
    got = _bits16(y).reshape(rows, ldy)
    assert np.array_equal(got[:, :cols], R.dropout_bf16(xb[:, :cols], keep, 1234567, 16))
    assert (got[:, cols:] == R.f2bf(np.float32(-3.0))).all()            # the gaps between the rows stay untouched


@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('rows,cols', [(29, 40), (4100, 1032)])        # 145 / 528 900 threads (8 elements each)
def test_dropout_bf16_pair_is_two_single_calls(rows, cols, keep):
    hip, lib = _lib()
    rng = np.random.default_rng(cols)
    ldx, ldy = cols + 16, cols + 8
    xb = _rand_bf16_bits(rng, (rows, ldx))
    x = _bf16_from_bits(xb)
    y0 = torch.zeros(rows * ldy, dtype=torch.bfloat16, device='cuda')
    y1 = torch.zeros_like(y0)
    s0, s1 = 18, 19
    keep = _keep(keep, 99, s1, (rows - 1) * cols + 3)
    hip.check(lib.las_dropout_bf16_pair(hip.p(x), ldx, hip.p(y0), hip.p(y1), ldy, rows, cols, keep, 99, s0, s1, hip.stream()))
    single = torch.zeros_like(y0)
    for y, s in ((y0, s0), (y1, s1)):
        hip.check(lib.las_dropout_bf16(hip.p(x), ldx, hip.p(single), ldy, rows, cols, keep, 99, s, hip.stream()))
        assert torch.equal(y.view(torch.int16), single.view(torch.int16))
        assert np.array_equal(_bits16(y).reshape(rows, ldy)[:, :cols], R.dropout_bf16(xb[:, :cols], keep, 99, s))


def test_dropout_pair_and_steps_reject_ragged_columns():
    hip, lib = _lib()
    x = torch.zeros(64 * 64, dtype=torch.bfloat16, device='cuda')
    y0, y1 = torch.zeros_like(x), torch.zeros_like(x)
    with pytest.raises(hip.LasError):
        hip.check(lib.las_dropout_bf16_pair(hip.p(x), 64, hip.p(y0), hip.p(y1), 64, 8, 60, 0.8, 1, 2, 3, hip.stream()))
    with pytest.raises(hip.LasError):
        hip.check(lib.las_dropout_bf16_steps(hip.p(x), 512, 64, 4, 8, 60, 0, 0.8, 1, 64, hip.stream()))
    torch.cuda.synchronize()
    assert int(y0.view(torch.int16).abs().sum()) == 0 and int(x.view(torch.int16).abs().sum()) == 0


@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('B,U,cols,idx_cols', [(3, 5, 24, 0), (5, 4, 16, 40), (64, 40, 1664, 1700)])
def test_dropout_bf16_steps_is_U_single_calls(B, U, cols, idx_cols, keep):
    hip, lib = _lib()
    rng = np.random.default_rng(B * U)
    ldt = cols + 16                      # columns [cols, ldt) of every row: untouched
    ldb = U * ldt + 8
    xb = _rand_bf16_bits(rng, (B * ldb,))
    x = _bf16_from_bits(xb)
    keep = _keep(keep, 4242, 64 + U - 1, (B - 1) * (idx_cols or cols) + 5)
    hip.check(lib.las_dropout_bf16_steps(hip.p(x), ldb, ldt, B, U, cols, idx_cols, keep, 4242, 64, hip.stream()))
    got = _bits16(x)
    grid = xb[:B * ldb].reshape(B, ldb)[:, :U * ldt].reshape(B, U, ldt)
    out = got.reshape(B, ldb)[:, :U * ldt].reshape(B, U, ldt)
    assert np.array_equal(out[..., :cols], R.dropout_bf16_steps(grid[..., :cols], keep, 4242, 64, idx_cols))
    assert np.array_equal(out[..., cols:], grid[..., cols:])
    assert np.array_equal(got.reshape(B, ldb)[:, U * ldt:], xb.reshape(B, ldb)[:, U * ldt:])
    # ... which is U launches of las_dropout_bf16 over rows of width idx_cols, stream 64 + t
    if idx_cols in (0, cols) and keep < 1 and B * cols < (1 << 16):
        for t in (0, U - 1):
            src = _bf16_from_bits(np.ascontiguousarray(grid[:, t, :cols]))
            y = torch.empty_like(src)
            hip.check(lib.las_dropout_bf16(hip.p(src), cols, hip.p(y), cols, B, cols, keep, 4242, 64 + t, hip.stream()))
            assert np.array_equal(_bits16(y).reshape(B, cols), out[:, t, :cols])


@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('total', [1000, (1 << 20) + 3])
def test_dropout_mask_bits(total, keep):
    hip, lib = _lib()
    out = torch.empty(total, device='cuda')
    keep = _keep(keep, 777, 17, total - 1)
    hip.check(lib.las_dropout_mask(hip.p(out), total, keep, 777, 17, hip.stream()))
    assert np.array_equal(_bits32(out.cpu().numpy()), _bits32(R.dropout_mask(total, keep, 777, 17)))


@pytest.mark.parametrize('with_b', [False, True])
@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('rows,cols', SHAPES)
def test_dropout_bwd_bits(rows, cols, keep, with_b):
    hip, lib = _lib()
    rng = np.random.default_rng(rows)
    a = (rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-20, 20, (rows, cols)))).astype(np.float32)
    b = rng.standard_normal((rows, cols)).astype(np.float32) if with_b else None
    ta = torch.from_numpy(a).cuda()
    tb = torch.from_numpy(b).cuda() if with_b else None
    out = torch.empty_like(ta)
    keep = _keep(keep, 31337, 21 if with_b else 20, rows * cols - 2)
    hip.check(lib.las_dropout_bwd(hip.p(ta), hip.p(tb), hip.p(out), rows, cols, keep, 31337, 20, 21, hip.stream()))
    assert np.array_equal(_bits32(out.cpu().numpy()), _bits32(R.dropout_bwd(a, b, keep, 31337, 20, 21)))


@pytest.mark.parametrize('with_a', [False, True])
@pytest.mark.parametrize('keep', KEEPS)
@pytest.mark.parametrize('rows,cols,idx_base,idx_ld', [(37, 61, 0, 61), (1031, 600, 5, 700), (64, 33, (3 << 32) + 11, 40),
                                                       (900, 640, (1 << 32) - 1000, 640)])
def test_add_masked_bits(rows, cols, idx_base, idx_ld, keep, with_a):
    hip, lib = _lib()
    rng = np.random.default_rng(cols)
    lda, ldb, ldo = cols + 1, cols + 7, cols + 2
    a = rng.standard_normal((rows, lda)).astype(np.float32)
    b = (rng.standard_normal((rows, ldb)) * 3).astype(np.float32)
    ta = torch.from_numpy(a).cuda() if with_a else None
    tb = torch.from_numpy(b).cuda()
    out = torch.full((rows, ldo), 7.0, device='cuda')
    keep = _keep(keep, 5, 65, idx_base + (rows - 1) * idx_ld + cols - 1)
    hip.check(lib.las_add_masked(hip.p(ta), lda, hip.p(tb), ldb, hip.p(out), ldo, rows, cols, keep, 5, 65, idx_base, idx_ld,
                                 hip.stream()))
    got = out.cpu().numpy()
    ref = R.add_masked(a[:, :cols] if with_a else None, b[:, :cols], keep, 5, 65, idx_base, idx_ld)
    assert np.array_equal(_bits32(got[:, :cols]), _bits32(ref))
    assert (got[:, cols:] == 7.0).all()


@pytest.mark.parametrize('keep,feed_width', [(1.0, 11), (0.8, 11), (0.05, 11), (0.8, 11 + 256)])
def test_onehot_bits_and_out_of_range_ids(keep, feed_width):
    hip, lib = _lib()
    B, U, V, ldo = 7, 9, 11, 16
    rng = np.random.default_rng(feed_width)
    ids = rng.integers(0, V, (B, U + 3))
    ids[0, 0], ids[3, 4], ids[6, U - 1] = -1, V, V + 100            # zero rows
    tid = torch.from_numpy(ids.astype(np.int32)).cuda()
    out = torch.full((B * U * ldo,), 5.0, dtype=torch.bfloat16, device='cuda')
    hip.check(lib.las_onehot_bf16(hip.p(tid), U + 3, B, U, V, hip.p(out), ldo, keep, 2024, 1, feed_width, hip.stream()))
    got = _bits16(out).reshape(B * U, ldo)
    assert np.array_equal(got, R.onehot_bf16(ids[:, :U], V, ldo, keep, 2024, 1, feed_width))
    assert not got[0].any() and not got[3 * U + 4].any() and not got[6 * U + U - 1].any()


def test_relu_bf16_and_relu_bwd_pin_the_special_values():
    """relu_bf16 clamps every value with the sign bit set to +0 -- -0, -inf and NEGATIVE NaNs included -- and keeps +NaN, +inf
    and positive denormals bit for bit; relu_bwd keeps d where the bf16 output is > 0 (positive denormals too) and zeroes it for
    +-0, negatives and NaNs of either sign."""
    hip, lib = _lib()
    special = np.array([0x0000, 0x8000, 0x7FC0, 0xFFC0, 0x7F81, 0xFF81, 0x7F80, 0xFF80, 0x0001, 0x8001, 0x007F, 0x807F,
                        0x3F80, 0xBF80], dtype=np.uint16)
    rng = np.random.default_rng(9)
    for n in (len(special), (1 << 19) + 1001):
        xb = np.concatenate([special, rng.integers(0, 1 << 16, max(0, n - len(special))).astype(np.uint16)])[:n]
        x = _bf16_from_bits(xb)
        hip.check(lib.las_relu_bf16(hip.p(x), n, hip.stream()))
        assert np.array_equal(_bits16(x), R.relu_bf16(xb))
        d = rng.standard_normal(n).astype(np.float32)
        td = torch.from_numpy(d).cuda()
        y = _bf16_from_bits(xb)
        hip.check(lib.las_relu_bwd(hip.p(td), hip.p(y), n, hip.stream()))
        assert np.array_equal(_bits32(td.cpu().numpy()), _bits32(R.relu_bwd(d, xb)))
    got = _bits16(_bf16_from_bits(special))
    assert [hex(int(v)) for v in R.relu_bf16(got)] == ['0x0', '0x0', '0x7fc0', '0x0', '0x7f81', '0x0', '0x7f80', '0x0', '0x1', '0x0',
                                                     '0x7f', '0x0', '0x3f80', '0x0']


def _sample_tokens(logits, teacher, teacher_stride, next_stride, prob, seed, step):
    hip, lib = _lib()
    B, V = logits.shape
    ldl = V + 3
    lg = torch.full((B, ldl), 1e30, device='cuda')          # the pad columns would win every draw if they were read
    lg[:, :V] = torch.from_numpy(logits)
    tt = None
    if teacher is not None:
        tt = torch.full((B * teacher_stride,), 12345, dtype=torch.int32, device='cuda')
        tt[::teacher_stride] = torch.from_numpy(teacher.astype(np.int32)).cuda()
    nx = torch.full((B * next_stride,), -7, dtype=torch.int32, device='cuda')
    hip.check(lib.las_sample_tokens(hip.p(lg), ldl, V, hip.p(tt), teacher_stride, hip.p(nx), next_stride, B, prob, seed, step,
                                    hip.stream()))
    got = nx.cpu().numpy()
    assert (np.delete(got, np.arange(0, B * next_stride, next_stride)) == -7).all()      # only next[b * stride] is written
    return got[::next_stride].astype(np.int64)


@pytest.mark.parametrize('prob', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('V', [1, 11, 64, 65, 1000])
def test_sample_tokens_select_exact_and_argmax_outside_the_margin(V, prob):
    rng = np.random.default_rng(V)
    B = 37
    exempt = total = 0
    for step in (0, 5, 1000):
        logits = (rng.standard_normal((B, V)) * 2).astype(np.float32)
        for teacher in (np.full(B, -5, dtype=np.int64), None):    # -5: no draw gives it, so the select decisions show
            got = _sample_tokens(logits, teacher, 3, 2, prob, 0xC0FFEE, step)
            ref, sel, margin = R.sample_tokens(logits, teacher, prob, 0xC0FFEE, step)
            if teacher is not None:
                assert np.array_equal(got == -5, ~sel)
            assert ((got >= 0) & (got < V) | (got == -5)).all()
            clear = ~sel | (margin > 1e-4)
            assert np.array_equal(got[clear], ref[clear])
            exempt += int((~clear).sum())
            total += int(sel.sum())
    assert exempt <= max(1, total // 100)


@pytest.mark.parametrize('prob', [0.0, 0.3, 1.0])
@pytest.mark.parametrize('nf', [1, 11, 64, 65])
def test_sample_features_select_exact_and_draws_outside_the_margin(nf, prob):
    hip, lib = _lib()
    rng = np.random.default_rng(nf)
    B = 37
    ldl, ldt, ldn = nf + 2, nf + 5, nf + 3
    for step in (0, 7, 70000):
        logits = (rng.standard_normal((B, nf)) * 3).astype(np.float32)
        logits[0, 0] = 0.0
        lg = torch.full((B, ldl), -1e30, device='cuda')
        lg[:, :nf] = torch.from_numpy(logits)
        for with_teacher in (True, False):
            teach = torch.full((B, ldt), 2.0, dtype=torch.bfloat16, device='cuda')       # 2.0: no draw gives it
            nx = torch.full((B, ldn), -1.0, dtype=torch.bfloat16, device='cuda')
            hip.check(lib.las_sample_features(hip.p(lg), ldl, nf, hip.p(teach) if with_teacher else None, ldt, hip.p(nx), ldn, B,
                                              prob, 0xFEED, step, hip.stream()))
            got = _bits16(nx).reshape(B, ldn)
            assert (got[:, nf:] == R.f2bf(np.float32(-1.0))).all()
            tb = np.full((B, nf), R.f2bf(np.float32(2.0)), dtype=np.uint16) if with_teacher else None
            ref, sel, margin = R.sample_features(logits, tb, prob, 0xFEED, step)
            got = got[:, :nf]
            if with_teacher:
                assert np.array_equal((got == 0x4000).all(1), ~sel)
            clear = ~sel[:, None] | (margin > 1e-6)
            assert np.array_equal(got[clear], ref[clear])
            assert int((~clear).sum()) <= 2


def test_normal_fill_and_add_noise_against_float64():
    hip, lib = _lib()
    for n in (1001, (1 << 20) + 17):
        out = torch.empty(n, device='cuda')
        hip.check(lib.las_normal_fill(hip.p(out), n, 99, 3, hip.stream()))
        got = out.cpu().numpy().astype(np.float64)
        ref = R.normal_fill(n, 99, 3)
        assert np.isfinite(got).all()
        assert (np.abs(got - ref) <= 1e-3 + 1e-4 * np.abs(ref)).all()
        p = np.random.default_rng(n).standard_normal(n).astype(np.float32)
        tp = torch.from_numpy(p).cuda()
        hip.check(lib.las_add_noise(hip.p(tp), n, 0.75, 99, 1003, hip.stream()))
        got = tp.cpu().numpy().astype(np.float64)
        ref = R.add_noise(p, 0.75, 99, 1003)
        assert np.isfinite(got).all() and (np.abs(got - ref) <= 1e-3 + 1e-4 * np.abs(ref)).all()


def test_normal_fill_at_the_extreme_uniforms():
    """(seed 20240611, stream 0): among draws [0, 2^22), u1 of draw 4049763 is 0 (clamped to 1e-12f) and of draw 81983 it is
    1 - 2^-24; the four largest and the smallest u1 of the range are checked by name as well."""
    hip, lib = _lib()
    seed, stream, n = 20240611, 0, 1 << 22
    bits = R.uniform_bits(seed, stream, 2 * np.arange(n, dtype=np.uint64))
    order = np.argsort(bits, kind='stable')
    picks = np.concatenate([order[:1], order[-4:]])
    assert int(bits[4049763]) == 0 and int(bits[81983]) == 0xFFFFFF and {4049763, 81983} <= set(picks.tolist())
    out = torch.empty(n, device='cuda')
    hip.check(lib.las_normal_fill(hip.p(out), n, seed, stream, hip.stream()))
    got = out.cpu().numpy().astype(np.float64)
    ref = R.normal_fill(n, seed, stream)
    assert np.isfinite(got[picks]).all(), got[picks]
    assert np.isfinite(got).all() and float(np.abs(got).max()) <= R.Z_MAX * (1 + 1e-4)
    assert (np.abs(got - ref) <= 1e-3 + 1e-4 * np.abs(ref)).all()


# (seed 20240611) Gumbel draw 6639505 is 1 - 2^-24, draw 25739857 is 0 (clamped to 1e-12f): with B = 1 the draw (step*B + b)*V + v
GUMBEL_MAX, GUMBEL_ZERO = 6639505, 25739857


@pytest.mark.parametrize('V', [2, 1000])
def test_sample_tokens_at_the_extreme_gumbel_uniforms(V):
    seed = 20240611
    assert int(R.uniform_bits(seed, R.GUMBEL_STREAM, np.uint64(GUMBEL_MAX))) == 0xFFFFFF
    assert int(R.uniform_bits(seed, R.GUMBEL_STREAM, np.uint64(GUMBEL_ZERO))) == 0
    rng = np.random.default_rng(V)
    for idx in (GUMBEL_MAX, GUMBEL_ZERO):
        step, v = idx // V, idx % V
        for scale in (0.0, 1.0, 10.0):
            logits = (rng.standard_normal((1, V)) * scale).astype(np.float32)
            got = _sample_tokens(logits, np.array([-5]), 1, 1, 1.0, seed, step)
            ref, sel, margin = R.sample_tokens(logits, np.array([-5]), 1.0, seed, step)
            assert sel.all() and 0 <= int(got[0]) < V
            if V == 2:
                assert int(got[0]) == int(ref[0]), (idx, scale, logits, margin)
            elif margin[0] > 1e-4:
                assert int(got[0]) == int(ref[0])
        if idx == GUMBEL_MAX and V == 2:     # equal logits: the token whose uniform is 1 - 2^-24 wins by a wide margin
            assert int(_sample_tokens(np.zeros((1, V), np.float32), None, 1, 1, 1.0, seed, step)[0]) == v


@pytest.mark.parametrize('keep', [0.8, 0.5])
@pytest.mark.parametrize('BT,D', [(200, 136), (1100, 256), (1100, 136)])       # the 64 x 64 kernel and the ring kernel
def test_listener_backward_regenerates_the_forward_masks(BT, D, keep):
    """The bidirectional listener layer draws its two input masks with las_dropout_bf16_pair over [B*T, Dp] (ops.bilstm); its
    backward applies them again inside las_gemm_nt_masked (dX = dZ_d K_x,d^T, one direction stores, the other accumulates) or
    through las_dropout_bwd, indexing [B*T, D].  With D == Dp (every layer whose dX is formed: ops.bilstm_backward refuses the
    rest) the three must agree element for element."""
    hip, lib = _lib()
    K, seed, s0 = 256, 0x5EED, 18
    x = torch.ones(BT, D, dtype=torch.bfloat16, device='cuda')
    pair = torch.empty(2, BT, D, dtype=torch.bfloat16, device='cuda')
    hip.check(lib.las_dropout_bf16_pair(hip.p(x), D, hip.p(pair[0]), hip.p(pair[1]), D, BT, D, keep, seed, s0, s0 + 1,
                                        hip.stream()))
    fwd = pair.float()                                         # mask_d / keep (1/keep is exact in bf16 for these keeps)
    A = torch.zeros(BT, 2 * K, dtype=torch.bfloat16, device='cuda')
    A[:, 0] = 1.0
    A[:, K] = 1.0
    Bm = torch.zeros(D, 2 * K, dtype=torch.bfloat16, device='cuda')
    Bm[:, 0] = 1.0
    Bm[:, K] = 1.0                                             # (A_d B_d^T)[r, c] = 1 for both directions
    dx = torch.full((BT, D), 9.0, device='cuda')
    for i in range(2):
        hip.check(lib.las_gemm_nt_masked(hip.addr(A, i * K), 2 * K, hip.addr(Bm, i * K), 2 * K, hip.p(dx), D, BT, D, K, int(i > 0),
                                         keep, seed, s0 + i, hip.stream()))
    assert torch.equal(dx, fwd[0] + fwd[1])
    ones = torch.ones(BT, D, device='cuda')
    out = torch.empty_like(ones)
    hip.check(lib.las_dropout_bwd(hip.p(ones), hip.p(ones), hip.p(out), BT, D, keep, seed, s0, s0 + 1, hip.stream()))
    assert torch.equal(out, fwd[0] + fwd[1])
    ref = [R.dropout_mask(BT * D, keep, seed, s0 + i).reshape(BT, D) for i in range(2)]
    assert np.array_equal(dx.cpu().numpy(), ref[0] + ref[1])
