"""Checks of attention at 256 tokens and below -- the single-tile kernels of attention.hip that every shipped config launches:
attn_kernel, attn_x6_kernel<4 / 8 / 12 / 16>, attn_bwd_q_kernel and attn_bwd_kv_kernel -- shared by the emulator suite
(tests/test_attn_tile_cpu.py) and the GPU suite (tests/test_attn_tile_gpu.py).  The reference is fp64 softmax attention with
autograd for the backward (_attn_long_checks._ref64); tolerances are the project's, max-abs error over max-abs reference
value: 2e-5 forward (TOL_GEMM) and backward (TOL_OP), and each of dq, dk and dv is held to it on its own, so that a wrong dk
cannot hide behind a larger dq or dv."""
import torch

from _util import rel_err
import _attn_long_checks as K
from _attn_long_checks import TOL_GEMM, TOL_OP, _inputs, _raw, _ref64

# (n, L, C) of the sweep.  Lk = L rounded up to 64 (keys per wave block), Lp = L rounded up to 32 (what P V walks)
CASES = [
    (2, 1, 32),        # one token; image stride of 1 row
    (1, 3, 32),        # fewer tokens than the 4 lanes of a softmax row
    (2, 17, 96),       # L % 4 != 0, C % 64 != 0, odd image stride, second image
    (1, 100, 160),     # ragged inside the second key block; C / 4 = 40 does not divide 256 (the tid / f4n chunk walk)
    (1, 130, 64),      # third key block and third query block hold 2 rows; Lp = 160 < Lk = 192
    (1, 255, 32),      # one short of full
    (1, 240, 320),     # second channel pass of 64 channels
    (1, 200, 512),     # widest shipped attention, two full channel passes, ragged L
    (2, 256, 256),     # the CIFAR model's own launch; backward never tested at this width
    (3, 256, 192),     # attn_x6_kernel<12> (bf16x6 mode)
    (11, 256, 64),     # X6 grid of 64 workgroups for 11 images: second round of the XCD map, 5 idle image slots
]
# the shapes that take attn_x6_kernel in bf16x6 mode; every other one runs attn_kernel in both modes
X6_CASES = {(2, 256, 256), (3, 256, 192), (11, 256, 64)}
CHAIN_CASES = [(2, 256, 256), (1, 100, 160)]


def _ops():
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    return ops, L


def expected_route(shape):
    ops, L = _ops()
    return L.ATTN_ROUTE_X6 if shape in X6_CASES and (L.attn_route_flags() & L.ATTNF_BF16X6) else L.ATTN_ROUTE_F32


def _parts(g, g64, c):
    """errors of dq, dk, dv, each over its own largest reference value, and of the pooled tensor"""
    return [rel_err(g[..., i * c:(i + 1) * c], g64[..., i * c:(i + 1) * c]) for i in range(3)], rel_err(g, g64)


def _assert_grads(what, shape, g, g64, c, pooled_only=False):
    eg, ep = _parts(g, g64, c)
    print("attention %s %s vs fp64 autograd: dq %.3g dk %.3g dv %.3g pooled %.3g" % (shape, what, *eg, ep))
    assert ep < TOL_OP, (what, shape, ep)
    if not pooled_only:
        assert max(eg) < TOL_OP, (what, shape, eg)


def check_shape(dev, n, l, c, monkeypatch):
    """A. forward against fp64; the backward, fed the fp32 rounding of the fp64 output (so that it measures the two backward
    kernels and not the forward's error passing through D = dO . O), against fp64 autograd per part.  At l == 1 the true dq
    and dk are exactly zero: the pooled error only, and the forward is v to the bit (the one softmax weight is 1)."""
    ops, L = _ops()
    shape = (n, l, c)
    qkv, d_o, y64, g64 = K.reference(n, l, c)
    monkeypatch.delenv("SSDE_ATTN_X6", raising=False)
    monkeypatch.delenv("SSDE_ATTN_STREAM", raising=False)
    route = expected_route(shape)
    assert ops.attention_route(n, l, c) == route, (shape, ops.attention_route(n, l, c), route)
    qd, dd = qkv.to(dev), d_o.to(dev)
    y = ops.attention(qd, c)
    e = rel_err(y, y64)
    print("attention %s forward (%s) vs fp64: %.3g" % (shape, "x6" if route == L.ATTN_ROUTE_X6 else "f32", e))
    assert e < TOL_GEMM, (shape, e)
    if l == 1:
        assert torch.equal(y.cpu(), qkv[..., 2 * c:])
    if route == L.ATTN_ROUTE_X6:
        monkeypatch.setenv("SSDE_ATTN_X6", "0")
        assert ops.attention_route(n, l, c) == L.ATTN_ROUTE_F32
        y32 = ops.attention(qd, c)
        monkeypatch.delenv("SSDE_ATTN_X6")
        e32 = rel_err(y32, y64)
        print("attention %s forward (f32, SSDE_ATTN_X6=0) vs fp64: %.3g" % (shape, e32))
        assert not torch.equal(y, y32)                         # (two different kernels ran)
        assert e32 < TOL_GEMM, (shape, e32)
        if dev != "cpu":                                       # (the emulator's bf16 MFMA arithmetic is not the hardware's: test_emulated_kernels.py)
            assert e <= 1.5 * e32 + 2e-7, (shape, e, e32)
    g = ops.attention_bwd(qd, y64.float().to(dev), dd, c)
    _assert_grads("backward", shape, g, g64, c, pooled_only=l == 1)


def check_chain(dev, n, l, c):
    """B. the engine's chain (backward.py): the backward is fed the kernel's own forward output"""
    ops, L = _ops()
    shape = (n, l, c)
    qkv, d_o, y64, g64 = K.reference(n, l, c)
    assert ops.attention_route(n, l, c) == expected_route(shape)
    qd = qkv.to(dev)
    y = ops.attention(qd, c)
    assert rel_err(y, y64) < TOL_GEMM, (shape, rel_err(y, y64))
    _assert_grads("forward -> backward", shape, ops.attention_bwd(qd, y, d_o.to(dev), c), g64, c)


def check_padding_is_inert(dev):
    """C. L = 100, C = 96 inside allocations of 164 rows whose tail is NaN (inputs) or a sentinel (outputs and statistics): the
    results are finite and equal to the bits of the run on exact-size tensors, and no row beyond L is written.  (Every access
    of the launch lies inside the first 100 rows, and every row the kernels could clamp to or overrun into is allocated.)"""
    ops, L = _ops()
    n, l, c, pad = 1, 100, 96, 64
    assert ops.attention_route(n, l, c) == L.ATTN_ROUTE_F32
    qkv, d_o = _inputs(n, l, c)
    y0 = ops.attention(qkv.to(dev), c)
    g0 = ops.attention_bwd(qkv.to(dev), y0, d_o.to(dev), c)

    def padded(t, fill):
        buf = torch.full((l + pad, t.shape[-1]), fill)
        buf[:l] = t[0].cpu()
        return buf.to(dev)
    SENT = -12345.0
    qb = padded(qkv, float("nan"))
    yb = torch.full((l + pad, c), SENT).to(dev)
    _raw(dev, qb, yb, l, c)
    assert bool(torch.isfinite(yb[:l]).all()) and torch.equal(yb[:l], y0[0])
    assert bool((yb[l:] == SENT).all())
    ob, dob = padded(y0, float("nan")), padded(d_o, float("nan"))
    gb = torch.full((l + pad, 3 * c), SENT).to(dev)
    sb = torch.full((l + pad, 4), SENT).to(dev)
    _raw(dev, qb, gb, l, c, bwd=(ob, dob, sb))
    assert bool(torch.isfinite(gb[:l]).all()) and torch.equal(gb[:l], g0[0])
    assert bool(torch.isfinite(sb[:l]).all())
    assert bool((gb[l:] == SENT).all()) and bool((sb[l:] == SENT).all())


def check_reproducible(dev):
    """D. forward and backward called twice agree to the bit"""
    ops, L = _ops()
    n, l, c = 1, 130, 64
    assert ops.attention_route(n, l, c) == L.ATTN_ROUTE_F32
    qkv, d_o, _, _ = K.reference(n, l, c)
    qd, dd = qkv.to(dev), d_o.to(dev)
    y = ops.attention(qd, c)
    assert torch.equal(y, ops.attention(qd, c))
    g = ops.attention_bwd(qd, y, dd, c)
    assert torch.equal(g, ops.attention_bwd(qd, y, dd, c))


TRANSPOSE_SHAPE = (1, 200, 224)
# softening of the backward's queries.  Query i scores q k / sqrt(C) on key perm[i] and 0 on the 199 others, so the selected key
# holds w = e^s / (e^s + 199), s = 400 f / sqrt(224).  check_transpose_detecting's f = 0.25 was chosen for L = C = 320 (w = 0.46);
# here it gives s = 6.68, w = 0.80, outside the 0.3 .. 0.7 this check requires.  f = 0.2: s = 5.35, w = 0.51
TRANSPOSE_SOFTEN = 0.2


def transpose_inputs():
    n, l, c = TRANSPOSE_SHAPE
    q, k = torch.zeros(n, l, c), torch.zeros(n, l, c)
    perm = torch.randperm(l, generator=torch.Generator().manual_seed(10))
    idx = torch.arange(l)
    q[0, idx, idx] = 400.0
    k[0, perm, idx] = 1.0
    v = torch.arange(l * c, dtype=torch.float32).reshape(1, l, c) / 100.0
    return q, k, v, perm


def transpose_backward_inputs():
    """(qkv, d_o, largest softmax weight of the fp64 reference)"""
    n, l, c = TRANSPOSE_SHAPE
    q, k, v, _ = transpose_inputs()
    qkv = torch.cat([q * TRANSPOSE_SOFTEN, k, v * 0.01], -1)
    d_o = torch.randn(n, l, c, generator=torch.Generator().manual_seed(11))
    w = torch.softmax(qkv[..., :c].double() @ k.double().transpose(1, 2) * c ** -0.5, -1)
    return qkv, d_o, float(w.max())


def check_transpose_detecting(dev):
    """E. query i selects key perm[i] through channel i, v is asymmetric: the output must be v[perm].  perm is no involution, so
    Q and K swapped (which selects perm^-1) shows, as does a transposed V or P.  Backward: the same permutation with a softer
    selection (the selected key holds about half of a row's weight: at q = 400 the true dq and dk are ~1e-8 while dP - D
    cancels from ~1e4) and values of order 10, every gradient against fp64 autograd."""
    ops, L = _ops()
    n, l, c = TRANSPOSE_SHAPE
    assert ops.attention_route(n, l, c) == L.ATTN_ROUTE_F32
    q, k, v, perm = transpose_inputs()
    assert int((perm[perm] != torch.arange(l)).sum()) >= 32
    y = ops.attention(torch.cat([q, k, v], -1).to(dev), c)
    assert rel_err(y, v[:, perm]) < 1e-5, rel_err(y, v[:, perm])
    qkv_b, d_o, wmax = transpose_backward_inputs()
    assert 0.3 < wmax < 0.7, wmax
    y64, g64 = _ref64(qkv_b, d_o, c)
    yb = ops.attention(qkv_b.to(dev), c)
    assert rel_err(yb, y64) < TOL_GEMM, rel_err(yb, y64)
    g = ops.attention_bwd(qkv_b.to(dev), y64.float().to(dev), d_o.to(dev), c)
    _assert_grads("transpose-detecting backward", (n, l, c), g, g64, c)


def check_ties_and_dominated_row(dev):
    """F. row 7: an all-zero query, every score 0: the plain mean of v.  Row 11: its score on key 42 exceeds the others by 141
    (q[11] and k[42] meet in channel 0 alone, sqrt(800) each, so neither dq nor dk amplifies the fp32 rounding of dP - D by
    more than 5): that key's v row.  Both gradients against fp64 autograd, per part."""
    ops, L = _ops()
    n, l, c = 1, 100, 32
    assert ops.attention_route(n, l, c) == L.ATTN_ROUTE_F32
    g = torch.Generator().manual_seed(78)
    q, k, v = (torch.randn(n, l, c, generator=g) for _ in range(3))
    d_o = torch.randn(n, l, c, generator=g)
    q[..., 0], k[..., 0] = 0.0, 0.0
    q[0, 7, :] = 0.0
    q[0, 11, :] = 0.0
    q[0, 11, 0], k[0, 42, 0] = 800.0 ** 0.5, 800.0 ** 0.5
    s = q.double() @ k.double().transpose(1, 2) * c ** -0.5
    others = torch.arange(l) != 42
    assert float(s[0, 7].abs().max()) == 0.0 and float(s[0, 11, 42] - s[0, 11, others].max()) > 100.0
    qkv = torch.cat([q, k, v], -1)
    y64, g64 = _ref64(qkv, d_o, c)
    y = ops.attention(qkv.to(dev), c)
    assert rel_err(y, y64) < TOL_GEMM, rel_err(y, y64)
    assert rel_err(y[0, 7], v[0].double().mean(0)) < TOL_GEMM, rel_err(y[0, 7], v[0].double().mean(0))
    assert rel_err(y[0, 11], v[0, 42]) < TOL_GEMM, rel_err(y[0, 11], v[0, 42])
    _assert_grads("ties and dominated row, backward", (n, l, c), ops.attention_bwd(qkv.to(dev), y64.float().to(dev), d_o.to(dev), c), g64, c)
