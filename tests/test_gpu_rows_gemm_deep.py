"""ops.rows_gemm_deep - the K = 1024 input gradients of the uvqk projection (W stored [N, K]) and of the decoding heads (W stored
[K, N]) - against the fp32 product of the same bf16 operands, its run-to-run equality, and its routing from the two autograd
functions that own those gradients.  Tolerance: that of test_rows_gemm_against_the_fp32_product (one bf16 rounding of the result
plus accumulation slack, with a factor 2); on the CPU two different fp32 summation orders at K = 1024 followed by the bf16
rounding stay below 1.0 tol at M in {32, 33, 77, 333, 4097}."""
import os
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

K, N = 1024, 256


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mhr_amd  # noqa: F401
    from mhr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def HF(ops):
    code = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")
    if code not in sys.path:
        sys.path.insert(0, code)
    from REC.model import hstu_functional
    return hstu_functional


def _operands(M, lda_pad=0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(11 + M + seed)
    a_full = (torch.randn(M, K + lda_pad, device="cuda", generator=g) * 0.5).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).bfloat16()
    return a_full, w


def _within(got, ref):
    tol = 2 ** -8 * ref.abs().clamp_min(1e-3) + 1e-6
    worst = float(((got - ref).abs() / tol).max())
    print(f"worst |got - ref| / tol = {worst:.3f} (limit 2)")
    return bool(((got - ref).abs() <= 2 * tol).all()), worst


@pytest.mark.parametrize("kn", [False, True])
@pytest.mark.parametrize("M,lda_pad,ldc_pad", [(32, 0, 0), (33, 0, 0), (77, 0, 0), (1000, 256, 0), (4097, 0, 0), (32 * 257, 0, 0),
                                               (333, 0, 64)])
def test_rows_gemm_deep_against_the_fp32_product(ops, M, lda_pad, ldc_pad, kn):
    """One tile, a one-row partial tile, ragged M, a strided source, an uneven tile count per stream with more workgroups than
    tiles, and the output as a column block of a wider buffer - both weight layouts.  The guard row behind M and the guard
    columns beyond N keep their fill."""
    a_full, w = _operands(M, lda_pad)
    a = a_full[:, :K]
    out = torch.full((M + 1, N + ldc_pad), 7.0, dtype=torch.bfloat16, device="cuda")
    w_dev = w.t().contiguous() if kn else w
    ops.rows_gemm_deep(a, w_dev, out=out[:M, :N], w_is_kn=kn)
    torch.cuda.synchronize()
    ref = a.float() @ w.float().t()
    ok, worst = _within(out[:M, :N].float(), ref)
    assert ok, worst
    assert bool((out[M] == 7.0).all())
    if ldc_pad:
        assert bool((out[:, N:] == 7.0).all())


@pytest.mark.parametrize("kn", [False, True])
def test_rows_gemm_deep_is_bitwise_repeatable(ops, kn):
    a_full, w = _operands(4097 + 64, seed=3)
    w_dev = w.t().contiguous() if kn else w
    first = ops.rows_gemm_deep(a_full, w_dev, w_is_kn=kn)
    second = ops.rows_gemm_deep(a_full, w_dev, w_is_kn=kn)
    torch.cuda.synchronize()
    assert torch.equal(first, second)


def test_input_gradients_of_uvqk_and_heads_run_on_rows_gemm_deep(ops, HF, monkeypatch):
    """SplitKLinearFn (the uvqk layout: y = x @ W, W [256, 1024]) and FusedHeadsLinearFn (W [1024, 256]) at 8192 + 32 rows: with
    the switch on, dx comes from ops.rows_gemm_deep and meets the kernel's tolerance against the fp32 product; every weight and
    bias gradient is bitwise what the switch-off run gives.  (In deterministic mode: outside it the column sums behind those
    gradients add with float atomics and differ in the last bits between any two runs, whatever computes dx.)"""
    M, D = 8192 + 32, 256
    g = torch.Generator(device="cuda").manual_seed(2)
    x = (torch.randn(M, D, device="cuda", generator=g) * 0.5).bfloat16()
    dy = (torch.randn(M, K, device="cuda", generator=g) * 0.5).bfloat16()
    w_uvqk = (torch.randn(D, K, device="cuda", generator=g) * K ** -0.5)
    w_heads = (torch.randn(K, D, device="cuda", generator=g) * K ** -0.5).bfloat16()
    b_heads = (torch.randn(K, device="cuda", generator=g) * 0.1).bfloat16()
    monkeypatch.setattr(HF, "ROWS_GEMM_DEEP_MIN_M", 1)
    real, calls = ops.rows_gemm_deep, []
    monkeypatch.setattr(ops, "rows_gemm_deep", lambda *a, **k: (calls.append((tuple(a[0].shape), k.get("w_is_kn"))), real(*a, **k))[1])

    def run(on):
        monkeypatch.setattr(HF, "ROWS_GEMM_DEEP", on)
        xs = x.clone().requires_grad_(True)
        ws = w_uvqk.clone().requires_grad_(True)
        HF.SplitKLinearFn.apply(xs, ws, None, False, None).backward(dy)
        xh = x.clone().requires_grad_(True)
        gw, gb = torch.zeros(K, D, device="cuda"), torch.zeros(K, device="cuda")
        HF.FusedHeadsLinearFn.apply(xh, w_heads, b_heads, gw, gb).backward(dy)
        torch.cuda.synchronize()
        return xs.grad, ws.grad, xh.grad, gw, gb

    n0 = len(calls)
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        dx_u, dw_u, dx_h, gw, gb = run(True)
        assert calls[n0:] == [((M, K), False), ((M, K), True)]
        off = run(False)
    finally:
        ops.set_deterministic(was)
    assert len(calls) == n0 + 2
    ok, worst = _within(dx_u.float(), dy.float() @ w_uvqk.bfloat16().float().t())
    assert ok, worst
    ok, worst = _within(dx_h.float(), dy.float() @ w_heads.float())
    assert ok, worst
    assert torch.equal(dw_u, off[1]) and torch.equal(gw, off[3]) and torch.equal(gb, off[4])
