"""The rejection inequality of the false-negative prefix filter (csrc/nce.hip: nce_fix_prefix_kernel), restated in numpy on
bf16-rounded data: a pair is rejected only if

    S_p <= thres - |thres| 2^-20 - 2^-100 - a_rem * b_rem - (D 2^-21) * a_full * b_full

(S_p the fp32 prefix product over the first 64 columns, a_* the target's remainder / full norm, b_* the largest such norms of
the negative's 32-row tile, every sum of squares raised by D 2^-126; all in fp32 as the kernel forms them), and no rejected
pair may have an fp32 dot product over all D columns (k ascending, as the exhaustive kernel accumulates) above thres.  Random
rows and the adversarial constructions of tests/test_gpu_nce_fix_filter.py; runs without a GPU."""
import numpy as np
import pytest
import torch

KP = 64
f32 = np.float32


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).bfloat16().float().numpy()


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _dot_k_ascending(t, n, k0, k1):
    """fp32 accumulation, k ascending: [rows, negs]"""
    acc = np.zeros((t.shape[0], n.shape[0]), f32)
    for k in range(k0, k1):
        acc = (acc + np.outer(t[:, k], n[:, k]).astype(f32)).astype(f32)
    return acc


def _sumsq(x):
    acc = np.zeros(x.shape[0], f32)
    for k in range(x.shape[1]):
        acc = (acc + x[:, k] * x[:, k]).astype(f32)
    return acc


def _rejected(t, n, thres):
    """The filter's decision for every (target row, negative) pair; t, n are the bf16 values the MFMAs see (as fp32)."""
    D = t.shape[1]
    floor, eps = f32(D * 2.0 ** -126), f32(D * 2.0 ** -21)
    with np.errstate(all="ignore"):
        a_rem = np.sqrt(_sumsq(t[:, KP:]) + floor).astype(f32)
        a_full = np.sqrt((_sumsq(t[:, :KP]) + _sumsq(t[:, KP:])).astype(f32) + floor).astype(f32)
        nr = np.sqrt(_sumsq(n[:, KP:]) + floor).astype(f32)
        nf = np.sqrt(_sumsq(n) + floor).astype(f32)

        def tile_max(v):           # NaN wins, as in the kernel
            v = v.reshape(-1, 32)
            m = np.where(np.isnan(v).any(1), f32(np.nan), np.nanmax(np.where(np.isnan(v), -np.inf, v), axis=1))
            return np.repeat(m.astype(f32), 32)
        b_rem, b_full = tile_max(nr), tile_max(nf)
        thr_lo = f32(f32(thres) - f32(abs(thres)) * f32(2.0 ** -20) - f32(2.0 ** -100))
        lim = (thr_lo - np.outer(a_rem, b_rem).astype(f32)).astype(f32)
        lim = (lim - np.outer((eps * a_full).astype(f32), b_full).astype(f32)).astype(f32)
        s_p = _dot_k_ascending(t, n, 0, KP)
        return s_p <= lim          # an unordered compare (NaN) does NOT reject


def _targets_as_kernel(p):
    """row_inv_norm + load_norm_frags: bf16(p * (1 / |p|)) with the norm in fp32"""
    with np.errstate(all="ignore"):
        inv = (f32(1.0) / np.sqrt(_sumsq(p.astype(f32)))).astype(f32)
        return _bf16(p.astype(f32) * inv[:, None])


def _near(t, cos, cols, rng):
    e = np.zeros_like(t)
    e[:, cols] = rng.standard_normal((t.shape[0], len(cols)))
    ts = np.zeros_like(t)
    ts[:, cols] = t[:, cols]
    e -= (e * ts).sum(-1, keepdims=True) / np.maximum((ts * ts).sum(-1, keepdims=True), 1e-30) * ts   # e . t = 0, e inside cols
    return _unit(t + np.sqrt(1.0 / cos ** 2 - 1.0)[:, None] * _unit(e))


def _pool(D, thres, scale, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((64, D))
    p[10:14, KP:] = 0.0                                   # all mass in the prefix
    p[14:18, :KP] = 0.0                                   # none there
    p[18:20] *= 1e-3
    tn = _unit(p)
    p[5] = 0.0                                            # zero row: NaN fragments
    n = _unit(rng.standard_normal((256, D)))
    n[0:8, KP:] = 0.0
    n[8:16, :KP] = 0.0
    n[0:16] = _unit(n[0:16])
    c = min(max(thres, -0.9), 0.999)
    cos = np.clip(c + (rng.random(32) * 2 - 1) * 1e-3, None, 0.99999)
    src = rng.integers(6, 64, 96)
    n[32:64] = tn[src[:32]]                                                   # planted: cos = 1
    n[64:96] = _near(tn[src[32:64]], cos, np.arange(0, KP), rng)              # difference inside the prefix
    n[96:128] = _near(tn[src[64:96]], cos, np.arange(KP, D), rng)             # difference outside it
    return _targets_as_kernel(p), _bf16(n * scale)


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("scale", [1.0, 3.0, 1e-3])
@pytest.mark.parametrize("thres", [0.99, 0.5, 0.0, -1.0])
def test_filter_never_rejects_a_pair_above_thres(thres, scale, D):
    t, n = _pool(D, thres, scale, seed=int(1000 * (thres + 2)) + D)
    rej = _rejected(t, n, thres)
    with np.errstate(all="ignore"):
        s = _dot_k_ascending(t, n, 0, D)
        hit = s > f32(thres)
    assert not (rej & hit).any(), f"{int((rej & hit).sum())} pairs above thres rejected"
    if scale >= 1.0:
        assert hit[6:, 32:64].any()                                           # the planted targets are hits
    assert not rej[5].any()                                                   # the NaN row is never rejected
    if thres == 0.99 and scale == 1.0:
        assert rej[20:, 128:].mean() > 0.999                                  # and the filter filters: random pairs go
    if thres <= 0.0 and scale == 1.0:
        assert rej[20:, 128:].mean() < 0.01                                   # nothing to reject at such a thres


def test_filter_survives_tiny_and_huge_magnitudes():
    """Squares that underflow (|x| ~ 1e-25) and negatives large enough to overflow the norm: the bound must still hold."""
    rng = np.random.default_rng(3)
    D = 256
    t = _targets_as_kernel(rng.standard_normal((32, D)))
    for mag in (1e-25, 1e-19, 1e19, 3e38):
        n = _bf16(_unit(rng.standard_normal((64, D))) * mag)
        n[:32, :KP] = 0.0                                                     # s_p = 0 exactly: only the remainder decides
        for thres in (0.0, -1e-30, 0.99):
            rej = _rejected(t, n, thres)
            with np.errstate(all="ignore"):
                hit = _dot_k_ascending(t, n, 0, D) > f32(thres)
            assert not (rej & hit).any(), (mag, thres)
