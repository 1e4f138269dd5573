"""Shared draws and expectations of the split_mode=average decode tests (test_cpu_decode_average.py, test_gpu_decode_average.py).

Operands: unit item rows from unit-normal draws; unit head rows with a component of 0.6 along a direction shared by the heads of
one user (so the mean over heads keeps a norm of about 0.65-0.8 and the k-th mean of a catalog sits well above 0).
Expected means: numpy on the fp32 operands, the -inf masks of the reference (tag word x row bits, then oracle.decode_oracle.
suppress for the pad id and the history), then the arithmetic of decode_oracle.average_heads_topk (sum of the finite heads /
(finite count + 1e-8), cast to fp32) and its order (value desc, index asc)."""
import numpy as np

from oracle import decode_oracle as DO

BIT31 = -(1 << 31)
STREAM_SEED = 25          # a draw whose k-th mean (B = 6, N = 6000, D = 64, k = 20) lies in 0.21-0.25 for all three head layouts


def l2n(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def layout_bits(layout, B, N, rng):
    """layout ("mult", S, C) / ("add", S, C): multi-hot tags; ("nce", H): no tag table.
    -> (H, tag_bits [N] int32 or None, row_bits [B, H] int32)."""
    kind = layout[0]
    if kind == "nce":
        H = layout[1]
        return H, None, np.full((B, H), BIT31, np.int32)
    S, C = layout[1], layout[2]
    tags = rng.random((N, C)) < 0.5
    tags[np.arange(N), rng.integers(0, C, N)] = True
    word = (tags.astype(np.int64) << np.arange(C)).sum(1) | (1 << 31)
    tag_bits = np.where(word >= (1 << 31), word - (1 << 32), word).astype(np.int32)
    if kind == "mult":
        H = S * C
        row = np.array([1 << (h % C) for h in range(H)], np.int64)
    else:
        H = S + C
        row = np.array([(1 << 31) if h < S else 1 << (h - S) for h in range(H)], np.int64)
    row = np.where(row >= (1 << 31), row - (1 << 32), row).astype(np.int32)
    return H, tag_bits, np.tile(row[None], (B, 1))


def draw(seed, B, N, D, layout, n_hist=0, shared=0.6):
    rng = np.random.default_rng(seed)
    H, tag_bits, row_bits = layout_bits(layout, B, N, rng)
    common = l2n(rng.standard_normal((B, 1, D)))
    heads = shared * common + np.sqrt(1.0 - shared * shared) * l2n(rng.standard_normal((B, H, D)))
    heads = l2n(heads.astype(np.float32)).astype(np.float32)
    items = l2n(rng.standard_normal((N, D)).astype(np.float32)).astype(np.float32)
    hist = [np.sort(rng.choice(np.arange(1, N), n_hist, replace=False)) for _ in range(B)] if n_hist else None
    return dict(B=B, H=H, N=N, D=D, heads=heads, items=items, tag_bits=tag_bits, row_bits=row_bits, hist=hist)


def masked_scores(d, dtype=np.float32):
    """[B, H, N] scores of the fp32 operands with the reference's -inf masks.  d["alias"] = (columns, source column): item rows
    that are copies of one row take that row's scores (a BLAS product need not give identical columns bit-equal results)."""
    sc = np.einsum("bhd,nd->bhn", d["heads"].astype(dtype), d["items"].astype(dtype)).astype(dtype)
    if d.get("alias") is not None:
        sc[:, :, d["alias"][0]] = sc[:, :, d["alias"][1]][:, :, None]
    tb = np.full(d["N"], BIT31, np.int32) if d["tag_bits"] is None else d["tag_bits"]
    dead = (d["row_bits"][:, :, None] & tb[None, None, :]) == 0
    sc[dead] = -np.inf
    if d["hist"] is not None:
        hu = np.concatenate([np.full(len(h), b) for b, h in enumerate(d["hist"])])
        hi = np.concatenate(d["hist"])
        return DO.suppress(sc, hu, hi)
    return DO.suppress(sc)


def mean_of_finite(sc):
    """decode_oracle.average_heads_topk's arithmetic -> [B, N] fp32."""
    finite = np.isfinite(sc)
    return (np.where(finite, sc, 0).sum(1) / (finite.sum(1) + 1e-8)).astype(np.float32)


def expected(d, k):
    """-> (means [B, N] fp32, order [B, k + 1]: the oracle's ranking, one past k for the gap below the k-th)."""
    means = mean_of_finite(masked_scores(d))
    order = np.stack([DO.topk_desc(means[b], k + 1)[0] for b in range(d["B"])])
    return means, order


def csr_history(d):
    if d["hist"] is None:
        return None, None
    ptr = np.concatenate([[0], np.cumsum([len(h) for h in d["hist"]])]).astype(np.int32)
    return ptr, np.concatenate(d["hist"]).astype(np.int64)


def compare(vals, idx, means, order, k, tied_cap=0.02, same=None):
    """The project's top-k tolerances (tests/test_gpu_kernels.py::test_exact_topk_matches_reference_scores): position j is untied
    when both neighbouring gaps of the oracle's sorted means exceed 1e-6; indices equal at untied positions; values within 2e-6
    of the oracle's mean of the RETURNED index.  Positions whose oracle mean is exactly 0 (items masked in every head) tie
    exactly and are compared exactly: ascending index is the select's and the oracle's rule; so are neighbours `same(a, b)`
    declares exact ties (identical rows).  Neither counts towards the tied share, which is capped at tied_cap of B*k."""
    B = means.shape[0]
    tied = 0
    for b in range(B):
        o = order[b]
        v = means[b, o].astype(np.float64)
        got = idx[b]
        assert len(set(got.tolist())) == k, (b, "duplicate items")
        np.testing.assert_allclose(vals[b], means[b, got], rtol=0, atol=2e-6, err_msg=f"user {b}")
        for j in range(k):
            def clear(a, c):
                return (v[a] - v[c] > 1e-6) or (v[a] == 0.0 and v[c] == 0.0) or (same is not None and same(b, o[a], o[c]))
            if (j == 0 or clear(j - 1, j)) and clear(j, j + 1):
                assert got[j] == o[j], (b, j, int(got[j]), int(o[j]), v[max(j - 1, 0):j + 2])
            else:
                tied += 1
    assert tied <= tied_cap * B * k, (tied, B * k)
    return tied
