"""split_mode=average on the CPU: the pattern table of the fused decode (ops.tag_patterns, plain torch) and the identity the
decode rests on - for every item whose tag word is w, the mean over the finite heads of <u[b,h], i[n]> equals <q[b,w], i[n]>
with q[b,w] the mean of the heads live for w (reference collector.py:227-230 on the masks of hstu.py:982-1015) - in numpy on
the shapes of the GPU tests."""
import numpy as np
import pytest
import torch

import decode_average_data as AD

LAYOUTS = [("mult", 2, 4), ("add", 2, 3), ("nce", 4)]


@pytest.fixture(scope="module")
def ops():
    import mhr_amd  # noqa: F401
    from mhr_amd import ops as _ops
    return _ops


def test_pattern_table_words_and_one_hot_bits(ops):
    d = AD.draw(3, 2, 500, 16, ("mult", 2, 4))
    tag_bits = torch.from_numpy(d["tag_bits"])
    words, pbits = ops.tag_patterns(tag_bits)
    assert words.dtype == torch.int32 and pbits.dtype == torch.int32 and pbits.shape == tag_bits.shape
    assert sorted(words.tolist()) == sorted(set(d["tag_bits"].tolist())) and len(words) == 15      # every non-empty subset of 4 tags
    pb = pbits.numpy().view(np.uint32)
    assert np.all((pb & (pb - 1)) == 0) and np.all(pb != 0)                                        # one-hot
    pid = np.log2(pb.astype(np.float64)).astype(np.int64)
    assert np.array_equal(words.numpy()[pid], d["tag_bits"])                                       # bit p <-> words[p]


def test_pattern_table_without_tags_is_one_pattern(ops):
    words, pbits = ops.tag_patterns(None)
    assert pbits is None and words.tolist() == [AD.BIT31]


def test_pattern_table_32_patterns_fit_33_raise(ops):
    words, pbits = ops.tag_patterns(torch.arange(32, dtype=torch.int32) | AD.BIT31)
    assert len(words) == 32 and sorted(pbits.numpy().view(np.uint32).tolist()) == [1 << p for p in range(32)]
    with pytest.raises(ValueError, match=r"at most 32.*predict\(\)"):
        ops.tag_patterns(torch.arange(33, dtype=torch.int32) | AD.BIT31)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: l[0])
def test_pattern_mean_queries_reproduce_the_mean_of_finite_heads(ops, layout):
    k = 20
    d = AD.draw(AD.STREAM_SEED, 6, 6000, 64, layout, n_hist=12)
    means, order = AD.expected(d, k)
    kth = means[np.arange(d["B"]), order[:, k - 1]]
    assert np.all((kth > 0.21) & (kth < 0.25)), kth                      # every user stays on the streaming path of the GPU decode
    words, pbits = ops.tag_patterns(None if d["tag_bits"] is None else torch.from_numpy(d["tag_bits"]))
    words = words.numpy()
    pid = np.zeros(d["N"], np.int64) if pbits is None else np.log2(pbits.numpy().view(np.uint32).astype(np.float64)).astype(np.int64)
    live = (d["row_bits"][:, :, None] & words[None, None, :]) != 0                                  # [B, H, P]
    cnt = live.sum(1)                                                                              # [B, P]
    q = np.einsum("bhp,bhd->bpd", live.astype(np.float32), d["heads"]) / np.maximum(cnt, 1)[..., None].astype(np.float32)
    got = np.einsum("bnd,nd->bn", q[:, pid, :], d["items"]).astype(np.float32)                     # <q[b, w(n)], i[n]>
    masked = ~np.isfinite(AD.masked_scores(d)).any(axis=1)                                         # pad id, history: no head is finite
    assert masked[:, 0].all() and masked.sum() == d["B"] * 13
    assert np.all(means[masked] == 0.0)                                                            # the reference's 0 / 1e-8
    assert np.abs(got[~masked] - means[~masked]).max() <= 1e-6
    # a word no live head admits: q = 0 exactly, and so is the reference's mean
    d["row_bits"][0, :] = 0
    assert np.all(AD.expected(d, k)[0][0] == 0.0)
