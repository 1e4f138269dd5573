"""Seeded inputs of the streaming-metrics tests and a numpy restatement of the sums the device accumulates (test helper, not
a test module).  Recall, NDCG and Entropy come from `oracle/metrics_oracle.py`; Hit, MRR, MAP and Precision are restated here
from the formulas of the reference's `evaluator/metrics.py` (67-69, 93-101, 131-142, 262-263)."""
import numpy as np

from oracle import metrics_oracle as MO

COLUMNS = ("recall", "ndcg", "hit", "mrr", "map", "precision")


def hit_curve(hits, pos_len):
    return (np.cumsum(hits, axis=1) > 0).astype(np.float64)


def mrr_curve(hits, pos_len):
    out = np.zeros(hits.shape, dtype=np.float64)
    for r in range(hits.shape[0]):
        nz = np.flatnonzero(hits[r])
        if nz.size:
            out[r, nz[0]:] = 1.0 / (nz[0] + 1)
    return out


def map_curve(hits, pos_len):
    K = hits.shape[1]
    ranks = np.arange(1, K + 1)
    pre = np.cumsum(hits, axis=1) / ranks
    sum_pre = np.cumsum(pre * hits.astype(np.float64), axis=1)
    return sum_pre / np.minimum(ranks[None, :], np.minimum(pos_len, K)[:, None])


def precision_curve(hits, pos_len):
    return np.cumsum(hits, axis=1) / np.arange(1, hits.shape[1] + 1)


CURVES = (MO.recall_curve, MO.ndcg_curve, hit_curve, mrr_curve, map_curve, precision_curve)


def pos_len_full(positives):
    """The collector's distinct-positive count: column p counts the distinct values among the first p + 1 of the ASCENDING
    SORTED row (reference collector.py:301-304 sorts before it counts; part of the contract)."""
    srt = np.sort(positives, axis=1)
    first = np.ones(srt.shape, dtype=bool)
    first[:, 1:] = srt[:, 1:] != srt[:, :-1]
    return np.cumsum(first, axis=1).astype(np.int32)


def hit_matrix(topk_idx, positives, p):
    return (topk_idx[:, :, None] == positives[:, None, :p + 1]).any(axis=2)


def sums_from_hits(hits, pos_len, group_masks, topk):
    """hits [B, K] bool, pos_len [B], group_masks [G, B] bool -> sums [G, 6, T], counts [G]."""
    cols = [k - 1 for k in topk]
    sums = np.zeros((len(group_masks), len(COLUMNS), len(topk)), dtype=np.float64)
    counts = np.zeros(len(group_masks), dtype=np.int64)
    for g, m in enumerate(group_masks):
        counts[g] = int(m.sum())
        for c, fn in enumerate(CURVES):
            sums[g, c] = np.asarray(fn(hits[m], pos_len[m]), dtype=np.float64).sum(axis=0)[cols]
    return sums, counts


def numpy_sums(topk_idx, positives, preds, topk, group_bits, n_groups, tag_table=None):
    """The contract of mhr_eval_metric_sums in numpy: sums [P, G, 6, T], counts [P, G], entropy [T] (None without tags)."""
    K = max(topk)
    plf = pos_len_full(positives)
    sums = np.zeros((len(preds), n_groups, len(COLUMNS), len(topk)), dtype=np.float64)
    counts = np.zeros((len(preds), n_groups), dtype=np.int64)
    for i, p in enumerate(preds):
        hits = hit_matrix(topk_idx, positives, p)[:, :K]
        masks = [((group_bits[:, i].astype(np.int64) >> g) & 1).astype(bool) for g in range(n_groups)]
        sums[i], counts[i] = sums_from_hits(hits, plf[:, p].astype(np.int64), masks, topk)
    entropy = None
    if tag_table is not None:
        e = MO.entropy(tag_table[topk_idx[:, :K]].astype(bool), topk)
        entropy = np.asarray([e[f"Entropy@{k}"] for k in topk], dtype=np.float64)
    return sums, counts, entropy


def make_case(seed, B, K, E, C, G, N=None, n_pred=None):
    """Seeded inputs with the edge cases the kernel can get wrong: duplicated positives, users without a hit, users in no group
    but bit 0, one empty group (the last but one when G > 2), pos_len > K when E > K."""
    rng = np.random.default_rng(seed)
    N = N or max(4 * K + 16, 64)
    topk_idx = np.stack([rng.permutation(np.arange(1, N))[:K] for _ in range(B)]).astype(np.int64)
    positives = rng.integers(1, N, size=(B, E)).astype(np.int64)
    for b in range(B):
        r = b % 4
        if r == 0:                                   # a hit at a random rank for the first target
            positives[b, 0] = topk_idx[b, rng.integers(0, K)]
        elif r == 1:                                 # several hits, one target duplicated
            take = rng.integers(0, K, size=E)
            positives[b] = topk_idx[b, take]
            if E > 1:
                positives[b, E - 1] = positives[b, 0]
        elif r == 2:                                 # no hit at all: targets outside the catalog slice of the list
            positives[b] = N + 1 + rng.integers(0, 5, size=E)
    preds = sorted({0, E - 1, max(E // 2 - 1, 0)})[:n_pred]
    bits = rng.integers(0, 2 ** G, size=(B, len(preds)), dtype=np.int64) | 1
    bits[::5] = 1                                    # users in no group but bit 0
    if G > 2:
        bits &= ~(1 << (G - 2))                      # one empty group
    group_bits = bits.astype(np.uint32)
    tags = rng.random((N + 8, C)) < 0.4
    tags[np.arange(N + 8), rng.integers(0, C, N + 8)] = True
    return dict(topk_idx=topk_idx, positives=positives, preds=preds, group_bits=group_bits, tags=tags, N=N + 8)
