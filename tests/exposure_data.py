"""Seeded inputs of the exposure-metric tests and a numpy restatement of the reference's five catalog metrics (test helper, not a
test module).  The formulas restate the reference's `evaluator/metrics.py`: ItemCoverage.get_coverage 505-516,
AveragePopularity.get_pop / metric_info / topk_result 550-585, ShannonEntropy.get_entropy 624-640, GiniIndex.get_gini 679-696,
TailPercentage.get_tail / metric_info 733-764 (tail_ratio default 724-725)."""
import math

import numpy as np

CUTS = [1, 5, 10, 20]
NAMES = ("itemcoverage", "averagepopularity", "shannonentropy", "giniindex", "tailpercentage")


def make_lists(seed, U, K, N, common_top1=True):
    """[U, K] int64 lists without a repeat inside a list.  One item is in every user's top-5 (count = U: the largest count an
    item can reach) - at rank 0 for everyone with common_top1, at ranks 0..4 in turn otherwise (then the top-1 lists still
    differ, which keeps the entropy at k = 1 away from 0); items 0 and N - 1 occur."""
    rng = np.random.default_rng(seed)
    common = 3 % N
    lists = np.empty((U, K), dtype=np.int64)
    for u in range(U):
        row = rng.permutation(N)[:K]
        row = row[row != common]
        row = np.concatenate(([common], row))[:K]
        if not common_top1:
            r = u % 5
            row[[0, r]] = row[[r, 0]]
        lists[u] = row
    for u, r, v in ((1, K - 1, 0), (2, 1, N - 1), (3, 2, 0), (4, 3, N - 1)):   # K - 1 lies past the last cut when K > max(CUTS)
        if u < U and v not in lists[u]:                                  # (never on the common item's rank, never a repeat)
            lists[u, r] = v
    return lists


def make_pop(seed, N):
    """Training interaction counts phi [N] int64: pad 0, a fifth of the items never seen, ties in phi (a small range)."""
    rng = np.random.default_rng(seed)
    pop = rng.integers(1, 9, size=N).astype(np.int64)
    pop[rng.random(N) < 0.2] = 0
    pop[0] = 0
    return pop


def band_histogram(lists, cuts, N):
    """band[t][i] = occurrences of item i at the ranks [cuts[t-1], cuts[t]) (the contract of mhr_exposure_accumulate)."""
    band = np.zeros((len(cuts), N), dtype=np.int64)
    lo = 0
    for t, hi in enumerate(cuts):
        np.add.at(band[t], lists[:, lo:hi].reshape(-1), 1)
        lo = hi
    return band


def tail_mask(pop, tail_ratio):
    """The reference's tail list (get_tail 743-749) over the counter {i >= 1 : pop[i] > 0}, as a 0/1 vector."""
    if tail_ratio is None or tail_ratio <= 0:
        tail_ratio = 0.1
    counter = {i: int(pop[i]) for i in range(1, len(pop)) if pop[i] > 0}
    if tail_ratio > 1:
        items = [i for i, c in counter.items() if c <= tail_ratio]
    else:
        srt = sorted(counter.items(), key=lambda kv: (kv[1], kv[0]))
        items = [i for i, _ in srt[:max(int(len(srt) * tail_ratio), 1)]]
    mask = np.zeros(len(pop), dtype=np.uint8)
    mask[items] = 1
    return mask


def _c_ln_c(c):
    """c ln c rounded once to fp64 (from the 80-bit log where numpy has one, so the helper's own term error stays near half an ulp)."""
    if np.finfo(np.longdouble).nmant >= 63:
        return float(np.longdouble(c) * np.log(np.longdouble(c)))
    return c * math.log(c)


def integer_sums(band, pop=None, tail=None):
    """The contract of mhr_exposure_finalize in Python integers: ints [n_cuts, 4] = (R, sum c phi, sum c tail, G), S [n_cuts]
    = fsum of c ln c.  G is formed as the reference forms it (get_gini 690-694): the sorted non-zero counts at idx N-R+1..N."""
    N = band.shape[1]
    ints, S = np.zeros((band.shape[0], 4), dtype=np.int64), np.zeros(band.shape[0], dtype=np.float64)
    cum = np.cumsum(band, axis=0)
    for t, c in enumerate(cum):
        nz = sorted(int(v) for v in c if v > 0)
        R = len(nz)
        G = sum((2 * idx - N - 1) * v for idx, v in zip(range(N - R + 1, N + 1), nz))
        P = sum(int(v) * int(p) for v, p in zip(c, pop)) if pop is not None else 0
        Tl = sum(int(v) for v, m in zip(c, tail) if m) if tail is not None else 0
        ints[t] = (R, P, Tl, G)
        S[t] = math.fsum(_c_ln_c(v) for v in nz)
    return ints, S


def reference_values(lists, cuts, N, pop, tail_ratio):
    """name@k -> value: the reference's five formulas, restated on the item matrix itself (no histogram)."""
    out = {}
    tail = set(np.flatnonzero(tail_mask(pop, tail_ratio)).tolist())
    pop_m = np.where(lists > 0, pop[np.clip(lists, 0, N - 1)], 0)         # item_count.get(id, 0): 550-565
    tail_m = np.vectorize(lambda i: 1 if i in tail else 0)(lists)         # 750-755
    ranks = np.arange(1, lists.shape[1] + 1)
    pop_c = (pop_m.cumsum(axis=1) / ranks).mean(axis=0)                   # 568, 581
    tail_c = (tail_m.cumsum(axis=1) / ranks).mean(axis=0)                 # 764, 777
    for k in cuts:
        m = lists[:, :k]
        ids, cnt = np.unique(m, return_counts=True)
        total = m.shape[0] * m.shape[1]
        out[f"itemcoverage@{k}"] = ids.shape[0] / N                       # 515-516
        out[f"averagepopularity@{k}"] = pop_c[k - 1]
        out[f"tailpercentage@{k}"] = tail_c[k - 1]
        h = 0.0
        for c in cnt.tolist():                                            # 636-640
            p = c / total
            h += -p * np.log(p)
        out[f"shannonentropy@{k}"] = h / len(cnt)
        srt = np.sort(cnt)                                                # 690-696
        idx = np.arange(N - len(srt) + 1, N + 1)
        out[f"giniindex@{k}"] = np.sum((2 * idx - N - 1) * srt) / total / N
    return out


def exposure_struct(ints, S, N, U, cuts):
    """What the collector hands out as 'rec.exposure_sums'."""
    return dict(ints=np.asarray(ints, dtype=np.int64), S=np.asarray(S, dtype=np.float64), N=int(N), U=int(U), cuts=list(cuts))


class Cfg(dict):
    """Missing keys read as None, like the project's Config."""

    def __getitem__(self, k):
        return dict.get(self, k)

    def get(self, k, d=None):
        v = dict.get(self, k)
        return d if v is None else v


def base_cfg(**kw):
    """The smallest configuration an Evaluator and a Collector accept: one head, one pred_len, the cut-offs CUTS."""
    return Cfg(dict(metrics=["Recall"], shared_metrics=[], topk=list(CUTS), eval_num_cats=1, eval_pred_len=1,
                    int_to_category={0: "cat0"}, metrics_pred_len_list=[0], head_interaction="multiplicative", num_segment_head=1,
                    num_prior_head=1, split_mode="combine"), **kw)
