"""Ranking metrics over the [users, K+1] hit matrix (reference `code/REC/evaluator/metrics.py:17-41, 145-238`,
`base_metric.py:37-81`; Hit / MRR / MAP / Precision: `metrics.py:44-142, 241-263`).  Host-side numpy: per-user curves @1..K are
summed over the rank's users; the trainer divides by the global user count after the all-reduce (reference
trainer.py:1109-1123).  With `stream_metrics` the collector hands out the sums themselves (`'rec.metric_sums'`,
`'rec.entropy_sums'`: the device reduced them batch by batch) and the classes only name them.
The catalog-exposure metrics (reference `metrics.py:473-780`) are final values formed from the integer sums of the device's item
histogram (`'rec.exposure_sums'`); they belong in `shared_metrics`."""
import numpy as np

COLUMNS = ('recall', 'ndcg', 'hit', 'mrr', 'map', 'precision')      # column order of 'rec.metric_sums' (mhr_eval_metric_sums)


class _TopkMetric:
    name = ''
    needs = ('rec.topk',)
    by_group = False                      # per-category / outlier breakdown (the reference has it for Recall and NDCG only)

    def __init__(self, config):
        self.topk = config['topk']
        self.num_prior_categories = config['eval_num_cats']
        self.eval_by_cat = config.get('eval_by_cat', True)
        self.eval_pred_len = config['eval_pred_len']
        self.outlier_user_metrics = config['outlier_user_metrics']
        self.int_to_category = config['int_to_category']

    def used_info(self, dataobject):
        rec = dataobject.get('rec.topk')
        rec = rec.numpy() if hasattr(rec, 'numpy') else np.asarray(rec)
        K = max(self.topk)
        return rec[:, :K].astype(bool), rec[:, K].astype(np.int64)

    def curve(self, hits, pos_len):
        raise NotImplementedError

    def _pack(self, curve, num_samples=None, prefix=None):
        s = curve.sum(axis=0)
        out = {}
        for k in self.topk:
            key = f'{self.name}@{k}' if prefix is None else f'{prefix}-{self.name}@{k}'
            out[key] = s[k - 1] if num_samples is None else (s[k - 1], num_samples)
        return out

    def _from_sums(self, ms, pred_len):
        """The streamed form: sums [G, 6, n_topk] / counts [G] with group 0 = every user, 1 + c = category c, last = outliers."""
        sums, counts = ms['sums'][:, COLUMNS.index(self.name)], ms['counts']

        def pack(g, prefix=None):
            out = {}
            for t, k in enumerate(self.topk):
                key = f'{self.name}@{k}' if prefix is None else f'{prefix}-{self.name}@{k}'
                out[key] = sums[g, t] if prefix is None else (sums[g, t], int(counts[g]))
            return out
        out = pack(0)
        if self.by_group and self.num_prior_categories > 1 and self.eval_by_cat and ms['cats']:
            for c in range(self.num_prior_categories):
                out.update(pack(1 + c, self.int_to_category[c]))
        if self.by_group and self.outlier_user_metrics is not None and pred_len == self.eval_pred_len - 1 and ms['outlier']:
            out.update(pack(len(counts) - 1, f'outlier_{self.outlier_user_metrics}'))
        return out

    def calculate_metric(self, dataobject, pred_len=1):
        if 'rec.metric_sums' in dataobject:
            return self._from_sums(dataobject.get('rec.metric_sums'), pred_len)
        hits, pos_len = self.used_info(dataobject)
        out = self._pack(self.curve(hits, pos_len))
        if not self.by_group:
            return out
        if self.num_prior_categories > 1 and self.eval_by_cat and 'rec.tgt_tags' in dataobject:
            tgt = dataobject.get('rec.tgt_tags')
            tgt = tgt.numpy() if hasattr(tgt, 'numpy') else np.asarray(tgt)
            for c in range(self.num_prior_categories):
                m = tgt[:, c].astype(bool)
                out.update(self._pack(self.curve(hits[m], pos_len[m]), int(m.sum()), self.int_to_category[c]))
        if self.outlier_user_metrics is not None and pred_len == self.eval_pred_len - 1 and 'rec.outlier_users' in dataobject:
            o = dataobject.get('rec.outlier_users')
            o = (o.numpy() if hasattr(o, 'numpy') else np.asarray(o)).astype(bool)
            out.update(self._pack(self.curve(hits[o], pos_len[o]), int(o.sum()), f'outlier_{self.outlier_user_metrics}'))
        return out


class Recall(_TopkMetric):
    name = 'recall'
    by_group = True

    def curve(self, hits, pos_len):
        return np.cumsum(hits, axis=1) / pos_len.reshape(-1, 1)


class NDCG(_TopkMetric):
    name = 'ndcg'
    by_group = True

    def curve(self, hits, pos_len):
        K = hits.shape[1]
        disc = 1.0 / np.log2(np.arange(2, K + 2, dtype=np.float64))
        ideal = np.cumsum(disc)[np.minimum(np.arange(K)[None, :], np.minimum(pos_len, K)[:, None] - 1)]
        return np.cumsum(np.where(hits, disc[None, :], 0.0), axis=1) / ideal


class Hit(_TopkMetric):
    name = 'hit'

    def curve(self, hits, pos_len):
        return (np.cumsum(hits, axis=1) > 0).astype(int)


class MRR(_TopkMetric):
    name = 'mrr'

    def curve(self, hits, pos_len):
        first = hits.argmax(axis=1)                                  # rank of the first hit (0 when there is none)
        rr = np.where(hits.any(axis=1), 1.0 / (first + 1), 0.0)
        return np.where(np.arange(hits.shape[1])[None, :] >= first[:, None], rr[:, None], 0.0)


class MAP(_TopkMetric):
    name = 'map'

    def curve(self, hits, pos_len):
        K = hits.shape[1]
        ranks = np.arange(1, K + 1)
        pre = hits.cumsum(axis=1) / ranks
        sum_pre = np.cumsum(pre * hits.astype(np.float64), axis=1)
        return sum_pre / np.minimum(ranks[None, :], np.minimum(pos_len, K)[:, None])


class Precision(_TopkMetric):
    name = 'precision'

    def curve(self, hits, pos_len):
        return hits.cumsum(axis=1) / np.arange(1, hits.shape[1] + 1)


class Entropy:
    """Category diversity of the recommended lists (shared across pred_len)."""
    name = 'entropy'
    needs = ('rec.topk',)

    def __init__(self, config):
        self.topk = config['topk']

    def calculate_metric(self, dataobject, pred_len=1):
        if 'rec.entropy_sums' in dataobject:
            return {f'Entropy@{k}': v for k, v in zip(self.topk, dataobject.get('rec.entropy_sums'))}
        tags = dataobject.get('rec.rec_tags')
        tags = tags.numpy() if hasattr(tags, 'numpy') else np.asarray(tags)
        counts = np.cumsum(tags.astype(np.float64), axis=1)
        out = {}
        for k in self.topk:
            c = counts[:, k - 1, :]
            with np.errstate(divide='ignore', invalid='ignore'):
                p = c / c.sum(axis=1, keepdims=True)
                h = -np.sum(np.where(p > 0, p * np.log2(p), 0.0), axis=1)
            out[f'Entropy@{k}'] = h.sum(axis=0)
        return out


class _ExposureMetric:
    """Catalog-level metrics of the merged recommendation lists (reference metrics.py:473-780), from the integer sums the device
    forms out of its item histogram (`'rec.exposure_sums'`, mhr_exposure_finalize): ints [n_cuts, 4] = (R, sum c*phi,
    sum c*tail, G) and S [n_cuts] = sum c ln c per ascending cut-off in `cuts`, N items, U users.  With T = U*k occurrences the
    values are final (not sums over users) and do not depend on pred_len: shared metrics."""
    name = ''
    needs = ('rec.exposure_sums',)
    needs_item_counts = False

    def __init__(self, config):
        self.topk = config['topk']

    def value(self, R, P, Tl, G, S, N, T):
        raise NotImplementedError

    def calculate_metric(self, dataobject, pred_len=-1):
        ex = dataobject.get('rec.exposure_sums')
        ints, S = np.asarray(ex['ints'], dtype=np.int64), np.asarray(ex['S'], dtype=np.float64)
        N, U, cuts = int(ex['N']), int(ex['U']), [int(c) for c in ex['cuts']]
        out = {}
        for k in self.topk:
            t = cuts.index(k)
            R, P, Tl, G = (int(v) for v in ints[t])
            out[f'{self.name}@{k}'] = float(self.value(R, P, Tl, G, np.float64(S[t]), N, U * k)) if U > 0 else 0.0
        return out


class ItemCoverage(_ExposureMetric):
    name = 'itemcoverage'

    def value(self, R, P, Tl, G, S, N, T):
        return np.float64(R) / np.float64(N)                                 # metrics.py:515-516


class AveragePopularity(_ExposureMetric):
    name = 'averagepopularity'
    needs_item_counts = True

    def value(self, R, P, Tl, G, S, N, T):
        return np.float64(P) / np.float64(T)                                 # metrics.py:568, 581: every user divides by the same k


class TailPercentage(_ExposureMetric):
    name = 'tailpercentage'
    needs_item_counts = True

    def value(self, R, P, Tl, G, S, N, T):
        return np.float64(Tl) / np.float64(T)                                # metrics.py:764, 777


class ShannonEntropy(_ExposureMetric):
    name = 'shannonentropy'

    def value(self, R, P, Tl, G, S, N, T):
        # metrics.py:634-640: sum -p ln p with p = c / T is ln T - S / T; the reference divides by the items recommended
        return max(np.log(np.float64(T)) - S / np.float64(T), np.float64(0.0)) / np.float64(R)


class GiniIndex(_ExposureMetric):
    name = 'giniindex'

    def value(self, R, P, Tl, G, S, N, T):
        return np.float64(G) / np.float64(T) / np.float64(N)                 # metrics.py:694-695


def tail_items(counts, tail_ratio):
    """The reference's long-tail set (TailPercentage.get_tail, metrics.py:743-749) as a uint8 mask [N]: the counter holds the
    items i >= 1 with counts[i] > 0; tail_ratio > 1 keeps those with counts <= tail_ratio, otherwise the first
    max(int(len(counter) * tail_ratio), 1) of the counter ordered by (count, id).  None or <= 0 reads as 0.1 (metrics.py:724)."""
    import torch
    counts = torch.as_tensor(counts).long()
    if tail_ratio is None or tail_ratio <= 0:
        tail_ratio = 0.1
    seen = counts > 0
    seen[0] = False
    mask = torch.zeros_like(counts, dtype=torch.uint8)
    if tail_ratio > 1:
        mask[seen & (counts <= tail_ratio)] = 1
        return mask
    ids = torch.nonzero(seen).flatten()                                      # ascending ids: a stable sort by count orders (count, id)
    if ids.numel():
        order = torch.sort(counts[ids], stable=True)[1]
        mask[ids[order[:max(int(ids.numel() * tail_ratio), 1)]]] = 1
    return mask


EXPOSURE_METRICS = {'itemcoverage': ItemCoverage, 'averagepopularity': AveragePopularity, 'shannonentropy': ShannonEntropy,
                    'giniindex': GiniIndex, 'tailpercentage': TailPercentage}
metrics_dict = {'recall': Recall, 'ndcg': NDCG, 'hit': Hit, 'mrr': MRR, 'map': MAP, 'precision': Precision, 'entropy': Entropy,
                **EXPOSURE_METRICS}
