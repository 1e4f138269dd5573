"""Multi-head decode collector (reference `code/REC/evaluator/collector.py:58-395`), fused.

`eval_batch_collect` accepts either the reference's dense `scores [B,H,N]` tensor (on the GPU) or the `FusedTopK`
that `HSTU.predict_topk` returns.  The cross-head merge + first-occurrence dedup (reference collector.py:249-275:
a [B,N] bool table and an H*K-step Python loop) and the hit matrix (collector.py:300-316) run in gfx950 kernels;
everything stays on the device until the per-pred_len `[B, K+1]` result is appended.

`stream_metrics: True` (default off) stores nothing per batch: one `eval_metric_sums` launch adds the batch's users onto a small
fp64 accumulator on the device (the summed metric curves at `topk`, over all users and per category / outlier group), and
`get_data_struct` hands the sums out as `'rec.metric_sums'` / `'rec.entropy_sums'` after one device->host copy.

A catalog-exposure metric in `shared_metrics` (ItemCoverage, AveragePopularity, ShannonEntropy, GiniIndex, TailPercentage), with
`stream_metrics` on or off, adds every batch's merged lists to an integer item histogram on the device (`exposure_accumulate`);
`get_data_struct(-1)` reduces it to a few integers per cut-off (`exposure_finalize`) and hands them out as
`'rec.exposure_sums'`.  The lists are the merged ones the accuracy metrics see, not the reference's per-head `rec.items`.
"""
import copy

import numpy as np
import torch

from .metrics import COLUMNS, EXPOSURE_METRICS, tail_items


class DataStruct(object):
    def __init__(self):
        self._tensor_lists = {}
        self._data_dict = {}

    def __getitem__(self, name):
        return self._data_dict[name]

    def __setitem__(self, name, value):
        self._data_dict[name] = value

    def __delitem__(self, name):
        self._data_dict.pop(name)

    def __contains__(self, key):
        return key in self._data_dict

    def get(self, name):
        if name not in self._data_dict:
            raise IndexError("Can not load the data without registration !")
        return self[name]

    def set(self, name, value):
        self._data_dict[name] = value

    def update_tensor(self, name, value):
        # per-batch results stay where they were produced (the device); the reference's `.cpu().clone()` per batch
        # (collector.py:48-54) would serialise the host against the GPU once per batch.
        self._tensor_lists.setdefault(name, []).append(value.detach())

    def finalize_tensors(self):
        # one concatenation and one device->host copy per key for the whole evaluation
        for name, lst in self._tensor_lists.items():
            if lst:
                self._data_dict[name] = torch.cat(lst, dim=0).cpu()
        self._tensor_lists.clear()


class Collector(object):
    def __init__(self, config):
        self.config = config
        self.metrics_pred_len_list = config['metrics_pred_len_list']
        self.eval_pred_len = config['eval_pred_len']
        self.data_struct = {p: DataStruct() for p in self.metrics_pred_len_list}
        self.data_struct[-1] = DataStruct()
        self.topk = config['topk']
        hi = config['head_interaction']
        if hi in ('multiplicative', 'hierarchical'):
            self.medusa_num_heads = config['num_segment_head'] * config['num_prior_head']
        elif hi == 'additive':
            self.medusa_num_heads = config['num_segment_head'] + config['num_prior_head']
        else:
            raise ValueError(f'Unknown head_interaction: {hi}')
        self.split_mode = config['split_mode']
        self.all_tags = None
        self.stream_metrics = bool(config.get('stream_metrics', False))
        if self.stream_metrics:
            self._stream_init(config)
        self.exposure = [m.lower() for m in (config.get('shared_metrics') or []) if m.lower() in EXPOSURE_METRICS]
        if self.exposure:
            self._exposure_init(config)

    def set_all_tags(self, item_tags):
        self.all_tags = item_tags
        if self.stream_metrics:
            self._tag_bits = self._pack_tag_bits(item_tags)

    def reset_all_tags(self):
        self.all_tags = None
        if self.stream_metrics:
            self._tag_bits = None

    # ---- stream_metrics: running sums instead of stored per-batch tensors -----------------------------------------------------
    def _stream_init(self, config):
        """Group layout of the accumulator: bit 0 every user, bits 1..n_cats the target categories, the last bit the outlier
        users (each only when the configuration evaluates it)."""
        n_cats = config['eval_num_cats'] or 0
        self._n_cats = n_cats if (n_cats > 1 and config.get('eval_by_cat', True)) else 0
        self._outlier = config['outlier_user_metrics'] is not None
        self.n_groups = 1 + self._n_cats + int(self._outlier)
        from mhr_amd.ops import METRIC_LIMITS as lim_of                        # the limits of mhr_eval_metric_sums (mhr.h)
        for what, n, lim in (('groups (1 + eval_num_cats + outlier)', self.n_groups, lim_of['n_groups']),
                             ('len(metrics_pred_len_list)', len(self.metrics_pred_len_list), lim_of['n_pred']),
                             ('len(topk)', len(self.topk), lim_of['n_topk']), ('max(topk)', max(self.topk), lim_of['K'])):
            if not 1 <= n <= lim:
                raise ValueError(f"stream_metrics: {what} = {n} is outside the kernel's limit [1, {lim}]")
        if self._outlier and self.eval_pred_len - 1 not in self.metrics_pred_len_list:
            raise ValueError("stream_metrics: outlier_user_metrics needs eval_pred_len - 1 in metrics_pred_len_list")
        self._tag_bits = None
        self._acc = None                 # device f64 words: sums [P, G, 6, T] | entropy [T] | counts [P, G] (int64 bits)
        self._host = None                # the one device->host copy of an evaluation, handed out slice by slice
        self._dirty = False
        self._seen = dict(tags=False, cats=False, outlier=False)

    def _pack_tag_bits(self, item_tags):
        """[N, C'] tag table -> [N] words, bit c = the item carries tag c (int32 storage of the uint32 bit pattern)."""
        C = item_tags.shape[1]
        from mhr_amd.ops import METRIC_LIMITS
        if C > METRIC_LIMITS['n_tags']:
            raise ValueError(f"stream_metrics: {C} item tags exceed the kernel's limit of {METRIC_LIMITS['n_tags']}")
        w = (item_tags != 0).long() << torch.arange(C, device=item_tags.device)
        return self._low32(w.sum(dim=1)), C

    @staticmethod
    def _low32(words):
        """int64 words in [0, 2^32) -> int32 storage of the same 32 bits."""
        return torch.where(words >= 2 ** 31, words - 2 ** 32, words).int().contiguous()

    def _stream_consts(self, dev):
        """Per-device constants of the group words: the pred_len columns, the weight 2^(1 + c) of category c, and the outlier
        weight 2^(G - 1) in the column of eval_pred_len - 1 (zero elsewhere)."""
        c = self.__dict__.setdefault('_consts', {}).get(dev)
        if c is None:
            P, G = len(self.metrics_pred_len_list), self.n_groups
            ow = torch.zeros(1, P, dtype=torch.int64)
            if self._outlier:
                ow[0, self.metrics_pred_len_list.index(self.eval_pred_len - 1)] = 2 ** (G - 1)
            c = self._consts[dev] = dict(pred=torch.tensor(list(self.metrics_pred_len_list), device=dev),
                                         cat_weight=(2 ** torch.arange(1, 1 + self._n_cats)).to(dev), outlier_weight=ow.to(dev))
        return c

    def _acc_views(self, buf):
        P, G, T = len(self.metrics_pred_len_list), self.n_groups, len(self.topk)
        n_sum = P * G * len(COLUMNS) * T
        return buf[:n_sum].view(P, G, len(COLUMNS), T), buf[n_sum:n_sum + T], buf[n_sum + T:].view(torch.int64).view(P, G)

    def _stream_collect(self, topk_idx, positive_i, pos_len_full, tag_category, outlier_users):
        from mhr_amd import ops
        dev, B = topk_idx.device, topk_idx.shape[0]
        P, G, T = len(self.metrics_pred_len_list), self.n_groups, len(self.topk)
        if positive_i.shape[1] <= max(self.metrics_pred_len_list):
            raise ValueError(f"stream_metrics: positives hold {positive_i.shape[1]} targets, metrics_pred_len_list needs "
                             f"{max(self.metrics_pred_len_list) + 1}")
        if self._acc is None or self._acc.device != dev:
            self._acc = torch.zeros(P * G * len(COLUMNS) * T + T + P * G, dtype=torch.float64, device=dev)
        # group words [B, P]: a handful of small launches whatever the number of pred_lens (int64 arithmetic, then the low 32 bits)
        consts = self._stream_consts(dev)
        if tag_category is not None and self._n_cats:
            seen = tag_category.to(dev)[:, :, :self._n_cats].ne(0).cumsum(dim=1).ne(0)        # any over targets [0 : e + 1]
            bits = (seen.index_select(1, consts['pred']) * consts['cat_weight']).sum(dim=2) + 1
            self._seen['cats'] = True
        else:
            bits = torch.ones(B, P, dtype=torch.int64, device=dev)
        if outlier_users is not None and self._outlier:
            bits = bits + outlier_users.to(dev).ne(0).long()[:, None] * consts['outlier_weight']
            self._seen['outlier'] = True
        bits = self._low32(bits)
        sums, entropy, counts = self._acc_views(self._acc)
        tag_bits, n_tags = (None, 0)
        if self.all_tags is not None:
            tag_bits, n_tags = self._tag_bits
            tag_bits = tag_bits.to(dev)
            self._tag_bits = (tag_bits, n_tags)
            self._seen['tags'] = True
        ops.eval_metric_sums(topk_idx.contiguous(), positive_i, pos_len_full, list(self.metrics_pred_len_list), list(self.topk),
                             bits, G, sums, counts, item_tag_bits=tag_bits, n_tags=n_tags,
                             entropy=entropy if tag_bits is not None else None)
        self._dirty = True

    def _stream_data_struct(self, pred_idx):
        """The sums of one pred_len (or the shared entropy sums at -1) as host numpy; what is handed out is zeroed, as the
        stored path deletes the keys it hands out."""
        if self._dirty:
            self._host = self._acc.cpu()                                   # the one device->host copy of the evaluation
            self._acc.zero_()
            self._dirty = False
        out = DataStruct()
        if self._host is None:
            return out
        sums, entropy, counts = self._acc_views(self._host)
        if pred_idx == -1:
            if self._seen['tags']:
                out.set('rec.entropy_sums', entropy.numpy().copy())
                entropy.zero_()
                self._seen['tags'] = False
            return out
        i = self.metrics_pred_len_list.index(pred_idx)
        out.set('rec.metric_sums', dict(sums=sums[i].numpy().copy(), counts=counts[i].numpy().copy(), n_cats=self._n_cats,
                                        cats=self._seen['cats'],
                                        outlier=self._seen['outlier'] and pred_idx == self.eval_pred_len - 1))
        sums[i].zero_()
        counts[i].zero_()
        return out

    # ---- catalog exposure: an integer item histogram instead of the reference's [users, max(topk)] item matrix ---------------
    def _exposure_init(self, config):
        from mhr_amd.ops import EXPOSURE_LIMITS
        self._ex_cuts = sorted(set(int(k) for k in self.topk))
        if len(self._ex_cuts) > EXPOSURE_LIMITS['n_cuts']:
            raise ValueError(f"exposure metrics: {len(self._ex_cuts)} distinct cut-offs exceed the kernel's limit of "
                             f"{EXPOSURE_LIMITS['n_cuts']}")
        self._ex_needs_counts = any(EXPOSURE_METRICS[m].needs_item_counts for m in self.exposure)
        self._ex_tail_ratio = config.get('tail_ratio')
        self._ex_item_num = config.get('item_num')
        self._ex_pop = self._ex_tail = None          # [N] int64 training counts / [N] uint8 long-tail mask (set_item_counts)
        self._ex_hist = None                         # device int32 [n_cuts, N]: occurrences per rank band and item
        self._ex_out = None                          # device int64 words: ints [n_cuts, 4] | S [n_cuts] (f64 bits) | bad (int32)
        self._ex_users = 0

    def set_item_counts(self, counts):
        """counts [N] int64: training interactions per item (phi; `SeqStore.item_train_counts`).  AveragePopularity and
        TailPercentage need it; the long-tail set (config `tail_ratio`) is built here, once."""
        if not self.exposure:
            return
        counts = torch.as_tensor(counts)
        if counts.dim() != 1 or counts.dtype != torch.int64:
            raise ValueError("set_item_counts: expected an int64 [item_num] tensor")
        if bool((counts < 0).any()):
            raise ValueError("set_item_counts: negative interaction counts")
        if self._ex_hist is not None and counts.numel() != self._ex_hist.shape[1]:
            raise ValueError(f"set_item_counts: {counts.numel()} items, the running histogram holds {self._ex_hist.shape[1]}")
        self._ex_pop, self._ex_tail = counts.contiguous(), tail_items(counts, self._ex_tail_ratio)

    def _exposure_check_counts(self):
        if self._ex_needs_counts and self._ex_pop is None:
            raise ValueError("AveragePopularity / TailPercentage need the items' training interaction counts: call "
                             "Collector.set_item_counts(SeqStore.item_train_counts()) before the evaluation")

    def _exposure_views(self, buf):
        T = len(self._ex_cuts)
        return buf[:4 * T].view(T, 4), buf[4 * T:5 * T].view(torch.float64), buf[5 * T:].view(torch.int32)[:1]

    def _exposure_collect(self, topk_idx):
        from mhr_amd import ops
        dev = topk_idx.device
        if self._ex_hist is None or self._ex_hist.device != dev:
            if self._ex_users:
                raise RuntimeError("exposure metrics: the evaluation changed its device between batches")
            N = self._ex_pop.numel() if self._ex_pop is not None else (
                self.all_tags.shape[0] if self.all_tags is not None else self._ex_item_num)
            if N is None:
                raise ValueError("exposure metrics: the catalog size is unknown (set_item_counts, set_all_tags or config['item_num'])")
            self._ex_hist = torch.zeros(len(self._ex_cuts), int(N), dtype=torch.int32, device=dev)
            self._ex_out = torch.zeros(5 * len(self._ex_cuts) + 1, dtype=torch.int64, device=dev)
        ops.exposure_accumulate(topk_idx.contiguous(), self._ex_cuts, self._ex_hist.shape[1], self._ex_hist,
                                self._exposure_views(self._ex_out)[2])
        self._ex_users += topk_idx.shape[0]

    def _exposure_hand_out(self, struct):
        """All-reduce the histogram and the user count, finalize, one small device->host copy, zero - as the streamed sums are
        handed out and zeroed."""
        if self._ex_hist is None:
            return
        from mhr_amd import distributed as D, ops
        T, N = self._ex_hist.shape
        ints, S, bad = self._exposure_views(self._ex_out)
        users = D.allreduce_exposure(self._ex_hist, self._ex_users, bad)
        if users == 0:
            return
        lim = ops.EXPOSURE_LIMITS['users']
        if users > lim or 2 * N * users * self._ex_cuts[-1] >= 2 ** 63:
            raise ValueError(f"exposure metrics: {users} users x {N} items x k = {self._ex_cuts[-1]} exceed the kernel's limits "
                             f"(users <= {lim}, 2 * items * users * k < 2^63)")
        dev = self._ex_hist.device
        pop = tail = None
        if self._ex_pop is not None:
            if self._ex_pop.numel() != N:
                raise ValueError(f"set_item_counts gave {self._ex_pop.numel()} items, the histogram holds {N}")
            if users * int(self._ex_pop.sum()) >= 2 ** 63:
                raise ValueError("exposure metrics: users x training interactions does not fit 63 bits")
            self._ex_pop, self._ex_tail = self._ex_pop.to(dev), self._ex_tail.to(dev)
            pop, tail = self._ex_pop, self._ex_tail
        ops.exposure_finalize(self._ex_hist, T, N, users, self._ex_cuts[-1], ints, S, bad, item_pop=pop, item_tail=tail)
        host = self._ex_out.cpu()                                          # the one device->host copy
        self._ex_hist.zero_()
        self._ex_out.zero_()
        self._ex_users = 0
        ints, S, bad = self._exposure_views(host)
        if int(bad[0]):
            raise RuntimeError(f"exposure metrics: {int(bad[0])} recommended ids outside [0, {N}) or items counted more often "
                               "than there are users (a list holding an item twice)")
        struct.set('rec.exposure_sums', dict(ints=ints.numpy().copy(), S=S.numpy().copy(), N=N, U=users, cuts=list(self._ex_cuts)))

    # ------------------------------------------------------------------------------------------
    def _decode(self, scores, top_k, detail):
        """-> merged item ids [B, top_k] int64 on the device."""
        from mhr_amd import ops
        fused = not torch.is_tensor(scores)         # (every torch.Tensor has an `indices` attribute: test the type, not the name)
        if fused:
            vals, idx = scores.values, scores.indices
            if vals.shape[-1] < top_k:
                raise ValueError(f"FusedTopK holds k={vals.shape[-1]} < max(topk)={top_k}")
            vals, idx = vals[..., :top_k].contiguous(), idx[..., :top_k].contiguous()
            B, H = vals.shape[:2]
        else:
            if not scores.is_cuda:
                raise RuntimeError("Collector: scores must live on the GPU (no CPU decode path)")
            scores = scores.float()
            B, H = scores.shape[:2]
            if H > 1 and self.split_mode == 'average':
                finite = torch.isfinite(scores)
                avg = torch.sum(scores.masked_fill(~finite, 0), dim=1) / (torch.sum(finite, dim=1) + 1e-8)
                return torch.topk(avg, top_k, dim=-1)[1]
            vals, idx = torch.topk(scores, top_k, dim=-1)
        if H == 1:
            if detail is not None:
                detail['values'], detail['idx'] = vals[:, 0], idx[:, 0]
            return idx[:, 0].contiguous()
        if self.split_mode != 'combine':
            if fused and self.split_mode == 'average':
                # the models' fused average decode hands ONE list per user ([B,1,k]: MultiHeadDecoding._decode_topk); per-head
                # lists cannot be averaged after the fact (an item's mean needs its score in every head)
                raise ValueError(f"split_mode=average: got per-head top-k lists [B,{H},k]; the mean over heads needs the fused "
                                 "average decode (a FusedTopK [B,1,k]) or dense scores [B,H,N]")
            raise ValueError(f'Unknown split_mode: {self.split_mode}')
        out_idx, out_val, out_src, status = ops.multihead_merge_dedup(vals.contiguous(), idx.contiguous(), B, H, top_k)
        if detail is not None:
            detail.update(values=out_val, head_source=out_src, idx=out_idx, values_by_head=vals, idx_by_head=idx, unique=status)
        return out_idx

    def eval_batch_collect(self, scores_tensor, positive_u, positive_i, tag_category=None, outlier_users=None,
                           log_detailed_results=False):
        from mhr_amd import ops
        stored = not self.stream_metrics
        if self.exposure:
            self._exposure_check_counts()
        if stored and tag_category is not None:
            for p in self.metrics_pred_len_list:
                self.data_struct[p].update_tensor('rec.tgt_tags', torch.any(tag_category[:, :p + 1].bool(), dim=1))
        if stored and outlier_users is not None:
            self.data_struct[self.eval_pred_len - 1].update_tensor('rec.outlier_users', outlier_users)
        top_k = max(self.topk)
        detail = {} if log_detailed_results else None
        topk_idx = self._decode(scores_tensor, top_k, detail)
        dev = topk_idx.device
        positive_i = positive_i.to(dev).contiguous()
        B = topk_idx.shape[0]
        if self.exposure:
            self._exposure_collect(topk_idx)
        if stored and self.all_tags is not None:
            self.data_struct[-1].update_tensor('rec.rec_tags', self.all_tags.to(dev)[topk_idx])
        # distinct positives among the ascending-sorted targets (reference collector.py:301-304)
        srt, _ = positive_i.sort(dim=1)
        first = torch.ones_like(srt, dtype=torch.bool)
        first[:, 1:] = srt[:, 1:] != srt[:, :-1]
        pos_len_full = first.cumsum(dim=1).int()
        if stored:
            for p in self.metrics_pred_len_list:
                hit = ops.hit_matrix(topk_idx, positive_i, p + 1)                       # cumulative over [0 : p+1]
                self.data_struct[p].update_tensor('rec.topk', torch.cat((hit.int(), pos_len_full[:, p:p + 1]), dim=1))
        else:
            self._stream_collect(topk_idx, positive_i, pos_len_full, tag_category, outlier_users)
        if log_detailed_results:
            out = {}
            for k_, v in detail.items():
                out[k_] = v.detach().cpu().numpy() if k_.startswith('values') or k_ in ('head_source', 'unique') else v.detach().cpu().tolist()
            return out
        return {}

    def get_data_struct(self, pred_idx=0):
        returned = self._collected_struct(pred_idx)
        if self.exposure and pred_idx == -1:
            self._exposure_hand_out(returned)
        return returned

    def _collected_struct(self, pred_idx):
        if self.stream_metrics:
            return self._stream_data_struct(pred_idx)
        self.data_struct[pred_idx].finalize_tensors()
        returned = copy.deepcopy(self.data_struct[pred_idx])
        for key in ('rec.rec_tags', 'rec.tgt_tags', 'rec.outlier_users', 'rec.topk'):
            if key in self.data_struct[pred_idx]:
                del self.data_struct[pred_idx][key]
        return returned
