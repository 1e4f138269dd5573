#!/usr/bin/env python3
"""Generate tests/golden/metrics_groups.npz from the REFERENCE metric classes: the by-category and outlier breakdowns of
Recall / NDCG and the reference's Hit / MRR / MAP / Precision, which no other fixture pins.

Runs only in the build container (needs the reference tree, like tests/gen_golden.py whose stubs it uses).
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/gen_golden_metrics.py

The fixture holds arrays and values only: the [B, K+1] hit matrices, the target tags per pred_len, the outlier flags and every
value the reference's Evaluator returns (sums and sample counts, as float64).
"""
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG  # noqa: E402

B, K, E, C = 37, 20, 4, 3
TOPK = [1, 5, 10, 20]
PRED = [0, 3]
METRICS = ["Recall", "NDCG", "Hit", "MRR", "MAP", "Precision"]
OUTLIER = "long_history"


def main():
    GG._setup()
    import numpy as np
    import torch
    from REC.evaluator.collector import DataStruct
    from REC.evaluator.evaluator import Evaluator
    cfg = GG.Cfg(metrics_pred_len_list=PRED, eval_pred_len=E, topk=TOPK, metrics=METRICS, shared_metrics=[],
                 eval_num_cats=C, eval_by_cat=True, outlier_user_metrics=OUTLIER,
                 int_to_category={i: f"cat{i}" for i in range(C)}, metric_decimal_place=7)
    g = torch.Generator().manual_seed(4107)
    ev = Evaluator(cfg)
    # per-target tags: category 2 is carried by no first target (empty at pred_len 0) but by later ones
    tag_category = torch.rand(B, E, C, generator=g) < 0.35
    tag_category[:, 0, 2] = False
    tag_category[torch.arange(B), 3, torch.randint(0, C, (B,), generator=g)] = True
    outlier = torch.rand(B, generator=g) < 0.3
    d = {"cfg/topk": np.asarray(TOPK), "cfg/pred_len_list": np.asarray(PRED), "cfg/K": np.asarray(K), "cfg/E": np.asarray(E),
         "cfg/C": np.asarray(C), "cfg/outlier_name": np.asarray(OUTLIER), "cfg/metrics": np.asarray(METRICS),
         "in/outlier_users": outlier.numpy()}
    for p in PRED:
        hits = torch.rand(B, K, generator=g) < (0.04 + 0.03 * p)
        hits[::7] = False                                              # users without a hit
        hits[1, 0] = True
        pos_len = torch.randint(1, p + 2, (B, 1), generator=g)
        pos_len = torch.maximum(pos_len, hits.sum(1, keepdim=True).clamp(max=p + 1))
        hits = hits & (hits.cumsum(1) <= pos_len)                      # never more hits than distinct positives
        rec = torch.cat((hits.int(), pos_len.int()), dim=1)
        tgt = torch.any(tag_category[:, :p + 1], dim=1)
        st = DataStruct()
        st.set("rec.topk", rec)
        st.set("rec.tgt_tags", tgt)
        if p == E - 1:
            st.set("rec.outlier_users", outlier)
        d[f"in/topk_{p}"] = rec.numpy()
        d[f"in/tgt_tags_{p}"] = tgt.numpy()
        order = []
        for k, v in ev.evaluate(st, pred_len=p).items():
            order.append(k)
            if isinstance(v, tuple):
                d[f"out/m{p}/{k}"] = np.asarray([v[0], v[1]], dtype=np.float64)
            else:
                d[f"out/m{p}/{k}"] = np.asarray(v, dtype=np.float64)
        d[f"out/order_{p}"] = np.asarray(order)
    assert not d["in/tgt_tags_0"][:, 2].any() and d["out/m0/cat2-recall@5"][1] == 0
    np.savez_compressed(os.path.join(GG.OUT, "metrics_groups.npz"), **d)
    print("metrics_groups:", len(d), "keys")


if __name__ == "__main__":
    main()
