"""Times the split_mode=average decode at the cfg1 evaluation shape (B = 256, H = 4, N = 453 938, D = 256, k = 200, four
single-tag categories, histories as synth draws them) on one MI355X, three variants ALTERNATING batch by batch in one process:

  (a) the fused average decode (MultiHeadDecoding._decode_topk under split_mode=average -> ops.catalog_topk_mean) + the collector
  (b) the dense route: predict()'s scores [B, H, N] + pad / history suppression + the collector's dense average branch
  (c) the fused combine decode of the same batch (ops.catalog_topk_exact + the cross-head merge in the collector)

All three start from the same L2-normalised user heads of a cfg1 model (the encoder is not timed), fresh and after a few
training steps; device events around each batch, median and 10th / 90th percentile over the timed batches.  Also printed: the
share of users the fused average decode re-ranked densely, and per-kernel events of one extra pass of (a).

    python tools/decode_average_bench.py [--batches 50] [--warmup 5] [--train-steps 40]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code"))
import mhr_amd.synth as synth  # noqa: E402
from mhr_amd import ops  # noqa: E402
from REC.config.configurator import Config, apply_run_fixups  # noqa: E402
from REC.evaluator.collector import Collector  # noqa: E402
from REC.trainer import Trainer  # noqa: E402
from REC.utils import get_model  # noqa: E402


def single_tag(data, seed=7):
    """Every item in exactly one of the C categories (item 0, the pad id, in none)."""
    g = torch.Generator(device=data.device).manual_seed(seed)
    cat = torch.randint(0, data.C, (data.item_num,), generator=g, device=data.device)
    tags = torch.nn.functional.one_hot(cat, data.C).bool()
    tags[0] = False
    data.item_tags = tags
    data.category_counts = {f"cat{c}": int(tags[:, c].sum()) for c in range(data.C)}
    data.cat_items = [torch.nonzero(tags[:, c]).flatten() for c in range(data.C)]


def measure(model, cfg, data, n_batches, warmup, B, k, tag):
    model.eval()
    N = data.item_num
    feat = model.compute_item_all()
    tags_cn = data.item_tags.long().t().contiguous()
    col = Collector(dict(cfg.final_config_dict, split_mode="average"))
    col_c = Collector(dict(cfg.final_config_dict, split_mode="combine"))
    batches = [data.eval_batch(B) for _ in range(4)]
    heads = [model._user_heads(eb[1]).float().contiguous() for eb in batches]

    def fused(i, mode, stats=None):
        eb = batches[i % 4]
        model.split_mode = mode
        out = model._decode_topk(None, feat, tags_cn, eb[6], eb[3], k, True, stats, N, heads_n=heads[i % 4])
        return (col if mode == "average" else col_c)._decode(out, k, None)

    def dense(i):
        eb = batches[i % 4]
        scores = model._dense_scores(None, feat, tags_cn, eb[6], False, heads_n=heads[i % 4])[0]
        scores[:, :, 0] = float("-inf")
        scores[eb[3][0], :, eb[3][1]] = float("-inf")
        return col._decode(scores, k, None)

    variants = {"a_fused_average": lambda i: fused(i, "average"), "b_dense_average": dense, "c_fused_combine": lambda i: fused(i, "combine")}
    # the fused average list is the dense route's wherever the means are untied
    ia, ib = variants["a_fused_average"](0), variants["b_dense_average"](0)
    print(f"[{tag}] fused average == dense average on {float((ia == ib).float().mean()) * 100:.2f} % of the {B} x {k} positions")
    times = {name: [] for name in variants}
    for i in range(warmup + n_batches):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(i)
            e1.record()
            if i >= warmup:
                times[name].append((e0, e1))
    torch.cuda.synchronize()
    res = {}
    for name, evs in times.items():
        ms = np.array([a.elapsed_time(b) for a, b in evs])
        res[name] = float(np.median(ms))
        print(f"[{tag}] {name}: median {np.median(ms):.3f} ms  (p10 {np.percentile(ms, 10):.3f}, p90 {np.percentile(ms, 90):.3f}, n = {len(ms)})")
    print(f"[{tag}] a / b = {res['a_fused_average'] / res['b_dense_average']:.3f},  a / c = {res['a_fused_average'] / res['c_fused_combine']:.3f}")
    n_dense = 0
    for i in range(4):
        st = {}
        fused(i, "average", st)
        n_dense += len(st["dense_users"])
    print(f"[{tag}] users re-ranked densely: {n_dense} of {4 * B} ({100.0 * n_dense / (4 * B):.2f} %); patterns {st['patterns']}, "
          f"uncertified rows {st['uncertified_rows']}, margin set {st['margin_mean']:.1f}")
    names = ["mhr_head_mean_queries", "mhr_catalog_score_emit_sliced", "mhr_topk_select_sliced", "mhr_rescore_mean_f32", "mhr_topk_select",
             "mhr_catalog_mean_rows_dense"]
    ops.PROFILE = {n: [] for n in names}
    for i in range(8):
        fused(i, "average")
    torch.cuda.synchronize()
    for n, v in ops.profile_summary().items():
        print(f"[{tag}]   {n}: {v[0] / 8:.1f} launches / batch, mean {v[1] * 1e3:.1f} us, {v[2] / 8:.3f} ms / batch")
    ops.PROFILE = None
    model.split_mode = "average"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--train-steps", type=int, default=40)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("-k", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    spec = synth.CONFIGS["cfg1"]
    cfg = apply_run_fixups(Config(config_dict=dict(spec["cfg"], device=dev, total_iters=max(a.train_steps, 1), eval_interval=0,
                                                   checkpoint_dir=None, save_model_note="x", split_mode="average")))
    data = synth.SyntheticData(cfg, spec["item_num"], dev)
    single_tag(data)
    cfg["int_to_category"] = data.int_to_category
    torch.manual_seed(1)
    model = get_model("HSTU")(cfg, data).to(dev)
    measure(model, cfg, data, a.batches, a.warmup, a.batch_size, a.k, "fresh")
    if a.train_steps > 0:
        tr = Trainer(cfg)
        tr.setup_model(model)
        model.train()
        tb = [data.train_batch(cfg["train_batch_size"]) for _ in range(4)]
        losses = [float(tr.train_step_fn(tb[i % 4], graph=False)["loss"]) for i in range(a.train_steps)]
        print(f"[train] {a.train_steps} steps, loss {losses[0]:.3f} -> {losses[-1]:.3f}")
        measure(model, cfg, data, a.batches, a.warmup, a.batch_size, a.k, "trained")


if __name__ == "__main__":
    main()
