"""`Trainer.fit` over the product's own loader (REC/data/batcher.py:SeqTrainBatcher) with `packed_rows` off and on.

A synthetic interaction store at cfg1's shape (catalog, categories, L = 200, P = 8, B = 128) whose user lengths are drawn
log-uniformly, so that a fair share of the users is shorter than L (their windows are front padded) and the long ones are
cut into full windows.  Runs of N steps of `Trainer.fit`, the key off and on in alternation (one trainer each, kept across the
runs so that the captured step graphs stay alive); prints ms per step of every run, the two medians, the batcher's own time
per batch (iterated alone, synchronised), and the histogram of the capacities the batcher handed out.

    python tools/fit_loader_bench.py [--steps 200] [--runs 6] [--users 3000] [--bucket N] [--json out.json]
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code"))
import mhr_amd  # noqa: E402,F401
import mhr_amd.synth as synth  # noqa: E402
from REC.config.configurator import Config, apply_run_fixups  # noqa: E402
from REC.data import SeqStore, SeqTrainBatcher  # noqa: E402
from REC.trainer import Trainer  # noqa: E402
from REC.utils import get_model  # noqa: E402


def make_store(n_users, item_num, C, L, dev, seed, lo, hi):
    g = np.random.default_rng(seed)
    lens = np.exp(g.uniform(np.log(lo), np.log(hi), n_users)).astype(np.int64)
    tags = g.random((item_num, C)) < 0.375
    tags[np.arange(item_num), g.integers(0, C, item_num)] = True
    tags[0] = False
    user_seq = [[]] + [g.integers(1, item_num, int(n)).tolist() for n in lens]
    train_len = [0] + [int(n) - 16 for n in lens]                # train prefix | 8 validation items | 8 test items
    short = float((lens - 16 <= L).mean())
    return SeqStore(user_seq, train_len, tags, device=dev), tags, short


class Counting:
    """The loader as `fit` sees it, noting the capacities it hands out."""

    def __init__(self, inner, hist):
        self.inner, self.hist = inner, hist

    def __iter__(self):
        for b in self.inner:
            self.hist[b.rows_cap] += 1
            yield b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=6, help="runs per setting (the first of each is reported and left out of the median)")
    ap.add_argument("--users", type=int, default=3000)
    ap.add_argument("--min-len", type=int, default=40)
    ap.add_argument("--max-len", type=int, default=900)
    ap.add_argument("--bucket", type=int, default=None, help="rows_bucket of the batcher (default: rows_capacity's own)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    spec = synth.CONFIGS["cfg1"]
    C = spec["cfg"]["num_prior_head"]
    L, B = spec["cfg"]["MAX_ITEM_LIST_LENGTH"], spec["cfg"]["train_batch_size"]
    store, tags, short = make_store(a.users, spec["item_num"], C, L, dev, 2020, a.min_len, a.max_len)

    class Meta:
        item_num = spec["item_num"]
        category_to_int = {f"cat{c}": c for c in range(C)}
        category_counts = {f"cat{c}": int(tags[:, c].sum()) for c in range(C)}

    sides = {}
    for name, on in (("off", False), ("on", True)):
        cfgd = dict(spec["cfg"], device=dev, total_iters=0, eval_interval=0, checkpoint_dir=None, save_model_note="x",
                    scheduler_args=None)
        if on:
            cfgd["packed_rows"] = True
        cfg = apply_run_fixups(Config(config_dict=cfgd))
        cfg["int_to_category"] = {c: f"cat{c}" for c in range(C)}
        torch.manual_seed(2020)
        model = get_model("HSTU")(cfg, Meta()).to(dev)
        tr = Trainer(cfg)
        tr.setup_model(model)
        hist = collections.Counter()
        loader = Counting(SeqTrainBatcher(cfg, store, seed=2020, rows_bucket=a.bucket), hist)
        sides[name] = dict(tr=tr, loader=loader, hist=hist, ms=[])
    n_loc = sides["on"]["loader"].inner.loc.shape[0]
    valid = float(sides["on"]["loader"].inner.loc[:, 1].clamp(max=L).float().mean()) / L
    print(f"store: {a.users} users, {n_loc} windows ({short:.0%} of the users no longer than L), "
          f"{valid:.1%} of the window rows valid, B = {B}, {len(sides['on']['loader'].inner)} batches per epoch")

    for r in range(a.runs):
        for name in ("off", "on"):
            s = sides[name]
            tr = s["tr"]
            tr.total_iters = tr.train_step + a.steps
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.fit(s["loader"], verbose=False, saved=False)
            torch.cuda.synchronize()
            s["ms"].append((time.perf_counter() - t0) / a.steps * 1e3)
            print(f"run {r} packed_rows {name:3s}: {s['ms'][-1]:.3f} ms/step  "
                  f"(step graphs alive: {len(getattr(tr, '_step_graphs', {}))}, graph failed: {getattr(tr, '_graph_failed', False)})")

    out = {"steps": a.steps, "runs": a.runs, "valid_rows": valid, "windows": n_loc}
    for name in ("off", "on"):
        s = sides[name]
        kept = s["ms"][1:] or s["ms"]
        out[name] = {"ms_per_step": s["ms"], "median": statistics.median(kept), "min": min(kept), "max": max(kept)}
        print(f"packed_rows {name:3s}: median {out[name]['median']:.3f} ms/step over {len(kept)} runs "
              f"(min {min(kept):.3f}, max {max(kept):.3f})")
        # the batcher alone: everything it enqueues for a batch, finished
        it, n = iter(s["loader"].inner), 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in zip(range(50), it):
            n += 1
        torch.cuda.synchronize()
        out[name]["batcher_ms"] = (time.perf_counter() - t0) / max(1, n) * 1e3
        print(f"packed_rows {name:3s}: batcher alone {out[name]['batcher_ms']:.3f} ms/batch")
    caps = {int(k): v for k, v in sorted(sides["on"]["hist"].items())}
    out["capacities"] = caps
    print(f"capacities handed out (of {B * L} window rows): {caps}")
    if len(caps) > 8:
        print(f"note: {len(caps)} live capacities - more than the 8 step graphs the Trainer keeps per packed signature")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
