"""Cost of the exposure metrics at cfg1's evaluation shapes: HIP events around warmed launches of `exposure_accumulate` for one
batch (B = 256 users, K = 200 ranks, N = 453 938 items, four cut-offs) and of `exposure_finalize` once per evaluation (the
histogram of `--batches` batches).  Two kinds of lists: uniform over the catalog (no two atomics meet) and popularity-skewed
(the synthetic data's own Zipf draw, every list also holding the same `--shared` head items - the contention a real decode
produces on popular items).  Compare against the eval step of `python bench.py --mode eval`.  Prints one
JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code"))
import mhr_amd  # noqa: E402,F401
from mhr_amd import ops  # noqa: E402


def timed(fn, reps, before=None):
    """Mean microseconds of fn over reps launches between two events, after a warm-up of a tenth of them."""
    for _ in range(max(reps // 10, 3)):
        fn()
    if before is not None:
        before()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def make_lists(kind, n, B, K, N, shared, gen):
    """n batches of [B, K] distinct ids per row."""
    if kind == "uniform":
        w = torch.ones(N, device="cuda")
    else:
        w = 1.0 / torch.arange(1, N + 1, device="cuda", dtype=torch.float32) ** 0.8
    w[0] = 0
    out = []
    for _ in range(n):
        rows = torch.multinomial(w.expand(B, N), K, replacement=False, generator=gen)
        if kind != "uniform" and shared:
            rows[:, :shared] = torch.arange(1, shared + 1, device="cuda")       # the same head items in every list
            rest = rows[:, shared:]
            rest[rest <= shared] += N // 2                                      # keep the rows free of repeats (ids stay < N)
        out.append(rows.contiguous())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--K", type=int, default=200)
    ap.add_argument("--N", type=int, default=453938)
    ap.add_argument("--cuts", type=int, nargs="+", default=[5, 10, 50, 200])
    ap.add_argument("--batches", type=int, default=64, help="batches of one evaluation (the finalize's histogram)")
    ap.add_argument("--shared", type=int, default=20, help="head items every skewed list holds")
    ap.add_argument("--reps", type=int, default=20000)
    ap.add_argument("--eval-step-ms", type=float, default=None, help="the eval step of bench.py --mode eval, for the share")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exposure_micro: no GPU (a measurement does not fall back)")
    gen = torch.Generator(device="cuda").manual_seed(11)
    T = len(a.cuts)
    res = dict(B=a.B, K=a.K, N=a.N, cuts=a.cuts, batches=a.batches, reps=a.reps, device=torch.cuda.get_device_name(0))
    pop = torch.randint(0, 1000, (a.N,), device="cuda", generator=gen)
    tail = (pop < 100).to(torch.uint8)
    for kind in ("uniform", "skewed"):
        lists = make_lists(kind, a.batches, a.B, a.K, a.N, a.shared, gen)
        hist = torch.zeros(T, a.N, dtype=torch.int32, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        n = [0]

        def acc():
            ops.exposure_accumulate(lists[n[0] % len(lists)], a.cuts, a.N, hist, bad)
            n[0] += 1
        res[f"accumulate_us_{kind}"] = round(timed(acc, a.reps, before=hist.zero_), 2)
        # the histogram of exactly one evaluation: every batch once
        hist.zero_()
        for rows in lists:
            ops.exposure_accumulate(rows, a.cuts, a.N, hist, bad)
        users = a.B * len(lists)
        out_int = torch.zeros(T, 4, dtype=torch.int64, device="cuda")
        out_f64 = torch.zeros(T, dtype=torch.float64, device="cuda")
        res[f"finalize_us_{kind}"] = round(timed(lambda: ops.exposure_finalize(hist, T, a.N, users, a.cuts[-1], out_int, out_f64, bad,
                                                                                item_pop=pop, item_tail=tail), max(a.reps // 10, 20)), 2)
        res[f"recommended_{kind}"] = out_int[:, 0].tolist()
        res[f"max_count_{kind}"] = int(hist.sum(dim=0).max())
        assert int(bad.item()) == 0 and int(out_int[-1, 0]) == int((hist.sum(dim=0) > 0).sum())
    if a.eval_step_ms:
        res["eval_step_ms"] = a.eval_step_ms
        res["accumulate_share_skewed"] = round(res["accumulate_us_skewed"] / (a.eval_step_ms * 1e3), 5)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
