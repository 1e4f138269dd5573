"""Micro-driver: the grouped flat Adam (ops.adam_flat_groups, 1 / 2 / 16 groups) next to the ungrouped one (ops.adam_flat) at the
cfg1 flat size, 2 945 608 padded fp32 elements, bf16 shadow written.  Per call: the median over 21 replays of a graph of 20
launches; the comparison is repeated three times, the variants alternating inside a repeat.
python tools/adam_groups_micro.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mhr_amd  # noqa: E402,F401
from mhr_amd import ops  # noqa: E402

N = 2945608
SEG = 65536                      # segment length: 45 segments, the groups taken round robin (an encoder's layers, roughly)
HIST = 64


def bench_median(fn, n=20, reps=21):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    ts = []
    with torch.cuda.stream(st):
        fn()
        g_ = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_, stream=st):
            for _ in range(n):
                fn()
        g_.replay()
        torch.cuda.synchronize()
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g_.replay()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / n * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    w = torch.randn(N, device=dev, generator=gen)
    g = torch.randn(N, device=dev, generator=gen) * 0.01
    m, v = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
    w16 = torch.zeros(N, dtype=torch.bfloat16, device=dev)
    step_dev = torch.full((1,), 5, dtype=torch.int64, device=dev)
    hist = torch.zeros(HIST, 4, device=dev)
    variants = {}
    for n_groups in (1, 2, 16):
        seg_off = list(range(0, N, SEG)) + [N]
        seg_group = [k % n_groups for k in range(len(seg_off) - 1)]
        if n_groups == 1:
            seg_off, seg_group = [0, N], [0]
        tables = ops.adam_group_tables(seg_off, seg_group, n_groups, dev)
        gconst = torch.zeros(HIST, n_groups, 4, device=dev)
        row = ops.adam_group_consts(torch.zeros(n_groups, 4), 5, [1e-3 * (1 + k) for k in range(n_groups)], [0.01] * n_groups)
        gconst[5].copy_(row)
        if n_groups == 1:
            hist[5].copy_(row[0])
        variants[f"groups={n_groups} ({len(seg_group)} segments)"] = (
            lambda t=tables, c=gconst: ops.adam_flat_groups(w, g, m, v, t, c, 1, w_bf16=w16, step_dev=step_dev))
    variants["adam_flat"] = lambda: ops.adam_flat(w, g, m, v, 1, 1e-3, weight_decay=0.01, w_bf16=w16, hist=hist, step_dev=step_dev)
    for rep in range(3):
        line = []
        for name, fn in list(variants.items())[::-1]:
            t = bench_median(fn)
            line.append(f"{name} {t:.2f} us ({N * 30 / t / 1e6:.2f} TB/s)")
        print(f"rep {rep}: " + " | ".join(line), flush=True)


if __name__ == "__main__":
    main()
