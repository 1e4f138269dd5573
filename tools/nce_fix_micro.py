"""Micro-driver: the false-negative bit table of the sampled softmax at the cfg1 shape (4 groups x 8192 negatives, D = 256,
4672 bf16 target rows, thres = 0.99, 2 % of the target rows planted in every pool): per-call time of the exhaustive kernel
(mhr_nce_fix_bits) and of the filtered form (mhr_nce_fix_bits_filtered: norm pass + 64-column prefix pass + exact pass), the
number of (row fragment, tile) units the prefix pass could not reject, and the words that hold a hit.

  python tools/nce_fix_micro.py             the table above, plus the degenerate pools (all duplicates; thres = -1)
  python tools/nce_fix_survivors.py ...     the same counter on the benchmark's own batches"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mhr_amd  # noqa: F401
from mhr_amd import lib

def time_call(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    ev[0].record()
    for i in range(n):
        fn(); ev[i + 1].record()
    torch.cuda.synchronize()
    ts = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(n))
    return ts[n // 2]

st = torch.cuda.current_stream().cuda_stream
D, n_rows, n_neg, G = 256, 4672, 8192, 4
rp, n_tiles = (n_rows + 255) // 256 * 256, n_neg // 32
g = torch.Generator(device="cuda").manual_seed(1)
t = torch.randn(n_rows, D, device="cuda", generator=g)
unit = lambda x: torch.nn.functional.normalize(x, dim=-1)
pools = {"random + 2 % planted": unit(torch.randn(G, n_neg, D, device="cuda", generator=g)),
         "all duplicates": unit(t[17])[None, None].expand(G, n_neg, D).contiguous()}
for gi in range(G):
    src = torch.randperm(n_rows, device="cuda", generator=g)[: n_rows // 50]
    pools["random + 2 % planted"][gi, torch.randperm(n_neg, device="cuda", generator=g)[: n_rows // 50]] = unit(t[src])
p = t.bfloat16()
words = torch.empty(G, n_tiles, rp, dtype=torch.int32, device="cuda")
fix_any = torch.zeros(G, rp, dtype=torch.int32, device="cuda")
nb = lib.load().mhr_nce_fix_bits_filtered_workspace_bytes(n_rows, n_neg, G)
ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
for name, pool in pools.items():
    negs = pool.bfloat16()
    for thres in (0.99, -1.0) if name == "all duplicates" else (0.99,):
        args = (p.data_ptr(), lib.BF16, n_rows, negs.data_ptr(), n_neg, D, G, thres, words.data_ptr(), 0, 0, 0, fix_any.data_ptr())
        t_old = time_call(lambda: lib.call("mhr_nce_fix_bits", *args, st))
        t_new = time_call(lambda: lib.call("mhr_nce_fix_bits_filtered", *args, ws.data_ptr(), nb, st))
        units = int(ws[:4].view(torch.int32).item())
        print(f"{name}, thres {thres}: exhaustive {t_old * 1e3:.1f} us, filtered {t_new * 1e3:.1f} us; units kept {units} of "
              f"{G * (rp // 32) * n_tiles} ({100.0 * units / (G * (rp // 32) * n_tiles):.3f} %), rows with a hit {int((fix_any != 0).sum())}", flush=True)
        fix_any.zero_()
