"""Survivor rate of the false-negative prefix filter on the benchmark's own batches: runs bench.py's train leg host-issued
(--no-graph, so every launch can be followed by a synchronise) and, after every mhr_nce_fix_bits_filtered call, reads the
candidate counter (first int32 of the workspace) and fix_any back.  A tool: nothing on the product path reads these on the host.

  python tools/nce_fix_survivors.py [bench.py arguments, default: --warmup 10 --steps 5]"""
import ctypes, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import mhr_amd  # noqa: F401
from mhr_amd import lib

hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
rows = []
_call = lib.call

def call(name, *args):
    _call(name, *args)
    if name == "mhr_nce_fix_bits_filtered":
        n_p_rows, n_neg, G, fix_any, ws = args[2], args[4], args[6], args[12], args[13]
        rp, n_tiles = (n_p_rows + 255) // 256 * 256, (n_neg + 31) // 32
        torch.cuda.synchronize()
        cnt = np.zeros(1, np.int32)
        anyb = np.zeros(G * rp, np.int32)
        assert hip.hipMemcpy(cnt.ctypes.data, ws, 4, 2) == 0 and hip.hipMemcpy(anyb.ctypes.data, fix_any, anyb.nbytes, 2) == 0
        rows.append((int(cnt[0]), G * (rp // 32) * n_tiles, int((anyb != 0).sum()), n_p_rows, G))

lib.call = call
import bench  # noqa: E402
sys.argv = ["bench.py", "--no-graph", "--no-cpu-baseline", "--no-eval-leg", "--no-host-probe", "--no-kernel-events"] + (sys.argv[1:] or ["--warmup", "10", "--steps", "5"])
bench.main()
for i, (c, cap, hit_rows, n_p, G) in enumerate(rows):
    print(f"fix_bits call {i}: units kept {c} of {cap} ({100.0 * c / cap:.4f} %), (group, target row) pairs with a hit {hit_rows} "
          f"of {G} x {n_p}")
if rows:
    print(f"mean over {len(rows)} calls: {np.mean([r[0] for r in rows]):.1f} units kept, {np.mean([r[2] for r in rows]):.1f} rows with a hit, "
          f"{100.0 * np.mean([r[0] / r[1] for r in rows]):.4f} % of the units")
