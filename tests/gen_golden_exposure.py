#!/usr/bin/env python3
"""Generate tests/golden/exposure_metrics.npz from the REFERENCE's ItemCoverage, AveragePopularity, ShannonEntropy, GiniIndex
and TailPercentage classes (evaluator/metrics.py:473-780), which no other fixture pins.

Runs only in the build container (needs the reference tree, like tests/gen_golden.py whose stubs it uses).
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/gen_golden_exposure.py

The fixture holds arrays and values only: per case the item matrix, phi, N and the cut-offs, and every value the reference's
classes return at decimal_place 12, for tail_ratio 0.25 and 3.  The generator asserts ln T / (ln T - S / T) < 50 at every cut-off
of its inputs: the entropy is the difference of those two terms, so this bounds how much the rounding of S is magnified.
"""
import math
import os
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as GG  # noqa: E402
import exposure_data as XD  # noqa: E402

#         name     seed  U    K   N
CASES = (("small", 5101, 101, 24, 97), ("wide", 5102, 37, 20, 4099))
TAIL_RATIOS = (0.25, 3)
CANCELLATION = 50.0


def main():
    GG._setup()
    import numpy as np
    import torch
    from REC.evaluator.collector import DataStruct
    from REC.evaluator.metrics import AveragePopularity, GiniIndex, ItemCoverage, ShannonEntropy, TailPercentage
    d = {"cfg/topk": np.asarray(XD.CUTS), "cfg/tail_ratios": np.asarray(TAIL_RATIOS, dtype=np.float64),
         "cfg/cases": np.asarray([c[0] for c in CASES])}
    for name, seed, U, K, N in CASES:
        lists = XD.make_lists(seed, U, K, N, common_top1=False)
        pop = XD.make_pop(seed + 50, N)
        assert (np.bincount(lists[:, :5].reshape(-1), minlength=N) == U).any()           # one item in every user's top-5
        assert (lists[:, :max(XD.CUTS)] == 0).any() and (lists[:, :max(XD.CUTS)] == N - 1).any()
        ints, S = XD.integer_sums(XD.band_histogram(lists, XD.CUTS, N))
        for t, k in enumerate(XD.CUTS):
            ln_t = math.log(U * k)
            assert ln_t / (ln_t - S[t] / (U * k)) < CANCELLATION, (name, k)
        st = DataStruct()
        st.set("rec.items", torch.from_numpy(lists))
        st.set("data.num_items", N)
        st.set("data.count_items", {i: int(pop[i]) for i in range(1, N) if pop[i] > 0})
        d[f"{name}/items"], d[f"{name}/pop"], d[f"{name}/N"] = lists, pop, np.asarray(N)
        for ratio in TAIL_RATIOS:
            cfg = GG.Cfg(topk=XD.CUTS, metric_decimal_place=10, tail_ratio=ratio, eval_pred_len=1, eval_num_cats=1,
                         int_to_category={0: "cat0"})
            for cls in (ItemCoverage, AveragePopularity, ShannonEntropy, GiniIndex, TailPercentage):
                m = cls(cfg)
                assert m.decimal_place == 12
                for key, v in m.calculate_metric(st, pred_len=-1).items():
                    d[f"{name}/out/tail_{ratio}/{key}"] = np.asarray(v, dtype=np.float64)
    assert len(d) == 3 + len(CASES) * (3 + len(TAIL_RATIOS) * 5 * len(XD.CUTS))
    np.savez_compressed(os.path.join(GG.OUT, "exposure_metrics.npz"), **d)
    print("exposure_metrics:", len(d), "keys")


if __name__ == "__main__":
    main()
