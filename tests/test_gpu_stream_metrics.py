"""Streaming evaluation metrics on the GPU: mhr_eval_metric_sums against the reference collector goldens and against the
numpy restatement (tests/stream_metrics_data.py), accumulation over launches and bitwise determinism, and the Collector /
Trainer with `stream_metrics` off against on.

Tolerances: the six top-k columns 1e-12 relative (fp64 on both sides, the same order of the running sums; the project's bound for
host metrics), counts exact.  Entropy: device and host log2 may differ by a few ulp per term, and terms add over tags and
users; the largest relative difference to the fp64 numpy value over the cases of KERNEL_CASES was measured on an MI355X as
7.0e-16 (ENTROPY_MEASURED; per case 0 to 6.99e-16), the tests assert 16 x that = 1.12e-14 (a bound of this kind is never taken
above 1e-9: metrics are printed to at most 7 decimals).  The golden
entropies carry float32 precision: 1e-6 there (test_cpu_host.py)."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import stream_metrics_data as SD

pytestmark = pytest.mark.gpu
CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")

RTOL = 1e-12
ENTROPY_MEASURED = 7.0e-16     # largest relative difference over KERNEL_CASES on the first MI355X run (6.989e-16, rounded up)
ENTROPY_RTOL = min(16 * ENTROPY_MEASURED, 1e-9)

#                B    K   E   C'  G
KERNEL_CASES = [(1, 1, 1, 1, 1), (63, 20, 4, 4, 5), (64, 200, 8, 32, 32), (65, 20, 8, 4, 5), (300, 200, 4, 4, 5),
                (300, 1, 4, 1, 1), (65, 200, 1, 32, 32), (300, 20, 8, 32, 32), (64, 20, 1, 1, 32)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if CODE not in sys.path:
        sys.path.insert(0, CODE)
    import REC  # noqa: F401
    import mhr_amd  # noqa: F401
    from mhr_amd import ops
    return ops


def dev(x):
    return (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x).cuda()


def cutoffs(K):
    return [k for k in dict.fromkeys((min(5, K), 1, max(K // 2, 1), K))]          # unsorted on purpose, distinct


def pack_bits(tags):
    """[N, C] bool -> [N] int32 words holding the uint32 pattern (bit c = tag c)."""
    w = (tags.astype(np.uint64) << np.arange(tags.shape[1], dtype=np.uint64)).sum(axis=1)
    return w.astype(np.uint32).view(np.int32)


class Device:
    """The inputs of one case on the device plus zeroed accumulators; `launch(rows)` adds those users."""

    def __init__(self, ops, topk_idx, positives, preds, topk, group_bits, n_groups, tags):
        self.ops, self.preds, self.topk, self.G = ops, list(preds), list(topk), n_groups
        self.idx, self.pos = dev(topk_idx), dev(positives)
        self.plen = dev(SD.pos_len_full(positives))
        self.bits = dev(group_bits.view(np.int32))
        self.tag_bits, self.n_tags = (dev(pack_bits(tags)), tags.shape[1]) if tags is not None else (None, 0)
        P, T = len(preds), len(topk)
        self.sums = torch.zeros(P, n_groups, 6, T, dtype=torch.float64, device="cuda")
        self.counts = torch.zeros(P, n_groups, dtype=torch.int64, device="cuda")
        self.entropy = torch.zeros(T, dtype=torch.float64, device="cuda") if tags is not None else None

    def launch(self, rows=slice(None)):
        self.ops.eval_metric_sums(self.idx[rows].contiguous(), self.pos[rows].contiguous(), self.plen[rows].contiguous(), self.preds,
                                  self.topk, self.bits[rows].contiguous(), self.G, self.sums, self.counts,
                                  item_tag_bits=self.tag_bits, n_tags=self.n_tags, entropy=self.entropy)
        return self

    def host(self):
        torch.cuda.synchronize()
        return self.sums.cpu().numpy(), self.counts.cpu().numpy(), None if self.entropy is None else self.entropy.cpu().numpy()


def rel_diff(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), np.finfo(np.float64).tiny)))


@pytest.mark.parametrize("name", ["collector_combine", "collector_additive", "collector_k200", "collector_single",
                                  "collector_smallcat"])
def test_kernel_reproduces_the_reference_collector_goldens(ops, name):
    g = load_golden(name)
    topk, preds = [int(k) for k in g["cfg/topk"]], [int(p) for p in g["cfg/pred_len_list"]]
    idx, pos, tags = g["out/idx"].astype(np.int64), g["in/positive_i"].astype(np.int64), g["in/all_tags"].astype(bool)
    bits = np.ones((len(idx), len(preds)), dtype=np.uint32)
    sums, counts, ent = Device(ops, idx, pos, preds, topk, bits, 1, tags).launch().host()
    assert (counts == len(idx)).all()
    for i, p in enumerate(preds):
        for c, col in enumerate(("recall", "ndcg")):
            for t, k in enumerate(topk):
                np.testing.assert_allclose(sums[i, 0, c, t], float(g[f"out/m{p}/{col}@{k}"]), rtol=RTOL, err_msg=f"{col}@{k} p={p}")
    for t, k in enumerate(topk):
        np.testing.assert_allclose(ent[t], float(g[f"out/shared/Entropy@{k}"]), rtol=1e-6, err_msg=f"Entropy@{k}")


@pytest.fixture(scope="module")
def kernel_cases():
    """The numpy restatement of every case, computed once."""
    out = {}
    for n, (B, K, E, C, G) in enumerate(KERNEL_CASES):
        case = SD.make_case(100 + n, B, K, E, C, G)
        topk = cutoffs(K)
        want = SD.numpy_sums(case["topk_idx"], case["positives"], case["preds"], topk, case["group_bits"], G, case["tags"])
        out[(B, K, E, C, G)] = (case, topk, want)
    return out


@pytest.mark.parametrize("shape", KERNEL_CASES, ids=lambda s: "B{}-K{}-E{}-C{}-G{}".format(*s))
def test_kernel_equals_the_numpy_restatement(ops, kernel_cases, shape):
    case, topk, (w_sums, w_counts, w_ent) = kernel_cases[shape]
    B, K, E, C, G = shape
    pl = SD.pos_len_full(case["positives"])
    if E > K:
        assert (pl[:, E - 1] > K).any()                                   # pos_len > K is among the inputs
    if G > 2:
        assert (w_counts[:, G - 2] == 0).all() and (w_counts[:, 0] == B).all()   # one empty group, bit 0 for everyone
    sums, counts, ent = Device(ops, case["topk_idx"], case["positives"], case["preds"], topk, case["group_bits"], G,
                               case["tags"]).launch().host()
    assert np.array_equal(counts, w_counts)
    np.testing.assert_allclose(sums, w_sums, rtol=RTOL, atol=0)
    d = rel_diff(ent, w_ent)
    print(f"entropy rel diff {shape}: {d:.3e}")
    assert d <= ENTROPY_RTOL, (d, ENTROPY_RTOL)


def test_sums_accumulate_over_launches_and_are_bitwise_reproducible(ops, kernel_cases):
    shape = (300, 200, 4, 4, 5)
    case, topk, (w_sums, w_counts, w_ent) = kernel_cases[shape]
    args = (ops, case["topk_idx"], case["positives"], case["preds"], topk, case["group_bits"], shape[4], case["tags"])
    one = Device(*args).launch().host()
    parts = (slice(0, 65), slice(65, 66), slice(66, 300))
    runs = []
    for _ in range(2):
        d = Device(*args)
        for rows in parts:
            d.launch(rows)
        runs.append(d.host())
    assert np.array_equal(runs[0][1], one[1]) and np.array_equal(one[1], w_counts)
    np.testing.assert_allclose(runs[0][0], one[0], rtol=RTOL, atol=0)
    np.testing.assert_allclose(runs[0][2], one[2], rtol=RTOL, atol=0)
    for a, b in zip(runs[0], runs[1]):                                    # the same launch sequence: the same bits
        assert a.tobytes() == b.tobytes()


# ---- Collector: key off against key on ----------------------------------------------------------------------------------------
class Cfg(dict):
    def __getitem__(self, k):
        return dict.get(self, k)

    def get(self, k, d=None):
        v = dict.get(self, k)
        return d if v is None else v


def _compare_results(off, on, entropy_rtol=ENTROPY_RTOL):
    assert list(on.keys()) == list(off.keys())
    for k, v in off.items():
        w = on[k]
        assert isinstance(w, tuple) == isinstance(v, tuple), k
        if isinstance(v, tuple):
            assert w[1] == v[1], k
            v, w = v[0], w[0]
        np.testing.assert_allclose(w, v, rtol=entropy_rtol if k.startswith("Entropy") else RTOL, atol=0, err_msg=k)


@pytest.mark.parametrize("fused", [False, True], ids=["dense", "fused_topk"])
def test_collector_streamed_equals_stored(ops, fused):
    from REC.evaluator import Evaluator
    from REC.evaluator.collector import Collector
    from REC.model.multihead import FusedTopK
    N, H, C, E, K = 400, 3, 3, 4, 20
    cfg = Cfg(metrics_pred_len_list=[0, 1, 3], eval_pred_len=E, topk=[1, 5, 10, K], head_interaction="multiplicative",
              num_segment_head=1, num_prior_head=C, split_mode="combine", metrics=["Recall", "NDCG", "Hit", "MRR", "MAP", "Precision"],
              shared_metrics=["Entropy"], eval_num_cats=C, eval_by_cat=True, outlier_user_metrics="long",
              int_to_category={i: f"cat{i}" for i in range(C)}, metric_decimal_place=7)
    g = torch.Generator().manual_seed(77)
    tags = torch.rand(N, C, generator=g) < 0.4
    tags[torch.arange(N), torch.randint(0, C, (N,), generator=g)] = True
    batches = []
    for B in (8, 8, 5):                                                   # the last batch is ragged
        base = torch.randn(B, 1, N, generator=g)
        scores = base + 0.35 * torch.randn(B, H, N, generator=g)          # correlated heads: cross-head duplicates to merge
        pos = torch.randint(1, N, (B, E), generator=g)
        pos[0, 1] = pos[0, 0]                                             # a duplicated target
        for b in range(0, B, 2):
            scores[b, :, pos[b, b % E]] += 3.0                            # hits at several target positions
        scores[:, :, 0] = float("-inf")
        tag_category = tags[pos].clone()                                  # [B, E, C]
        tag_category[:, :, 2] &= torch.arange(E)[None, :] > 0             # category 2 is empty at pred_len 0
        outlier = torch.rand(B, generator=g) < 0.4
        inp = scores.cuda()
        if fused:
            v, i = torch.topk(inp, K + 4, dim=-1)                         # holds more than max(topk): the collector cuts it
            inp = FusedTopK(v, i)
        batches.append((inp, torch.arange(B).unsqueeze(-1).repeat(1, E), pos.cuda(), tag_category.cuda(), outlier.cuda()))
    results = {}
    for key in (False, True):
        col = Collector(Cfg(cfg, stream_metrics=key))
        col.set_all_tags(tags.long().cuda())
        for inp, pu, pi, tc, ol in batches:
            assert col.eval_batch_collect(inp, pu, pi, tag_category=tc, outlier_users=ol) == {}
        if key:                                                           # nothing grows per batch
            assert all(not col.data_struct[p]._tensor_lists and not col.data_struct[p]._data_dict for p in col.data_struct)
        ev = Evaluator(cfg)
        res = {-1: ev.evaluate(col.get_data_struct(-1), pred_len=-1)}
        col.reset_all_tags()
        for p in cfg["metrics_pred_len_list"]:
            res[p] = ev.evaluate(col.get_data_struct(p), pred_len=p)
        results[key] = res
        if key:                                                           # handed out = zeroed: a second evaluation starts from nothing
            assert "rec.entropy_sums" not in col.get_data_struct(-1)
            assert not col.get_data_struct(0).get("rec.metric_sums")["sums"].any()
    for p in results[False]:
        _compare_results(results[False][p], results[True][p])
    assert results[True][0]["cat2-recall@5"] == (0.0, 0) and "outlier_long-ndcg@20" in results[True][3]
    assert float(results[True][3]["hit@20"]) > 0


def test_trainer_evaluate_streamed_equals_stored(ops):
    import mhr_amd.synth as synth
    from REC.config.configurator import Config, apply_run_fixups
    from REC.trainer import Trainer
    from REC.utils import get_model
    device = torch.device("cuda", 0)
    summaries = {}
    for key in (False, True):
        torch.manual_seed(1)
        cfgd = synth.base_config(MAX_ITEM_LIST_LENGTH=20, pred_len=4, eval_pred_len=4, n_layers=1, n_heads=2, item_embedding_size=32,
                                 hstu_embedding_size=32, loss='prior', medusa_num_layers=1, num_prior_head=3, num_segment_head=1,
                                 eval_num_cats=3, num_negatives=64, topk=[5, 10, 20], device=device, total_iters=4, eval_interval=0,
                                 checkpoint_dir=None, save_model_note="t", hidden_dropout_prob=0.0, outlier_user_metrics="long",
                                 metrics=["Recall", "NDCG", "Hit", "MRR", "MAP", "Precision"], stream_metrics=key)
        cfg = apply_run_fixups(Config(config_dict=cfgd))
        data = synth.SyntheticData(cfg, 900, device)
        cfg["int_to_category"] = data.int_to_category
        model = get_model("HSTU")(cfg, data).to(device)
        tr = Trainer(cfg)
        tr.setup_model(model)
        assert tr.eval_collector.stream_metrics is key
        batches = []
        for n in range(3):
            eb = list(data.eval_batch(8))
            eb[7] = torch.arange(8, device=device) % 3 == n                # some outlier users in every batch
            batches.append(tuple(eb))

        class Loader(list):
            item_tags = data.item_tags
        summaries[key] = tr.evaluate(Loader(batches))
    off, on = summaries[False], summaries[True]
    dp = 7
    assert list(on.keys()) == list(off.keys())
    for name in off:
        assert list(on[name].keys()) == list(off[name].keys()), name
        for k, v in off[name].items():
            assert abs(on[name][k] - v) <= 2 * 10.0 ** -dp, (name, k, on[name][k], v)
    assert "Entropy@5" in on["shared"] and "outlier_long-recall@5" in on["pred_3"] and "precision@20" in on["pred_0"]
