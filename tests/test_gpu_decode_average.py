"""split_mode=average, fused (ops.catalog_topk_mean and the three kernels of csrc/catalog_mean.hip), on a real MI355X against
the CPU oracle: numpy on the fp32 operands, the reference's -inf masks, oracle.decode_oracle.suppress, then the arithmetic
and the order of decode_oracle.average_heads_topk (reference collector.py:227-230; draws and comparison: decode_average_data).

Tolerances are the project's own (tests/test_gpu_kernels.py::test_exact_topk_matches_reference_scores): a position is untied
when both neighbouring gaps of the oracle's sorted means exceed 1e-6; indices equal at untied positions; values within 2e-6 of
the oracle's mean of the returned index; the tied share is capped at 2 % of B*k (0 for the oracle alone on these draws)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import decode_average_data as AD
from conftest import ROOT, load_golden
from oracle import decode_oracle as DO
from oracle import metrics_oracle as MO

pytestmark = pytest.mark.gpu
CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if CODE not in sys.path:
        sys.path.insert(0, CODE)
    import mhr_amd  # noqa: F401
    from mhr_amd import ops as _ops
    return _ops


def cu(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def run_mean(ops, d, k, stats=None):
    hp, hi = AD.csr_history(d)
    items = cu(d["items"])
    items_bf = items.to(torch.bfloat16)
    if items_bf.shape[0] % 32:
        items_bf = torch.cat([items_bf, items_bf.new_zeros(32 - items_bf.shape[0] % 32, items_bf.shape[1])]).contiguous()
    v, i = ops.catalog_topk_mean(cu(d["heads"]), items_bf, items, cu(d["tag_bits"]), cu(d["row_bits"].reshape(-1)), cu(hp), cu(hi), k,
                                 n_items=d["N"], stats=stats)
    torch.cuda.synchronize()
    assert v.shape == (d["B"], k) and v.dtype == torch.float32 and i.dtype == torch.int64
    return v.cpu().numpy(), i.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# 1. streaming path, three head layouts
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,n_patterns", [(("mult", 2, 4), 15), (("add", 2, 3), 7), (("nce", 4), 1)], ids=["mult", "add", "nce"])
def test_streaming_path_matches_oracle(ops, layout, n_patterns):
    k = 20
    d = AD.draw(AD.STREAM_SEED, 6, 6000, 64, layout, n_hist=12)
    means, order = AD.expected(d, k)
    kth = means[np.arange(d["B"]), order[:, k - 1]]
    assert np.all((kth > 0.21) & (kth < 0.25)), kth                          # > 0 for every user: nobody takes the dense path
    stats = {}
    v, i = run_mean(ops, d, k, stats)
    print(f"[{layout[0]}] stats {stats}")
    assert stats["patterns"] == n_patterns and stats["dense_users"] == [], stats
    tied = AD.compare(v, i, means, order, k)
    print(f"[{layout[0]}] tied positions {tied} of {d['B'] * k}")
    v2, i2 = run_mean(ops, d, k)                                             # the one-host-read form (no stats) takes the same path
    assert np.array_equal(i, i2) and np.array_equal(v, v2)


# ----------------------------------------------------------------------------------------------------------------------
# 2. small catalog: the scorers' keep-every-score form
# ----------------------------------------------------------------------------------------------------------------------
def test_small_catalog_matches_oracle(ops):
    k = 20
    d = AD.draw(31, 6, 300, 32, ("mult", 2, 4), n_hist=12)
    means, order = AD.expected(d, k)
    stats = {}
    v, i = run_mean(ops, d, k, stats)
    print(f"[small] stats {stats}; k-th means {means[np.arange(6), order[:, k - 1]]}")
    AD.compare(v, i, means, order, k)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the zero quirk: items masked in every head score 0 and outrank negative means
# ----------------------------------------------------------------------------------------------------------------------
def test_zero_scores_of_masked_items_surface_in_small_catalogs(ops):
    k = 30
    d = AD.draw(41, 6, 48, 32, ("mult", 2, 4), n_hist=6)
    d["row_bits"][5, :] = 0                                                  # one user with every head switched off
    means, order = AD.expected(d, k)
    kth = means[np.arange(d["B"]), order[:, k - 1]]
    need = [b for b in range(d["B"]) if kth[b] <= 0]
    print(f"[zero] k-th means {kth}")
    assert len(need) >= 1 and 5 in need
    stats = {}
    v, i = run_mean(ops, d, k, stats)
    print(f"[zero] stats {stats}")
    assert set(need) <= set(stats["dense_users"]), (need, stats)
    AD.compare(v, i, means, order, k)                                        # zero-valued positions are compared exactly
    zeros = means[np.arange(d["B"])[:, None], order[:, :k]] == 0
    assert zeros.any() and np.array_equal(i[zeros], order[:, :k][zeros]) and np.all(v[zeros] == 0.0)
    assert np.array_equal(i[5], np.arange(k)) and np.all(v[5] == 0.0)


# ----------------------------------------------------------------------------------------------------------------------
# 4. uncertified rows: more near-ties than the candidate list has slots -> kernel C
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [("nce", 4), ("mult", 1, 2)], ids=["nce", "mult"])
def test_uncertified_rows_are_repaired_densely(ops, layout):
    """1 200 IDENTICAL item rows near the users' common direction: the margin set of the pattern rows they fall into holds more
    near-ties than the candidate list has slots (306 at k = 50), so those rows cannot be certified and their users are ranked
    from every item's mean.  Copies with the same tag word tie EXACTLY there (same arithmetic per item): ascending index decides."""
    k, B, N, D = 50, 6, 8192, 64
    d = AD.draw(51, B, N, D, layout)
    rng = np.random.default_rng(52)
    base = AD.l2n(rng.standard_normal((1, D)))
    dup = np.arange(100, 1300)
    d["items"][dup] = AD.l2n(base + 0.05 * rng.standard_normal((1, D))).astype(np.float32)
    d["items"][dup] = AD.l2n(d["items"][dup]).astype(np.float32)
    d["heads"] = AD.l2n(base[None] + 0.5 * rng.standard_normal((B, d["H"], D)) / D ** 0.5).astype(np.float32)
    d["heads"] = AD.l2n(d["heads"]).astype(np.float32)
    d["alias"] = (dup, int(dup[0]))
    # every user has seen a slice of the duplicated block and some other items
    d["hist"] = [np.array(sorted(set(rng.integers(1, N, 30).tolist()) | set(range(100 + 7 * b, 100 + 7 * b + 150, 3)))) for b in range(B)]
    means, order = AD.expected(d, k)
    stats = {}
    v, i = run_mean(ops, d, k, stats)
    print(f"[uncertified {layout[0]}] stats {stats}")
    assert stats["uncertified_rows"] > 0 and stats["dense_users"] == list(range(B)), stats
    word = np.zeros(N, np.int64) if d["tag_bits"] is None else d["tag_bits"]
    dup_lo, dup_hi = int(dup[0]), int(dup[-1])

    def same(b, a, c):
        return dup_lo <= a <= dup_hi and dup_lo <= c <= dup_hi and word[a] == word[c]
    AD.compare(v, i, means, order, k, same=same)
    assert all(len(set(i[b].tolist()) & set(dup.tolist())) == k for b in range(B))          # the duplicated block IS what was ranked
    v2, i2 = run_mean(ops, d, k)
    assert np.array_equal(i, i2) and np.array_equal(v, v2)


# ----------------------------------------------------------------------------------------------------------------------
# 5. the kernels alone, through the C ABI
# ----------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def test_kernel_head_mean_queries(ops):
    from mhr_amd import lib
    d = AD.draw(61, 3, 400, 72, ("mult", 1, 3))                              # D = 72: no multiple of the 64 lanes x 4
    d["row_bits"][1, :] = 0                                                  # every row of user 1 is dead
    d["row_bits"][2, 0] = 0                                                  # user 2: the word {cat 0} alone has no live head
    words, _ = ops.tag_patterns(torch.from_numpy(d["tag_bits"]))
    B, H, D, P = 3, d["H"], 72, len(words)
    assert P == 7
    q = torch.full((B * P, D), 7.0, device="cuda")
    qb = torch.full((B * P,), -1, dtype=torch.int32, device="cuda")
    heads, rb, w = cu(d["heads"]), cu(d["row_bits"].reshape(-1)), words.cuda()
    lib.call("mhr_head_mean_queries", heads.data_ptr(), rb.data_ptr(), w.data_ptr(), B, H, P, D, 1, q.data_ptr(), qb.data_ptr(), _stream())
    torch.cuda.synchronize()
    live = (d["row_bits"][:, :, None] & words.numpy()[None, None, :]) != 0
    cnt = live.sum(1)
    want = np.einsum("bhp,bhd->bpd", live.astype(np.float64), d["heads"].astype(np.float64)) / np.maximum(cnt, 1)[..., None]
    got = q.cpu().numpy().reshape(B, P, D)
    assert np.abs(got - want).max() <= 1e-6
    assert np.all(got[cnt == 0] == 0.0) and (cnt == 0).sum() == P + 1
    want_bits = np.where(cnt > 0, (1 << np.arange(P))[None, :], 0)
    assert np.array_equal(qb.cpu().numpy().reshape(B, P), want_bits)
    # without a tag table: one pattern, the word the scorers give every item
    w1 = torch.tensor([AD.BIT31], dtype=torch.int32, device="cuda")
    rb1 = torch.tensor([AD.BIT31, AD.BIT31, 0, 0, AD.BIT31, 0, 0, 0, 0], dtype=torch.int32, device="cuda")
    q1 = torch.empty(B, D, device="cuda")
    qb1 = torch.empty(B, dtype=torch.int32, device="cuda")
    lib.call("mhr_head_mean_queries", heads.data_ptr(), rb1.data_ptr(), w1.data_ptr(), B, H, 1, D, 0, q1.data_ptr(), qb1.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert qb1.tolist() == [AD.BIT31, AD.BIT31, 0]
    h = d["heads"].astype(np.float64)
    assert np.abs(q1.cpu().numpy() - np.stack([(h[0, 0] + h[0, 1]) / 2, h[1, 1], np.zeros(D)])).max() <= 1e-6


@pytest.mark.parametrize("D", [64, 320])                                      # 320: more than one 256-wide step per row
def test_kernel_rescore_mean(ops, D):
    from mhr_amd import lib
    d = AD.draw(62 + D, 2, 500, D, ("mult", 2, 3))
    d["row_bits"][1, [0, 3]] = 0                                             # user 1: both heads of category 0 off
    B, H, N, P, k2 = 2, d["H"], 500, 2, 8
    only0 = np.nonzero(d["tag_bits"] == (1 | AD.BIT31))[0]                   # items of category 0 alone: masked everywhere for user 1
    assert len(only0) >= 2
    rng = np.random.default_rng(5)
    cand = rng.integers(1, N, (B * P, k2)).astype(np.int64)
    cand[2, 1], cand[3, 0] = only0[0], only0[1]
    cnt = np.array([5, 8, 8, 3], np.int32)
    ov = torch.full((B * P, k2), 9.0, device="cuda")
    oi = torch.full((B * P, k2), -7, dtype=torch.int32, device="cuda")
    args = [cu(d["heads"]), cu(d["items"]), cu(d["tag_bits"]), cu(d["row_bits"].reshape(-1)), cu(cand), cu(cnt)]
    lib.call("mhr_rescore_mean_f32", args[0].data_ptr(), args[1].data_ptr(), D, N, H, P, args[2].data_ptr(), args[3].data_ptr(),
             args[4].data_ptr(), B * P, k2, args[5].data_ptr(), ov.data_ptr(), oi.data_ptr(), _stream())
    torch.cuda.synchronize()
    sc = np.einsum("bhd,nd->bhn", d["heads"], d["items"])
    fin = (d["row_bits"][:, :, None] & d["tag_bits"][None, None, :]) != 0
    want = (np.where(fin, sc, 0).sum(1) / (fin.sum(1) + 1e-8)).astype(np.float32)          # pad / history are not this kernel's
    gv, gi = ov.cpu().numpy(), oi.cpu().numpy()
    for r in range(B * P):
        c = cnt[r]
        assert np.array_equal(gi[r, :c], cand[r, :c]) and np.all(gi[r, c:] == -7) and np.all(gv[r, c:] == 9.0)
        assert np.abs(gv[r, :c] - want[r // P, cand[r, :c]]).max() <= 2e-6
    assert gv[2, 1] == 0.0 and gv[3, 0] == 0.0


@pytest.mark.parametrize("S", [2, 3], ids=["H8", "H12"])                         # H = 12: the dots in two groups of heads
def test_kernel_mean_rows_dense(ops, S):
    from mhr_amd import lib
    N, D = 1000, 64
    d = AD.draw(70 + S, 3, N, D, ("mult", S, 4), n_hist=25)
    d["row_bits"][2, 1::4] = 0                                               # user 2: every head of category 1 off
    means = AD.mean_of_finite(AD.masked_scores(d))
    hp, hi = AD.csr_history(d)
    users = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
    val = torch.full((2, N), 9.0, device="cuda")
    idx = torch.full((2, N), -7, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert lib.load().mhr_catalog_mean_rows_dense_workspace_bytes(2, N) == 2 * (N * 8 + 4)
    args = [cu(d["heads"]), cu(d["items"]), cu(d["tag_bits"]), cu(d["row_bits"].reshape(-1)), cu(hp), cu(hi)]
    lib.call("mhr_catalog_mean_rows_dense", args[0].data_ptr(), args[1].data_ptr(), D, N, users.data_ptr(), 2, d["H"], args[2].data_ptr(),
             args[3].data_ptr(), args[4].data_ptr(), args[5].data_ptr(), val.data_ptr(), idx.data_ptr(), cnt.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert cnt.tolist() == [N, N] and np.array_equal(idx.cpu().numpy(), np.tile(np.arange(N, dtype=np.int32), (2, 1)))
    got = val.cpu().numpy()
    for j, b in enumerate((2, 0)):
        masked = ~np.isfinite(AD.masked_scores(d)[b]).any(axis=0)
        assert masked[0] and masked[d["hist"][b]].all() and masked.sum() >= 26 + (b == 2)   # user 2: items of category 1 alone too
        assert np.all(got[j][masked] == 0.0) and not np.signbit(got[j][masked]).any()       # exact +0, not -inf
        assert np.abs(got[j] - means[b]).max() <= 2e-6


# ----------------------------------------------------------------------------------------------------------------------
# 6. model level
# ----------------------------------------------------------------------------------------------------------------------
def _tiny_hstu(split_mode, N=900, **over):
    import mhr_amd.synth as synth
    import REC  # noqa: F401
    from REC.config.configurator import Config, apply_run_fixups
    from REC.utils import get_model
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    kw = dict(MAX_ITEM_LIST_LENGTH=20, pred_len=4, eval_pred_len=4, n_layers=1, n_heads=2, item_embedding_size=32,
              hstu_embedding_size=32, loss='prior', medusa_num_layers=1, num_prior_head=3, num_segment_head=1,
              eval_num_cats=3, num_negatives=64, topk=[5, 10, 20], device=dev, total_iters=4, eval_interval=0,
              checkpoint_dir=None, save_model_note="t", hidden_dropout_prob=0.0, split_mode=split_mode)
    kw.update(over)
    cfg = apply_run_fixups(Config(config_dict=synth.base_config(**kw)))
    data = synth.SyntheticData(cfg, N, dev)
    cfg["int_to_category"] = data.int_to_category
    model = get_model("HSTU")(cfg, data).to(dev)
    return cfg, data, model


def _suppressed_dense_scores(model, eb, feat, tags_cn):
    """The reference's route: predict() scores [B,H,N] + trainer.py:724-726, on the device."""
    scores = model.predict(eb[1], None, feat, tags_cn, eb[6])[0].float()
    scores[:, :, 0] = float("-inf")
    scores[eb[3][0], :, eb[3][1]] = float("-inf")
    return scores


def _check_fused_against_dense(fused, scores, k):
    assert tuple(fused.values.shape) == (scores.shape[0], 1, k) and tuple(fused.indices.shape) == (scores.shape[0], 1, k)
    sc = scores.cpu().numpy()
    want = DO.decode_topk(sc.copy(), k, "average")
    means = AD.mean_of_finite(sc)
    order = np.stack([DO.topk_desc(means[b], k + 1)[0] for b in range(sc.shape[0])])
    assert np.array_equal(order[:, :k], want)
    AD.compare(fused.values[:, 0].cpu().numpy(), fused.indices[:, 0].cpu().numpy(), means, order, k)


@pytest.mark.parametrize("variant", ["prior", "nce2"])
def test_predict_topk_average_matches_dense_average(ops, variant):
    """Fails on the parent commit: predict_topk handed per-head lists and the collector raised `needs dense scores`."""
    from REC.evaluator.collector import Collector
    over = {} if variant == "prior" else dict(loss='nce', num_prior_head=1, num_segment_head=2, neg_sample_by_cat=False)
    cfg, data, model = _tiny_hstu("average", **over)
    model.eval()
    assert model.medusa_num_heads == (3 if variant == "prior" else 2)
    feat = model.compute_item_all()
    tags_cn = data.item_tags.long().t().contiguous()
    k = 20
    eb = data.eval_batch(8)
    fused = model.predict_topk(eb[1], feat, tags_cn, eb[6], eb[3], k=k)
    scores = _suppressed_dense_scores(model, eb, feat, tags_cn)
    _check_fused_against_dense(fused, scores, k)
    c1, c2 = Collector(cfg), Collector(cfg)
    c1.eval_batch_collect(fused, eb[4], eb[2])
    c2.eval_batch_collect(scores, eb[4], eb[2])
    for p in cfg["metrics_pred_len_list"]:
        a, b = c1.get_data_struct(p)['rec.topk'], c2.get_data_struct(p)['rec.topk']
        assert torch.equal(a, b), p
    # per-head lists cannot be averaged after the fact: the collector says what it needs
    model.split_mode = 'combine'
    per_head = model.predict_topk(eb[1], feat, tags_cn, eb[6], eb[3], k=k)
    with pytest.raises(ValueError, match="fused average decode"):
        Collector(cfg).eval_batch_collect(per_head, eb[4], eb[2])


# ----------------------------------------------------------------------------------------------------------------------
# 7. Trainer.evaluate end to end
# ----------------------------------------------------------------------------------------------------------------------
def test_trainer_evaluate_average_metrics_match_oracle_decode(ops):
    """Trainer.evaluate with split_mode: average on synthetic users: Recall/NDCG from the fused decode == metrics of the oracle's
    average decode of the dense scores of the same user heads."""
    from REC.trainer import Trainer
    cfg, data, model = _tiny_hstu("average")
    tr = Trainer(cfg)
    tr.setup_model(model)
    batches = [data.eval_batch(8) for _ in range(3)]

    class Loader(list):
        item_tags = data.item_tags
    res = tr.evaluate(Loader(batches))
    model.eval()
    feat = model.compute_item_all()
    tags = data.item_tags.long().t().contiguous()
    K = 20
    sums = {p: {} for p in cfg["metrics_pred_len_list"]}
    n = 0
    for eb in batches:
        users = model._user_heads(eb[1]).float().cpu()
        sc = (users @ feat.float().cpu().T).numpy()
        for h in range(sc.shape[1]):
            sc[:, h, ~tags[h % 3].bool().cpu().numpy()] = -np.inf
        DO.suppress(sc, eb[3][0].cpu().numpy(), eb[3][1].cpu().numpy())
        topk = DO.decode_topk(sc, K, "average")
        hits = DO.hit_matrices(topk, eb[2].cpu().numpy(), cfg["metrics_pred_len_list"])
        for p in cfg["metrics_pred_len_list"]:
            for k, v in MO.recall_ndcg(hits[p], cfg["topk"]).items():
                sums[p][k] = sums[p].get(k, 0.0) + v
        n += sc.shape[0]
    for p in cfg["metrics_pred_len_list"]:
        for k, v in sums[p].items():
            assert abs(res[f"pred_{p}"][k] - v / n) < 1e-6, (p, k, res[f"pred_{p}"][k], v / n)


class _FakeData:
    def __init__(self, cfg):
        self.item_num = cfg["item_num"]
        self.category_counts = cfg["category_counts"]
        self.category_to_int = cfg["category_to_int"]


@pytest.mark.parametrize("name", ["ComiRec", "REMI"])
def test_interest_models_decode_average_through_the_shared_mixin(ops, name):
    """ComiRec / REMI (the interests are the decode's heads, no tag table: one pattern): the fused average decode against the
    average of their own dense scores."""
    import REC  # noqa: F401
    from REC.config.configurator import Config
    from REC.evaluator.collector import Collector
    from REC.utils import get_model
    g = load_golden("comirec_nce" if name == "ComiRec" else "remi_nce")
    c = json.loads(str(g["cfg/json"]))
    c["int_to_category"] = {int(k): v for k, v in c["int_to_category"].items()}
    c["split_mode"] = "average"
    model = get_model(name)(Config(config_dict=c), _FakeData(c))
    model.load_state_dict({k[2:]: torch.from_numpy(np.array(v)) for k, v in g.items() if k.startswith("w/")}, strict=True)
    model = model.cuda().eval()
    seq = torch.from_numpy(g["in/item_seq"]).cuda()
    feat = model.compute_item_all()
    k = 10
    fused = model.predict_topk(seq, feat, None, None, None, k=k, suppress_history=False)
    scores = model.predict(seq, None, feat, None, None)[0].float()
    scores[:, :, 0] = float("-inf")
    assert scores.shape[1] == model.medusa_num_heads > 1
    _check_fused_against_dense(fused, scores, k)
    cc = dict(dict(head_interaction='multiplicative', num_segment_head=1, num_prior_head=1), **c)
    cc.update(metrics_pred_len_list=[0], topk=[k], eval_pred_len=1)
    col = Collector(cc)
    pos = torch.randint(1, scores.shape[2], (scores.shape[0], 1), device="cuda")
    col.eval_batch_collect(fused, None, pos)
    assert tuple(col.get_data_struct(0)['rec.topk'].shape) == (scores.shape[0], k + 1)


@pytest.mark.parametrize("name", ["ComiRec", "REMI"])
def test_trainer_evaluate_average_runs_for_the_interest_models(ops, name):
    """Trainer.evaluate with split_mode: average on a toy ComiRec / REMI (the reference-contract route raised in the collector)."""
    import mhr_amd.synth as synth
    import REC  # noqa: F401
    from REC.config.configurator import Config, apply_run_fixups
    from REC.trainer import Trainer
    from REC.utils import get_model
    dev = torch.device("cuda", 0)
    torch.manual_seed(2)
    cfg = apply_run_fixups(Config(config_dict=synth.base_config(
        MAX_ITEM_LIST_LENGTH=16, pred_len=2, eval_pred_len=2, n_layers=1, n_heads=2, item_embedding_size=32, hstu_embedding_size=32,
        loss='nce', num_negatives=64, topk=[5, 10], device=dev, total_iters=4, eval_interval=0, checkpoint_dir=None,
        save_model_note="t", hidden_dropout_prob=0.0, split_mode="average", interest_num=3)))
    data = synth.SyntheticData(cfg, 400, dev)
    cfg["int_to_category"] = data.int_to_category
    model = get_model(name)(cfg, data).to(dev)
    assert model.medusa_num_heads == 3 and model.split_mode == "average"
    tr = Trainer(cfg)
    tr.setup_model(model)

    class Loader(list):
        item_tags = data.item_tags
    res = tr.evaluate(Loader([data.eval_batch(8) for _ in range(2)]))
    vals = [v for p in cfg["metrics_pred_len_list"] for v in res[f"pred_{p}"].values()]
    assert len(vals) > 0 and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in vals), res


def test_hllm_decodes_average_through_the_shared_mixin(ops):
    from test_gpu_llm import _build_hllm, _hllm_cfg
    cfgd = _hllm_cfg(split_mode="average")
    N, B, K = 301, 6, 20
    L, C = cfgd["MAX_ITEM_LIST_LENGTH"], cfgd["num_prior_head"]
    g = torch.Generator().manual_seed(23)
    item_tags = (torch.rand(N, C, generator=g) < 0.5).long()
    item_tags[torch.arange(N), torch.randint(0, C, (N,), generator=g)] = 1
    table = torch.randn(N, 64, generator=g)
    seq = torch.randint(1, N, (B, L), generator=g)
    for b in range(B):
        seq[b, :int(torch.randint(0, L - 1, (1,), generator=g))] = 0
    tt = item_tags[torch.randint(1, N, (B, cfgd["eval_pred_len"]), generator=g)]
    model = _build_hllm(cfgd, N).eval()
    model.set_all_item_embeds(table.cuda())
    feat = model.compute_item_all()
    tags_cn = item_tags.t().contiguous().cuda()
    scores = model((seq.cuda(), None, feat, tags_cn, tt.cuda()), mode='predict')[0].float()
    scores[:, :, 0] = float("-inf")
    fused = model.predict_topk(seq.cuda(), feat, tags_cn, tt.cuda(), None, k=K, suppress_history=False)
    _check_fused_against_dense(fused, scores, K)
