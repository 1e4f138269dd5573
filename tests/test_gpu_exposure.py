"""Catalog-exposure metrics on the GPU: the item histogram of mhr_exposure_accumulate and the sums of mhr_exposure_finalize
against the numpy restatement (tests/exposure_data.py), invariance under the batch split, ids outside the catalog, and
Trainer.evaluate end to end with `stream_metrics` off and on.

Shapes: the smallest at which these kernels can go wrong - 101 users in batches of 64 + 32 + 5 (a ragged last workgroup of the
accumulate), K = 24 with cut-offs [1, 5, 10, 20] (ranks 20..23 are ignored), N = 97 (many collisions, counts well above 1, one
item in every top-1: count = users = the last slot of the count-of-counts table), items 0 and N - 1 present; N = 4099 for the
finalize (five workgroups of 1024 items, the last one holding three).

Tolerances: the histogram and out_int are integers - exact.  S = sum c ln c against math.fsum: (R + 4) * 2^-53 * S, one
rounding per addition plus two ulp per term (the device's log and product against the helper's).  End to end: the summary is
rounded to metric_decimal_place = 7, the comparison allows one unit of that."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import exposure_data as XD

pytestmark = pytest.mark.gpu
CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")

U, K, N = 101, 24, 97
SPLIT = (64, 32, 5)
MARK = 0x5A5A5A5A


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


@pytest.fixture(scope="module")
def small():
    """The inputs and the numpy restatement of the small case, computed once."""
    lists, pop = XD.make_lists(7101, U, K, N), XD.make_pop(7151, N)
    tail = XD.tail_mask(pop, 0.25)
    band = XD.band_histogram(lists, XD.CUTS, N)
    ints, S = XD.integer_sums(band, pop, tail)
    return dict(lists=lists, pop=pop, tail=tail, band=band, ints=ints, S=S)


@pytest.fixture(scope="module")
def wide():
    Uw, Kw, Nw = 37, 20, 4099
    lists, pop = XD.make_lists(7102, Uw, Kw, Nw), XD.make_pop(7152, Nw)
    tail = XD.tail_mask(pop, 3)
    band = XD.band_histogram(lists, XD.CUTS, Nw)
    ints, S = XD.integer_sums(band, pop, tail)
    return dict(lists=lists, pop=pop, tail=tail, band=band, ints=ints, S=S, U=Uw, N=Nw)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class Device:
    """A zeroed histogram with one spare row past the n_cuts x n_items the kernels are told about, prefilled with a marker: a
    missing guard shows as a changed marker, never as an access outside owned memory."""

    def __init__(self, ops, n_items, cuts=XD.CUTS):
        self.ops, self.n_items, self.cuts = ops, n_items, list(cuts)
        self.hist = torch.zeros(len(cuts) + 1, n_items, dtype=torch.int32, device="cuda")
        self.hist[-1] = MARK
        self.bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.out_int = torch.full((len(cuts) + 1, 4), MARK, dtype=torch.int64, device="cuda")
        self.out_f64 = torch.full((len(cuts) + 1,), float(MARK), dtype=torch.float64, device="cuda")

    def add(self, lists, sizes=None):
        rows = dev(lists)
        lo = 0
        for n in sizes or (len(lists),):
            self.ops.exposure_accumulate(rows[lo:lo + n].contiguous(), self.cuts, self.n_items, self.hist, self.bad)
            lo += n
        assert lo == len(lists)
        return self

    def bands(self):
        h = self.hist.cpu().numpy()
        assert (h[-1] == MARK).all()                                       # the spare row is untouched
        return h[:-1].astype(np.int64)

    def finalize(self, users, pop=None, tail=None):
        self.ops.exposure_finalize(self.hist, len(self.cuts), self.n_items, users, self.cuts[-1], self.out_int, self.out_f64,
                                   self.bad, item_pop=None if pop is None else dev(pop), item_tail=None if tail is None else dev(tail))
        torch.cuda.synchronize()
        oi, of = self.out_int.cpu().numpy(), self.out_f64.cpu().numpy()
        assert (oi[-1] == MARK).all() and of[-1] == float(MARK) and (self.hist[-1] == MARK).all()
        return oi[:-1], of[:-1], int(self.bad.item())


def s_bound(ints, S):
    return (ints[:, 0] + 4) * 2.0 ** -53 * S


def test_the_inputs_hold_the_edge_cases(small, wide):
    c = small["band"].cumsum(axis=0)
    assert c[0].max() == U and (c[0] > 0).sum() == 1                       # one item in every top-1: count = users
    assert c[-1, 0] > 0 and c[-1, N - 1] > 0                               # items 0 and N - 1
    assert (small["lists"][:, 20:] == 0).any() and c[-1].sum() == U * 20   # ranks 20..23 hold a valid id and are ignored
    assert np.sort(c[-1])[-2] > 5                                          # counts well above 1
    assert all(len(set(r.tolist())) == K for r in small["lists"])          # no repeat inside a list
    assert -(-wide["N"] // 1024) == 5 and wide["N"] % 1024 == 3
    assert small["ints"][:, 3].min() > 0 and small["ints"][-1, 2] > 0 and wide["ints"][-1, 1] > 0


def test_the_histogram_is_the_numpy_histogram_band_by_band(ops, small, wide):
    got = Device(ops, N).add(small["lists"], SPLIT)
    assert np.array_equal(got.bands(), small["band"])
    assert int(got.bad.item()) == 0
    got = Device(ops, wide["N"]).add(wide["lists"])
    assert np.array_equal(got.bands(), wide["band"])
    one = Device(ops, N, cuts=[24]).add(small["lists"])                    # a single band up to K itself
    assert np.array_equal(one.bands()[0], np.bincount(small["lists"].reshape(-1), minlength=N))


@pytest.mark.parametrize("case", ["small", "wide"])
def test_finalize_gives_the_helpers_integers_and_entropy_sum(ops, small, wide, case):
    d = small if case == "small" else wide
    n, users = (N, U) if case == "small" else (wide["N"], wide["U"])
    oi, of, bad = Device(ops, n).add(d["lists"]).finalize(users, d["pop"], d["tail"])
    assert bad == 0
    assert np.array_equal(oi, d["ints"]), (oi, d["ints"])
    err, bound = np.abs(of - d["S"]), s_bound(d["ints"], d["S"])
    print(f"S {case}: err {err.tolist()} bound {bound.tolist()}")
    assert (err <= bound).all(), (err, bound)
    # without phi / the tail mask those two columns are zero and the others unchanged
    oi2, of2, _ = Device(ops, n).add(d["lists"]).finalize(users)
    assert np.array_equal(oi2[:, [0, 3]], d["ints"][:, [0, 3]]) and not oi2[:, 1:3].any()
    assert of2.tobytes() == of.tobytes()


def test_the_batch_split_changes_no_bit(ops, small):
    runs = []
    for sizes in ((U,), SPLIT, SPLIT, (5, 32, 64)):
        d = Device(ops, N).add(small["lists"], sizes)
        oi, of, bad = d.finalize(U, small["pop"], small["tail"])
        assert bad == 0
        runs.append((d.bands().tobytes(), oi.tobytes(), of.tobytes()))
    assert runs[0] == runs[1] == runs[2] == runs[3]


def test_ids_outside_the_catalog_write_nothing_and_are_counted(ops, small):
    lone = Device(ops, N, cuts=[2])
    before = lone.hist.clone()
    lone.add(np.asarray([[N, -1]], dtype=np.int64))                        # one past the catalog, and a negative id
    torch.cuda.synchronize()
    assert torch.equal(lone.hist, before) and int(lone.bad.item()) == 2    # every histogram word unchanged, the spare row included
    # inside a real list the other ranks still count, and the count is sticky over later launches
    row = small["lists"][:1]
    wrong = row.copy()
    wrong[0, 2], wrong[0, 7] = N, -1                                       # ranks 2 and 7: the bands 1 and 2
    wrong[0, 22] = N + 5                                                   # beyond the last cut-off: never looked at
    rest = XD.band_histogram(row, XD.CUTS, N)
    rest[1, row[0, 2]] -= 1
    rest[2, row[0, 7]] -= 1
    d = Device(ops, N).add(wrong)
    assert np.array_equal(d.bands(), rest) and int(d.bad.item()) == 2
    d.add(small["lists"])
    assert np.array_equal(d.bands(), rest + small["band"])
    assert d.finalize(U + 1)[2] == 2


def test_the_collector_raises_at_hand_out_after_an_id_outside_the_catalog(ops):
    from REC.evaluator.collector import Collector
    from REC.model.multihead import FusedTopK
    col = Collector(XD.base_cfg(shared_metrics=["ItemCoverage"], topk=[1, 5], item_num=50))
    idx = torch.arange(1, 11).view(2, 1, 5).cuda()
    idx[1, 0, 3] = 50
    col.eval_batch_collect(FusedTopK(torch.zeros(2, 1, 5).cuda(), idx), None, torch.ones(2, 1, dtype=torch.long))
    with pytest.raises(RuntimeError, match="outside"):
        col.get_data_struct(-1)
    # handed out = zeroed: the next evaluation starts clean
    idx[1, 0, 3] = 49
    col.eval_batch_collect(FusedTopK(torch.zeros(2, 1, 5).cuda(), idx), None, torch.ones(2, 1, dtype=torch.long))
    ex = col.get_data_struct(-1).get("rec.exposure_sums")
    assert ex["U"] == 2 and ex["N"] == 50 and ex["cuts"] == [1, 5] and ex["ints"][:, 0].tolist() == [2, 10]
    assert "rec.exposure_sums" not in col.get_data_struct(-1)


NAMES = ["ItemCoverage", "AveragePopularity", "ShannonEntropy", "GiniIndex", "TailPercentage"]


def _evaluate(stream, shared):
    import mhr_amd.synth as synth
    from REC.config.configurator import Config, apply_run_fixups
    from REC.trainer import Trainer
    from REC.utils import get_model
    device = torch.device("cuda", 0)
    torch.manual_seed(1)
    cfgd = synth.base_config(MAX_ITEM_LIST_LENGTH=20, pred_len=4, eval_pred_len=4, n_layers=1, n_heads=2, item_embedding_size=32,
                             hstu_embedding_size=32, loss='prior', medusa_num_layers=1, num_prior_head=3, num_segment_head=1,
                             eval_num_cats=3, num_negatives=64, topk=[5, 10, 20], device=device, total_iters=4, eval_interval=0,
                             checkpoint_dir=None, save_model_note="t", hidden_dropout_prob=0.0, outlier_user_metrics="long",
                             metrics=["Recall", "NDCG"], shared_metrics=shared, stream_metrics=stream, tail_ratio=0.25,
                             metric_decimal_place=7)
    cfg = apply_run_fixups(Config(config_dict=cfgd))
    data = synth.SyntheticData(cfg, 900, device)
    cfg["int_to_category"] = data.int_to_category
    model = get_model("HSTU")(cfg, data).to(device)
    tr = Trainer(cfg)
    tr.setup_model(model)
    batches = []
    for n in range(3):
        eb = list(data.eval_batch(8 if n < 2 else 5))
        eb[7] = torch.arange(len(eb[1]), device=device) % 3 == n
        batches.append(tuple(eb))
    pop = torch.from_numpy(XD.make_pop(7153, 900))

    class Loader(list):
        item_tags = data.item_tags
        item_counts = pop
    seen = []
    collect = tr.eval_collector.eval_batch_collect

    def spy(*a, **kw):
        out = collect(*a, log_detailed_results=True, **kw)
        seen.append(np.asarray(out["idx"], dtype=np.int64))
        return {}
    tr.eval_collector.eval_batch_collect = spy
    summary = tr.evaluate(Loader(batches))
    return summary, np.concatenate(seen), pop.numpy()


@pytest.mark.parametrize("stream", [False, True], ids=["stored", "streamed"])
def test_trainer_evaluate_matches_the_restated_formulas_on_the_merged_lists(ops, stream):
    plain_summary = _evaluate(stream, ["Entropy"])[0]
    summary, lists, pop = _evaluate(stream, ["Entropy"] + NAMES)
    assert lists.shape == (21, 20)
    want = XD.reference_values(lists, [5, 10, 20], 900, pop, 0.25)
    shared = summary["shared"]
    for name in NAMES:
        for k in (5, 10, 20):
            key = f"{name.lower()}@{k}"
            print(key, shared[key], want[key])
            assert abs(shared[key] - want[key]) <= 1e-7, (key, shared[key], want[key])
            assert shared[key] == round(shared[key], 7)
    assert shared["itemcoverage@20"] > shared["itemcoverage@5"] > 0 and shared["averagepopularity@5"] > 0
    # every key the evaluation had without the new names is unchanged (the same seeds: the same model, batches and lists)
    assert list(summary) == list(plain_summary)
    for part, res in plain_summary.items():
        assert [k for k in summary[part] if k.split("@")[0] not in [n.lower() for n in NAMES]] == list(res), part
        for k, v in res.items():
            assert summary[part][k] == v, (part, k, summary[part][k], v)
