"""Packed encoder rows from the product batchers, end to end on the GPU:

  * mhr_seq_pack_maps_guarded (csrc/rows_pack.hip): the maps of mhr_seq_pack_maps bit for bit, plus the sticky overflow record
    (overflowing calls, largest count, its capacity, 0) that no launch clears - also inside a replayed graph;
  * Trainer.fit / Trainer.evaluate over SeqTrainBatcher / SeqEvalBatcher with `packed_rows`: the encoder runs at the capacities
    the batchers handed out; a CPU-collated loader gets its capacity from `batch_rows_cap`;
  * a capacity hint below the batch's valid positions that arrives AFTER the first host-checked steps (replayed or host-issued)
    is caught by HSTU.check_pack_guard where the Trainer already synchronises.
The overflowing batches are a defined, clamped condition (rows past the capacity are dropped), not a fault."""
import os
import sys

import pytest
import torch

from conftest import ROOT
from rows_hint_data import B, BUCKET, C, L, N, config_dict, make_data

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


# ----------------------------------------------------------------------------------------------------------------------
# the guard kernel
# ----------------------------------------------------------------------------------------------------------------------
def _same_maps(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("Bq,Lq", [(5, 70), (300, 3)])     # a window across the 64-lane boundary; a scan thread owning two sequences
def test_guarded_pack_maps_match_and_record_overflow(ops, Bq, Lq):
    g = torch.Generator().manual_seed(11 + Bq)
    kv = (torch.rand(Bq, Lq, generator=g) < 0.6)
    kv[0], kv[1] = False, True                                # one empty sequence, one full one
    count = int(kv.sum())
    kv = kv.to(torch.uint8).cuda().contiguous()
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    for cap in (count, count + 37):
        got = ops.seq_pack_maps(kv, Bq, Lq, cap, guard=guard)
        assert _same_maps(got, ops.seq_pack_maps(kv, Bq, Lq, cap)) and int(got[3]) == 0
        assert guard.tolist() == [0, 0, 0, 0]
    for cap in (count - 1, count // 2):
        got = ops.seq_pack_maps(kv, Bq, Lq, cap, guard=guard)
        assert _same_maps(got, ops.seq_pack_maps(kv, Bq, Lq, cap)) and int(got[3]) == count
    assert guard.tolist() == [2, count, count - 1, 0]
    ops.seq_pack_maps(kv, Bq, Lq, count, guard=guard)         # a fitting call clears nothing
    assert guard.tolist() == [2, count, count - 1, 0]


def test_guard_survives_graph_replays(ops):
    Bq, Lq, cap = 4, 40, 64
    fits = torch.zeros(Bq, Lq, dtype=torch.uint8)
    fits[:, 25:] = 1                                          # 60 valid positions
    over = torch.zeros(Bq, Lq, dtype=torch.uint8)
    over[:, 15:] = 1                                          # 100
    fits, over = fits.cuda(), over.cuda()
    static_mask = fits.clone()
    guard = torch.zeros(4, dtype=torch.int32, device="cuda")
    ops.seq_pack_maps(static_mask, Bq, Lq, cap, guard=guard)  # (host-issued once: library loaded, allocator warm)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.seq_pack_maps(static_mask, Bq, Lq, cap, guard=guard)
    static_mask.copy_(fits)
    graph.replay()
    assert guard.tolist() == [0, 0, 0, 0] and int(out[3]) == 0
    assert _same_maps(out, ops.seq_pack_maps(fits, Bq, Lq, cap))
    static_mask.copy_(over)
    graph.replay()
    graph.replay()
    assert guard.tolist() == [2, 100, cap, 0] and int(out[3]) == 100
    assert _same_maps(out, ops.seq_pack_maps(over, Bq, Lq, cap))
    static_mask.copy_(fits)
    graph.replay()
    assert guard.tolist() == [2, 100, cap, 0] and int(out[3]) == 0


# ----------------------------------------------------------------------------------------------------------------------
# the trainer over the batchers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store(ops):
    from REC.data import SeqStore
    user_seq, train_len, tags = make_data()
    return SeqStore(user_seq, train_len, tags, device="cuda"), tags


def _setup(tags, seed=0, **over):
    from mhr_amd import synth
    from REC.config.configurator import Config, apply_run_fixups
    from REC.trainer import Trainer
    from REC.utils import get_model
    kw = dict(n_layers=1, n_heads=2, item_embedding_size=32, hstu_embedding_size=32, num_prior_head=C, medusa_num_layers=1,
              total_iters=10, eval_interval=0, topk=[5, 20], hidden_dropout_prob=0.0, checkpoint_dir=None, save_model_note="t",
              device="cuda", optim_args={'learning_rate': 3e-3, 'weight_decay': 0.0}, scheduler_args=None, metrics_pred_len_list=[1])
    kw.update(over)
    cfgd = synth.base_config(**config_dict(**kw))
    cfg = apply_run_fixups(Config(config_dict=cfgd))
    cfg["int_to_category"] = {c: f"cat{c}" for c in range(C)}

    class Meta:
        item_num = N
        category_to_int = {f"cat{c}": c for c in range(C)}
        category_counts = {f"cat{c}": int(tags[:, c].sum()) for c in range(C)}
    torch.manual_seed(seed)
    model = get_model("HSTU")(cfg, Meta()).cuda()
    tr = Trainer(cfg)
    tr.setup_model(model)
    return cfg, model, tr


class _Recording:
    """A loader that notes what its batcher handed out: (batch size, rows_cap) per batch."""

    def __init__(self, inner):
        self.inner, self.handed = inner, []

    def __iter__(self):
        for b in self.inner:
            self.handed.append((b[2].shape[0], b.rows_cap))
            yield b


def _spy(ops, monkeypatch):
    calls, real = [], ops.seq_pack_maps
    monkeypatch.setattr(ops, "seq_pack_maps", lambda *a, **k: (calls.append((a[1], a[3])), real(*a, **k))[1])
    return calls


def test_fit_over_the_train_batcher_packs_at_its_capacities(ops, store, monkeypatch):
    from REC.data import SeqTrainBatcher
    st, tags = store
    calls = _spy(ops, monkeypatch)
    cfg, model, tr = _setup(tags, packed_rows=True)
    loader = _Recording(SeqTrainBatcher(cfg, st, seed=1, rows_bucket=BUCKET))
    tr.fit(loader, verbose=False, saved=False)
    assert tr.train_step == 10 and len(calls) >= 3, calls
    assert set(calls) <= set(loader.handed), (calls, loader.handed)
    assert all(0 < cap < b * L for b, cap in calls), calls
    assert model.check_pack_guard() is None
    n_on = len(calls)
    cfg, model, tr = _setup(tags)                                       # the key absent: window rows, as before
    tr.fit(SeqTrainBatcher(cfg, st, seed=1), verbose=False, saved=False)
    assert tr.train_step == 10 and len(calls) == n_on


def test_evaluate_over_the_eval_batcher_packs_and_agrees(ops, store, monkeypatch):
    from REC.data import SeqEvalBatcher
    st, tags = store
    calls = _spy(ops, monkeypatch)
    cfg, model, tr = _setup(tags, packed_rows=True)
    plain_cfg = _setup(tags)[0]
    plain = tr.evaluate(SeqEvalBatcher(plain_cfg, st, phase="valid"), item_tags=st.item_tags)
    assert calls == []
    loader = SeqEvalBatcher(cfg, st, phase="valid", rows_bucket=BUCKET)
    packed = tr.evaluate(loader, item_tags=st.item_tags)
    assert len(calls) == len(loader) == 10 and all(0 < cap < b * L for b, cap in calls), calls
    # the tolerance of tests/test_gpu_configs.py::test_cfg1_eval_user_heads_on_packed_rows (packed against window user heads):
    # 2e-2 of the largest magnitude of the window path's values
    assert list(packed) == list(plain)
    for name in plain:
        assert list(packed[name]) == list(plain[name])
        tol = 2e-2 * max([abs(float(v)) for v in plain[name].values()] or [0.0])
        for k in plain[name]:
            print(f"evaluate {name} {k}: window {plain[name][k]} packed {packed[name][k]} (tolerance {tol:.3g})")
        for k in plain[name]:
            assert abs(float(packed[name][k]) - float(plain[name][k])) <= tol, (name, k, plain[name][k], packed[name][k])


def test_fit_packs_a_cpu_collated_loader(ops, store, monkeypatch):
    from REC.data import SeqTrainBatcher
    from REC.data.batcher import batch_rows_cap
    st, tags = store
    calls = _spy(ops, monkeypatch)
    cfg, model, tr = _setup(tags, packed_rows=True, hip_graph=False)    # host-issued: one seq_pack_maps call per packed step
    batches = [tuple(t.cpu() for t in b) for b in SeqTrainBatcher(_setup(tags)[0], st, seed=1)]
    assert len(batches) == 10 and all(type(b) is tuple and not hasattr(b[2], "_mhr_rows_cap") for b in batches)
    tr.fit(batches, verbose=False, saved=False)
    caps = [(b[2].shape[0], batch_rows_cap(b[2], L)) for b in batches]
    # (a capacity that does not undercut the window rows - the short last batch under the default bucket - is not packed)
    want = [(bs, cap) for bs, cap in caps if cap < bs * L]
    assert len(calls) > 0 and calls == want, (calls, caps)
    assert model.check_pack_guard() is None


@pytest.mark.parametrize("graph", [False, None])
def test_a_lying_hint_is_caught_after_the_early_checks(ops, store, graph):
    from REC.data import SeqTrainBatcher
    from REC.data.batcher import Batch
    st, tags = store
    over = {} if graph is None else {"hip_graph": graph}

    def seven(lie):
        cfg, model, tr = _setup(tags, packed_rows=True, total_iters=7, **over)
        it = iter(SeqTrainBatcher(cfg, st, seed=1, rows_bucket=256))
        batches = [next(it) for _ in range(7)]
        assert all(b[2].shape[0] == B and b.rows_cap == 256 for b in batches)       # every full batch: capacity 256
        if lie:
            items, neg, mask, tg = batches[6]
            mask = mask.clone()
            mask[:, :L] = 1                                              # 384 valid positions ...
            mask._mhr_rows_cap = 256                                     # ... under a hint of 256
            batches[6] = Batch((items, neg, mask, tg), 256)
        return model, tr, batches

    model, tr, batches = seven(lie=True)
    with pytest.raises(RuntimeError, match="capacity"):
        tr.fit(batches, verbose=False, saved=False)
    assert model.check_pack_guard() is None                              # (raising cleared the record)
    # the loss tokens of the dropped rows were counted as bad ids (csrc/tokens.hip), in a counter the whole process shares:
    # read - and thereby reset - it, so that no later fit reports them
    assert ops.bad_id_count() > 0
    model, tr, batches = seven(lie=False)
    tr.fit(batches, verbose=False, saved=False)
    assert tr.train_step == 7 and model.check_pack_guard() is None
