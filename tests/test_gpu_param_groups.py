"""Per-group learning rate and weight decay in the fused AdamW (FusedAdamW(param_groups=...), include/mhr.h:
mhr_adam_flat_groups; the reference's `lr_mult_prefix` / `lr_mult_rate`, trainer.py:268-291): the grouped kernel bitwise against
the ungrouped one run segment by segment, the grouped optimizer against torch.optim.AdamW with two param groups (CPU, fp32) with
and without clipping, lazy == dense, the Trainer's keys, replayed == host-issued, and the state_dict round trip."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def rec():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if CODE not in sys.path:
        sys.path.insert(0, CODE)
    import REC  # noqa: F401
    return REC


@pytest.fixture(scope="module")
def ops(rec):
    from mhr_amd import ops as _ops
    return _ops


# ---- 1. the kernel, bitwise against mhr_adam_flat run segment by segment ------------------------------------------------
RATIO = [1.0, 4.0, 0.25, 7.0]
DECAY = [0.01, 0.0, 0.1, 0.003]
HIST = 64
GUARD = 64

SHAPES = {
    "n8_one_segment": ([0, 8], [0], 1),
    "n8200_edges_at_8_and_at_the_chunk_edge": ([0, 8, 8192, 8200], [0, 1, 0], 2),
    "n24584_alternating_then_two_chunk_span": (list(range(0, 8192 + 1, 8)) + [24584], [k % 3 for k in range(1024)] + [1], 3),
    "n40_five_segments_one_group_empty": ([0, 8, 16, 24, 32, 40], [0, 1, 3, 1, 0], 4),
}


def _buffers(n, gen):
    """w, m, v (fp32) and the bf16 shadow as views of buffers with GUARD sentinel elements behind them."""
    full = [torch.randn(n + GUARD, generator=gen).to(DEV), torch.zeros(n + GUARD, device=DEV), torch.zeros(n + GUARD, device=DEV),
            torch.full((n + GUARD,), 3.0, dtype=torch.bfloat16, device=DEV)]
    for t in full:
        t[n:] = -7.0
    return full


@pytest.mark.parametrize("form", ["step_argument", "step_dev_and_history", "step_argument_scale_dev"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_grouped_kernel_is_bitwise_the_ungrouped_kernel_per_segment(ops, shape, form):
    seg_off, seg_group, n_groups = SHAPES[shape]
    n = seg_off[-1]
    assert len(set(seg_group)) == (n_groups if "empty" not in shape else n_groups - 1)
    tables = ops.adam_group_tables(seg_off, seg_group, n_groups, DEV)
    assert tables.chunk_seg.numel() == -(-n // 8192)
    gen = torch.Generator().manual_seed(n)
    got = _buffers(n, gen)
    want = [t.clone() for t in got]
    gconst = torch.zeros(HIST, n_groups, 4, device=DEV)
    hists = torch.zeros(n_groups, HIST, 4, device=DEV)                # the ungrouped kernel's history, one per group
    row = torch.zeros(n_groups, 4)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    scale = torch.tensor([123.0, 0.37], device=DEV) if form.endswith("scale_dev") else None
    for step, lr in ((63, 1e-2), (64, 3e-3), (65, 2e-2)):             # rows 63, 0, 1 of the history: across the wrap
        g = torch.randn(n, generator=gen).to(DEV)
        lrs = [lr * r for r in RATIO[:n_groups]]
        ops.adam_group_consts(row, step, lrs, DECAY[:n_groups])
        gconst[step % HIST].copy_(row)
        hists[:, step % HIST].copy_(row)
        step_dev.fill_(step)
        by_dev = form == "step_dev_and_history"
        ops.adam_flat_groups(got[0][:n], g, got[1][:n], got[2][:n], tables, gconst, 1 if by_dev else step, 0.5, w_bf16=got[3][:n],
                             step_dev=step_dev if by_dev else None, scale_dev=scale)
        for a, b, grp in zip(seg_off, seg_off[1:], seg_group):
            if a == b:
                continue
            ops.adam_flat(want[0][a:b], g[a:b], want[1][a:b], want[2][a:b], 1 if by_dev else step, 1.0 if by_dev else lrs[grp], 0.5,
                          weight_decay=7.0 if by_dev else DECAY[grp], w_bf16=want[3][a:b], hist=hists[grp] if by_dev else None,
                          step_dev=step_dev if by_dev else None, scale_dev=scale)
        for name, x, y in zip(("w", "m", "v", "w_bf16"), got, want):
            assert torch.equal(x, y), (name, step)                    # (the guard elements included: nothing written past n)
    assert float(got[0][n]) == -7.0 and float(got[3][n]) == -7.0
    assert not torch.equal(got[0][:n], _buffers(n, torch.Generator().manual_seed(n))[0][:n])     # and it did move


def test_one_group_of_ratio_one_is_adam_flat_on_the_whole_buffer(ops):
    n = 2 * 8192 + 1016                                                # three chunks, the last one short
    tables = ops.adam_group_tables([0, n], [0], 1, DEV)
    gen = torch.Generator().manual_seed(1)
    got = _buffers(n, gen)
    want = [t.clone() for t in got]
    gconst = torch.zeros(HIST, 1, 4, device=DEV)
    row = torch.zeros(1, 4)
    for step, lr in ((1, 1e-2), (2, 3e-3), (3, 2e-2)):
        g = torch.randn(n, generator=gen).to(DEV)
        gconst[step % HIST].copy_(ops.adam_group_consts(row, step, [lr * 1.0], [0.01]))
        ops.adam_flat_groups(got[0][:n], g, got[1][:n], got[2][:n], tables, gconst, step, w_bf16=got[3][:n])
        ops.adam_flat(want[0][:n], g, want[1][:n], want[2][:n], step, lr, weight_decay=0.01, w_bf16=want[3][:n])
        for x, y in zip(got, want):
            assert torch.equal(x, y), step
    # without the shadow: the same fp32 results, the shadow untouched
    before = got[3].clone()
    g = torch.randn(n, generator=gen).to(DEV)
    gconst[4].copy_(ops.adam_group_consts(row, 4, [1e-2], [0.01]))
    ops.adam_flat_groups(got[0][:n], g, got[1][:n], got[2][:n], tables, gconst, 4)
    ops.adam_flat(want[0][:n], g, want[1][:n], want[2][:n], 4, 1e-2, weight_decay=0.01)
    assert all(torch.equal(x, y) for x, y in zip(got[:3], want[:3])) and torch.equal(got[3], before)


# ---- 2, 3. the optimizer against torch.optim.AdamW with two param groups (CPU, fp32) -------------------------------------
N_T, D_T = 300, 64
KEYS = ["item_embedding.weight", "other", "mat"]
HIGH = 4.0                                                               # lr ratio of the table's group
MAGS = {None: (1.0, 1.0, 1.0, 1.0, 1.0), 1.0: (3.0, 0.002, 0.5, 0.001, 0.004)}      # (clipping: norms on both sides of 1.0)
BASE_LR = (1e-2, 7e-3, 1.3e-2, 2e-3, 9e-3)                               # param_groups[0]["lr"], different every step


class Tiny(torch.nn.Module):
    def __init__(self, n=N_T, d=D_T):
        super().__init__()
        self.item_embedding = torch.nn.Embedding(n, d)
        self.other = torch.nn.Parameter(torch.randn(7))                 # 7 elements: the flat buffer pads it to 8
        self.mat = torch.nn.Parameter(torch.randn(5, 9))
        self.sparse_grad = None


GROUPS = [{"prefixes": ["item_embedding", "mat"], "lr_ratio": HIGH, "weight_decay": 0.0}]     # group 0: `other`, decay 0.01


def _feed(ops, model, slot, ids, rows, dense_grads):
    from REC.model.hstu_functional import SparseRowGrad
    sorted_ids, perm = torch.sort(ids)
    out_rows = torch.zeros(ids.numel(), rows.shape[1], device=rows.device)
    ops.sparse_rows_segment_sum(sorted_ids, perm, rows, None, None, 0, 0, out_rows, slot)
    model.sparse_grad = SparseRowGrad(sorted_ids, out_rows, slot, slot.numel())
    for p, g in zip((model.other, model.mat), dense_grads):
        p.grad.copy_(g)
    return model.sparse_grad


def _inputs(clip):
    gen = torch.Generator().manual_seed(5)
    steps = []
    for mag in MAGS[clip]:
        ids = (torch.rand(64, generator=gen) ** 2 * (N_T - 1)).long()
        # the rows on a grid of mag * 2^-10 (to the power of two below): rows of one id then sum exactly in fp32 in any order,
        # so the oracle's index_add_ and the port's segment sum hand the two optimizers the same gradient bits
        q = 2.0 ** (math.floor(math.log2(mag)) - 10)
        rows = torch.round(torch.randn(64, D_T, generator=gen) * mag / q) * q
        steps.append((ids, rows, torch.randn(7, generator=gen) * mag, torch.randn(5, 9, generator=gen) * mag))
    return steps


_ORACLE = {}


def _oracle(clip, init):
    """torch.optim.AdamW over two param groups on the CPU in fp32 (+ torch's clip_grad_norm_), computed once per threshold:
    per step {weights, m, v per key} and the pre-clip norm."""
    if clip in _ORACLE:
        return _ORACLE[clip]
    params = {k: torch.nn.Parameter(init[k].clone()) for k in KEYS}
    opt = torch.optim.AdamW([{"params": [params["other"]], "lr": BASE_LR[0], "weight_decay": 0.01},
                             {"params": [params["item_embedding.weight"], params["mat"]], "lr": BASE_LR[0] * HIGH, "weight_decay": 0.0}],
                            betas=(0.9, 0.999), eps=1e-8)
    out = []
    for t, (ids, rows, g_other, g_mat) in enumerate(_inputs(clip)):
        params["item_embedding.weight"].grad = torch.zeros(N_T, D_T).index_add_(0, ids, rows)
        params["other"].grad, params["mat"].grad = g_other.clone(), g_mat.clone()
        norm = None
        if clip is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(list(params.values()), clip, norm_type=2))
        opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = BASE_LR[t], BASE_LR[t] * HIGH
        opt.step()
        out.append(({k: params[k].detach().clone() for k in KEYS}, {k: opt.state[params[k]]["exp_avg"].clone() for k in KEYS},
                    {k: opt.state[params[k]]["exp_avg_sq"].clone() for k in KEYS}, norm))
    _ORACLE[clip] = out
    return out


def _run_fused(ops, clip, lazy):
    from mhr_amd.optim import FusedAdamW
    torch.manual_seed(21)
    model = Tiny().to(DEV)
    init = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    want = _oracle(clip, init)
    opt = FusedAdamW(model, lr=BASE_LR[0], weight_decay=0.01, lazy_table=lazy, clip_grad_norm=clip, param_groups=GROUPS)
    assert opt.lazy == lazy and opt._table_group == 1 and opt._seg_lists[:2] == ([0, 8, 56], [0, 1])
    slot = torch.full((N_T,), -1, dtype=torch.int32, device=DEV)
    clipped = []
    for t, (ids, rows, g_other, g_mat) in enumerate(_inputs(clip)):
        ids = ids.to(DEV)
        opt.catch_up(ids)
        _feed(ops, model, slot, ids, rows.to(DEV), [g_other.to(DEV), g_mat.to(DEV)])
        opt.param_groups[0]["lr"] = BASE_LR[t]
        opt.step()
        opt.zero_grad()
        assert opt.param_groups[1]["lr"] == BASE_LR[t] * HIGH          # written back for logging
        w_ref, m_ref, v_ref, norm = want[t]
        if clip is not None:
            got_norm = float(opt.grad_norm)
            print(f"step {t}: grad_norm {got_norm:.8g}, torch {norm:.8g}")
            assert abs(got_norm - norm) <= 1e-6 * norm, (t, got_norm, norm)
            clipped.append(norm > clip)
        opt.flush_table()
        off_o, off_m = model.other._mhr_flat_off, model.mat._mhr_flat_off
        for k, p, m_, v_ in (("item_embedding.weight", model.item_embedding.weight, opt.t_m, opt.t_v),
                             ("other", model.other, opt.flat_m[off_o:off_o + 7], opt.flat_v[off_o:off_o + 7]),
                             ("mat", model.mat, opt.flat_m[off_m:off_m + 45].view(5, 9), opt.flat_v[off_m:off_m + 45].view(5, 9))):
            np.testing.assert_allclose(p.detach().cpu().numpy(), w_ref[k].numpy(), rtol=2e-5, atol=1e-6, err_msg=f"{k} step {t}")
            np.testing.assert_allclose(m_.cpu().numpy(), m_ref[k].numpy(), rtol=2e-5, atol=1e-6, err_msg=f"m {k} step {t}")
            np.testing.assert_allclose(v_.cpu().numpy(), v_ref[k].numpy(), rtol=2e-5, atol=1e-9, err_msg=f"v {k} step {t}")
    if clip is not None:
        assert any(clipped) and not all(clipped), clipped
    assert int((slot != -1).sum()) == 0
    return model, opt


@pytest.mark.parametrize("clip", [None, 1.0])
def test_grouped_optimizer_against_torch_adamw_with_two_param_groups(rec, ops, clip):
    (m_lazy, o_lazy), (m_dense, o_dense) = _run_fused(ops, clip, True), _run_fused(ops, clip, False)
    # lazy against dense: bitwise
    assert torch.equal(m_lazy.item_embedding.weight, m_dense.item_embedding.weight)
    for name in ("t_m", "t_v", "flat_w", "flat_m", "flat_v", "flat_w16"):
        assert torch.equal(getattr(o_lazy, name), getattr(o_dense, name)), name


# ---- 4. the Trainer ----------------------------------------------------------------------------------------------------
KEYS_ON = dict(lr_mult_prefix=['item_embedding', 'position_embedding'], lr_mult_rate=4)


def _model(graph, **over):
    import mhr_amd.synth as synth
    from REC.config.configurator import Config, apply_run_fixups
    from REC.utils import get_model
    dev = torch.device("cuda", 0)
    kw = dict(MAX_ITEM_LIST_LENGTH=12, n_layers=1, n_heads=1, item_embedding_size=16, hstu_embedding_size=16, num_negatives=64,
              total_iters=40, eval_interval=0, checkpoint_dir=None, save_model_note="t",
              scheduler_args={'type': 'cosine', 'warmup': 0.25}, optim_args={'learning_rate': 2e-3, 'weight_decay': 0.01},
              device=dev, hip_graph=graph)
    kw.update(over)
    cfg = apply_run_fixups(Config(config_dict=synth.base_config(**kw)))
    data = synth.SyntheticData(cfg, 400, dev)
    cfg["int_to_category"] = data.int_to_category
    torch.manual_seed(11)
    return cfg, get_model("HSTU")(cfg, data).to(dev), data


def _trainer(graph, **over):
    from REC.trainer import Trainer
    cfg, model, data = _model(graph, **over)
    tr = Trainer(cfg)
    tr.setup_model(model)
    return tr, model, data


def test_trainer_keys_give_the_hand_driven_grouped_optimizer_bitwise_and_differ_from_no_keys(rec, ops):
    from mhr_amd.optim import FusedAdamW
    ops.set_deterministic(True)
    try:
        tr_on, m_on, data = _trainer(False, **KEYS_ON)
        tr_off, m_off, _ = _trainer(False)
        _, m_hand, _ = _model(False)                                      # no Trainer: the optimizer below is built by hand
        assert all(torch.equal(a, b) for a, b in zip(m_on.state_dict().values(), m_hand.state_dict().values()))
        assert tr_off.optimizer.groups is None and len(tr_on.optimizer.groups) == 2
        names = tr_on.optimizer.groups[1]["names"]
        assert "item_embedding.weight" in names and any(n.startswith("position_embedding") for n in names)
        assert len(tr_on.optimizer._seg_lists[1]) >= 2                    # the position table is a segment of its own in the flat buffer
        hand = FusedAdamW(m_hand, lr=2e-3, weight_decay=0.01, lazy_table=True,
                          param_groups=[{"prefixes": ['item_embedding', 'position_embedding'], "lr_ratio": 4.0, "weight_decay": None}])
        hand.enable_partial_arena(True)
        batches = [data.train_batch(8) for _ in range(3)]
        n_steps = 5
        for i in range(n_steps):
            b = batches[i % len(batches)]
            tr_on.train_step_fn(b, graph=False)
            tr_off.train_step_fn(b, graph=False)
            out = m_hand(b)
            out["loss"].backward()
            hand.param_groups[0]["lr"] = tr_on._lr_at(i)
            hand.step()
            hand.zero_grad()
        assert tr_on.optimizer.param_groups[1]["lr"] == tr_on._lr_at(n_steps - 1) * 4.0
        sd_on, sd_off, sd_hand = m_on.state_dict(), m_off.state_dict(), m_hand.state_dict()      # (flushes the lazy tables)
        for k in sd_on:
            assert torch.equal(sd_on[k], sd_hand[k]), k
        for name in ("flat_w", "flat_m", "flat_v", "flat_w16", "t_m", "t_v"):
            assert torch.equal(getattr(tr_on.optimizer, name), getattr(hand, name)), name
        # without the keys the run ends elsewhere: the table and the position table moved four times as fast
        assert not torch.equal(sd_on["item_embedding.weight"], sd_off["item_embedding.weight"])
        assert not torch.equal(tr_on.optimizer.flat_w, tr_off.optimizer.flat_w)
    finally:
        ops.set_deterministic(False)


def test_replayed_grouped_steps_are_the_host_issued_steps_bit_for_bit(rec, ops):
    ops.set_deterministic(True)
    try:
        tr_e, m_e, data = _trainer(False, **KEYS_ON)
        tr_g, m_g, _ = _trainer(True, **KEYS_ON)
        batches = [data.train_batch(8) for _ in range(4)]
        n_steps = 9                                                       # three host-issued warm-up steps, six replayed
        le, lg = [], []
        for i in range(n_steps):
            b = batches[i % len(batches)]
            le.append(float(tr_e.train_step_fn(b, graph=False)["loss"]))
            lg.append(float(tr_g.train_step_fn(b)["loss"]))
        assert tr_g.graph_active and not tr_e.graph_active
        assert tr_g._step_graph.n == n_steps - 3
        assert le == lg, (le, lg)
        assert tr_g.optimizer.param_groups[1]["lr"] == tr_e.optimizer.param_groups[1]["lr"] == tr_e._lr_at(n_steps - 1) * 4
        sd_e, sd_g = m_e.state_dict(), m_g.state_dict()
        for k in sd_e:
            assert torch.equal(sd_e[k], sd_g[k]), k
        for name in ("flat_w", "flat_m", "flat_v", "t_m", "t_v"):
            assert torch.equal(getattr(tr_e.optimizer, name), getattr(tr_g.optimizer, name)), name
    finally:
        ops.set_deterministic(False)


# ---- 5. state_dict round trip ------------------------------------------------------------------------------------------
def test_state_dict_round_trip_with_and_without_the_groups_record(rec, ops):
    from mhr_amd.optim import FusedAdamW

    def fresh():
        torch.manual_seed(31)
        m = Tiny().to(DEV)
        return m, FusedAdamW(m, lr=1e-2, weight_decay=0.01, lazy_table=True, param_groups=GROUPS), \
            torch.full((N_T,), -1, dtype=torch.int32, device=DEV)

    def one_step(m, o, slot, inp, lr):
        ids, rows, g_other, g_mat = inp
        ids = ids.to(DEV)
        o.catch_up(ids)
        _feed(ops, m, slot, ids, rows.to(DEV), [g_other.to(DEV), g_mat.to(DEV)])
        o.param_groups[0]["lr"] = lr
        o.step()
        o.zero_grad()

    inputs = _inputs(None)
    m_a, o_a, s_a = fresh()
    for t in range(2):
        one_step(m_a, o_a, s_a, inputs[t], BASE_LR[t])
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in o_a.state_dict().items()}
    assert sd["groups"][1] == {"lr_ratio": HIGH, "weight_decay": 0.0, "names": ["mat", "item_embedding.weight"]}
    old = {k: v for k, v in sd.items() if k != "groups"}                  # a state saved before the groups existed
    finals = []
    for state in (sd, old):
        m_b, o_b, s_b = fresh()
        m_b.load_state_dict(m_a.state_dict())
        o_b.load_state_dict(state)
        assert o_b.step_count == 2
        finals.append((m_b, o_b, s_b))
    for m, o, s in [(m_a, o_a, s_a)] + finals:
        one_step(m, o, s, inputs[2], BASE_LR[2])
        o.flush_table()
    for m_b, o_b, _ in finals:
        assert torch.equal(m_b.item_embedding.weight, m_a.item_embedding.weight)
        for name in ("flat_w", "flat_m", "flat_v", "t_m", "t_v"):
            assert torch.equal(getattr(o_b, name), getattr(o_a, name)), name
