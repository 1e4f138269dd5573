"""Gradient clipping by global norm on the device (FusedAdamW(clip_grad_norm=...), include/mhr.h: mhr_grad_sqnorm_* /
mhr_grad_clip_coef / mhr_adam_*_scaled): the norm kernels against numpy fp64, the coefficient against torch's formula, the
clipped optimizer against torch.nn.utils.clip_grad_norm_ + the AdamW oracle, and the properties the fused step must keep -
off is bitwise today's step, lazy == dense, replayed == host-issued, data-parallel replicas stay replicas."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import optim_oracle as OO

pytestmark = pytest.mark.gpu
CODE = os.path.join(ROOT, "multi-head-recommendation-with-human-priors_amd", "code")
NEW_ENTRIES = ("mhr_grad_sqnorm_flat", "mhr_grad_sqnorm_rows", "mhr_grad_clip_coef", "mhr_adam_flat_scaled",
               "mhr_adam_rows_scaled", "mhr_adam_rows_lazy_scaled")


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


DEV = "cuda:0"


def _wide(shape, gen):
    """randn * 10^uniform(-3, 3): squares spread over twelve decades."""
    return torch.randn(shape, generator=gen) * 10.0 ** (torch.rand(shape, generator=gen) * 6.0 - 3.0)


def _norm_record(ops, partials, n_p, pre_scale=1.0, max_norm=1e30):
    out = torch.zeros(2, dtype=torch.float32, device=DEV)
    ops.grad_clip_coef(partials, n_p, pre_scale, max_norm, out)
    return out.cpu().numpy()


# ---- 3. the norm kernels against numpy fp64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 7, 8, 4097, 2 ** 20 + 3])
def test_flat_squared_norm_against_numpy_fp64(ops, n):
    gen = torch.Generator().manual_seed(100 + n % 97)
    x = _wide((n,), gen)
    want = float(np.sum(x.numpy().astype(np.float64) ** 2))
    xd = x.to(DEV)
    n_p = ops.grad_sqnorm_partials(n)
    off = 3                                                          # the offset is honoured, nothing else is written
    partials = torch.full((off + n_p + 2,), -7.0, dtype=torch.float64, device=DEV)
    assert ops.grad_sqnorm_flat(xd, partials, off) == n_p
    p = partials.cpu().numpy()
    assert np.all(p[:off] == -7.0) and np.all(p[off + n_p:] == -7.0)
    got = float(np.sum(p[off:off + n_p]))
    print(f"n={n}: partials {n_p}, squared sum rel err {abs(got - want) / max(want, 1e-300):.2e}")
    assert abs(got - want) <= 1e-10 * want                            # fp64 accumulation of <= 2^20 non-negative terms
    assert n > 0 or (n_p == 1 and got == 0.0)                          # n = 0 writes zeros
    norm = _norm_record(ops, partials[off:], n_p)[0]
    assert abs(float(norm) - math.sqrt(want)) <= 3e-7 * math.sqrt(want)   # one fp32 rounding of the root
    again = torch.zeros_like(partials)
    ops.grad_sqnorm_flat(xd, again, off)
    assert torch.equal(again[off:off + n_p], partials[off:off + n_p])  # a pure function of the input bits


@pytest.mark.parametrize("dim", [16, 64, 256])
def test_rows_squared_norm_counts_in_range_segment_heads_only(ops, dim):
    N, n_ids = 50, 96
    gen = torch.Generator().manual_seed(7 + dim)
    ids = torch.randint(0, N, (n_ids,), generator=gen)
    ids[5], ids[40], ids[41], ids[77] = -1, N, N, -1                 # ids outside [0, N): left out of the update and of the norm
    assert ids.unique().numel() < n_ids - 20                          # duplicates
    src = _wide((n_ids, dim), gen)
    sorted_ids, perm = torch.sort(ids)
    sorted_ids, perm = sorted_ids.to(DEV), perm.to(DEV)
    out_rows = torch.zeros(n_ids, dim, device=DEV)
    slot = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    ops.sparse_rows_segment_sum(sorted_ids, perm, src.to(DEV), None, None, 0, 0, out_rows, slot)
    s = sorted_ids.cpu()
    head = torch.ones(n_ids, dtype=torch.bool)
    head[1:] = s[1:] != s[:-1]
    counted = head & (s >= 0) & (s < N)
    rows = out_rows.cpu().numpy().astype(np.float64)
    assert float(np.abs(rows[(head & ~counted).numpy()]).sum()) > 0    # the out-of-range heads do hold a gradient
    want = float(np.sum(rows[counted.numpy()] ** 2))
    n_p = ops.grad_sqnorm_partials(n_ids, dim)
    assert n_p == -(-n_ids // max(1, 8192 // dim))                     # more than one workgroup at dim 256
    partials = torch.zeros(n_p, dtype=torch.float64, device=DEV)
    assert ops.grad_sqnorm_rows(out_rows, sorted_ids, N, partials) == n_p
    got = float(partials.cpu().numpy().sum())
    print(f"dim={dim}: partials {n_p}, squared sum rel err {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-10 * want
    norm = _norm_record(ops, partials, n_p)[0]
    assert abs(float(norm) - math.sqrt(want)) <= 3e-7 * math.sqrt(want)
    # only heads are read: whatever the other rows hold - here NaN - the result has the same bits
    poisoned = out_rows.clone()
    poisoned[(~head).to(DEV)] = float("nan")
    p2 = torch.zeros_like(partials)
    ops.grad_sqnorm_rows(poisoned, sorted_ids, N, p2)
    assert torch.equal(p2, partials) and bool(torch.isfinite(p2).all())
    p3 = torch.zeros_like(partials)
    ops.grad_sqnorm_rows(out_rows, sorted_ids, N, p3)
    assert torch.equal(p3, partials)
    # no ids at all: one zero
    p0 = torch.full((2,), 5.0, dtype=torch.float64, device=DEV)
    assert ops.grad_sqnorm_rows(out_rows[:0], sorted_ids[:0], N, p0) == 1
    assert p0.tolist() == [0.0, 5.0]


# ---- 4. the coefficient ------------------------------------------------------------------------------------------------
def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("pre_scale", [1.0, 0.5])
def test_clip_coefficient_is_torchs_formula_to_one_ulp(ops, pre_scale):
    max_norm = 1.0
    for norm in (100.0 / pre_scale, (1.0 + 3e-6) / pre_scale, 1.0 / pre_scale, 0.5 / pre_scale, 0.0):   # well above, just above, equal, below
        partials = torch.tensor([0.25 * norm * norm, 0.75 * norm * norm], dtype=torch.float64, device=DEV)
        got = _norm_record(ops, partials, 2, pre_scale, max_norm)
        total = math.sqrt(float(partials.cpu().sum())) * pre_scale
        coef = pre_scale * min(1.0, max_norm / (total + 1e-6))
        assert abs(float(got[0]) - total) <= _ulp32(total), (norm, got, total)
        assert abs(float(got[1]) - coef) <= _ulp32(coef), (norm, got, coef)
        if norm * pre_scale <= 0.5:
            assert float(got[1]) == np.float32(pre_scale)               # below the threshold: exactly the plain 1/W scale
        elif norm > 0:
            assert float(got[1]) < pre_scale                            # (at the threshold too: max / (max + 1e-6) < 1)
    # the norm of a halved gradient: pre_scale = 0.5 over g is pre_scale = 1 over g / 2
    gen = torch.Generator().manual_seed(3)
    g = _wide((4097,), gen).to(DEV)
    pa, pb = (torch.zeros(1, dtype=torch.float64, device=DEV) for _ in range(2))
    ops.grad_sqnorm_flat(g, pa)
    ops.grad_sqnorm_flat(g * 0.5, pb)
    a, b = _norm_record(ops, pa, 1, 0.5, 1e-3), _norm_record(ops, pb, 1, 1.0, 1e-3)
    assert a[0] == b[0] and abs(float(a[1]) - 0.5 * float(b[1])) <= _ulp32(float(a[1]))
    # a non-finite norm propagates as torch's formula propagates it: inf -> coefficient 0, nan -> nan
    for bad, want in ((float("inf"), 0.0), (float("nan"), float("nan"))):
        r = _norm_record(ops, torch.tensor([bad], dtype=torch.float64, device=DEV), 1, 1.0, 1.0)
        assert (math.isnan(r[0]) and math.isnan(r[1])) if math.isnan(want) else (math.isinf(r[0]) and r[1] == 0.0)


# ---- 5 - 7. one optimizer ----------------------------------------------------------------------------------------------
N_T, D_T = 300, 32


class Tiny(torch.nn.Module):
    def __init__(self, n=N_T, d=D_T):
        super().__init__()
        self.item_embedding = torch.nn.Embedding(n, d)
        self.other = torch.nn.Parameter(torch.randn(7))             # 7 elements: the flat buffer pads it to 8
        self.mat = torch.nn.Parameter(torch.randn(5, 9))
        self.sparse_grad = None


def _feed(ops, model, slot, ids, rows, dense_grads):
    """One backward's worth of gradients as the optimizer finds them: a SparseRowGrad on the module (the real segment sum)
    and the dense gradients in the flat buffer."""
    from REC.model.hstu_functional import SparseRowGrad
    sorted_ids, perm = torch.sort(ids)
    out_rows = torch.zeros(ids.numel(), rows.shape[1], device=rows.device)
    ops.sparse_rows_segment_sum(sorted_ids, perm, rows, None, None, 0, 0, out_rows, slot)
    model.sparse_grad = SparseRowGrad(sorted_ids, out_rows, slot, slot.numel())
    for p, g in zip((model.other, model.mat), dense_grads):
        p.grad.copy_(g)
    return model.sparse_grad


@pytest.mark.parametrize("lazy", [True, False])
def test_clipped_optimizer_against_torch_clip_grad_norm_and_the_adamw_oracle(rec, ops, lazy):
    from mhr_amd.optim import FusedAdamW
    torch.manual_seed(21)
    model = Tiny().to(DEV)
    ref = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    keys = ["item_embedding.weight", "other", "mat"]
    mom = {k: (torch.zeros_like(ref[k]), torch.zeros_like(ref[k])) for k in keys}
    max_norm, lr, wd = 1.0, 1e-2, 0.01
    opt = FusedAdamW(model, lr=lr, weight_decay=wd, lazy_table=lazy, clip_grad_norm=max_norm)
    assert opt.lazy == lazy
    slot = torch.full((N_T,), -1, dtype=torch.int32, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    clipped = []
    for t, mag in enumerate((3.0, 0.002, 0.5, 0.001, 0.004)):         # gradient norms on both sides of max_norm
        ids = (torch.rand(64, device=DEV, generator=gen) ** 2 * (N_T - 1)).long()
        rows = torch.randn(64, D_T, device=DEV, generator=gen) * mag
        dg = [torch.randn(7, device=DEV, generator=gen) * mag, torch.randn(5, 9, device=DEV, generator=gen) * mag]
        opt.catch_up(ids)
        sg = _feed(ops, model, slot, ids, rows, dg)
        grads = {"item_embedding.weight": sg.to_dense().cpu(), "other": dg[0].cpu(), "mat": dg[1].cpu()}
        opt.step()
        got_norm = float(opt.grad_norm)
        opt.zero_grad()
        params = []
        for k in keys:
            p = torch.nn.Parameter(ref[k])
            p.grad = grads[k].clone()
            params.append(p)
        want_norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False))
        assert abs(got_norm - want_norm) <= 1e-6 * want_norm, (t, got_norm, want_norm)
        clipped.append(want_norm > max_norm)
        with torch.no_grad():
            for k, p in zip(keys, params):
                OO.adamw_step(ref[k], p.grad, mom[k][0], mom[k][1], t + 1, lr, weight_decay=wd)
        opt.flush_table()
        for k, p, m_, v_ in (("item_embedding.weight", model.item_embedding.weight, opt.t_m, opt.t_v),
                             ("other", model.other, *(b[model.other._mhr_flat_off:][:7] for b in (opt.flat_m, opt.flat_v))),
                             ("mat", model.mat, *(b[model.mat._mhr_flat_off:][:45].view(5, 9) for b in (opt.flat_m, opt.flat_v)))):
            np.testing.assert_allclose(p.detach().cpu().numpy(), ref[k].numpy(), rtol=2e-5, atol=1e-6, err_msg=f"{k} step {t}")
            np.testing.assert_allclose(m_.cpu().numpy(), mom[k][0].numpy(), rtol=2e-5, atol=1e-6, err_msg=f"m {k} step {t}")
            np.testing.assert_allclose(v_.cpu().numpy(), mom[k][1].numpy(), rtol=2e-5, atol=1e-9, err_msg=f"v {k} step {t}")
    assert any(clipped) and not all(clipped), clipped
    assert int((slot != -1).sum()) == 0


def test_a_model_without_item_table_is_clipped_on_its_flat_gradient_alone(rec, ops, monkeypatch):
    """The HLLM twin has no trainable table: one squared-norm launch, the coefficient, the flat Adam."""
    from mhr_amd import lib
    from mhr_amd.optim import FusedAdamW
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])

    class NoTable(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.randn(7))
            self.b = torch.nn.Parameter(torch.randn(33, 9))

    torch.manual_seed(23)
    model = NoTable().to(DEV)
    ref = [p.detach().cpu().clone() for p in (model.a, model.b)]
    mom = [(torch.zeros_like(r), torch.zeros_like(r)) for r in ref]
    opt = FusedAdamW(model, lr=1e-2, clip_grad_norm=2.0)
    assert opt.table is None
    gen = torch.Generator(device=DEV).manual_seed(9)
    for t, mag in enumerate((1.0, 0.01)):
        gs = [torch.randn(p.shape, device=DEV, generator=gen) * mag for p in (model.a, model.b)]
        for p, g in zip((model.a, model.b), gs):
            p.grad.copy_(g)
        calls.clear()
        opt.step()
        assert [c for c in calls if c in NEW_ENTRIES] == ["mhr_grad_sqnorm_flat", "mhr_grad_clip_coef", "mhr_adam_flat_scaled"]
        got = float(opt.grad_norm)
        opt.zero_grad()
        params = [torch.nn.Parameter(r) for r in ref]
        for p, g in zip(params, gs):
            p.grad = g.cpu()
        want = float(torch.nn.utils.clip_grad_norm_(params, 2.0))
        assert abs(got - want) <= 1e-6 * want and (want > 2.0) == (t == 0)
        with torch.no_grad():
            for r, p, (m_, v_) in zip(ref, params, mom):
                OO.adamw_step(r, p.grad, m_, v_, t + 1, 1e-2)
        for p, r in zip((model.a, model.b), ref):
            np.testing.assert_allclose(p.detach().cpu().numpy(), r.numpy(), rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(opt.flat_m[model.b._mhr_flat_off:][:297].view(33, 9).cpu().numpy(), mom[1][0].numpy(), rtol=2e-5, atol=1e-6)


def test_dense_table_gradient_mode_is_clipped_through_the_flat_norm_kernel(rec, ops):
    """`dense_embedding_grad` mode: the table's gradient is `table.grad`; its norm comes from the flat kernel."""
    from mhr_amd.optim import FusedAdamW
    torch.manual_seed(24)
    model = Tiny().to(DEV)
    keys = ["item_embedding.weight", "other", "mat"]
    ref = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    mom = {k: (torch.zeros_like(ref[k]), torch.zeros_like(ref[k])) for k in keys}
    opt = FusedAdamW(model, lr=1e-2, weight_decay=0.01, clip_grad_norm=1.0)
    gen = torch.Generator(device=DEV).manual_seed(10)
    for t, mag in enumerate((0.1, 0.001)):
        grads = {k: torch.randn(ref[k].shape, device=DEV, generator=gen) * mag for k in keys}
        model.item_embedding.weight.grad = grads["item_embedding.weight"].clone()
        model.other.grad.copy_(grads["other"])
        model.mat.grad.copy_(grads["mat"])
        opt.step()
        got = float(opt.grad_norm)
        opt.zero_grad()
        params = [torch.nn.Parameter(ref[k]) for k in keys]
        for p, k in zip(params, keys):
            p.grad = grads[k].cpu()
        want = float(torch.nn.utils.clip_grad_norm_(params, 1.0))
        assert abs(got - want) <= 1e-6 * want and (want > 1.0) == (t == 0), (got, want)
        with torch.no_grad():
            for k, p in zip(keys, params):
                OO.adamw_step(ref[k], p.grad, mom[k][0], mom[k][1], t + 1, 1e-2, weight_decay=0.01)
        np.testing.assert_allclose(model.item_embedding.weight.detach().cpu().numpy(), ref[keys[0]].numpy(), rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(opt.t_m.cpu().numpy(), mom[keys[0]][0].numpy(), rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(opt.t_v.cpu().numpy(), mom[keys[0]][1].numpy(), rtol=2e-5, atol=1e-9)
        np.testing.assert_allclose(model.mat.detach().cpu().numpy(), ref["mat"].numpy(), rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("lazy", [True, False])
def test_off_is_todays_step_and_a_loose_threshold_is_the_identity(rec, ops, lazy, monkeypatch):
    from mhr_amd import lib
    from mhr_amd.optim import FusedAdamW
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    torch.manual_seed(22)
    models = [Tiny().to(DEV) for _ in range(3)]
    for m in models[1:]:
        m.load_state_dict(models[0].state_dict())
    opts = [FusedAdamW(models[0], lr=1e-2, weight_decay=0.01, lazy_table=lazy),                        # the parent's call
            FusedAdamW(models[1], lr=1e-2, weight_decay=0.01, lazy_table=lazy, clip_grad_norm=None),
            FusedAdamW(models[2], lr=1e-2, weight_decay=0.01, lazy_table=lazy, clip_grad_norm=1e30)]
    slots = [torch.full((N_T,), -1, dtype=torch.int32, device=DEV) for _ in opts]
    gen = torch.Generator(device=DEV).manual_seed(6)
    seen = []
    for t in range(6):
        ids = (torch.rand(64, device=DEV, generator=gen) ** 2 * (N_T - 1)).long()
        rows = torch.randn(64, D_T, device=DEV, generator=gen)
        dg = [torch.randn(7, device=DEV, generator=gen), torch.randn(5, 9, device=DEV, generator=gen)]
        for m, o, s in zip(models, opts, slots):
            o.catch_up(ids)
            _feed(ops, m, s, ids, rows, dg)
            calls.clear()
            o.step()
            seen.append(sorted(set(c for c in calls if c in NEW_ENTRIES)))
            o.zero_grad()
    assert all(s == [] for s in seen[0::3]) and all(s == [] for s in seen[1::3])        # off: none of the new entry points
    assert all(len(s) == 5 for s in seen[2::3]), seen[2]                                # on: two norms, the coefficient, two Adams
    assert float(opts[2].grad_norm) > 1.0 and opts[0].grad_norm is None
    for o in opts:
        o.flush_table()
    for m, o in zip(models[1:], opts[1:]):
        assert torch.equal(m.item_embedding.weight, models[0].item_embedding.weight)
        for name in ("flat_w", "flat_m", "flat_v", "flat_w16", "t_m", "t_v"):
            assert torch.equal(getattr(o, name), getattr(opts[0], name)), name


def test_lazy_equals_dense_bitwise_with_clipping(rec, ops):
    """`test_lazy_table_adam_is_bitwise_the_dense_update` with a threshold most steps exceed: 70 steps, across one flush."""
    from mhr_amd.optim import FusedAdamW, LAZY_HIST
    N, D = 3000, 64
    torch.manual_seed(4)
    m_lazy, m_dense = Tiny(N, D).to(DEV), Tiny(N, D).to(DEV)
    m_dense.load_state_dict(m_lazy.state_dict())
    # 96 rows of 64 unit normals: a norm near 78 (less where ids repeat); every fourth step is scaled down below the threshold
    o_lazy = FusedAdamW(m_lazy, lr=1e-3, weight_decay=0.01, lazy_table=True, clip_grad_norm=20.0)
    o_dense = FusedAdamW(m_dense, lr=1e-3, weight_decay=0.01, lazy_table=False, clip_grad_norm=20.0)
    assert o_lazy.lazy and not o_dense.lazy
    gen = torch.Generator(device=DEV).manual_seed(8)
    slot_l = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    slot_d = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    norms = []
    for t in range(70):
        ids = ((torch.rand(96, device=DEV, generator=gen) ** 4 * (N - 1)).long() + 1).clamp_(max=N - 1)
        o_lazy.catch_up(ids)
        assert torch.equal(m_lazy.item_embedding.weight[ids], m_dense.item_embedding.weight[ids]), t
        rows = torch.randn(96, D, device=DEV, generator=gen) * (0.1 if t % 4 == 3 else 1.0)
        dg = [torch.randn(7, device=DEV, generator=gen), torch.randn(5, 9, device=DEV, generator=gen)]
        _feed(ops, m_lazy, slot_l, ids, rows, dg)
        _feed(ops, m_dense, slot_d, ids, rows, dg)
        lr = 1e-3 * (0.5 + 0.5 * math.cos(t / 40.0))
        for opt in (o_lazy, o_dense):
            opt.param_groups[0]["lr"] = lr
            opt.step()
            opt.zero_grad()
        assert torch.equal(o_lazy.grad_norm, o_dense.grad_norm)
        norms.append(float(o_lazy.grad_norm))
        if (t + 1) % LAZY_HIST == 0:
            assert int((o_lazy.last_step < o_lazy.step_count).sum()) == 0            # the periodic flush happened
    n_clipped = sum(n > 20.0 for n in norms)
    assert n_clipped > 40 and n_clipped < 70, n_clipped                               # most steps clip, some do not
    o_lazy.flush_table()
    assert torch.equal(m_lazy.item_embedding.weight, m_dense.item_embedding.weight)
    assert torch.equal(o_lazy.t_m, o_dense.t_m) and torch.equal(o_lazy.t_v, o_dense.t_v)
    assert torch.equal(o_lazy.flat_w, o_dense.flat_w) and torch.equal(o_lazy.flat_v, o_dense.flat_v)


# ---- 8. replayed == host-issued ----------------------------------------------------------------------------------------
SMALL = dict(MAX_ITEM_LIST_LENGTH=16, pred_len=2, eval_pred_len=2, n_layers=2, n_heads=2, item_embedding_size=32,
             hstu_embedding_size=32, loss='prior', num_prior_head=2, num_segment_head=1, medusa_num_layers=1,
             neg_sample_by_cat=True, num_negatives=128, total_iters=40, eval_interval=0, checkpoint_dir=None,
             save_model_note="t", scheduler_args={'type': 'cosine', 'warmup': 0.25},
             optim_args={'learning_rate': 5e-4, 'weight_decay': 0.0}, topk=[5, 20])


def _trainer(graph, **over):
    import mhr_amd.synth as synth
    from REC.config.configurator import Config, apply_run_fixups
    from REC.trainer import Trainer
    from REC.utils import get_model
    dev = torch.device("cuda", 0)
    kw = dict(SMALL, device=dev, hip_graph=graph)
    kw.update(over)
    cfg = apply_run_fixups(Config(config_dict=synth.base_config(**kw)))
    data = synth.SyntheticData(cfg, 400, dev)
    cfg["int_to_category"] = data.int_to_category
    torch.manual_seed(11)
    model = get_model("HSTU")(cfg, data).to(dev)
    tr = Trainer(cfg)
    tr.setup_model(model)
    return tr, model, data, cfg


def test_replayed_clipped_steps_are_the_host_issued_steps_bit_for_bit(rec, ops):
    ops.set_deterministic(True)
    try:
        probe, _, data, _ = _trainer(False, clip_grad_norm=1e30)          # an identity threshold: the norm is measured, not guessed
        batches = [data.train_batch(8) for _ in range(4)]
        typical = []
        for b in batches[:3]:
            probe.train_step_fn(b, graph=False)
            typical.append(float(probe.optimizer.grad_norm))
        assert all(math.isfinite(n) and n > 0 for n in typical)
        clip = 0.25 * min(typical)
        tr_e, m_e, _, _ = _trainer(False, clip_grad_norm=clip)
        tr_g, m_g, _, _ = _trainer(True, clip_grad_norm=clip)
        n_steps = 10                                                      # three host-issued warm-up steps, seven replayed
        le, lg, ne, ng = [], [], [], []
        for i in range(n_steps):
            b = batches[i % len(batches)]
            le.append(float(tr_e.train_step_fn(b, graph=False)["loss"]))
            ne.append(float(tr_e.optimizer.grad_norm))
            lg.append(float(tr_g.train_step_fn(b)["loss"]))
            ng.append(float(tr_g.optimizer.grad_norm))
        assert tr_g.graph_active and not tr_e.graph_active
        assert tr_g._step_graph.n == n_steps - 3 >= 5
        assert all(n > clip for n in ne), (clip, ne)                      # every step clipped
        assert le == lg and ne == ng, (le, lg, ne, ng)
        assert torch.equal(tr_e.optimizer.grad_norm, tr_g.optimizer.grad_norm)
        sd_e, sd_g = m_e.state_dict(), m_g.state_dict()                   # (flushes the lazy table)
        for k in sd_e:
            assert torch.equal(sd_e[k], sd_g[k]), k
        for name in ("flat_w", "flat_m", "flat_v", "t_m", "t_v"):
            assert torch.equal(getattr(tr_e.optimizer, name), getattr(tr_g.optimizer, name)), name
    finally:
        ops.set_deterministic(False)


# ---- 9. model level against the oracle ---------------------------------------------------------------------------------
def test_model_level_grad_norm_against_the_fp32_oracle(rec, ops):
    """Three clipped steps of the small model next to the fp32 CPU oracle (torch autograd over `HO.train_forward`, torch's
    clip_grad_norm_, the oracle's AdamW): the port's pre-clip norm against the oracle's total norm.  Bound: 6e-2 relative - the
    fraction of a gradient's scale that the whole-model gradient comparison of this suite accepts between the bf16-mixed port
    and an fp32 reference (tests/test_gpu_model.py: `test_train_step_vs_reference_golden`, every gradient within 6e-2 of its
    max-abs).  Measured port / oracle: 1.0019, 0.9993, 1.0026 over the three steps.  Dropout is off: the oracle has no dropout
    masks to share."""
    from oracle import hstu_oracle as HO
    tr, model, data, cfg = _trainer(False, clip_grad_norm=1e30, hidden_dropout_prob=0.0, attn_dropout_prob=0.0)
    probe_batch = data.train_batch(8)
    w = HO.tie_repeated_resblocks({k: v.detach().cpu().clone().requires_grad_(v.is_floating_point())
                                   for k, v in model.state_dict().items()})
    ocfg = dict(cfg.final_config_dict)
    ocfg.update(int_to_category=data.int_to_category, category_counts=data.category_counts, category_to_int=data.category_to_int,
                item_num=400)
    uniq = {}
    for k, v in w.items():
        if torch.is_tensor(v) and v.requires_grad:
            uniq.setdefault(id(v), (k, v))
    params = [v for _, v in uniq.values()]
    mom = [(torch.zeros_like(p), torch.zeros_like(p)) for p in params]

    def oracle_backward(b):
        for p in params:
            p.grad = None
        HO.train_forward(w, ocfg, tuple(x.cpu() for x in b))["loss"].backward()
        return [p for p in params if p.grad is not None]

    # the threshold from a measured norm (of the oracle, before any step): half of it, so that every step clips
    live = oracle_backward(probe_batch)
    clip = 0.5 * float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in live)))
    tr.optimizer.clip_grad_norm = clip
    ratios = []
    for t in range(3):
        b = data.train_batch(8)
        lr = tr._lr_at(tr.train_step)
        tr.train_step_fn(b, graph=False)
        got = float(tr.optimizer.grad_norm)
        live = oracle_backward(b)
        want = float(torch.nn.utils.clip_grad_norm_(live, clip))
        ratios.append(got / want)
        print(f"step {t}: port grad_norm {got:.6f}, oracle {want:.6f}, ratio {got / want:.5f}, threshold {clip:.6f}")
        assert want > clip
        assert abs(got - want) <= 6e-2 * want, (t, got, want)
        with torch.no_grad():
            for p, (m_, v_) in zip(params, mom):
                if p.grad is not None:
                    OO.adamw_step(p, p.grad, m_, v_, t + 1, lr, weight_decay=0.0)


# ---- 10. data parallel -------------------------------------------------------------------------------------------------
DP_CLIP_SCRIPT = r'''
import os, sys
import numpy as np, torch, torch.distributed as dist
root, code, out_dir = sys.argv[1:4]
sys.path.insert(0, root); sys.path.insert(0, code)
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
import mhr_amd.synth as synth
from REC.config.configurator import Config, apply_run_fixups
from REC.trainer import Trainer
from REC.utils import get_model
cfgd = synth.base_config(**eval(open(os.path.join(out_dir, "cfg.txt")).read()), device=dev)
cfg = apply_run_fixups(Config(config_dict=cfgd))
data = synth.SyntheticData(cfg, 3000, dev, seed=11, rank=rank, world=world)
cfg["int_to_category"] = data.int_to_category
torch.manual_seed(5)
model = get_model("HSTU")(cfg, data).to(dev)
tr = Trainer(cfg); tr.setup_model(model); tr.train_step = 30
opt = tr.optimizer
assert opt.clip_grad_norm == 1e30
# one step under the identity threshold measures the norm (the same bits on both ranks); a quarter of it is the threshold
tr.train_step_fn(data.train_batch(8), graph=False)
n0 = float(opt.grad_norm)
opt.clip_grad_norm = 0.25 * n0
norms, refs = [n0], []
for _ in range(3):
    # one step as the Trainer issues it, minus zero_grad(): the exchanged gradient is still there to be measured
    out = model(data.train_batch(8))
    out["loss"].backward()
    opt.param_groups[0]["lr"] = tr._lr_at(tr.train_step); tr.train_step += 1
    opt.step()
    sg = model.sparse_grad
    head = torch.ones_like(sg.sorted_ids, dtype=torch.bool)
    head[1:] = sg.sorted_ids[1:] != sg.sorted_ids[:-1]
    sq = (opt.flat_g.double() / world).pow(2).sum() + (sg.rows[head].double() / world).pow(2).sum()
    refs.append(float(sq.sqrt()))
    norms.append(float(opt.grad_norm))
    opt.zero_grad()
model.sync_table()
torch.cuda.synchronize()
np.savez(os.path.join(out_dir, f"clip{rank}.npz"), table=model.item_embedding.weight.detach().cpu().numpy(),
         flat=opt.flat_w.cpu().numpy(), flat_m=opt.flat_m.cpu().numpy(), norms=np.array(norms, dtype=np.float64),
         refs=np.array(refs, dtype=np.float64), clip=np.array(opt.clip_grad_norm))
dist.barrier()
dist.destroy_process_group()
'''


def test_data_parallel_clipped_steps_two_ranks_one_card(rec, tmp_path):
    import subprocess
    kw = dict(MAX_ITEM_LIST_LENGTH=16, pred_len=2, eval_pred_len=2, n_layers=2, n_heads=2, item_embedding_size=64,
              hstu_embedding_size=64, num_negatives=256, total_iters=100, eval_interval=0, checkpoint_dir=None,
              save_model_note="t", hidden_dropout_prob=0.0, attn_dropout_prob=0.0, loss='prior', num_prior_head=3,
              medusa_num_layers=1, eval_num_cats=3, clip_grad_norm=1e30)
    (tmp_path / "cfg.txt").write_text(repr(kw))
    script = tmp_path / "dp_clip.py"
    script.write_text(DP_CLIP_SCRIPT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29671", WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT, CODE, str(tmp_path)], env=dict(env, RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, (o[-2000:], e[-4000:])
    a, b = (np.load(tmp_path / f"clip{i}.npz") for i in range(2))
    assert np.array_equal(a["norms"], b["norms"]) and float(a["clip"]) == float(b["clip"])          # the same grad_norm bits
    for k in ("table", "flat", "flat_m"):
        assert np.array_equal(a[k], b[k]), k                                                        # replicas stay replicas
    assert np.all(a["norms"][1:] > float(a["clip"]))                                                # three clipped steps
    # the norm of the AVERAGED gradient (torch fp64 over the exchanged buffers / W), to fp32 rounding
    print("grad_norm", a["norms"][1:], "fp64 norm of the averaged gradient", a["refs"])
    assert np.all(np.abs(a["norms"][1:] - a["refs"]) <= 3e-7 * a["refs"])
