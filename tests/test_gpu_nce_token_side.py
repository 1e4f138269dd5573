"""Token side of the row-sharing sampled softmax (csrc/nce_shared.hip): the per-query-row forward (mhr_nce_shared_fwd_rows) and
the row-wise backward (mhr_nce_shared_bwd_rows: float atomics / read-modify-write / store into zeroed rows).

Oracle and tolerances are those of test_nce_shared_query_rows_match_per_token_oracle and
test_nce_window_backward_without_token_atomics (tests/test_gpu_kernels.py): the pinned per-token oracle on bf16-rounded operands;
loss 1e-4, log counters exact / rank within 1 (fp32 ties), gradients 2e-2 of the max-abs.  On top of that the new forward entry
must equal the per-token entry BITWISE in all four outputs, the store mode must equal the read-modify-write on zeros bitwise, and
two deterministic-mode backwards must be bitwise equal.

Shapes: B = 3, L = 40; D in {64, 256} (lanes past dim); G in {1, 3}; P in {3, 8, 34} (P = 34: rows of more than 32 tokens run the
chunk loop; P > 8: more than one round of target rows in flight); n_neg in {96, 200} (a pool that is no multiple of 32).  Every
case has an odd live row count per live group (the unpaired last half-wave), a row whose tokens all have weight 0 (lw_row = +inf),
and target rows copied into the pools so that some tokens have one suppressed negative, some several, and two neighbouring rows
(the two halves of one wave) both have such tokens; the G = 3 cases have a group without a live token."""
import math

import numpy as np
import pytest
import torch

from kernel_oracles import nce_oracle
from oracle import hstu_oracle as HO

pytestmark = pytest.mark.gpu

B, L = 3, 40
CASES = [(64, 1, 3, 96), (256, 3, 8, 200), (64, 3, 34, 200), (256, 1, 34, 96)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import mhr_amd  # noqa: F401
    from mhr_amd import ops as _ops
    return _ops


def dev(t):
    return t.cuda().contiguous()


_CASE = {}


def _case(ops, D, G, P, n_neg):
    """One window-structured batch per shape, its forward record and its oracle (built once, shared by the tests, not modified)."""
    key = (D, G, P, n_neg)
    if key in _CASE:
        return _CASE[key]
    g = torch.Generator().manual_seed(1000 + D + 10 * G + P + n_neg)
    H = G
    head_rows = torch.randn(B * H * L, D, generator=g) * 2
    e_rows = torch.randn(B * (L + P), D, generator=g)
    valid = torch.rand(G, B, L, P, generator=g) < 0.5
    valid[:, 0, 0] = True                                  # two neighbouring full rows: all P offsets (P = 34: more than 32 tokens)
    valid[:, 0, 1] = True
    if G > 1:
        valid[1] = False                                   # a group without a live token
    for gi in range(G):                                    # an odd number of live rows per live group
        rows_live = valid[gi].any(-1)
        if int(rows_live.sum()) and int(rows_live.sum()) % 2 == 0:
            b_l = rows_live.reshape(-1).nonzero()[-1].item()
            valid[gi].reshape(B * L, P)[b_l] = False
    b_ = torch.arange(B)[None, :, None, None]
    l_ = torch.arange(L)[None, None, :, None]
    p_ = torch.arange(P)[None, None, None, :]
    h_ = torch.arange(G)[:, None, None, None]
    q_all = ((b_ * H + h_) * L + l_).expand(G, B, L, P).reshape(G, -1).int().contiguous()
    p_all = (b_ * (L + P) + l_ + 1 + p_).expand(1, B, L, P).reshape(-1).int().contiguous()
    o_all = p_.expand(1, B, L, P).reshape(-1).int().contiguous()
    q_idx, p_idx, o_idx, n_tok, tos = ops.token_compact(dev(valid.reshape(G, B * L * P)), dev(q_all), dev(p_all), dev(o_all), slot_map=True)
    cap = q_idx.shape[1]
    n_tok_h = [int(v) for v in n_tok.cpu()]
    negs = HO.l2n(torch.randn(G, n_neg, D, generator=g)).to(torch.bfloat16)
    p_idx_h = p_idx.cpu().long()

    def plant(gi, tok, slots, exact=False):
        """The token's own target becomes negative `slots` of its group's pool: an exact copy (as the sampler can draw it), or
        near-duplicates (cosine 0.999 to the target, each with its own noise).  Only ONE exact copy per group: an exact copy ties
        with the positive of every token that points at this target, and the rank tolerance below is one tie per token."""
        for j in slots:
            t = e_rows[p_idx_h[gi, tok]]
            if not exact:
                t = t + 0.04 * float(t.norm()) / math.sqrt(D) * torch.randn(D, generator=g)
            negs[gi, j % n_neg] = HO.l2n(t[None])[0].to(torch.bfloat16)

    for gi in range(G):
        n = n_tok_h[gi]
        if n == 0:
            continue
        plant(gi, 0, (3,), exact=True)                     # row 0 (half 0 of the first wave): one suppressed negative
        plant(gi, P, (40, 41, 77))                         # row 1 (half 1 of the same wave): several, in two 32-negative tiles
        plant(gi, P + 1, (n_neg - 1,))                     # ... and the last negative of the pool
        for k in range(2 * P + 5, n, 23):                  # a sprinkle over the rest of the list
            plant(gi, k, (k * 5,))
    ls = torch.tensor(math.log(15.0))
    lsd = ls.reshape(1).cuda()
    sv = ops.nce_fwd(dev(head_rows), q_idx, dev(e_rows), p_idx, dev(negs), n_tok, cap, lsd, 0.99, want_logs=True,
                     share_rows=True, window=(tos, L, P))
    assert sv.shared and sv.window is not None
    torch.cuda.synchronize()
    # per-token weights; the tokens of one row (the third live row of each live group) all get weight 0
    w = torch.rand(G, cap, generator=g)
    q_idx_h = q_idx.cpu().long()
    dead_rows = []
    for gi in range(G):
        n = n_tok_h[gi]
        w[gi, n:] = 0
        if n:
            w[gi, 7] = 0                                   # a zero-weight token inside a row that keeps other weights
            qr = q_idx_h[gi, :n].unique_consecutive()[2]
            w[gi, :n][q_idx_h[gi, :n] == qr] = 0
            dead_rows.append((gi, 2))
    # oracle: every token on its own
    hq = head_rows.clone().requires_grad_(True)
    ep = e_rows.clone().requires_grad_(True)
    nn_ = negs.float().clone().requires_grad_(True)
    lsr = ls.clone().requires_grad_(True)
    total, per_group = 0.0, []
    for gi in range(G):
        n = n_tok_h[gi]
        if n == 0:
            per_group.append(None)
            continue
        qi, pi = q_idx_h[gi, :n], p_idx_h[gi, :n]
        loss, logits, keep, neg, pos = nce_oracle(hq[qi], ep[pi], nn_[gi], lsr, 0.99)
        total = total + (loss * w[gi, :n]).sum()
        per_group.append((loss.detach(), torch.logsumexp(logits.detach(), -1), keep, neg, pos))
    total.backward()
    c = dict(D=D, G=G, P=P, n_neg=n_neg, sv=sv, lsd=lsd, q_idx=q_idx, p_idx=p_idx, n_tok=n_tok_h, cap=cap, w=dev(w), w_h=w,
             q_idx_h=q_idx_h, dead_rows=dead_rows, per_group=per_group, n_q_rows=B * H * L, n_p_rows=B * (L + P),
             ref=dict(dq=hq.grad, dp=ep.grad, dn=nn_.grad, dls=lsr.grad))
    _CASE[key] = c
    return c


@pytest.mark.parametrize("D,G,P,n_neg", CASES)
def test_forward_rows_entry_matches_oracle_and_token_entry_bitwise(ops, D, G, P, n_neg):
    """The product forward (which runs mhr_nce_shared_fwd_rows) against the per-token oracle: loss 1e-4, log counters of the rows'
    first tokens; then both token-side entry points on the same inputs (the saved row state, arbitrary row sums and counters so
    that every output bit is exercised): s_pos, sum_tok, n_valid_tok, rank_tok bitwise equal over the live tokens."""
    from mhr_amd import lib
    c = _case(ops, D, G, P, n_neg)
    sv = c["sv"]
    suppressed_tokens = 0
    for gi in range(G):
        n = c["n_tok"][gi]
        if n == 0:
            assert float(sv.loss[gi].abs().max()) == 0.0
            continue
        loss, lse, keep, neg, pos = c["per_group"][gi]
        np.testing.assert_allclose(sv.loss[gi, :n].cpu().numpy(), loss.numpy(), rtol=1e-4, atol=1e-4)
        assert float(sv.loss[gi, n:].abs().max()) == 0.0
        per_tok = (~keep).sum(-1)
        suppressed_tokens += int((per_tok > 0).sum())
        assert int((per_tok == 1).sum()) > 0 and int((per_tok > 1).sum()) > 0       # one and several suppressed negatives
        qh = c["q_idx_h"][gi, :n]
        first = torch.ones(n, dtype=torch.bool)
        first[1:] = qh[1:] != qh[:-1]
        assert int(first.sum()) % 2 == 1 and int(sv.n_row_dev[gi]) == int(first.sum())    # the unpaired last half-wave
        row_of = first.long().cumsum(0) - 1
        hit_rows = set(row_of[per_tok > 0].tolist())
        assert 0 in hit_rows and 1 in hit_rows                                         # both halves of the first wave
        if P > 32:
            assert int(torch.bincount(row_of).max()) > 32                              # the chunk loop
        np.testing.assert_array_equal(sv.n_valid[gi, :n].cpu().numpy()[first.numpy()], (keep.sum(-1) + 1).numpy()[first.numpy()])
        rank_ref = (keep & (neg > pos)).sum(-1)
        assert int((sv.rank[gi, :n].cpu() - rank_ref)[first].abs().max()) <= 1         # ties at fp32 rounding level
    assert suppressed_tokens > 0
    # --- the two entry points on the same inputs
    dvc, cap, row_cap = sv.negs.device, sv.cap, sv.row_cap
    g = torch.Generator().manual_seed(7)
    sum_row = torch.rand(G, row_cap, generator=g) * 3
    sum_row[:, 1::2] = 1e-30                               # below any suppressed negative's term exp(scale (s_j - 1)) >= e^-30: the clamp
    sum_row = dev(sum_row)
    nv_row = dev(torch.randint(0, n_neg, (G, row_cap), generator=g).int())
    rk_row = dev(torch.randint(0, 4, (G, row_cap), generator=g).int())          # small: max(rank - above, 0) clamps somewhere
    outs = []
    for entry in ("mhr_nce_shared_fwd_tokens", "mhr_nce_shared_fwd_rows"):
        s_pos = torch.full((G, cap), -7.0, device=dvc)
        ssum = torch.full((G, cap), -7.0, device=dvc)
        nv = torch.full((G, cap), -7, dtype=torch.int32, device=dvc)
        rk = torch.full((G, cap), -7, dtype=torch.int32, device=dvc)
        maps = ((sv.tok2row.data_ptr(), G, sv.n_tok_dev.data_ptr()) if entry.endswith("tokens") else
                (sv.row_first.data_ptr(), sv.n_row_dev.data_ptr(), G))
        lib.call(entry, sv.pn.data_ptr(), sv.n_p_rows, sv.p_idx.data_ptr(), *maps, cap, row_cap, sv.qn.data_ptr(), sum_row.data_ptr(),
                 nv_row.data_ptr(), rk_row.data_ptr(), sv.negs.data_ptr(), sv.n_neg, D, c["lsd"].data_ptr(), sv.fix_words.data_ptr(),
                 ops._ptr(sv.fix_slot), sv.fix_any.data_ptr(), s_pos.data_ptr(), ssum.data_ptr(), nv.data_ptr(), rk.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((s_pos, ssum, nv, rk))
    for name, a, b2 in zip(("s_pos", "sum_tok", "n_valid_tok", "rank_tok"), outs[0], outs[1]):
        assert torch.equal(a.view(torch.int32), b2.view(torch.int32)), name     # live tokens written alike, the rest left alone
        for gi in range(G):
            n = c["n_tok"][gi]
            assert n == 0 or not bool((b2[gi, :n] == -7).any()), name
            assert bool((b2[gi, n:] == -7).all()), name
    for gi in range(G):
        n = c["n_tok"][gi]
        if n:
            assert float(outs[1][1][gi, :n].min()) == 0.0 and int(outs[1][3][gi, :n].min()) == 0      # both clamps reached


def _backward(ops, c, exclusive, zero, lw_row=None):
    sv = c["sv"]
    dq = torch.zeros(c["n_q_rows"], c["D"], device="cuda")
    dp = torch.zeros(c["n_p_rows"], c["D"], device="cuda")
    dn, dls = ops.nce_bwd(sv, c["w"], c["lsd"], c["q_idx"], c["p_idx"], dq, dp, lw_row=lw_row, exclusive_q_rows=exclusive,
                          dq_rows_zero=zero)
    torch.cuda.synchronize()
    return dq, dp, dn, dls


@pytest.mark.parametrize("D,G,P,n_neg", CASES)
def test_backward_rows_modes_match_oracle_and_store_is_rmw_bitwise(ops, D, G, P, n_neg):
    """dq_rows, d(logit_scale) and d_negs (whose suppressed pairs the row kernel takes back out) against the per-token oracle at
    2e-2 of the max-abs, with float atomics, with the read-modify-write and with the store into zeroed rows; lw_row against
    -log2 sum_t w_t exp(-lse_t) of the oracle's log-sums; the store mode bitwise equal to the read-modify-write on zeros.
    lw_row tolerance: lse carries the loss tolerance (1e-4 + 1e-4 |lse|), times log2(e) = 1.443, rounded up: 2e-4 (1 + |ref|)."""
    c = _case(ops, D, G, P, n_neg)
    sv, ref = c["sv"], c["ref"]
    runs = {}
    for mode, (excl, zero) in (("atomic", (False, False)), ("rmw", (True, False)), ("store", (True, True))):
        lw_row = torch.full((G, sv.row_cap), float("inf"), device="cuda")
        dq, dp, dn, dls = _backward(ops, c, excl, zero, lw_row)
        runs[mode] = (dq, dp, dn, dls, lw_row)
        for name, got, r in (("dq", dq.cpu(), ref["dq"]), ("dp", dp.cpu(), ref["dp"]), ("dneg", dn.cpu(), ref["dn"])):
            gs = float(r.abs().max())
            err = float((got - r).abs().max())
            print(mode, name, "err", err, "scale", gs)
            assert err < 2e-2 * gs, (mode, name, err, gs)
        assert abs(float(dls.cpu()) - float(ref["dls"])) < 2e-2 * abs(float(ref["dls"])) + 1e-4, mode
        for gi in range(G):
            n = c["n_tok"][gi]
            got = lw_row[gi].cpu()
            if n == 0:
                assert bool(torch.isinf(got).all())
                continue
            lse = c["per_group"][gi][1].double()
            qh = c["q_idx_h"][gi, :n]
            first = torch.ones(n, dtype=torch.bool)
            first[1:] = qh[1:] != qh[:-1]
            row_of = first.long().cumsum(0) - 1
            n_row = int(first.sum())
            acc = torch.zeros(n_row, dtype=torch.float64).index_add_(0, row_of, c["w_h"][gi, :n].double() * torch.exp(-lse))
            lw_ref = -torch.log2(acc)                                      # (+inf where every token of the row has weight 0)
            dead = torch.isinf(lw_ref)
            assert bool(dead[2]) and int(dead.sum()) >= 1
            assert bool((got[:n_row][dead] == float("inf")).all()) and bool(torch.isinf(got[n_row:]).all())
            live = ~dead
            assert bool(((got[:n_row][live].double() - lw_ref[live]).abs() <= 2e-4 * (1 + lw_ref[live].abs())).all()), mode
    # dq (no atomics in either mode), dp and lw_row are bitwise reproducible; d_negs and d(logit_scale) are float atomics
    assert torch.equal(runs["store"][0].view(torch.int32), runs["rmw"][0].view(torch.int32))
    assert torch.equal(runs["store"][1], runs["rmw"][1]) and torch.equal(runs["store"][4], runs["rmw"][4])
    # rows no live (group, row) names stay exactly zero in every mode
    named = torch.zeros(c["n_q_rows"], dtype=torch.bool)
    for gi in range(G):
        named[c["q_idx_h"][gi, :c["n_tok"][gi]]] = True
    for mode in runs:
        assert float(runs[mode][0].cpu()[~named].abs().max()) == 0.0, mode


@pytest.mark.parametrize("D,G,P,n_neg", [CASES[1], CASES[2]])
def test_backward_deterministic_mode_twice_bitwise(ops, D, G, P, n_neg):
    """Deterministic mode (fixed-point d_negs, ordered d(logit_scale) partials): two backwards of the same record are bitwise
    equal in every output, in the store mode and in the read-modify-write mode, and the two modes agree bitwise."""
    c = _case(ops, D, G, P, n_neg)
    was = ops.DETERMINISTIC
    ops.set_deterministic(True)
    try:
        a = _backward(ops, c, True, True)
        b2 = _backward(ops, c, True, True)
        r = _backward(ops, c, True, False)
    finally:
        ops.set_deterministic(was)
    for name, x, y, z in zip(("dq", "dp", "dneg", "dls"), a, b2, r):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name
        assert torch.equal(x.view(torch.int32), z.view(torch.int32)), name
    ref = c["ref"]
    for name, got, rf in (("dq", a[0].cpu(), ref["dq"]), ("dneg", a[2].cpu(), ref["dn"])):
        assert float((got - rf).abs().max()) < 2e-2 * float(rf.abs().max()), name
